"""CPU-only checks of global-norm clipping and parameter groups in the detector's train step: the C ABI declares, exports and
validates the new entry points of csrc/optim_multi.hip without a device (ABI 6 still, the three older entry points untouched);
tests/clip_oracle.py follows torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW with two groups in float64; detector_param_groups
partitions the detector's parameters; refusals and the warmup line.  No kernel is launched here."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from layoutdit_amd import _lib, ops, training
from layoutdit_amd import config as cfgs
from layoutdit_amd import detector_training as dt
from layoutdit_amd.modeling import LayoutDetectionModel
from tests import clip_oracle as co
from tests import optim_oracle as oo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Seg, Hyper = _lib.LditOptSegment, _lib.LditOptHyper
ENC = "model.backbone.backbone.dit."


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ldit.h")).read(), flags=re.S)


def test_header_declares_and_library_exports_the_entry_points():
    text = _header()
    lib = _lib.load()
    want = {"ldit_grad_norm_partials": ("int64_t", ["const ldit_opt_segment *", "int32_t"]),
            "ldit_grads_check_norm_multi_f32": ("int", ["const ldit_opt_segment *", "int32_t", "ldit_opt_state *", "double *", "int64_t", "ldit_stream"]),
            "ldit_clip_finish": ("int", ["const ldit_opt_state *", "ldit_clip_state *", "const double *", "int64_t", "ldit_stream"]),
            "ldit_adamw_groups_multi_f32": ("int", ["const ldit_opt_segment *", "const ldit_opt_hyper *", "int32_t", "const ldit_opt_state *",
                                                    "const ldit_clip_state *", "double", "double", "float", "ldit_stream"])}
    ctype = {"int": C.c_int, "int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float, "double": C.c_double, "ldit_stream": C.c_void_p,
             "ldit_opt_state *": C.c_void_p, "const ldit_opt_state *": C.c_void_p, "ldit_clip_state *": C.c_void_p,
             "const ldit_clip_state *": C.c_void_p, "double *": C.c_void_p, "const double *": C.c_void_p,
             "const ldit_opt_segment *": C.POINTER(Seg), "const ldit_opt_hyper *": C.POINTER(Hyper)}
    for n, (res, types) in want.items():
        assert n in _lib.SIGNATURES and hasattr(lib, n), n
        args = re.search(r"\b%s\s+%s\s*\(([^)]*)\)" % (res, n), text).group(1)
        got = [re.sub(r"\s*\w+$", "", a.strip()).strip() for a in args.split(",")]
        assert got == types, (n, got)
        assert _lib.SIGNATURES[n] == (ctype[res], [ctype[t] for t in types]), n
    assert "#define LDIT_ABI_VERSION 6" in text and _lib.LDIT_ABI_VERSION == 6 and lib.ldit_abi_version() == 6     # purely additive
    # the two new structs: field order and size
    body = re.search(r"typedef struct ldit_clip_state \{(.*?)\} ldit_clip_state;", text, flags=re.S).group(1)
    fields = re.findall(r"(int32_t|float)\s+(\w+);", body)
    assert tuple(f for _, f in fields) == _lib.CLIP_STATE_FIELDS == co.FIELDS
    assert [t for t, _ in fields] == ["float", "float", "float", "int32_t"] and C.sizeof(_lib.LditClipState) == 16
    body = re.search(r"typedef struct ldit_opt_hyper \{(.*?)\} ldit_opt_hyper;", text, flags=re.S).group(1)
    assert re.findall(r"float\s+(\w+);", body) == [f for f, _ in Hyper._fields_] == ["lr_scale", "weight_decay"] and C.sizeof(Hyper) == 8
    # what the older tests freeze
    assert C.sizeof(_lib.LditOptState) == 40 and C.sizeof(Seg) == 48 and ops.OPT_MAX_SEGMENTS == 64 and ops.OPT_GROUP_SEGMENTS == 48
    assert _lib.SIGNATURES["ldit_adamw_multi_f32"] == (C.c_int, [C.POINTER(Seg), C.c_int32, C.c_void_p, C.c_double, C.c_double, C.c_float,
                                                                  C.c_float, C.c_float, C.c_void_p])


def _segs(*rows):
    arr = (Seg * max(len(rows), 1))()
    for s, (p, g, m, v, n, mirror) in zip(arr, rows):
        s.p, s.g, s.m, s.v, s.n, s.bf16_mirror = p, g, m, v, n, mirror
    return arr


def _hyper(*rows):
    arr = (Hyper * max(len(rows), 1))()
    for h, (s, w) in zip(arr, rows):
        h.lr_scale, h.weight_decay = s, w
    return arr


def test_arguments_are_validated_before_any_launch():
    lib = _lib.load()
    err = lambda: lib.ldit_last_error().decode()                                      # noqa: E731
    good = (16, 32, 48, 64, 8, None)
    ST, CL, PA = 256, 512, 1024

    def norm(segs=_segs(good), S=1, state=ST, partials=PA, length=1):
        return lib.ldit_grads_check_norm_multi_f32(segs, S, state, partials, length, None)

    def update(segs=_segs(good), hyper=_hyper((1.0, 0.0)), S=1, state=ST, clip=CL, b1=0.9, b2=0.999):
        return lib.ldit_adamw_groups_multi_f32(segs, hyper, S, state, clip, b1, b2, 1e-8, None)

    def finish(state=ST, clip=CL, partials=PA, n=1):
        return lib.ldit_clip_finish(state, clip, partials, n, None)

    for fn in (norm, update):
        assert fn(S=-1) == _lib.LDIT_EINVAL and "negative" in err()
        assert fn(segs=None) == _lib.LDIT_EINVAL and "null" in err()
        assert fn(state=None) == _lib.LDIT_EINVAL and "state" in err()
        assert fn(state=258) == _lib.LDIT_EINVAL and "aligned" in err()
        assert fn(segs=_segs((16, 32, 48, 64, -1, None))) == _lib.LDIT_EINVAL and "negative length" in err()
        assert fn(segs=_segs((16, None, 48, 64, 8, None))) == _lib.LDIT_EINVAL and "null" in err()
        assert fn(segs=_segs((16, 34, 48, 64, 8, None))) == _lib.LDIT_EINVAL and "4-byte" in err()
    two = _segs(good, (16, 32, 48, 64, -5, None))
    assert norm(segs=two, S=2, length=2) == _lib.LDIT_EINVAL and "segment 1" in err()
    assert update(segs=two, hyper=_hyper((1.0, 0.0), (1.0, 0.0)), S=2) == _lib.LDIT_EINVAL and "segment 1" in err()
    # the partials buffer: counted per 1 024 elements of each segment, a shorter one refused, 8-byte aligned
    three = _segs((16, 32, 48, 64, 1025, None), (None, None, None, None, 0, None), (16, 32, 48, 64, 1, None))
    assert lib.ldit_grad_norm_partials(three, 3) == 3 and lib.ldit_grad_norm_partials(three, 0) == 0
    assert lib.ldit_grad_norm_partials(None, 1) == -1 and "null" in err()
    assert lib.ldit_grad_norm_partials(two, 2) == -1 and "segment 1" in err()
    assert lib.ldit_grad_norm_partials(three, -1) == -1 and "negative" in err()
    assert norm(segs=three, S=3, length=2) == _lib.LDIT_EINVAL and "need 3" in err()
    assert norm(length=-1) == _lib.LDIT_EINVAL and "negative" in err()
    assert norm(partials=None) == _lib.LDIT_EINVAL and "null partials" in err()
    assert norm(partials=1028) == _lib.LDIT_EINVAL and "8-byte" in err()
    # the update: p, m, v and the mirror as in ldit_adamw_multi_f32, the hyper-parameters, the clip block
    for k in (0, 2, 3):
        row = list(good)
        row[k] = None
        assert update(segs=_segs(tuple(row))) == _lib.LDIT_EINVAL and "null" in err()
        row[k] = 18
        assert update(segs=_segs(tuple(row))) == _lib.LDIT_EINVAL and "4-byte" in err()
    assert update(segs=_segs((16, 32, 48, 64, 8, 65))) == _lib.LDIT_EINVAL and "mirror" in err()
    assert update(hyper=None) == _lib.LDIT_EINVAL and "hyper" in err()
    assert update(segs=_segs(good, good), hyper=_hyper((1.0, 0.0), (-0.5, 0.0)), S=2) == _lib.LDIT_EINVAL and "segment 1" in err()
    assert update(hyper=_hyper((1.0, -1.0))) == _lib.LDIT_EINVAL and "segment 0" in err()
    assert update(hyper=_hyper((float("nan"), 0.0))) == _lib.LDIT_EINVAL
    assert update(clip=514) == _lib.LDIT_EINVAL and "clip" in err()
    assert update(b1=1.0) == _lib.LDIT_EINVAL and update(b2=-0.1) == _lib.LDIT_EINVAL and "betas" in err()
    # the finish
    assert finish(state=None) == _lib.LDIT_EINVAL and "state" in err()
    assert finish(clip=None) == _lib.LDIT_EINVAL and "clip" in err()
    assert finish(clip=514) == _lib.LDIT_EINVAL and "clip" in err()
    assert finish(n=-1) == _lib.LDIT_EINVAL and "negative" in err()
    assert finish(partials=None) == _lib.LDIT_EINVAL and "null partials" in err()
    assert finish(partials=1028) == _lib.LDIT_EINVAL and "8-byte" in err()

    if not torch.cuda.is_available():
        # no device: the library's HIP error, for empty work too.  (Where a device exists these well-formed calls would launch on
        # made-up addresses; there only the launch-free ones are made.)
        assert norm() == _lib.LDIT_EHIP and "hip" in err().lower()
        assert update() == _lib.LDIT_EHIP and update(clip=None) == _lib.LDIT_EHIP and finish() == _lib.LDIT_EHIP
        assert norm(S=0, partials=None, length=0) == _lib.LDIT_EHIP
        assert update(segs=_segs((None, None, None, None, 0, None))) == _lib.LDIT_EHIP
    else:
        assert norm(S=0, partials=None, length=0) == _lib.LDIT_OK and update(segs=_segs((None, None, None, None, 0, None))) == _lib.LDIT_OK


def test_clip_oracle_follows_torch_clip_grad_norm_and_adamw_groups_in_float64():
    """Five steps, two groups (lr x 1 with decay 0.01, lr x 0.5 without), loss scale 1024, max_norm 1: the gradient scale of steps
    0, 2 and 4 puts the norm above the bound, that of steps 1 and 3 below it."""
    rng = np.random.RandomState(5)
    sizes, scales, wds, LR, MAXN = (257, 31), (1.0, 0.5), (0.01, 0.0), 1e-2, 1.0
    p0 = [rng.normal(0, 1, size=n) for n in sizes]
    ref = [torch.nn.Parameter(torch.from_numpy(x.copy())) for x in p0]
    opt = torch.optim.AdamW([{"params": [q], "lr": LR * s, "weight_decay": w} for q, s, w in zip(ref, scales, wds)], lr=LR,
                            betas=(0.9, 0.999), eps=1e-8)
    st, clip = oo.new_state(scale=1024.0, lr=LR), co.new_clip(MAXN)
    mine = [(x.copy(), np.zeros_like(x), np.zeros_like(x)) for x in p0]
    active = []
    for i in range(5):
        grads = [rng.normal(0, 0.2 if i % 2 == 0 else 0.01, size=n) for n in sizes]
        for q, g in zip(ref, grads):
            q.grad = torch.from_numpy(g.copy())
        norm = torch.nn.utils.clip_grad_norm_(ref, MAXN)
        opt.step()
        scaled = [g * 1024.0 for g in grads]
        st = oo.advance(oo.check(st, scaled))
        clip = co.finish(st, clip, scaled)
        active.append(clip["clip_coef"] < 1.0)
        np.testing.assert_allclose(clip["total_norm"], float(norm), rtol=1e-12)
        mine = [co.adamw_groups(p, g, m, v, st, lr_scale=s, weight_decay=w, coef=clip["clip_coef"])
                for (p, m, v), g, s, w in zip(mine, scaled, scales, wds)]
    assert active == [True, False, True, False, True] and clip["clipped_steps"] == 3
    for (p, m, v), q in zip(mine, ref):
        np.testing.assert_allclose(p, q.detach().numpy(), rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(m, opt.state[q]["exp_avg"].numpy(), rtol=1e-12, atol=1e-18)
        np.testing.assert_allclose(v, opt.state[q]["exp_avg_sq"].numpy(), rtol=1e-12, atol=1e-20)
    # a non-finite gradient: the norm is not finite, the step is skipped, nothing else of the block moves
    bad = [np.full(n, 1.0) for n in sizes]
    bad[1][-1] = np.nan
    st = oo.advance(oo.check(st, bad))
    after = co.finish(st, clip, bad)
    assert st["skip"] == 1 and not np.isfinite(after["total_norm"])
    assert (after["clip_coef"], after["clipped_steps"]) == (clip["clip_coef"], clip["clipped_steps"])
    q, _, _ = co.adamw_groups(mine[0][0], bad[0], mine[0][1], mine[0][2], st, coef=after["clip_coef"])
    np.testing.assert_array_equal(q, mine[0][0])
    # squares that overflow fp32 are nothing to float64
    assert co.finish(oo.advance(oo.new_state(scale=1.0)), co.new_clip(1.0), [np.full(4, 1e20, np.float32)])["total_norm"] == pytest.approx(2e20, rel=1e-7)


def test_detector_param_groups_partition_the_micro_detector():
    cfg = cfgs.vit_micro()
    model = LayoutDetectionModel(config=cfg)
    L = cfg.num_hidden_layers
    named = dict(model.named_parameters())
    groups = training.detector_param_groups(model, layer_decay=0.75, weight_decay=0.05)
    listed = [n for g in groups for n in g["params"]]
    assert sorted(listed) == sorted(named) and len(set(listed)) == len(listed)          # every parameter in exactly one group
    where = {n: (g["lr_scale"], g["weight_decay"]) for g in groups for n in g["params"]}
    assert where[ENC + "embeddings.patch_embeddings.projection.weight"] == (0.75 ** (L + 1), 0.05)
    assert where[ENC + "embeddings.cls_token"] == (0.75 ** (L + 1), 0.0) and where[ENC + "embeddings.position_embeddings"] == (0.75 ** (L + 1), 0.0)
    for k in range(1, L + 1):
        assert where[ENC + f"encoder.layer.{k - 1}.intermediate.dense.weight"] == (0.75 ** (L + 1 - k), 0.05)
        assert where[ENC + f"encoder.layer.{k - 1}.lambda_1"] == (0.75 ** (L + 1 - k), 0.0)
        assert where[ENC + f"encoder.layer.{k - 1}.layernorm_before.weight"] == (0.75 ** (L + 1 - k), 0.0)
    assert where[ENC + f"encoder.layer.{L - 1}.output.dense.bias"] == (0.75, 0.0)
    assert where["model.roi_heads.box_head.fc6.weight"] == (1.0, 0.05) and where["model.roi_heads.box_head.fc6.bias"] == (1.0, 0.0)
    assert where["model.backbone.fpn.layer_blocks.0.0.weight"] == (1.0, 0.05) and where["model.rpn.head.cls_logits.bias"] == (1.0, 0.0)
    for n, p in named.items():                                                         # the rule, over every parameter
        plain = p.dim() <= 1 or n.endswith(("cls_token", "position_embeddings"))
        assert where[n][1] == (0.0 if plain else 0.05), n
        if not n.startswith(ENC):
            assert where[n][0] == 1.0, n
    # the switches: no layer decay -> every scale 1; no_decay off -> one decay
    flat = training.detector_param_groups(model, weight_decay=0.1)
    assert {g["lr_scale"] for g in flat} == {1.0} and {g["weight_decay"] for g in flat} == {0.0, 0.1}
    one = training.detector_param_groups(model, no_decay=False, weight_decay=0.1)
    assert len(one) == 1 and sorted(one[0]["params"]) == sorted(named)
    with pytest.raises(ValueError, match="layer_decay"):
        training.detector_param_groups(model, layer_decay=1.5)
    # and they resolve to one entry per parameter
    assert dt.resolve_param_groups(model, groups) == where


def test_param_groups_refusals():
    model = LayoutDetectionModel(config=cfgs.vit_micro())
    w, b = "model.roi_heads.box_head.fc7.weight", "model.roi_heads.box_head.fc7.bias"
    named = dict(model.named_parameters())
    got = dt.resolve_param_groups(model, [{"params": [w], "lr_scale": 0.5}, {"params": [named[b]], "weight_decay": 0.0}], weight_decay=0.02)
    assert got == {w: (0.5, 0.02), b: (1.0, 0.0)}                                      # names or parameters; defaults filled in
    with pytest.raises(ValueError, match="two groups"):
        dt.resolve_param_groups(model, [{"params": [w]}, {"params": [b, w]}])
    with pytest.raises(ValueError, match="two groups"):
        dt.resolve_param_groups(model, [{"params": [w, named[w]]}])
    with pytest.raises(ValueError, match="unknown"):
        dt.resolve_param_groups(model, [{"params": ["model.roi_heads.box_head.fc8.weight"]}])
    with pytest.raises(ValueError, match="unknown"):
        dt.resolve_param_groups(model, [{"params": [torch.nn.Parameter(torch.zeros(2))]}])
    with pytest.raises(ValueError, match="negative"):
        dt.resolve_param_groups(model, [{"params": [w], "lr_scale": -1.0}])
    with pytest.raises(ValueError, match="negative"):
        dt.resolve_param_groups(model, [{"params": [w], "weight_decay": -0.1}])
    with pytest.raises(ValueError, match="params"):
        dt.resolve_param_groups(model, [{"lr_scale": 1.0}])
    # the ops front ends: form first, then the device
    f = lambda n=4: torch.zeros(n)                                                     # noqa: E731
    state, clip, part = torch.zeros(10, dtype=torch.int32), ops.new_clip_state("cpu", 2.0), torch.zeros(4, dtype=torch.float64)
    assert clip.dtype == torch.float32 and clip.tolist() == [2.0, 0.0, 0.0, 0.0]
    with pytest.raises(ValueError, match="positive"):
        ops.new_clip_state("cpu", 0.0)
    with pytest.raises(ValueError, match="float64"):
        ops.grads_check_norm_multi([f()], state, torch.zeros(4))
    with pytest.raises(ValueError, match="need 2"):
        ops.grads_check_norm_multi([f(1025)], state, part[:1])
    with pytest.raises(ValueError, match="GPU"):
        ops.grads_check_norm_multi([f()], state, part)
    with pytest.raises(ValueError, match="clip"):
        ops.clip_finish(state, torch.zeros(3), part, 1)
    with pytest.raises(ValueError, match="partials"):
        ops.clip_finish(state, clip, part, 5)
    with pytest.raises(ValueError, match="GPU"):
        ops.clip_finish(state, clip, part, 1)
    with pytest.raises(ValueError, match="entries"):
        ops.adamw_groups_multi([f()], [f()], [f()], [f()], state, [1.0, 1.0], [0.0])
    with pytest.raises(ValueError, match=">= 0"):
        ops.adamw_groups_multi([f()], [f()], [f()], [f()], state, [-1.0], [0.0])
    with pytest.raises(ValueError, match="GPU"):
        ops.adamw_groups_multi([f()], [f()], [f()], [f()], state, [1.0], [0.0], clip)
    assert ops.grad_norm_partials([f(0), f(1), f(1024), f(1025)]) == 4


def test_warmup_is_a_line_from_the_factor_to_one():
    lr = 2e-4
    got = [dt.warmup_lr(lr, it, 4, 0.001) for it in range(7)]
    want = [lr * (0.001 + 0.999 * it / 4) for it in range(4)] + [lr] * 3
    assert got == want and got[0] == lr * 0.001 and got[4] == lr
    assert dt.warmup_lr(lr, 0, 0, 0.001) == lr                                         # no warmup: the rate itself, from the first call
    assert all(a < b for a, b in zip(got[:4], got[1:5]))
    import inspect
    sig = inspect.signature(training.DetectorTrainStep.__init__).parameters
    assert (sig["max_grad_norm"].default, sig["param_groups"].default, sig["warmup_iters"].default, sig["warmup_factor"].default) == (None, None, 0, 1e-3)
    doc = dt.__doc__ + training.DetectorTrainStep.__doc__
    assert "no gradient clipping" not in doc and "One parameter group" not in doc
