"""Gradient accumulation under DetectorTrainStep on the GPU: the fold kernel of csrc/optim_multi.hip bit for bit
against torch on the same device, and the step built on it against a twin that updates from ``g1 + g2`` by hand.

Every comparison is exact.  Overwrite mode is a copy of bits; add mode is ONE fp32 addition per element, which torch's ``acc + g``
performs too; the multiplier ``1024 * 0.5`` is a power of two, so ``g1`` and ``g2`` made with it on an identically built model are the
gradients the step folds; and the update runs the same kernels on the same inputs as the twin's."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from layoutdit_amd import ops                                                     # noqa: E402
from layoutdit_amd.detector_training import BUCKET_ALIGN, bucket_layout, detector_param_groups, warmup_lr     # noqa: E402
from layoutdit_amd.training import DetectorTrainStep                              # noqa: E402
from tests import detector_accum_cases as cases                                   # noqa: E402

DEV = cases.DEV
SCALE = cases.SCALE
PAD, SENTINEL = 8, 12345.0
SPECIALS = (0x80000000 - (1 << 32), 0x7f800000, 0x7fc12345, 0xff800000 - (1 << 32), 0x7f812345, 0xffc00001 - (1 << 32))   # -0.0, +inf, NaNs with payloads, -inf


# ---- the kernel ------------------------------------------------------------------------------------------------------------------------
class Problem:
    """(acc, g) pairs of lengths 0, 1, 3, 4, 5, 1023, 1024, 1025, one of 1030 whose acc starts one element off the 16-byte grid, one
    of 1030 whose g alone does, tiny ones up to ops.ACC_MAX_SEGMENTS + 1 non-empty segments (a second launch), and 4099 last.  Every
    tensor sits PAD sentinels inside its own parent, as Problem of tests/test_gpu_detector_step.py does."""

    def __init__(self, seed=0):
        rng = np.random.RandomState(seed)
        spec = [(0, 0, 0), (1, 0, 0), (3, 0, 0), (4, 0, 0), (5, 0, 0), (1023, 0, 0), (1024, 0, 0), (1025, 0, 0), (1030, 1, 0), (1030, 0, 1)]
        tiny = [1, 2, 3, 5, 7]
        while sum(1 for n, _, _ in spec if n) < ops.ACC_MAX_SEGMENTS:
            spec.append((tiny[len(spec) % 5], 0, 0))
        spec.append((4099, 0, 0))
        assert sum(1 for n, _, _ in spec if n) == ops.ACC_MAX_SEGMENTS + 1
        self.spec, self.parents, self.acc, self.g = spec, [], [], []
        for n, acc_shift, g_shift in spec:
            def view(shift):
                parent = torch.full((n + 2 * PAD + 1,), SENTINEL, dtype=torch.float32, device=DEV)
                self.parents.append((parent, PAD + shift, n))
                return parent[PAD + shift: PAD + shift + n]
            acc, g = view(acc_shift), view(g_shift)
            g.copy_(torch.from_numpy(rng.normal(0, 1, size=n).astype(np.float32)))
            acc.copy_(torch.from_numpy(rng.normal(0, 1, size=n).astype(np.float32)))
            self.acc.append(acc), self.g.append(g)
        assert self.acc[8].data_ptr() % 16 == 4 and self.g[8].data_ptr() % 16 == 0
        assert self.acc[9].data_ptr() % 16 == 0 and self.g[9].data_ptr() % 16 == 4
        assert self.acc[7].data_ptr() % 16 == 0 and self.g[7].data_ptr() % 16 == 0

    def plant_specials(self, tensors):
        """-0.0, infinities and NaNs with payloads as bits: at the head, in the last quad and in the scalar tail of every segment."""
        for t in tensors:
            bits, n = t.view(torch.int32), t.numel()
            for k, where in enumerate((0, 1, n // 2, n - 2, n - 1, n - 3)):
                if 0 <= where < n:
                    bits[where] = SPECIALS[(k + n) % len(SPECIALS)]

    def sentinels_intact(self):
        return all(bool((torch.cat([parent[:off], parent[off + n:]]) == SENTINEL).all()) for parent, off, n in self.parents)


def _bits(ts):
    return [t.clone().view(torch.int32) for t in ts]


def test_overwrite_copies_the_bits():
    prob = Problem()
    prob.plant_specials(prob.g)
    for acc in prob.acc:
        acc.view(torch.int32).fill_(-1)                                                # 0xFF bytes: a NaN that must never be read
    before = _bits(prob.g)
    assert any(int((b == SPECIALS[0]).sum()) for b in before) and any(int((b == SPECIALS[2]).sum()) for b in before)
    ops.grads_accumulate_multi(prob.acc, prob.g, True)
    torch.cuda.synchronize()
    for i, (acc, want) in enumerate(zip(prob.acc, before)):
        assert torch.equal(acc.view(torch.int32), want), f"segment {i} of {prob.spec[i]}"
    assert all(torch.equal(a, b) for a, b in zip(before, _bits(prob.g)))               # g unchanged
    assert prob.sentinels_intact()


def test_add_is_one_fp32_addition_per_element():
    prob = Problem(seed=1)
    prob.plant_specials(prob.g[::2])
    prob.plant_specials(prob.acc[1::3])
    before = _bits(prob.g)
    for fold in range(2):                                                              # the second on what the first left
        want = [acc + g for acc, g in zip(prob.acc, prob.g)]                           # torch on the same device: one addition each
        ops.grads_accumulate_multi(prob.acc, prob.g, False)
        torch.cuda.synchronize()
        for i, (acc, w) in enumerate(zip(prob.acc, want)):
            nan = torch.isnan(w)
            assert torch.equal(torch.isnan(acc), nan), f"fold {fold}, segment {i}: NaNs elsewhere than torch's"
            assert torch.equal(acc.view(torch.int32)[~nan], w.view(torch.int32)[~nan]), f"fold {fold}, segment {i} of {prob.spec[i]}"
    assert any(bool(torch.isnan(a).any()) for a in prob.acc) and any(bool(torch.isinf(a).any()) for a in prob.acc)
    assert all(torch.equal(a, b) for a, b in zip(before, _bits(prob.g)))
    assert prob.sentinels_intact()


def test_equal_inputs_give_equal_bits_and_empty_lists_launch_nothing():
    a, b = Problem(seed=2), Problem(seed=2)
    for prob in (a, b):
        ops.grads_accumulate_multi(prob.acc, prob.g, False)
    torch.cuda.synchronize()
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a.acc, b.acc))
    ops.grads_accumulate_multi([], [], True)
    empty = torch.empty(0, device=DEV)
    ops.grads_accumulate_multi([empty], [empty], False)


# ---- the step ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batches():
    return cases.micro_batches()


@pytest.fixture(scope="module")
def grads(batches):
    """(g1, g2): name -> gradient at SCALE * 0.5 of each micro-batch, on an identically built model.  Computed once, never modified."""
    return cases.reference_grads(batches)


def _state(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def _two_steps(step, batches):
    return [step.step(*batches[k], generator=cases.seeded(cases.GEN_SEEDS[k])) for k in range(2)]


def test_bucket_holds_the_sum_of_the_micro_batch_gradients(batches, grads):
    g1, g2 = grads
    m = cases.model()
    initial = _state(m)
    step = DetectorTrainStep(m, accumulate=2, init_scale=SCALE)
    assert step.bucket is None and step.pending_micro_batches == 0
    for k in range(2):
        cases.grads_of(m, batches[k], cases.GEN_SEEDS[k], SCALE * 0.5)
        step.accumulate_grads()
        assert step.pending_micro_batches == k + 1
        if k == 0:
            first = step.accumulated_grads()
            assert set(first) == set(g1) and all(torch.equal(first[n], g1[n]) for n in g1)       # the first fold overwrites
    with pytest.raises(RuntimeError, match="micro-batches"):
        step.state_dict()
    got = step.accumulated_grads()
    assert set(got) == set(g1) == set(g2) and len(got) > 60
    for n in g1:
        assert torch.equal(got[n], g1[n] + g2[n]), n
    # the layout: one 256-byte aligned slice per segment, the whole encoder one slice of its own length, at bucket_layout's offsets
    lengths = [s.numel() for s in step._bucket_slices]
    offsets, total = bucket_layout(lengths)
    assert step.bucket.numel() == total and step.bucket.dtype == torch.float32
    assert all(s.data_ptr() == step.bucket.data_ptr() + 4 * o and s.data_ptr() % (4 * BUCKET_ALIGN) == 0 for s, o in zip(step._bucket_slices, offsets))
    assert m.model.backbone.backbone.dit._flat_state.numel in lengths
    assert all(torch.equal(v, initial[k]) for k, v in m.state_dict().items())                      # nothing moved yet
    # a micro-batch whose segments differ is refused by name; the bucket and the count stay
    name = [n for n, p in m.named_parameters() if p.grad is not None][-1]
    dict(m.named_parameters())[name].grad = None
    with pytest.raises(RuntimeError, match=re.escape(name)):
        step.accumulate_grads()
    assert step.pending_micro_batches == 2


def test_no_bucket_with_the_defaults(batches):
    from layoutdit_amd import dp
    m = cases.model()
    for kw in ({}, {"accumulate": 1, "rank": dp.Rank(rank=0, world=1, local_rank=0, backend="gloo")}):
        step = DetectorTrainStep(m, init_scale=SCALE, **kw)
        step.step(*batches[0], generator=cases.seeded(2))
        assert step.bucket is None and step.pending_micro_batches == 0 and step.steps == 1 and step.iters == 1
        with pytest.raises(RuntimeError, match="bucket"):
            step.accumulate_grads()
    fresh = DetectorTrainStep(cases.model(), accumulate=2)
    with pytest.raises(RuntimeError, match="nothing was folded"):
        fresh.apply()


@pytest.mark.parametrize("options", ["plain", "clip_and_groups"])
def test_update_equals_a_twin_updated_from_the_summed_gradient(batches, grads, options):
    m = cases.model()
    kw = {"lr": 1e-3, "weight_decay": 0.01}
    if options == "clip_and_groups":
        kw.update(max_grad_norm=0.05, weight_decay=0.05, param_groups=detector_param_groups(m, layer_decay=0.8, weight_decay=0.05))
    twin, twin_step = cases.twin_update(batches, *grads, **kw)
    initial = _state(m)
    step = DetectorTrainStep(m, accumulate=2, init_scale=SCALE, **kw)
    losses = _two_steps(step, batches)
    torch.cuda.synchronize()
    assert all(sorted(l) == ["loss_box_reg", "loss_classifier", "loss_objectness", "loss_rpn_box_reg"] for l in losses)
    assert all(np.isfinite(v.item()) and not v.requires_grad for l in losses for v in l.values())
    assert (step.steps, step.skipped_steps, step.iters, step.pending_micro_batches, step.scale) == (1, 0, 1, 0, SCALE)
    assert (twin_step.steps, twin_step.skipped_steps) == (1, 0)
    sa, sb = m.state_dict(), twin.state_dict()
    moved = 0
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
        moved += int(not torch.equal(sa[k], initial[k]))
    assert moved > 60
    if options == "clip_and_groups":
        print("grad norm", float(step.grad_norm), "clipped steps", step.clipped_steps)
        assert torch.equal(step.grad_norm, twin_step.grad_norm) and step.clipped_steps == twin_step.clipped_steps == 1
    ma, mb = step.state_dict(), twin_step.state_dict()
    assert ma["state"] == mb["state"] and set(ma["exp_avg"]) == set(mb["exp_avg"])
    assert all(torch.equal(ma["exp_avg"][k], mb["exp_avg"][k]) and torch.equal(ma["exp_avg_sq"][k], mb["exp_avg_sq"][k]) for k in ma["exp_avg"])


def test_a_non_finite_micro_batch_skips_the_whole_update(batches):
    m = cases.model()
    initial = _state(m)
    step = DetectorTrainStep(m, lr=1e-3, accumulate=2, init_scale=SCALE)
    step.step(*cases.poisoned(batches[0]), generator=cases.seeded(cases.GEN_SEEDS[0]))
    assert step.pending_micro_batches == 1
    step.step(*batches[1], generator=cases.seeded(cases.GEN_SEEDS[1]))                  # clean, and added to a non-finite bucket
    torch.cuda.synchronize()
    assert (step.steps, step.skipped_steps, step.scale, step.iters, step.pending_micro_batches) == (0, 1, SCALE / 2, 1, 0)
    assert all(torch.equal(v, initial[k]) for k, v in m.state_dict().items())
    _two_steps(step, batches)                                                           # the first of them overwrites the bucket
    torch.cuda.synchronize()
    assert (step.steps, step.skipped_steps, step.scale, step.iters) == (1, 1, SCALE / 2, 2)
    assert sum(int(not torch.equal(v, initial[k])) for k, v in m.state_dict().items()) > 60


def test_warmup_counts_updates_not_micro_batches(batches):
    m = cases.model()
    lr, wi, wf = 1e-3, 3, 0.1
    step = DetectorTrainStep(m, lr=lr, accumulate=2, init_scale=SCALE, warmup_iters=wi, warmup_factor=wf)
    seen = []
    for call in range(4):
        step.step(*batches[call % 2], generator=cases.seeded(cases.GEN_SEEDS[call % 2]))
        seen.append(step._read_state()["lr"])
    want = [float(np.float32(warmup_lr(lr, k, wi, wf))) for k in (0, 0, 1, 1)]
    assert seen == want and want[0] < want[2] < lr
    assert (step.iters, step.steps + step.skipped_steps) == (2, 2)
