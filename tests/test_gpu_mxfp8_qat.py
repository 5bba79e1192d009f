"""Quantisation-aware training of the mxfp8 build on the GPU: the train variants of the forward's kernels against the inference
kernels, train/eval identity of the whole forward, and the fused AdamW + re-quantisation against a fresh pack."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from layoutdit_amd import _lib, config as cfgs, ops, synth          # noqa: E402
from tests.test_mxfp8_format import mx_dequant, mx_quant_ref          # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _micro():
    return dataclasses.replace(cfgs.vit_micro(), drop_path_rate=0.0)


def _enc(cfg, w, qat=True):
    from layoutdit_amd.modeling import DiTEncoder
    return DiTEncoder(cfg, compute_dtype="mxfp8", qat=qat).load_numpy(w).to(DEV)


@pytest.mark.parametrize("rows,C", [(197, 768), (33, 128)])
def test_layernorm_train_variant_is_the_inference_operand_plus_its_dequantised_copy(rows, C):
    g = torch.Generator().manual_seed(rows)
    x = (torch.randn(rows, C, generator=g) * 3).to(DEV)
    gam = (1 + 0.1 * torch.randn(C, generator=g)).to(DEV)
    bet = (0.1 * torch.randn(C, generator=g)).to(DEV)
    c0, s0 = ops.layernorm_mxfp8(x, gam, bet)
    c1, s1, d = ops.layernorm_mxfp8_train(x, gam, bet)
    assert torch.equal(c0.view(torch.uint8), c1.view(torch.uint8)) and torch.equal(s0, s1)
    ref = mx_dequant(c1.view(torch.uint8).cpu().numpy(), s1.cpu().numpy())
    assert np.array_equal(d.float().cpu().numpy().astype(np.float64), ref)


def test_train_forward_is_bit_identical_to_eval_forward():
    cfg = _micro()
    w = synth.synth_weights(cfg, 7)
    x = torch.from_numpy(synth.synth_images(3, 64, 64, seed=5)).to(DEV)
    m = _enc(cfg, w).train()
    tr = [t.detach().clone() for t in m(x, taps=[1, 2, 3]).hidden_states if t is not None]
    m.eval()
    with torch.no_grad():
        ev = [t for t in m(x, taps=[1, 2, 3]).hidden_states if t is not None]
    for a, b in zip(tr, ev):
        assert torch.equal(a, b)


def test_default_mxfp8_encoder_still_refuses_training():
    cfg = _micro()
    m = _enc(cfg, synth.synth_weights(cfg, 1), qat=False).train()
    with pytest.raises(NotImplementedError, match="inference only.*qat=True"):
        m(torch.zeros(1, 3, 64, 64, device=DEV))


def _pack_train(st):
    fresh = st.packed.clone()          # (slots the mirror does not use keep their bytes: only what a pack writes is compared)
    _lib.check(_lib.load().ldit_pack_train(C.byref(st.lcfg), st.params.data_ptr(), fresh.data_ptr(), fresh.numel(),
                                           torch.cuda.current_stream().cuda_stream))
    return fresh


@pytest.mark.parametrize("layers", [1, 3])
def test_pack_train_leaves_nothing_the_forward_reads_to_the_mirrors_old_bytes(layers):
    """ldit_pack_train (mxfp8) = the convert pass over the whole flat block + ONE launch that re-makes the matrices and the fused
    bias of every layer (one layer: the zero-stride branch of the host side).  Everything the training forward reads must come from
    those two: the pack into a mirror of 0x00 bytes and into one of 0xFF bytes gives bit-equal taps, and they are the eval
    forward's (which reads ldit_pack_weights' block: codes, scales and folded bias made by another kernel)."""
    from layoutdit_amd.training import flat_state
    cfg = dataclasses.replace(cfgs.vit_micro(), drop_path_rate=0.0, num_hidden_layers=layers, taps=[])
    taps = list(range(layers + 1))
    m = _enc(cfg, synth.synth_weights(cfg, 7))
    x = torch.from_numpy(synth.synth_images(2, 64, 64, seed=5)).to(DEV)
    st = flat_state(m, 64, 64)
    st.repack(force=True)
    outs = []
    with torch.no_grad():
        for fill in (0x00, 0xFF):
            st.packed.fill_(fill)
            st.repack(force=True)
            outs.append([t.clone() for t in st.forward(x, taps, None, st.new_saved(2))])
        m.eval()
        ev = [t for t in m(x, taps=taps).hidden_states if t is not None]
    assert len(outs[0]) == len(outs[1]) == len(ev) == layers + 1
    for t, a, b, e in zip(taps, outs[0], outs[1], ev):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), t
        assert torch.equal(a.view(torch.int32), e.view(torch.int32)), t


def _trainstep_run(cfg, w, x, steps=3):
    from layoutdit_amd.training import TrainStep
    m = _enc(cfg, w)
    ts = TrainStep(m, lr=1e-3, drop_path_rate=0.0)
    for _ in range(steps):
        ts.step(x)
    torch.cuda.synchronize()
    return m, ts


def test_trainstep_mirror_is_a_fresh_pack_and_runs_are_reproducible():
    cfg = _micro()
    w = synth.synth_weights(cfg, 3)
    x = torch.from_numpy(synth.synth_images(2, 64, 64, seed=9)).to(DEV)
    from layoutdit_amd.training import flat_state
    p0 = flat_state(_enc(cfg, w), 64, 64).params.clone()
    m, ts = _trainstep_run(cfg, w, x)
    assert torch.isfinite(ts.state.params).all()
    moved = (ts.state.params != p0).float().mean().item()
    assert moved > 0.5, moved                                   # the update reached (almost) every parameter
    assert torch.equal(ts.state.packed, _pack_train(ts.state))
    _, ts2 = _trainstep_run(cfg, w, x)
    assert torch.equal(ts.state.params, ts2.state.params)
    # eval after training = a fresh mxfp8 model loaded with the updated weights; and the TRAINING forward (which reads the mirror
    # the fused update wrote) = that fresh model's inference forward
    from layoutdit_amd.modeling import DiTEncoder
    tr = ts.state.forward(x, [cfg.num_hidden_layers], None, ts.state.new_saved(x.shape[0]))[0]
    fresh = DiTEncoder(cfg, compute_dtype="mxfp8").to(DEV)
    fresh.load_state_dict(m.state_dict())
    m.eval()
    fresh.eval()
    with torch.no_grad():
        a, b = m(x).last_hidden_state, fresh(x).last_hidden_state
    assert torch.equal(a, b)
    assert torch.equal(tr, b)


def test_autograd_loop_reduces_a_regression_loss():
    cfg = _micro()
    m = _enc(cfg, synth.synth_weights(cfg, 11)).train()
    x = torch.from_numpy(synth.synth_images(2, 64, 64, seed=3)).to(DEV)
    target = torch.randn(2, cfg.tokens(64, 64), cfg.hidden_size, device=DEV, generator=torch.Generator(DEV).manual_seed(0))
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=0.0)
    losses = []
    for _ in range(20):
        opt.zero_grad()
        loss = torch.nn.functional.mse_loss(m(x).last_hidden_state, target)
        loss.backward()
        opt.step()
        m.mark_parameters_changed()
        losses.append(float(loss))
    assert np.isfinite(losses).all()
    assert losses[-1] < 0.9 * losses[0], losses


# ---- unit tests of the train variants: the tile kernels (M > 64) and the peeled tail (M <= 64) ----------------------------------
def _mx_pair(t):
    c, s = ops.quant_mxfp8(t)
    return c, s


def _deq(pair):
    c, s = pair
    return mx_dequant(c.view(torch.uint8).cpu().numpy(), s.cpu().numpy())


def _gelu_grad_ref(v):
    a = 2.0 * np.sqrt(2.0 / np.pi)
    b = 0.044715 * a
    sg = 1.0 / (1.0 + np.exp(-(a * v + b * v ** 3)))
    return sg + v * sg * (1 - sg) * (a + 3 * b * v * v)


@pytest.mark.parametrize("M,N,K", [(40, 256, 256), (600, 768, 256), (12608 // 16, 768, 768), (12608, 768, 256)])
def test_linear_mxfp8_train_epilogues(M, N, K):
    g = torch.Generator().manual_seed(M + N)
    x = _mx_pair(torch.randn(M, K, generator=g).to(DEV))
    w = _mx_pair((torch.randn(N, K, generator=g) / K ** 0.5).to(DEV))
    bias = (0.1 * torch.randn(N, generator=g)).to(DEV)
    lam = (0.5 + torch.rand(N, generator=g)).to(DEV)
    R = torch.randn(M, N, generator=g).to(DEV)
    rs = (torch.rand(M, generator=g) < 0.7).float().to(DEV) / 0.7
    acc = _deq(x) @ _deq(w).T + bias.cpu().numpy().astype(np.float64)
    # scale + residual: Y bit-equal to the inference epilogue (no rowscale), Ypre = the branch output before LayerScale
    y0 = ops.linear_mxfp8(x, w, bias, _lib.EPI_SCALE_RESID, lam=lam, residual=R)
    y1, pre = ops.linear_mxfp8_train(x, w, bias, _lib.EPI_SCALE_RESID, lam=lam, residual=R)
    assert torch.equal(y0, y1)
    assert np.abs(pre.float().cpu().numpy() - acc).max() <= 1e-2 * max(1.0, np.abs(acc).max())
    # with per-row factors: Y = R + rs lam (.) pre
    y2, _ = ops.linear_mxfp8_train(x, w, bias, _lib.EPI_SCALE_RESID, lam=lam, residual=R, rowscale=rs)
    ref = R.cpu().numpy() + rs.cpu().numpy()[:, None] * lam.cpu().numpy()[None] * acc
    assert np.abs(y2.cpu().numpy() - ref).max() < 1e-3 * max(1.0, np.abs(ref).max())
    # bias + GELU: the MX output bit-equal to the inference epilogue, Yd its exact dequantisation, gelu' of the accumulator
    (c0, s0) = ops.linear_mxfp8(x, w, bias, _lib.EPI_BIAS_GELU)
    (c1, s1), gp, yd = ops.linear_mxfp8_train(x, w, bias, _lib.EPI_BIAS_GELU)
    assert torch.equal(c0.view(torch.uint8), c1.view(torch.uint8)) and torch.equal(s0, s1)
    assert np.array_equal(yd.float().cpu().numpy().astype(np.float64), _deq((c1, s1)))
    assert np.abs(gp.float().cpu().numpy() - _gelu_grad_ref(acc)).max() < 2e-2


@pytest.mark.parametrize("M,N,K", [(700, 768, 256), (600, 544, 384)])
def test_linear_mxfp8_train_is_the_same_on_every_tile(M, N, K):
    """The train GEMM on each forced tile (LDIT_GEMM_FP8_TILE = 0..4: 256 x 256, 256 x 128, 128 x 128, 192 x 256, 320 x 256; M ragged
    for all of them, N = 544 also ragged in the columns): every tile walks K in the same order with the same instruction, so Y and the
    side outputs (gelu', the dequantised output, Ypre) are bit-equal across tiles, and Y is bit-equal to the inference epilogue's."""
    g = torch.Generator().manual_seed(M + N)
    x = _mx_pair(torch.randn(M, K, generator=g).to(DEV))
    w = _mx_pair((torch.randn(N, K, generator=g) / K ** 0.5).to(DEV))
    bias = (0.1 * torch.randn(N, generator=g)).to(DEV)
    lam = (0.5 + torch.rand(N, generator=g)).to(DEV)
    R = torch.randn(M, N, generator=g).to(DEV)
    rs = (torch.rand(M, generator=g) < 0.7).float().to(DEV) / 0.7
    acc = _deq(x) @ _deq(w).T + bias.cpu().numpy().astype(np.float64)
    c0, s0 = ops.linear_mxfp8(x, w, bias, _lib.EPI_BIAS_GELU)
    y0 = ops.linear_mxfp8(x, w, bias, _lib.EPI_SCALE_RESID, lam=lam, residual=R)
    first = None
    try:
        for tile in ("0", "1", "2", "3", "4"):
            _lib.set_switch("LDIT_GEMM_FP8_TILE", tile)
            (c1, s1), gp, yd = ops.linear_mxfp8_train(x, w, bias, _lib.EPI_BIAS_GELU)
            y1, pre = ops.linear_mxfp8_train(x, w, bias, _lib.EPI_SCALE_RESID, lam=lam, residual=R)      # (tile 4: runs as 256 x 256)
            y2, pre2 = ops.linear_mxfp8_train(x, w, bias, _lib.EPI_SCALE_RESID, lam=lam, residual=R, rowscale=rs)
            assert torch.equal(c0.view(torch.uint8), c1.view(torch.uint8)) and torch.equal(s0, s1), tile
            assert torch.equal(y0, y1) and torch.equal(pre, pre2), tile
            assert np.array_equal(yd.float().cpu().numpy().astype(np.float64), _deq((c1, s1))), tile
            got = [t.clone() for t in (gp, yd, pre, y2)]
            if first is None:
                first = got
                assert np.abs(gp.float().cpu().numpy() - _gelu_grad_ref(acc)).max() < 2e-2
                assert np.abs(pre.float().cpu().numpy() - acc).max() <= 1e-2 * max(1.0, np.abs(acc).max())
            for name, t0, t1 in zip(("gelu'", "Yd", "Ypre", "Y with rowscale"), first, got):
                bits = torch.int16 if t0.dtype == torch.bfloat16 else torch.int32
                assert torch.equal(t0.view(bits), t1.view(bits)), (tile, name)
    finally:
        _lib.set_switch("LDIT_GEMM_FP8_TILE", None)


@pytest.mark.parametrize("B,N,H", [(2, 197, 2), (1, 290, 12), (3, 17, 2)])
def test_attention_mxfp8_train_outputs(B, N, H):
    C = 64 * H
    g = torch.Generator().manual_seed(N)
    qkv = torch.randn(B, N, 3 * C, generator=g)
    qkv[..., :C] *= (64 ** -0.5) * 1.4426950408889634         # q folded, as the mxfp8 build packs W_q / b_q
    qkv = qkv.to(torch.bfloat16).to(DEV).contiguous()
    (codes, scales), lse, ob, od = ops.attention_mxfp8_train(qkv, H)
    assert np.array_equal(od.float().cpu().numpy().astype(np.float64), _deq((codes, scales)))
    # lse and O of the bf16 train-step kernel in the same (folded) convention: scale ln 2 gives c = scale log2 e = 1
    lib = _lib.load()
    o_ref = torch.empty(B * N, C, dtype=torch.bfloat16, device=DEV)
    lse_ref = torch.empty(B, H, N, device=DEV)
    base = qkv.data_ptr()
    _lib.check(lib.ldit_attention_fwd_lse_bf16(base, base + 2 * C, base + 4 * C, o_ref.data_ptr(), lse_ref.data_ptr(), B, N, H, 64,
                                               3 * C, 3 * C, 3 * C, C, float(np.float32(np.log(2.0))),
                                               torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert (lse - lse_ref).abs().max().item() < 1e-3
    assert (ob.float() - o_ref.float()).abs().max().item() < 2e-2
    # the codes quantise the pre-quantisation O (up to the bf16 rounding Ob went through)
    assert np.abs(_deq((codes, scales)) - ob.float().cpu().numpy()).max() <= 0.07 * np.abs(ob.float().cpu().numpy()).max()


def test_adamw_mxfp8_is_adamw_plus_a_fresh_mx_pack():
    from layoutdit_amd.modeling import DiTEncoder
    from layoutdit_amd.training import flat_state
    cfg = _micro()
    w = synth.synth_weights(cfg, 21)
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    m = _enc(cfg, w)
    st = flat_state(m, 64, 64)
    st.repack(force=True)
    n = st.numel
    g = torch.randn(n, device=DEV, generator=torch.Generator(DEV).manual_seed(1)) * 1e-2
    a, ma, va = st.params.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    _lib.check(lib.ldit_adamw_step(a.data_ptr(), g.data_ptr(), ma.data_ptr(), va.data_ptr(), n, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, 1.0,
                                   None, stream))
    # ldit_pack_weights(LDIT_MXFP8) of the updated master, through a second encoder whose flat block is overwritten with it
    m2 = _enc(cfg, w)
    st2 = flat_state(m2, 64, 64)
    with torch.no_grad():
        st2.params.copy_(a)
    fresh = DiTEncoder(cfg, compute_dtype="mxfp8").to(DEV)
    fresh.load_state_dict(m2.state_dict())
    lcfg = fresh._lcfg(64, 64, [cfg.num_hidden_layers])
    packed = fresh._pack(lcfg, fresh._position_table(4, 4), torch.device(DEV))
    flat_bytes = lib.ldit_flat_param_bytes(C.byref(st.lcfg))
    off = (flat_bytes // 2 + 255) // 256 * 256
    assert st.packed.numel() == off + packed.numel()
    with torch.no_grad():
        st.packed[off:].copy_(packed)                          # slots the update does not write keep the pack's bytes
    mb, vb = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    _lib.check(lib.ldit_adamw_step_mxfp8(C.byref(st.lcfg), st.params.data_ptr(), g.data_ptr(), mb.data_ptr(), vb.data_ptr(), 1e-3, 0.9,
                                         0.999, 1e-8, 0.01, 1, 1.0, st.packed.data_ptr(), st.packed.numel(), stream))
    torch.cuda.synchronize()
    assert torch.equal(st.params, a) and torch.equal(mb, ma) and torch.equal(vb, va)
    assert torch.equal(st.packed[off:], packed)                # codes, scales and folded bias = ldit_pack_weights(LDIT_MXFP8)
    # bf16 part: the dequantised codes of mx_quant_ref(master x fold) on the q third, of the master elsewhere
    Cc = cfg.hidden_size
    o = st.offsets[4 + 2]                                      # layer 0 wqkv
    wqkv = a[o: o + 3 * Cc * Cc].view(3 * Cc, Cc).cpu().numpy().copy()
    wqkv[:Cc] *= np.float32((64 ** -0.5) * 1.4426950408889634)
    codes, scales, _ = mx_quant_ref(wqkv)
    ref = mx_dequant(codes, scales)
    got = st.packed[:flat_bytes // 2].view(torch.bfloat16)[o: o + 3 * Cc * Cc].view(3 * Cc, Cc).float().cpu().numpy()
    assert np.array_equal(got.astype(np.float64), ref)
    v0 = st.offsets[4]                                         # layer 0 ln1_w: a vector, bf16 of the master
    assert torch.equal(st.packed[:flat_bytes // 2].view(torch.bfloat16)[v0: v0 + Cc], a[v0: v0 + Cc].to(torch.bfloat16))


def test_vit_base_bs64_train_forward_is_bit_identical_to_eval_forward():
    cfg = dataclasses.replace(cfgs.vit_base(), drop_path_rate=0.0)
    w = synth.synth_weights(cfg, 2)
    x = torch.from_numpy(synth.synth_images(64, 224, 224, seed=8)).to(DEV)
    m = _enc(cfg, w).train()
    tr = [t.detach().clone() for t in m(x).hidden_states if t is not None]
    m.eval()
    with torch.no_grad():
        ev = [t for t in m(x).hidden_states if t is not None]
    assert len(tr) == len(ev) == 4
    for a, b in zip(tr, ev):
        assert torch.equal(a, b)


def test_reference_style_fpn_loop_then_eval_equals_a_fresh_model():
    from layoutdit_amd.modeling import DiTEncoder, DiTWithFPN
    cfg = _micro()
    model = DiTWithFPN(config=cfg, compute_dtype="mxfp8", qat=True)
    model.backbone.dit.load_numpy(synth.synth_weights(cfg, 4))
    model = model.to(DEV).train()
    x = torch.from_numpy(synth.synth_images(4, 64, 64, seed=2)).to(DEV)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    for _ in range(2):
        opt.zero_grad()
        loss = sum(f.float().pow(2).mean() for f in model(x).values())
        loss.backward()
        opt.step()
        model.backbone.dit.mark_parameters_changed()
    dit = model.backbone.dit.eval()
    fresh = DiTEncoder(cfg, compute_dtype="mxfp8").to(DEV).eval()
    fresh.load_state_dict(dit.state_dict())
    with torch.no_grad():
        a, b = dit(x).last_hidden_state, fresh(x).last_hidden_state
    assert torch.equal(a, b)


# ---- the straight-through oracle: train_reference's equations in float64 with Q at the four activation points and on the
# folded weights, identity backward through every Q ---------------------------------------------------------------------------
def _q(t):
    """MX quantise-dequantise along the last axis, straight-through (the value of Q, the gradient of the identity)"""
    K = t.shape[-1]
    v = t.detach().reshape(-1, K).numpy().astype(np.float32)
    codes, scales, _ = mx_quant_ref(v)
    qv = torch.from_numpy(mx_dequant(codes, scales)).reshape(t.shape).to(t.dtype)
    return t + (qv - t).detach()


def _gelu_lp64(v):
    a = 2.0 * np.sqrt(2.0 / np.pi)
    return v * torch.sigmoid(a * v + 0.044715 * a * v ** 3)


def ste_reference(cfg, weights, x, dtaps, taps, drop_scales=None):
    import torch.nn.functional as F
    dt = torch.float64
    w = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dt).requires_grad_(True) for k, v in weights.items()
         if "mask_token" not in k and not k.startswith("pooler.")}
    xt = torch.from_numpy(np.ascontiguousarray(x)).to(dt)
    B, Cc, H = xt.shape[0], cfg.hidden_size, cfg.num_attention_heads
    D = Cc // H
    fold = (D ** -0.5) * 1.4426950408889634
    s = None if drop_scales is None else torch.from_numpy(np.ascontiguousarray(drop_scales)).to(dt)
    e = F.conv2d(xt, w["embeddings.patch_embeddings.projection.weight"], w["embeddings.patch_embeddings.projection.bias"],
                 stride=cfg.patch_size).flatten(2).transpose(1, 2)
    pe = w["embeddings.position_embeddings"]
    gh, gw = xt.shape[2] // cfg.patch_size, xt.shape[3] // cfg.patch_size
    g0 = int(round((pe.shape[1] - 1) ** 0.5))
    if (gh, gw) != (g0, g0):
        patch = pe[:, 1:].reshape(1, g0, g0, Cc).permute(0, 3, 1, 2)
        patch = F.interpolate(patch, size=(gh, gw), mode="bicubic", align_corners=False)
        pe = torch.cat((pe[:, :1], patch.permute(0, 2, 3, 1).reshape(1, gh * gw, Cc)), dim=1)
    h = torch.cat((w["embeddings.cls_token"].expand(B, -1, -1), e), dim=1) + pe
    out = {0: h} if 0 in taps else {}
    for l in range(cfg.num_hidden_layers):
        p = f"encoder.layer.{l}."
        y = _q(F.layer_norm(h, (Cc,), w[p + "layernorm_before.weight"], w[p + "layernorm_before.bias"], cfg.layer_norm_eps))
        q = F.linear(y, _q(fold * w[p + "attention.attention.query.weight"]), fold * w[p + "attention.attention.query.bias"])
        k = F.linear(y, _q(w[p + "attention.attention.key.weight"]))
        v = F.linear(y, _q(w[p + "attention.attention.value.weight"]), w[p + "attention.attention.value.bias"])
        q, k, v = (t.view(B, -1, H, D).transpose(1, 2) for t in (q, k, v))
        a = torch.softmax((q @ k.transpose(-1, -2)) * np.log(2.0), dim=-1) @ v        # q folded: exp2-domain scores
        a = _q(a.transpose(1, 2).reshape(B, -1, Cc))
        a = w[p + "lambda_1"] * F.linear(a, _q(w[p + "attention.output.dense.weight"]), w[p + "attention.output.dense.bias"])
        h = (a if s is None else a * s[l, 0].view(B, 1, 1)) + h
        y = _q(F.layer_norm(h, (Cc,), w[p + "layernorm_after.weight"], w[p + "layernorm_after.bias"], cfg.layer_norm_eps))
        m = _q(_gelu_lp64(F.linear(y, _q(w[p + "intermediate.dense.weight"]), w[p + "intermediate.dense.bias"])))
        m = w[p + "lambda_2"] * F.linear(m, _q(w[p + "output.dense.weight"]), w[p + "output.dense.bias"])
        h = (m if s is None else m * s[l, 1].view(B, 1, 1)) + h
        if (l + 1) in taps:
            out[l + 1] = h
    loss = sum((out[t] * torch.from_numpy(np.ascontiguousarray(d)).to(dt)).sum() for t, d in zip(taps, dtaps))
    names = list(w)
    grads = torch.autograd.grad(loss, [w[n] for n in names], allow_unused=True)
    return ([out[t].detach().numpy() for t in taps],
            {n: (torch.zeros_like(w[n]) if gr is None else gr).numpy() for n, gr in zip(names, grads)})


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-30))


def _check_grads(cfg, w, x_np, imgs=None, seed=0, gate=3e-2):
    """GPU straight-through gradients (autograd through the library) vs the float64 STE oracle, every parameter within
    rel-L2 3e-2; taps within 3e-2.  imgs: the images that receive upstream gradients (all when None)."""
    from tests.util import rel_l2
    taps = list(cfg.taps)
    B = x_np.shape[0]
    T = cfg.tokens(x_np.shape[2], x_np.shape[3])
    rng = np.random.default_rng(seed)
    dtaps = [rng.standard_normal((B, T, cfg.hidden_size)).astype(np.float32) / np.sqrt(B * T * cfg.hidden_size) for _ in taps]
    sel = list(range(B)) if imgs is None else list(imgs)
    for d in dtaps:
        mask = np.zeros(B, bool)
        mask[sel] = True
        d[~mask] = 0.0
    m = _enc(cfg, w).train()
    hs = m(torch.from_numpy(x_np).to(DEV), taps=taps).hidden_states
    loss = sum((hs[t] * torch.from_numpy(d).to(DEV)).sum() for t, d in zip(taps, dtaps))
    loss.backward()
    ref_taps, ref = ste_reference(cfg, w, x_np[sel], [d[sel] for d in dtaps], taps)
    for t, rt in zip(taps, ref_taps):
        assert rel_l2(hs[t].detach()[sel].cpu().numpy(), rt) < 3e-2, t
    worst = {}
    for name, p in m.named_parameters():
        if name not in ref or p.grad is None:
            continue
        if "key.bias" in name:
            continue
        worst[name] = _rel(p.grad.cpu().numpy(), ref[name])
    assert len(worst) >= 4 + 14 * cfg.num_hidden_layers, sorted(worst)
    bad = {k: v for k, v in worst.items() if not v < gate}
    assert not bad, bad
    return worst


@pytest.mark.parametrize("B,H,W", [(8, 64, 64), (4, 96, 64), (1, 272, 272)])
def test_micro_gradients_match_the_straight_through_oracle(B, H, W):
    cfg = _micro()
    w = synth.synth_weights(cfg, 13)
    x = synth.synth_images(B, H, W, seed=17)
    worst = _check_grads(cfg, w, x)
    print("worst gradient rel-L2:", max(worst.values()))


def test_vit_base_bs64_gradients_match_the_straight_through_oracle_on_three_images():
    cfg = dataclasses.replace(cfgs.vit_base(), drop_path_rate=0.0)
    w = synth.synth_weights(cfg, 6)
    x = synth.synth_images(64, 224, 224, seed=31)
    # gate 7e-2, not 3e-2: see DESIGN section 16 - at twelve layers the oracle's float64 activations cross e4m3 rounding
    # boundaries the GPU's do not (and back), so the compared quantised operands themselves differ by a few percent, uniformly
    # over layers and images; the micro geometries above hold the 3e-2 gate
    worst = _check_grads(cfg, w, x, imgs=(0, 31, 63), gate=7e-2)
    print("worst gradient rel-L2:", max(worst.values()))


def test_stochastic_depth_under_no_grad_matches_the_oracle():
    from layoutdit_amd.training import flat_state
    from tests.util import rel_l2
    cfg = dataclasses.replace(cfgs.vit_micro(), drop_path_rate=0.3)
    w = synth.synth_weights(cfg, 5)
    x_np = synth.synth_images(6, 64, 64, seed=4)
    m = _enc(cfg, w).train()
    L = cfg.num_hidden_layers
    ds = np.ones((L, 2, 6), np.float32)
    ds[1, 0, [1, 4]] = 0.0
    ds[2, 1, [0, 2, 5]] = 0.0
    ds[2, 0, 3] = 1.0 / 0.7
    st = flat_state(m, 64, 64)
    st.repack()
    taps = [1, 2, 3]
    with torch.no_grad():
        outs = st.forward(torch.from_numpy(x_np).to(DEV), taps, torch.from_numpy(ds).to(DEV), st.saved_nograd(6))
    zero = [np.zeros((6, cfg.tokens(64, 64), cfg.hidden_size), np.float32) for _ in taps]
    ref, _ = ste_reference(cfg, w, x_np, zero, taps, drop_scales=ds)
    for o, r in zip(outs, ref):
        assert rel_l2(o.cpu().numpy(), r) < 3e-2


def test_trainstep_matches_autograd_with_torch_adamw_after_three_steps():
    from layoutdit_amd.training import TrainStep, flat_state
    cfg = _micro()
    w = synth.synth_weights(cfg, 8)
    x = torch.from_numpy(synth.synth_images(8, 64, 64, seed=6)).to(DEV)
    m1 = _enc(cfg, w)
    ts = TrainStep(m1, lr=1e-3, drop_path_rate=0.0)
    for _ in range(3):
        ts.step(x)
    dt = ts._upstream(x)
    m2 = _enc(cfg, w).train()
    p0 = flat_state(m2, 64, 64).params.clone()
    opt = torch.optim.AdamW(m2.parameters(), lr=1e-3, weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8)
    for _ in range(3):
        opt.zero_grad()
        hs = m2(x, taps=list(cfg.taps)).hidden_states
        loss = sum((hs[t] * d).sum() for t, d in zip(cfg.taps, dt))
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    d1 = (ts.state.params - p0).cpu().numpy()
    d2 = (flat_state(m2, 64, 64).params - p0).cpu().numpy()
    assert _rel(d1, d2.astype(np.float64)) < 2e-2
