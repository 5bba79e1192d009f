"""The ``"mxfp8"`` inference build on the GPU: MX quantiser, block-scaled GEMM (v_mfma_scale_f32_32x32x64_f8f6f4 with VGPR
scales), its epilogues, and the whole forward.  The format and its numpy reference: tests/test_mxfp8_format.py.

Gates as in tests/test_gpu_fp8.py (its docstring: the fp8 MFMA aligns a k-group's products to the largest one, so fp32 results are
within rel-L2 1e-4, |err| <= 1e-3 max(|ref|, 1) of the oracle on the dequantised operands; bf16 results 3e-3; requantised results
equal except a small fraction one code step away).  The lane map of the scale operands is checked EXACTLY: small-integer codes
under per-(row, block) power-of-two scales keep every product and every sum exact in fp32, so a wrong row / block / operand
assignment of a scale cannot pass."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from layoutdit_amd import _lib, config as cfgs, ops, synth          # noqa: E402
from oracle import oracle                                            # noqa: E402
from tests.test_mxfp8_format import edge_blocks, mx_dequant, mx_exponent, mx_quant_ref   # noqa: E402
from tests.util import max_rel, rel_l2                               # noqa: E402

DEV = "cuda:0"
F8 = torch.float8_e4m3fn


def _rand(seed, *shape, scale=1.0):
    n = int(np.prod(shape))
    return (scale * synth.normal(seed, 9, n)).astype(np.float32).reshape(shape)


def _cos(a, b):
    a, b = a.reshape(-1).astype(np.float64), b.reshape(-1).astype(np.float64)
    return float(a @ b / np.sqrt((a @ a) * (b @ b)))


def _mx(x):
    """numpy MX operand -> (device codes, device scales, float32 dequantised values)"""
    codes, scales, _ = mx_quant_ref(x)
    return (torch.from_numpy(codes).view(F8).to(DEV), torch.from_numpy(scales).to(DEV),
            mx_dequant(codes, scales).astype(np.float32))


# ---- quantiser -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,K", [(1, 32), (37, 96), (300, 768), (129, 3072), (5, 128)])
def test_quant_mx_bit_exact(rows, K):
    x = _rand(rows * 7 + K, rows, K) * np.exp2(np.arange(rows) % 41 - 20).astype(np.float32)[:, None]
    codes, scales = ops.quant_mxfp8(torch.from_numpy(x).to(DEV))
    wc, ws, _ = mx_quant_ref(x)
    np.testing.assert_array_equal(scales.cpu().numpy(), ws)
    np.testing.assert_array_equal(codes.view(torch.uint8).cpu().numpy(), wc)


def test_quant_mx_edge_blocks_and_row_stride():
    x = edge_blocks()
    wide = np.zeros((x.shape[0], x.shape[1] + 36), np.float32)         # a non-unit row stride (lds = K + 36)
    wide[:, :x.shape[1]] = x
    xd = torch.from_numpy(wide).to(DEV)[:, :x.shape[1]]
    codes, scales = ops.quant_mxfp8(xd)
    wc, ws, fin = mx_quant_ref(x)
    np.testing.assert_array_equal(scales.cpu().numpy(), ws)
    m = np.repeat(fin, 32, axis=1)
    np.testing.assert_array_equal(codes.view(torch.uint8).cpu().numpy()[m], wc[m])


@pytest.mark.parametrize("rows,C", [(3, 128), (394, 768), (9000, 768), (70, 1024), (17, 2048)])
def test_layernorm_mxfp8_is_the_mx_operand_of_the_fp32_layernorm(rows, C):
    """LayerNorm with MX output (8 lanes per 32-channel block): bit for bit the MX quantisation of the fp32 kernel's rows."""
    x = _rand(rows + C, rows, C, scale=3.0) + _rand(5, C)[None, :]
    g, b = _rand(6, C, scale=0.5) + 1.0, _rand(7, C, scale=0.1)
    xd, gd, bd = (torch.from_numpy(t).to(DEV) for t in (x, g, b))
    codes, scales = ops.layernorm_mxfp8(xd, gd, bd)
    y = ops.layernorm(xd, gd, bd).cpu().numpy()
    wc, ws, _ = mx_quant_ref(y)
    np.testing.assert_array_equal(scales.cpu().numpy(), ws)
    np.testing.assert_array_equal(codes.view(torch.uint8).cpu().numpy(), wc)


# ---- the scale operands' lane map, exactly -----------------------------------------------------------------------------------
def _exact_operands(seed, M, N, K):
    """small-integer codes (|c| <= 4) and per-(row, block) scales: X in 2^-3 .. 2^0, W in 2^0 .. 2^3 (asymmetric W, different
    scales per operand) - every product 2^-3 .. 2^7, every sum of K <= 4096 of them exact in fp32"""
    rng = np.random.default_rng(seed)
    xc = rng.integers(-4, 5, (M, K)).astype(np.float64)
    wc = rng.integers(-4, 5, (N, K)).astype(np.float64)
    wc[:, 0] += np.arange(N) % 3                                        # no row symmetry
    ex = rng.integers(-3, 1, (M, K // 32))
    ew = rng.integers(0, 4, (N, K // 32))
    x = (xc * np.repeat(np.exp2(ex), 32, axis=1)).astype(np.float32)
    w = (wc * np.repeat(np.exp2(ew), 32, axis=1)).astype(np.float32)
    return x, w


def _check_exact(x, w, tile):
    M, N = x.shape[0], w.shape[0]
    xq, xs, xv = _mx(x)
    wq, ws, wv = _mx(w)
    assert np.array_equal(xv, x) and np.array_equal(wv, w)              # the operands are exactly representable
    ref = x.astype(np.float64) @ w.astype(np.float64).T
    ref32 = ref.astype(np.float32)
    assert np.array_equal(ref32.astype(np.float64), ref)               # ... and so is their product
    if tile is not None:
        _lib.set_switch("LDIT_GEMM_FP8_TILE", tile)
    try:
        # bias epilogue: bf16 of the exact fp32 accumulator (round to nearest even), every tile
        yb = ops.linear_mxfp8((xq, xs), (wq, ws)).cpu()
        assert torch.equal(yb, torch.from_numpy(ref32).to(torch.bfloat16)), tile
        if tile != "4":                                                 # (the 320-row tile has no scale+residual instantiation)
            zero = torch.zeros((M, N), device=DEV)
            y = ops.linear_mxfp8((xq, xs), (wq, ws), epilogue=_lib.EPI_SCALE_RESID, lam=torch.ones(N, device=DEV), residual=zero,
                                 out=zero)
            got = y.cpu().numpy()
            bad = got != ref32
            assert not bad.any(), (tile, int(bad.sum()), np.argwhere(bad)[:5].tolist())
    finally:
        _lib.set_switch("LDIT_GEMM_FP8_TILE", None)


@pytest.mark.parametrize("tile", [None, "0", "1", "2", "3", "4"])
@pytest.mark.parametrize("M,N,K", [(512, 512, 256), (600, 520, 640), (37, 50, 128)])
def test_scale_lane_map_is_exact_on_every_tile(tile, M, N, K):
    x, w = _exact_operands(M + N + K, M, N, K)
    _check_exact(x, w, tile)


def test_scale_lane_map_is_exact_on_the_peeled_tail():
    """M = 256 * 16 + 16 with 16 column tiles: the last 16 rows run in gemm_fp8_tail<.., MX> (the launch peels them off)."""
    x, w = _exact_operands(7, 4112, 4096, 128)
    _check_exact(x, w, None)


# ---- epilogues against the oracle on the dequantised operands -------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(394, 576, 256), (1025, 2304, 768), (4500, 768, 3072)])
def test_linear_mxfp8_bias_and_scale_residual(M, N, K):
    x, w, b = _rand(1, M, K), _rand(2, N, K, scale=0.05), _rand(3, N, scale=0.1)
    xq, xs, xv = _mx(x)
    wq, ws, wv = _mx(w)
    bd = torch.from_numpy(b).to(DEV)
    y = ops.linear_mxfp8((xq, xs), (wq, ws), bd).float().cpu().numpy()
    ref = oracle.linear(xv, wv) + b
    assert rel_l2(y, ref) < 3e-3
    assert max_rel(y, ref) < 1.6e-2
    lam, r = _rand(7, N, scale=0.3), _rand(8, M, N)
    rd = torch.from_numpy(r).to(DEV)
    y2 = torch.empty_like(rd)
    yr = ops.linear_mxfp8((xq, xs), (wq, ws), bd, epilogue=_lib.EPI_SCALE_RESID, lam=torch.from_numpy(lam).to(DEV), residual=rd,
                          out=rd, out2=y2)
    assert yr.data_ptr() == rd.data_ptr() and torch.equal(yr, y2)
    refr = r + lam * ref
    assert rel_l2(yr.cpu().numpy(), refr) < 1e-4
    assert max_rel(yr.cpu().numpy(), refr) < 1e-3


@pytest.mark.parametrize("M,N,K", [(394, 320, 128), (2000, 3072, 768), (70, 3072, 768)])
def test_linear_mxfp8_gelu_writes_mx(M, N, K):
    x, w, b = _rand(9, M, K), _rand(10, N, K, scale=0.05), _rand(11, N, scale=0.2)
    xq, xs, xv = _mx(x)
    wq, ws, wv = _mx(w)
    pre = (oracle.linear(xv, wv) + b).astype(np.float64)
    ref = (pre / (1.0 + np.exp(-(1.5957691216 * pre + 0.0713548163 * pre ** 3)))).astype(np.float32)   # gelu_lp (ldit_common.h)
    codes, scales = ops.linear_mxfp8((xq, xs), (wq, ws), torch.from_numpy(b).to(DEV), epilogue=_lib.EPI_BIAS_GELU)
    gc, gs = codes.view(torch.uint8).cpu().numpy(), scales.cpu().numpy()
    wc, wsc, _ = mx_quant_ref(ref)
    # scales: equal except where a block's amax sits on a power-of-two boundary within the MFMA's error
    amax = np.abs(ref.reshape(M, N // 32, 32)).max(-1).astype(np.float64)
    tol = 1e-3 * np.maximum(np.abs(pre).reshape(M, N // 32, 32).max(-1), 1.0)
    boundary = mx_exponent(amax - tol) != mx_exponent(amax + tol)
    assert np.all((gs == wsc) | boundary), int(((gs != wsc) & ~boundary).sum())
    assert (gs != wsc).mean() < 1e-2
    # codes: equal except a small fraction one code step away (blocks with equal scales)
    same = np.repeat(gs == wsc, 32, axis=1)
    gv, wv8 = mx_dequant(gc, gs), mx_dequant(wc, wsc)
    differ = (gv != wv8) & same
    assert differ.mean() < 1e-2, differ.mean()
    step = np.repeat(np.ldexp(1.0, gs.astype(np.int64) - 127), 32, axis=1)
    bad = np.abs(gv - ref) > np.maximum(np.abs(ref) * 0.0625, 2.0 ** -9 * step) + 1.2e-3 * np.maximum(np.abs(pre), 1.0)
    assert not bad.any(), int(bad.sum())


def test_block_scales_keep_every_rows_dynamic_range():
    """Rows of X scaled by 2^r, r in [-30, 30]: with block scales every row keeps its relative accuracy; one per-tensor fp8 scale
    flushes the small rows to zero (linear_fp8, for the record)."""
    M, N, K = 244, 256, 512
    r = np.arange(M) % 61 - 30
    x = _rand(31, M, K) * np.exp2(r).astype(np.float32)[:, None]
    w = _rand(32, N, K, scale=0.05)
    xq, xs, xv = _mx(x)
    wq, ws, wv = _mx(w)
    y = ops.linear_mxfp8((xq, xs), (wq, ws), epilogue=_lib.EPI_SCALE_RESID, lam=torch.ones(N, device=DEV),
                         residual=torch.zeros((M, N), device=DEV)).cpu().numpy()
    ref = x.astype(np.float64) @ w.astype(np.float64).T
    err = np.array([rel_l2(y[i], ref[i]) for i in range(M)])
    base = err[r == 0].max()
    assert base < 1e-1 and err.max() <= 1.5 * base, (base, err.max())
    # per-tensor fp8: one scale for X, one for W
    sx, sw = float(np.abs(x).max()) / 448.0, float(np.abs(w).max()) / 448.0
    xt = (torch.from_numpy(x) / sx).clamp(-448, 448).to(F8)
    wt = (torch.from_numpy(w) / sw).clamp(-448, 448).to(F8)
    yt = ops.linear_fp8(xt.to(DEV), wt.to(DEV), sx * sw, epilogue=_lib.EPI_SCALE_RESID, lam=torch.ones(N, device=DEV),
                        residual=torch.zeros((M, N), device=DEV)).cpu().numpy()
    small = r <= -10
    assert np.all(yt[small] == 0.0)                                     # the small rows are gone
    assert np.all(err[small] < 1e-1)                                    # ... and kept by the block scales


# ---- whole forward ----------------------------------------------------------------------------------------------------------
def _enc(cfg, w, dtype="mxfp8"):
    from layoutdit_amd.modeling import DiTEncoder
    return DiTEncoder(cfg, compute_dtype=dtype).load_numpy(w).to(DEV).eval()


def test_mxfp8_forward_micro_vs_oracle_with_no_setup():
    cfg = cfgs.vit_micro()
    w = synth.synth_weights(cfg, 5)
    x = synth.synth_images(4, 64, 64, seed=21)
    m = _enc(cfg, w)
    with torch.no_grad():
        out = m(torch.from_numpy(x).to(DEV), taps=[0, 1, 2, 3])          # the first call: nothing set up before it
    _, hidden = oracle.vit_forward(cfg, w, x, all_hidden=True)
    for t in range(4):
        h = out.hidden_states[t].cpu().numpy()
        assert np.isfinite(h).all()
        assert rel_l2(h, hidden[t]) < (1e-2 if t == 0 else 1e-1), t
        assert _cos(h, hidden[t]) > 0.995, t
    m.train()
    with pytest.raises(NotImplementedError, match="inference only"):
        m(torch.from_numpy(x).to(DEV))


def test_mxfp8_forward_base_vs_fp32_build_and_batch_invariance():
    """ViT-B/16 224^2 bs=8 against the fp32 build; a re-run slice equals the full batch's rows bit for bit (a row's scales
    depend on that row alone)."""
    cfg = cfgs.vit_base()
    w = synth.synth_weights(cfg, 0)
    x = torch.from_numpy(synth.synth_images(8, 224, 224, seed=1234)).to(DEV)
    m32, mx = _enc(cfg, w, "f32"), _enc(cfg, w)
    with torch.no_grad():
        ref = m32(x).hidden_states
        got = mx(x).hidden_states
        part = mx(x[5:7]).hidden_states
        one = mx(x[3:4]).hidden_states
    for t in cfg.taps:
        a, b = got[t].cpu().numpy(), ref[t].cpu().numpy()
        assert rel_l2(a, b) < (1e-2 if t == 0 else 1e-1), t
        assert _cos(a, b) > 0.995, t
        assert torch.equal(got[t][5:7], part[t]), t
        assert torch.equal(got[t][3:4], one[t]), t


def test_mxfp8_forward_ragged_rectangular_and_graph_replay():
    from tests.util import resample_pos
    cfg = cfgs.vit_micro()
    w = synth.synth_weights(cfg, 9)
    x = synth.synth_images(3, 96, 64, seed=31)                    # 6 x 4 grid, 25 tokens, M = 75 rows
    m = _enc(cfg, w)
    xd = torch.from_numpy(x).to(DEV)
    with torch.no_grad():
        hs = m(xd).hidden_states
    eager = [h.clone() for h in hs if h is not None]
    pos = resample_pos(w["embeddings.position_embeddings"], 4, 6, 4)
    _, hidden = oracle.vit_forward(cfg, w, x, pos=pos, all_hidden=True)
    for t in sorted(set(cfg.taps)):
        a = hs[t].cpu().numpy()
        assert rel_l2(a, hidden[t]) < 1e-1 and _cos(a, hidden[t]) > 0.995, t
    static_x = xd.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.no_grad():
        with torch.cuda.stream(s):
            m(static_x)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_out = [h for h in m(static_x).hidden_states if h is not None]
        graph.replay()
        torch.cuda.synchronize()
    for a, b in zip(static_out, eager):
        assert torch.equal(a, b)


def test_mxfp8_forward_image_list_equals_the_two_step_path():
    from layoutdit_amd.modeling.detector_input import DetectorInputTransform
    cfg = cfgs.vit_micro()
    w = synth.synth_weights(cfg, 4)
    sizes = [(80, 50), (64, 64), (33, 129)]
    imgs = [torch.from_numpy(np.clip(0.5 + 0.3 * _rand(30 + i, 3, h, wd), 0, 1)).to(DEV) for i, (h, wd) in enumerate(sizes)]
    m = _enc(cfg, w)
    t = DetectorInputTransform(fixed_size=(64, 64))
    with torch.no_grad():
        want = m(t(imgs)[0].tensors).hidden_states
        got = m.forward_image_list(imgs, size=(64, 64)).hidden_states
    for tp in cfg.taps:
        assert torch.equal(got[tp], want[tp]), tp


def test_mxfp8_backbone_maps_within_the_gate():
    from layoutdit_amd.modeling import DiTBackbone
    cfg = cfgs.vit_base()
    w = synth.synth_weights(cfg, 1)
    x = torch.from_numpy(synth.synth_images(2, 224, 224, seed=77)).to(DEV)
    feats = {}
    for dt in ("f32", "mxfp8"):
        bb = DiTBackbone(config=cfg, compute_dtype=dt)
        bb.dit.load_numpy(w)
        bb = bb.to(DEV).eval()
        with torch.no_grad():
            feats[dt] = {k: v.float().cpu().numpy() for k, v in bb(x).items()}
    for k in feats["f32"]:
        a, b = feats["mxfp8"][k], feats["f32"][k]
        assert a.shape == b.shape, k
        assert rel_l2(a, b) < 1e-1 and _cos(a, b) > 0.995, k


def test_mxfp8_has_no_stale_state_after_a_weight_update():
    """In-place weight update + mark_parameters_changed(): the output equals that of a freshly built model with the new
    weights, bit for bit - no recalibration exists to forget."""
    cfg = cfgs.vit_micro()
    w = synth.synth_weights(cfg, 12)
    x = torch.from_numpy(synth.synth_images(2, 64, 64, seed=5)).to(DEV)
    m = _enc(cfg, w)
    with torch.no_grad():
        before = m(x).hidden_states[cfg.taps[-1]].clone()
        for p in m.parameters():
            p.data.mul_(1.5)
        m.mark_parameters_changed()
        after = m(x).hidden_states[cfg.taps[-1]]
    w2 = {k: (v * np.float32(1.5)).astype(np.float32) for k, v in w.items()}
    fresh = _enc(cfg, w2)
    with torch.no_grad():
        want = fresh(x).hidden_states[cfg.taps[-1]]
    assert not torch.equal(before, after)
    assert torch.equal(after, want)


def test_mxfp8_outlier_stress():
    """The x60 outlier weights of test_gpu_lowp_pinning (ViT-B bs=1): gated like the fp8 build; the numbers of both builds on
    the same batch are printed and, when LDIT_REPORT_DIR names a directory, written to outlier_stress_mxfp8.json there (reported
    in DESIGN.md, not gated against each other)."""
    from tests.test_gpu_lowp_pinning import CAL_SEED, _outlier_weights
    cfg = cfgs.vit_base()
    w = _outlier_weights(cfg, 4, 60.0)
    x = synth.synth_images(1, 224, 224, seed=1234)
    ref, _ = oracle.vit_forward(cfg, w, x)
    xd = torch.from_numpy(x).to(DEV)
    mx = _enc(cfg, w)
    m8 = _enc(cfg, w, "fp8")
    m8.calibrate_fp8(torch.from_numpy(synth.synth_images(2, 224, 224, seed=CAL_SEED)).to(DEV))
    with torch.no_grad():
        hx, h8 = mx(xd).hidden_states, m8(xd).hidden_states
    rec = {}
    for t, r in zip(cfg.taps, ref):
        a, b = hx[t].cpu().numpy(), h8[t].cpu().numpy()
        rec[str(t)] = {"mxfp8_rel_l2": rel_l2(a, r), "mxfp8_cos": _cos(a, r), "fp8_rel_l2": rel_l2(b, r), "fp8_cos": _cos(b, r)}
    print(json.dumps(rec))
    if os.environ.get("LDIT_REPORT_DIR"):
        os.makedirs(os.environ["LDIT_REPORT_DIR"], exist_ok=True)
        with open(os.path.join(os.environ["LDIT_REPORT_DIR"], "outlier_stress_mxfp8.json"), "w") as f:
            json.dump(rec, f, indent=1)
    for t, v in rec.items():
        assert v["mxfp8_rel_l2"] < 1e-1 and v["mxfp8_cos"] > 0.995, (t, v)
