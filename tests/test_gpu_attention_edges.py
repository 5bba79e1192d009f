"""Every attention entry point at softmax's edges, against float64 on the same rounded operands and
against exact expectations - never against another kernel of this library.

  ldit_attention_f32, ldit_attention_bf16 (plain and prescaled, both LDIT_ATTN_BF16_NW widths), ldit_attention_planes (2 / 3
  planes), ldit_attention_fwd_lse_bf16, ldit_attention_bwd_bf16 (one-block N <= 256 and blocked), ldit_attention_mxfp8_train

Inputs (tests/attention_cases.py, pinned on the CPU by tests/test_attention_cases_cpu.py):
  selecting   exactly one-hot / two-hot softmax rows: bf16 outputs must EQUAL the expectation, fp32 outputs to a few ulps
  shifted     every logit of a row moved by t natural units (t = -512 .. +512, and +t / -t on alternating rows of one wave):
              results stay finite and inside the kernels' existing tensor gates AND per-element bounds derived from the float64
              P, dP, delta (one wrong row among thousands moves a tensor's relative-L2 by less than its gate)
  gaussian    the suite's usual inputs, under the same per-element bounds
All operands are column slices of a fused [B, N, 3C] tensor, as the forward passes them.  The worst observed ratio to every bound
is written to attention_edges.json in the directory tests/test_gpu_split_fp32.py records its margins in."""
import functools
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from layoutdit_amd import _lib, ops                                   # noqa: E402
from tests import attention_cases as ac                              # noqa: E402
from tests.test_gpu_split_fp32 import OUT                             # noqa: E402  (the suite's directory for measured margins)
from tests.mx_checks import check_mx_pack                            # noqa: E402

DEV = "cuda:0"
BF = torch.bfloat16
B, H, D = 2, 2, ac.D
C = H * D
NS = (17, 33, 197, 256, 257, 300)          # one partial tile; two tiles; the detector's length; the one-block limit; blocked; blocked
LONG = (600, 1025)                         # three / five 256-row blocks of the blocked backward, 10 / 17 chunks of the forwards
QC = np.float32(ac.SCALE * ac.LOG2E)       # the fold of the prescaled entries: q' = bf16(q c)
LN2 = float(np.log(2.0))
MARGINS = {}


@pytest.fixture(scope="module", autouse=True)
def _record_margins():
    assert torch.cuda.is_available(), "gpu-marked test running without a GPU"
    _lib.load()
    yield
    _lib.set_switch("LDIT_ATTN_BF16_NW", None)
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "attention_edges.json"), "w") as f:
        json.dump(dict(sorted(MARGINS.items())), f, indent=1)


def _margin(key, ratio):
    MARGINS[key] = max(MARGINS.get(key, 0.0), float(ratio))


# ---- cases and their float64 references: computed once, shared, never modified ---------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(kind, N, t=0, alternate=False):
    if kind == "selecting":
        return ac.selecting(B, N, H, seed=5)
    if kind == "gaussian":
        return ac.gaussian(B, N, H, seed=7)
    return ac.shifted(B, N, H, t, seed=7, alternate=alternate)


@functools.lru_cache(maxsize=None)
def _plain(kind, N, t=0, alternate=False):
    """(case, float64 reference) of the plain convention: logits q . k / 8."""
    case = _case(kind, N, t, alternate)
    return case, ac.reference(*case.parts(), case.do, H)


@functools.lru_cache(maxsize=None)
def _folded(kind, N, t=0, alternate=False):
    """(fused tensor with q' = bf16(q c), float64 reference of THOSE operands): exp2-domain logits q' . k."""
    case = _case(kind, N, t, alternate)
    qkv = case.qkv.clone()
    qkv[..., :C] = (case.qkv[..., :C].float() * QC).to(BF)
    return qkv, ac.reference(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], case.do, H, ln_scale=LN2)


@functools.lru_cache(maxsize=None)
def _f32(kind, N, t=0, alternate=False):
    """(fused fp32 tensor with q' = fl32(q c), float64 reference of those operands) for the planes kernel."""
    case = _case(kind, N, t, alternate)
    qkv = case.qkv.float()
    qkv[..., :C] = qkv[..., :C] * QC
    return qkv, ac.reference(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], case.do, H, ln_scale=LN2)


# ---- the entry points ---------------------------------------------------------------------------------------------------------
def _stream():
    return torch.cuda.current_stream().cuda_stream


def _split(t):
    return t[..., :C], t[..., C:2 * C], t[..., 2 * C:]


def run_f32(qkv):
    return ops.attention(*_split(qkv.float().to(DEV)), heads=H).cpu().double()


def run_bf16(qkv, prescaled=False, nw=None):
    _lib.set_switch("LDIT_ATTN_BF16_NW", nw)
    try:
        return ops.attention_bf16(*_split(qkv.to(DEV)), heads=H, prescaled=prescaled).cpu()
    finally:
        _lib.set_switch("LDIT_ATTN_BF16_NW", None)


def run_planes(qkv_f32, planes):
    N = qkv_f32.shape[1]
    qp = ops.split_planes(qkv_f32.reshape(B * N, 3 * C).to(DEV), planes).reshape(B, N, planes * 3 * C)
    out = ops.attention_planes(qp, H, planes)
    return sum(out[..., s * C:(s + 1) * C].double() for s in range(planes)).cpu()


def run_fwd_lse(qkv, scale=ac.SCALE):
    lib = _lib.load()
    N = qkv.shape[1]
    t = qkv.to(DEV)
    q, k, v = _split(t)
    o = torch.full((B, N, C), float("nan"), dtype=BF, device=DEV)
    lse = torch.full((B, H, N), float("nan"), dtype=torch.float32, device=DEV)
    _lib.check(lib.ldit_attention_fwd_lse_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), B, N, H, D,
                                               3 * C, 3 * C, 3 * C, C, scale, _stream()))
    torch.cuda.synchronize()
    return t, o, lse


def run_bwd(t, o, lse, do, scale=ac.SCALE):
    """dq | dk | dv as the train step gets them: one fused [B, N, 3C] tensor, from the forward kernel's own o and lse."""
    lib = _lib.load()
    N = t.shape[1]
    q, k, v = _split(t)
    g = do.to(DEV)
    dqkv = torch.full((B, N, 3 * C), float("nan"), dtype=BF, device=DEV)
    _lib.check(lib.ldit_attention_bwd_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), g.data_ptr(), lse.data_ptr(),
                                           dqkv.data_ptr(), dqkv[..., C:].data_ptr(), dqkv[..., 2 * C:].data_ptr(), B, N, H, D,
                                           3 * C, C, C, 3 * C, scale, _stream()))
    torch.cuda.synchronize()
    return _split(dqkv.cpu())


def run_mxfp8(qkv_folded):
    N = qkv_folded.shape[1]
    (codes, scales), lse, ob, od = ops.attention_mxfp8_train(qkv_folded.to(DEV).contiguous(), H)
    torch.cuda.synchronize()
    return (codes.view(torch.uint8).cpu().numpy(), scales.cpu().numpy(), lse.cpu(), ob.cpu().reshape(B, N, C), od.cpu().reshape(B, N, C))


# ---- gates ----------------------------------------------------------------------------------------------------------------------
def _rel_l2(got, ref):
    return float((got.double() - ref).norm() / ref.norm().clamp_min(1e-30))


def _gate(name, got, ref, bound, tensor_gate, shifted_case, with_channel0=True):
    """finite; relative-L2 inside the kernel's existing tensor gate, with and (shifted cases) without channel 0 of every head;
    every element inside `bound`.  The figures are printed before anything is asserted.  with_channel0 = False: the tensor gate is
    asserted without the offset channel only (the figure with it is still printed and recorded)."""
    got = got.double()
    finite = bool(torch.isfinite(got).all())
    err = (got - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).nan_to_num(nan=float("inf")).max())
    rl = [_rel_l2(got, ref)] + ([_rel_l2(ac.drop_channel0(got, H), ac.drop_channel0(ref, H))] if shifted_case else [])
    print(f"{name}: finite {finite}  rel-L2 {rl[0]:.3e} (gate {tensor_gate:.1e})"
          + (f", without channel 0 {rl[1]:.3e}" if shifted_case else "") + f"  worst element / bound {ratio:.3f}")
    if finite:
        _margin(name + "/element", ratio)
        _margin(name + "/rel_l2_over_gate", (max(rl) if with_channel0 else rl[-1]) / tensor_gate)
        if not with_channel0:
            _margin(name + "/rel_l2_over_gate_with_the_offset_channel_at_512", rl[0] / tensor_gate)
            rl = rl[1:]
    assert finite, f"{name}: non-finite values in {int((~torch.isfinite(got)).reshape(got.shape[0], got.shape[1], -1).any(-1).sum())} rows"
    assert max(rl) < tensor_gate, (name, rl)
    assert ratio <= 1.0, (name, ratio)


def _gate_lse(name, lse, ref):
    err = (lse.double() - ref.lse2).abs()
    finite = bool(torch.isfinite(lse).all())
    ratio = float((err / ac.lse_bound(ref)).nan_to_num(nan=float("inf")).max())
    print(f"{name}: finite {finite}  worst |lse - ref| {float(err.max()):.3e}  / bound {ratio:.3f}")
    if finite:
        _margin(name + "/element", ratio)
    assert finite and ratio <= 1.0, (name, ratio)


def _logit_noise(ref, v):
    """[B, N, C]: what the fp32 accumulation of the LOGITS can move an output by.  Each logit is a sum of D products accumulated in
    fp32 (by the MFMA, in k order), so its error is at most eps_i = D 2^-24 ln_scale max_j sum_d |q_id k_jd| natural units - the
    same bound lse_bound uses.  Perturbing every logit of a row by at most eps changes each p_ij by a factor within e^(+-2 eps)
    (numerator e^(+-eps), denominator e^(-+eps)), hence o_id by at most (e^(2 eps) - 1) sum_j p_ij |v_jd|.  This term matters only
    where one product dwarfs the logit's spread (the shifted cases: |q_0 k_0| = 8 |t| against logits of order 1); the relative-L2
    and 1e-5 max(|ref|, 1) gates of the fp32-grade kernels assume sum_d |q k| of order D."""
    eps = D * 2.0 ** -24 * ref.ln_scale * ref.absqk
    return ac._tokens(torch.expm1(2 * eps)[..., None] * (ref.P @ ac._heads(v, H).abs()))


def _fp32_grade_gates(name, got, ref, v, gate, shifted_case):
    """The fp32 kernel and the planes kernels: the existing per-element gate `gate` max(|ref|, 1) and relative-L2 gate.  On the
    shifted cases both get the logit-accumulation term of _logit_noise added (as an element bound, and as its norm over the
    reference's norm): honest fp32 accumulation of a logit that holds a product of 8 |t| cannot keep 1e-5 of a result of order 1."""
    bound = gate * ref.o.abs().clamp_min(1.0)
    tensor_gate = gate
    if shifted_case:
        noise = _logit_noise(ref, v)
        bound = bound + noise
        tensor_gate = gate + float(noise.norm() / ref.o.norm())
        plain = float(((got.double() - ref.o).abs() / (gate * ref.o.abs().clamp_min(1.0))).max())
        _margin(name + "/element_without_the_logit_term", plain)
        _margin(name + "/rel_l2_over_gate_without_the_logit_term", _rel_l2(got, ref.o) / gate)
    _gate(name, got, ref.o, bound, tensor_gate, shifted_case)


# ---- mxfp8: the codes against the host MX pack (tests/mx_checks.py, shared with the LayerNorm edges) --------------------------------
def _check_mx_pack(name, codes, scales, ob, od, exact):
    check_mx_pack(name, codes, scales, ob.float().numpy(), od.float().numpy(), exact, MARGINS)


# ================================================================================================================ exact selection
def _expect(case):
    eo, edq, edk, edv, _ = ac.select_expectation(case)
    return tuple(torch.from_numpy(a) for a in (eo, edq, edk, edv))


def _same(name, got, expect):
    """A bf16 result EQUALS its expectation (as values: every expected value is bf16-representable)."""
    bad = got.double() != expect
    assert not bool(bad.any()), (name, int(bad.sum()), "elements differ; first:", got.double()[bad][:4].tolist(), expect[bad][:4].tolist())


@pytest.mark.parametrize("N", NS + LONG)
def test_selection_is_exact_in_every_forward(N):
    """One-hot / two-hot rows.  The selected probabilities are equal, every other one underflows to exactly 0, so
    o = (v_a + v_b) / 2 whatever p and l round to: p_a = p_b = p, l = 2 p (one exact doubling) -
      bf16 kernels   P is rounded to bf16, l sums the unrounded p: o = bf16(p) (v_a + v_b) / (2 p), within 2^-9 + a few 2^-24 of a
                     value in {-1, -1/2, 0, 1/2, 1} ... the final bf16 rounding returns exactly that value PROVIDED |bf16(p) / p - 1| is
                     well below 2^-9.  It is: plain entries p = exp2(fma(s, c, -fl(m c))), off 1 by half an ulp of m c = 1270
                     (6e-5) - bf16(p) = 1; prescaled entries carry m = 1271.875 exactly as two bf16 (14 significant bits:
                     tests/test_attention_cases_cpu.py), p = 1.
      fp32 kernel    p v / l with p and l equal up to the doubling but not exactly 1: product, reciprocal, product, one rounding
                     each, plus one spare: 4 * 2^-24 relative.
      planes         the result is a sum of 2 / 3 bf16 planes of the fp32 o: 2^-17 / 2^-24 relative (the representation bounds of
                     test_split_planes_reconstruct_the_value)."""
    case, ref = _plain("selecting", N)
    eo = _expect(case)[0]
    assert ref.gap * ac.LOG2E > 150
    qf, reff = _folded("selecting", N)
    assert reff.gap * ac.LOG2E > 150 and float((reff.o - eo).abs().max()) < 1e-60        # selection survives bf16(q c)
    # fp32
    o = run_f32(case.qkv)
    r = float(((o - eo).abs() / (4 * 2.0 ** -24 * eo.abs()).clamp_min(1e-300)).max())
    print(f"f32: worst |o - expect| / (4 2^-24 |expect|) = {r:.3f}")
    _margin("selecting/f32/o", r)
    assert r <= 1.0
    # bf16, both entry modes, both workgroup widths
    for nw in (None, "4", "8"):
        _same(f"bf16 NW={nw}", run_bf16(case.qkv, nw=nw), eo)
        _same(f"bf16 prescaled NW={nw}", run_bf16(qf, prescaled=True, nw=nw), eo)
    # planes: the folded queries bf16(q c) as fp32 operands (the planes kernel carries its running maximum as two bf16, like the
    # prescaled bf16 entry: 1271.875 is exact there, fl32(128 c) * 55 would not be, and p = 1 is what makes the row exact)
    for planes, rep in ((2, 2.0 ** -17), (3, 2.0 ** -24)):
        o = run_planes(qf.float(), planes)
        r = float(((o - eo).abs() / (rep * eo.abs()).clamp_min(1e-300)).max())
        print(f"planes {planes}: worst |o - expect| / (representation bound) = {r:.3f}")
        _margin(f"selecting/planes{planes}/o", r)
        assert r <= 1.0
    # train forward
    _, o, lse = run_fwd_lse(case.qkv)
    _same("fwd_lse o", o.cpu(), eo)
    _gate_lse("selecting/fwd_lse/lse", lse.cpu(), ref)
    # mxfp8 train forward
    codes, scales, lse, ob, od = run_mxfp8(qf)
    _same("mxfp8_train ob", ob, eo)
    _gate_lse("selecting/mxfp8_train/lse", lse, reff)
    _check_mx_pack("selecting/mxfp8_train", codes, scales, ob.reshape(B * N, C), od.reshape(B * N, C), exact=True)


@pytest.mark.parametrize("N", NS + LONG)
def test_selection_is_exact_in_the_backward(N):
    """dq, dk, dv of the one-block (N <= 256) and the blocked backward EQUAL the expectation.  The recomputed p = exp2(c s - L2) is
    1/2 (or 1) only up to an ulp of L2 = 1270 (1.3e-4 relative), but every product it enters is rounded to bf16 before it is
    summed: bf16(p) = 1/2 exactly (dv = sum of halves of dO rows in {-1, 0, 1}); dS = p (dP - delta) / 8 has an exact value with
    at most 6 significant bits ((dP_a - dP_b) / 64, integers below 64), which the bf16 rounding returns; the sums dq = dS K
    (integers <= 2 in the spare dims), dk = dS^T Q (+-128) are then exact in fp32 and bf16-representable."""
    case, ref = _plain("selecting", N)
    _, edq, edk, edv = _expect(case)
    t, o, lse = run_fwd_lse(case.qkv)
    dq, dk, dv = run_bwd(t, o, lse, case.do)
    _same("dv", dv, edv)
    _same("dk", dk, edk)
    _same("dq", dq, edq)


# ======================================================================================================= level shifts, per element
LEVELS = [("gaussian", N, 0, False) for N in NS] + [("shifted", N, t, False) for N in NS for t in ac.SHIFTS] \
    + [("shifted", N, t, True) for N in NS for t in (96, 512)] + [("shifted", 600, -96, False), ("shifted", 1025, -96, True)]
_ids = [f"{k}-N{N}-t{t}{'-alternating' if a else ''}" for k, N, t, a in LEVELS]


@pytest.mark.parametrize("kind,N,t,alternate", LEVELS, ids=_ids)
def test_forwards_at_every_level(kind, N, t, alternate):
    """Every forward on logits at level t: finite, inside its existing tensor gate (with and without the offset channel) and inside
    the per-element bound.  bf16 kernels: |o^ - o| <= 1.25 * 2u * (P |V|) (P to bf16 and the output to bf16, u = 2^-9 each; 1.25
    for fp32 accumulation and v_exp_f32).  The mxfp8 train kernel rounds P to bf16 like the others (attention_flash.hip: the same
    `pf[st][jj] = (bf16_t)s[kt][...]`; only its OUTPUT is MX), so it keeps u.  lse: 2e-3 + D 2^-24 c max_j sum_d |q k|."""
    sh = kind == "shifted"
    case, ref = _plain(kind, N, t, alternate)
    q, k, v = case.parts()
    bo = ac.fwd_bound_bf16(ref, v, H)
    _fp32_grade_gates("f32/o", run_f32(case.qkv), ref, v, 1e-5, sh)
    _gate("bf16/o", run_bf16(case.qkv), ref.o, bo, 6e-3, sh)
    t_dev, o, lse = run_fwd_lse(case.qkv)
    _gate("fwd_lse/o", o.cpu(), ref.o, bo, 6e-3, sh)
    _gate_lse("fwd_lse/lse", lse.cpu(), ref)
    qf, reff = _folded(kind, N, t, alternate)
    bof = ac.fwd_bound_bf16(reff, v, H)
    _gate("bf16_prescaled/o", run_bf16(qf, prescaled=True), reff.o, bof, 6e-3, sh)
    codes, scales, lse, ob, od = run_mxfp8(qf)
    _gate("mxfp8_train/ob", ob, reff.o, bof, 6e-3, sh)
    _gate_lse("mxfp8_train/lse", lse, reff)
    _check_mx_pack("mxfp8_train", codes, scales, ob.reshape(B * N, C), od.reshape(B * N, C), exact=False)
    q32, ref32 = _f32(kind, N, t, alternate)
    for planes, gate in ((2, 2e-5), (3, 2e-6)):
        _fp32_grade_gates(f"planes{planes}/o", run_planes(q32, planes), ref32, v, gate, sh)


def _backward(kind, N, t, alternate):
    case, ref = _plain(kind, N, t, alternate)
    t_dev, o, lse = run_fwd_lse(case.qkv)
    return case, ref, run_bwd(t_dev, o, lse, case.do)


@pytest.mark.parametrize("kind,N,t,alternate", LEVELS, ids=_ids)
def test_backward_at_every_level(kind, N, t, alternate):
    """ldit_attention_bwd_bf16 (one-block for N <= 256, blocked above) on the train forward's own o and lse: dq, dk, dv finite,
    relative-L2 <= 1.5e-2 with and without the offset channel, and per element (u = 2^-9, h(x) = half a bf16 ulp of x)
        dv:      1.25 (h(P)^T |dO| + h(dv))
        dq, dk:  E_ij = scale p_ij ((2u + 2^-22 |L2_i|) |dP_ij - delta_i| + u sum_d |dO_id o_id|),
                 1.25 (sum_j E_ij |k_j| + u |dq_i|),  1.25 (sum_i E_ij |q_i| + u |dk_j|).
    dv's bound has h(x) where it was first written u |x|: half an ulp of x is up to 2u |x|, and the design's exact arithmetic
    exceeds the u form at N = 17 (1.06 on the Gaussian case, 1.01 on the shifted ones - the CPU emulation of
    tests/test_attention_cases_cpu.py gives the same two figures as the kernel).
    dq's tensor gate WITH the offset channel is not asserted at |t| = 512: see the test below.
    Before the padded keys of the last, partial key block were masked (attention_bwd_bf16.hip) every dq element of every row with
    L2 < ~-128 was NaN whenever N % 32 != 0: t <= -96 here, at every N but 256 (66 of 66 rows at N = 33, 394 of 394 at N = 197,
    514 at 257, 600 at 300)."""
    sh = kind == "shifted"
    case, ref, (dq, dk, dv) = _backward(kind, N, t, alternate)
    q, k, v = case.parts()
    for name, g in (("dq", dq), ("dk", dk), ("dv", dv)):
        bad = ~torch.isfinite(g.float())
        assert not bool(bad.any()), f"{name}: non-finite values in {int(bad.any(-1).sum())} of {B * N} rows"
    bq, bk = ac.dqdk_bounds(ref, q, k, case.do, H)
    _gate("bwd/dv", dv, ref.dv, ac.dv_bound(ref, case.do, H), 1.5e-2, sh)
    _gate("bwd/dk", dk, ref.dk, bk, 1.5e-2, sh)
    _gate("bwd/dq", dq, ref.dq, bq, 1.5e-2, sh, with_channel0=abs(t) < 512)


@pytest.mark.parametrize("kind,N,t,alternate", [pytest.param(*c, marks=pytest.mark.xfail(
    strict=True, reason="dS is rounded to bf16 before dq = dS K: channel 0 of dq (exactly 0) gets 64 x the rounding errors of dS"))
    for c in LEVELS if abs(c[2]) == 512], ids=[i for i, c in zip(_ids, LEVELS) if abs(c[2]) == 512])
def test_backward_dq_with_the_offset_channel_at_512(kind, N, t, alternate):
    """dq's relative-L2 gate of 1.5e-2 INCLUDING the offset channel, at |t| = 512: not met, 2.0e-2 .. 2.4e-2 at every N (without
    that channel: 2.4e-3, and every element is inside its bound in the test above).  Cause, by reading attention_bwd_bf16.hip:
    dq_i0 = scale sum_j dS_ij k_j0 is 0 in exact arithmetic (k[:, 0] = t / 8 is one constant and sum_j dS_ij = 0), but phase 2 packs dS
    to bf16 (pack8) before the K^T dS^T product, so dq_i0 = 64 sum_j (bf16(dS_ij) - dS_ij): 64 times the rounding errors, nothing
    to cancel them.  Any kernel that feeds one bf16 dS to the matrix pipe gives the same figure (the CPU emulation in
    tests/test_attention_cases_cpu.py: 2.2e-2); meeting the gate takes dS in two bf16 planes for the dq product.  strict: a kernel
    that does will flag this mark."""
    _, ref, (dq, _, _) = _backward(kind, N, t, alternate)
    assert bool(torch.isfinite(dq.float()).all())
    assert _rel_l2(dq, ref.dq) < 1.5e-2
