"""The input constructions of tests/attention_cases.py have the properties the GPU tests (tests/test_gpu_attention_edges.py) rely
on, and the fault the shifted cases look for is visible to them.  CPU tensors only; no library code is involved."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import attention_cases as ac          # noqa: E402

BF = torch.bfloat16


def _is_bf16(t) -> bool:
    t = torch.as_tensor(t, dtype=torch.float64)
    return bool((t.to(BF).double() == t).all())


@pytest.mark.parametrize("N", ac.SELECT_N)
def test_selecting_rows_are_exactly_one_or_two_hot(N):
    """Gap from the matching logit to any other > 150 / log2 e (so exp2 underflows to 0 in fp32: 2^-149 is the smallest subnormal);
    every pair chosen by at most two queries; the first tile reaches the last, partial tile and back; the float64 softmax reference
    equals the expectation built from the construction alone, and that expectation is bf16-representable."""
    B, H = 2, 2
    case = ac.selecting(B, N, H, seed=5)
    q, k, v = case.parts()
    ref = ac.reference(q, k, v, case.do, H)
    assert ref.gap > 150 / ac.LOG2E and ref.gap >= 160.0
    npair = (N + 1) // 2
    for b in range(B):
        for h in range(H):
            assert np.bincount(case.target[b, h], minlength=npair).max() <= 2
            assert case.target[b, h, 0] == npair - 1 and (N < 3 or case.target[b, h, N - 1] == 0)
    assert not np.array_equal(case.target[0, 0], case.target[1, 1])                 # another map per image and head
    hot = (ref.P > 0.25).sum(-1)
    assert int(hot.max()) == 2 and int(hot.min()) == (1 if N % 2 else 2)
    eo, edq, edk, edv, elz = ac.select_expectation(case)
    for name, e, r in (("o", eo, ref.o), ("dq", edq, ref.dq), ("dk", edk, ref.dk), ("dv", edv, ref.dv)):
        assert _is_bf16(e), name
        assert float((torch.from_numpy(e) - r).abs().max()) < 1e-65, name
    assert float((torch.from_numpy(elz) - ref.lse2).abs().max()) < 1e-9
    # dq lives in the spare dims only; dk holds multiples of 4
    dq = edq.reshape(B, N, H, ac.D)
    assert not dq[..., :ac.CODE_DIMS].any() and dq[..., ac.CODE_DIMS:].any()
    assert np.array_equal(edk, 4 * np.round(edk / 4)) and 0 < np.abs(edk).max() <= 256


@pytest.mark.parametrize("N", [33, 197, 300])
def test_selection_survives_the_prescaled_queries_rounding(N):
    """The prescaled and mxfp8 entries get bf16(q c), c = log2 e / 8: 128 c = 23.08 rounds to 23.125, the gap in the exp2 domain
    is 10 * 23.125 = 231 > 150, and the matching exponent 55 * 23.125 = 1271.875 has 14 significant bits: the sum of two bf16."""
    case = ac.selecting(2, N, 2, seed=5)
    q, k, v = case.parts()
    qp = (q.float() * np.float32(ac.SCALE * ac.LOG2E)).to(BF)
    ref = ac.reference(qp, k, v, case.do, 2, ln_scale=np.log(2.0))
    assert ref.gap * ac.LOG2E > 150
    top = float(ref.lse2.max())
    hi = torch.tensor(1271.875).to(BF).float()
    lo = (torch.tensor(1271.875) - hi).to(BF).float()
    assert float(hi + lo) == 1271.875 and abs(top - 1272.875) < 1e-9
    eo = ac.select_expectation(case)[0]
    assert float((torch.from_numpy(eo) - ref.o).abs().max()) < 1e-60


def test_shifted_moves_every_logit_of_a_row_and_nothing_else():
    B, N, H = 2, 197, 2
    base = ac.shifted(B, N, H, 0, seed=3)
    r0 = ac.reference(*base.parts(), base.do, H)
    for t in ac.SHIFTS:
        case = ac.shifted(B, N, H, t, seed=3)
        q, k, v = case.parts()
        assert _is_bf16(q.double()) and float(k[0, 0, 0]) == t / 8.0 and float(q[0, 5, ac.D]) == 64.0
        r = ac.reference(q, k, v, case.do, H)
        assert float((r.lse2 - r0.lse2 - t * ac.LOG2E).abs().max()) < 1e-9
        for a, b in ((r.o, r0.o), (r.dq, r0.dq), (r.dv, r0.dv), (ac.drop_channel0(r.dk, H), ac.drop_channel0(r0.dk, H))):
            assert float((a - b).abs().max()) < 1e-9 * max(1.0, abs(t))
    alt = ac.shifted(B, N, H, -96, seed=3, alternate=True)
    ra = ac.reference(*alt.parts(), alt.do, H)
    d = (ra.lse2 - r0.lse2) / ac.LOG2E
    assert float((d[..., 0::2] + 96).abs().max()) < 1e-9 and float((d[..., 1::2] - 96).abs().max()) < 1e-9


def test_shifted_lse_levels_and_the_padded_key_fault_they_expose():
    """N = 197, D = 64: a shift of -96 puts the log2-domain LSE of all 197 rows at -130 .. -129.6, where exp2f(-L2) is inf in fp32;
    -64 leaves it near -84, finite.  The stand-in of the unmasked backward (a zero-padded key with p = exp2(-L2), multiplied by its
    zero K row) then reports NaN in dq for -96 and none for -64; with the padded probability selected away it reports none."""
    B, N, H = 2, 197, 2
    levels = {}
    for t in (-96, -64):
        case = ac.shifted(B, N, H, t, seed=3)
        q, k, v = case.parts()
        ref = ac.reference(q, k, v, case.do, H)
        levels[t] = (float(ref.lse2.min()), float(ref.lse2.max()))
        with np.errstate(over="ignore"):
            pad_p = torch.exp2(-ref.lse2.float())
        bad = ac.padded_key_backward_standin(q, k, case.do, ref, H, mask=False)
        good = ac.padded_key_backward_standin(q, k, case.do, ref, H, mask=True)
        assert not torch.isnan(good).any() and not good.any()
        if t == -96:
            assert bool(torch.isinf(pad_p).all())
            assert bool(torch.isnan(bad).reshape(B, H, N, -1).all(-1).all())       # every dq element of every row
        else:
            assert bool(torch.isfinite(pad_p).all()) and not torch.isnan(bad).any() and not bad.any()
    assert -131.0 < levels[-96][0] and levels[-96][1] < -128.0, levels
    assert -86.5 < levels[-64][0] and levels[-64][1] < -82.0, levels


def _inside(got, want, bound):
    return float(((got - want).abs() / bound.clamp_min(1e-300)).max())


def test_bounds_hold_for_a_bf16_emulation_and_catch_one_wrong_row():
    """A torch emulation of the bf16 kernels' roundings (P, dS, O to bf16; fp32 elsewhere) stays inside every per-element bound;
    the same result with ONE query row 30 % off - which moves the tensor's relative-L2 by less than the backward's 1.5e-2 gate -
    does not."""
    B, N, H = 2, 300, 2
    case = ac.shifted(B, N, H, -64, seed=11)
    q, k, v = case.parts()
    ref = ac.reference(q, k, v, case.do, H)
    o, dq, dk, dv = ac.emulate_bf16_backward(case, ref)
    bq, bk = ac.dqdk_bounds(ref, q, k, case.do, H)
    bo, bv = ac.fwd_bound_bf16(ref, v, H), ac.dv_bound(ref, case.do, H)
    for name, got, want, bound in (("o", o, ref.o, bo), ("dq", dq, ref.dq, bq), ("dk", dk, ref.dk, bk), ("dv", dv, ref.dv, bv)):
        assert _inside(got, want, bound) <= 1.0, name
    wrong = dq.clone()
    wrong[1, 77] *= 1.3
    assert float((wrong - ref.dq).norm() / ref.dq.norm()) < 1.5e-2
    assert _inside(wrong, ref.dq, bq) > 1.0


def test_what_honest_bf16_arithmetic_does_to_two_of_the_gates():
    """Two places where the emulation - the design's arithmetic with nothing wrong in it - leaves a gate as first written, so the
    GPU tests cannot hold a kernel to it (tests/test_gpu_attention_edges.py says what they do instead):
      * dv at N = 17 exceeds 1.25 (u P^T |dO| + u |dv|) by 1.06: u |x| understates half an ulp of x by up to 2; with the exact
        half-ulp the same result sits at 0.62 of the bound;
      * dq at |t| = 512: channel 0 of dq is 0 in exact arithmetic (k[:, 0] is one constant and sum_j dS_ij = 0), but the kernel
        sums bf16(dS_ij) k_j0 with |k_j0| = 64, i.e. 64 times the rounding errors of dS: 2.2e-2 of |dq|, above the 1.5e-2 tensor
        gate, while dq without that channel is at 2.5e-3."""
    B, H = 2, 2
    case = ac.gaussian(B, 17, H, seed=7)
    ref = ac.reference(*case.parts(), case.do, H)
    dv = ac.emulate_bf16_backward(case, ref)[3]
    assert 1.0 < _inside(dv, ref.dv, ac.dv_bound(ref, case.do, H, exact_half_ulp=False)) < 1.1
    assert _inside(dv, ref.dv, ac.dv_bound(ref, case.do, H)) < 0.7
    for N in (17, 197):
        case = ac.shifted(B, N, H, 512, seed=7)
        ref = ac.reference(*case.parts(), case.do, H)
        dq = ac.emulate_bf16_backward(case, ref)[1]
        assert float(ac.drop_channel0(ref.dq, H).norm() / ref.dq.norm()) > 1 - 1e-12          # channel 0 of the reference is ~0
        assert 1.5e-2 < float((dq - ref.dq).norm() / ref.dq.norm()) < 3e-2
        assert float((ac.drop_channel0(dq, H) - ac.drop_channel0(ref.dq, H)).norm() / ref.dq.norm()) < 4e-3
