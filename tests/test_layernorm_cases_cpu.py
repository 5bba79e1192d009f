"""CPU pin of tests/layernorm_cases.py (no GPU): the exact rows are exact, the fp32 emulation in the kernels' own order sits inside
every bound, and the bounds are not vacuous - five deliberately wrong emulations are caught at every width."""
import numpy as np
import pytest

from layoutdit_amd import _lib
from tests import layernorm_cases as lc

F32, F64 = np.float32, np.float64
ALL_WIDTHS = tuple(sorted(set(lc.WIDTHS + lc.MX_WIDTHS)))
ROWS = 137          # 18 / 35 partial rows: the tall second stage with a ragged tail; a fused wave of C > 1024 walks a second row


def _ratio(got, ref, bound):
    err = np.abs(np.asarray(got, F64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.nan_to_num(r, nan=np.inf).max())


def test_one_over_c_is_exact_at_every_width_used():
    bad = [C for C in range(4, 4097, 4) if not lc.inv_c_is_exact(C)]
    assert len(bad) == 137 and bad[:2] == [164, 188]
    assert not set(bad) & set(ALL_WIDTHS)
    for C in ALL_WIDTHS:                    # and with the product, the sum and eps in ONE rounding (an fma), for every a = 2^k
        for k in range(-3, 4):
            a2 = 4.0 ** k
            assert F32(F64(C) * a2 * F64(F32(1.0) / F32(C)) + 1e-12) == F32(a2), (C, k)
            assert F32(F32(a2) + lc.EPS) == F32(a2)


@pytest.mark.parametrize("C", ALL_WIDTHS)
@pytest.mark.parametrize("rowscale", [True, False])
def test_exact_rows_are_exact(C, rowscale):
    c = lc.exact_case(ROWS, C, rowscale)
    e = c.expect
    x, g, dy = c.x.astype(F64), c.gamma.astype(F64), c.dy.astype(F64)
    # float64: the claims of the construction
    a = np.abs(x[:, :1])
    assert np.array_equal(np.abs(x), np.broadcast_to(a, x.shape)) and set(np.log2(a).ravel()) <= set(range(-3, 4))
    quads = x.reshape(ROWS, -1, 4)
    assert not quads.sum(-1).any() and not ((quads[..., 0] + quads[..., 1]) + (quads[..., 2] + quads[..., 3])).any()    # mu = 0 in any order
    assert np.array_equal((x * x).mean(1, keepdims=True), a * a)                       # var = a^2
    xh, gy = np.sign(x), dy * g
    assert set(np.abs(gy).ravel()) <= {1.0, 2.0, 3.0}
    assert not gy.reshape(ROWS, -1, 4).sum(-1).any() and not (gy * xh).reshape(ROWS, -1, 4).sum(-1).any()      # m1 = m2 = 0, group by group
    assert np.array_equal(e.dh_out, c.dh.astype(F64) + gy / a)
    for name in ("y", "dh_out", "dgamma", "dbeta", "dlam", "dzbias"):                  # every expectation is an fp32 value
        v = getattr(e, name)
        assert np.array_equal(v.astype(F32).astype(F64), v), name
    assert np.array_equal(lc.bf16_round(e.dz.astype(F32)).astype(F64), e.dz)           # dz is a bf16 value
    assert np.array_equal(lc.bf16_round(c.z), c.z)
    # every partial sum of a column is an integer multiple of the column's unit below 2^24: exact in any order
    for term, unit in ((dy * xh, 1 / g), (dy, 1 / g), (e.dz, c.lam.astype(F64) / 8), (e.dz / c.lam.astype(F64) * c.z, 1 / 8)):
        n = np.abs(term / unit)
        assert np.array_equal(n, np.round(n)) and float(n.sum(0).max()) < 2 ** 24
    for d in (1, 4, 256, 1024):                                                      # neighbours never share gamma, beta or lambda
        if d < C:
            assert not (c.gamma[d:] == c.gamma[:-d]).any() and not (c.beta[d:] == c.beta[:-d]).any() and not (c.lam[d:] == c.lam[:-d]).any()
    # fp32 emulation, contracted and not: the expectation bit for bit
    for fma in (True, False):
        assert np.array_equal(lc.emulate_forward(c, fma).astype(F64), e.y)
        for fused in (False, True):
            got = lc.emulate_backward(c, fused, fma)
            for name, v in got.items():
                assert np.array_equal(v.astype(F64), getattr(e, name)), (name, fma, fused)
    if C % 64 == 0:
        r = lc.exact_resid_case(ROWS, C, rowscale)
        got = lc.emulate_resid(r)
        for name, v in got.items():
            assert np.array_equal(v.astype(F64), getattr(r.expect, name)), name
        assert np.array_equal(lc.bf16_round(r.expect.dz.astype(F32)).astype(F64), r.expect.dz)


def _ratios(c, fma):
    ref = lc.reference(c)
    out = {"y": _ratio(lc.emulate_forward(c, fma), ref.y, lc.forward_bound(c, ref))}
    for entry in ("bwd", "fused"):
        got, b = lc.emulate_backward(c, entry == "fused", fma), lc.column_bounds(c, ref, entry)
        for name, v in got.items():
            out[f"{entry}/{name}"] = _ratio(v, getattr(ref, name), b[name])
    return out


@pytest.mark.parametrize("C", ALL_WIDTHS)
@pytest.mark.parametrize("kind", lc.KINDS)
def test_the_emulation_sits_inside_every_bound(kind, C):
    worst = {}
    for rows, rowscale in ((ROWS, True), (5, False)):
        c = lc.case(kind, rows, C, rowscale)
        for fma in (True, False):
            for k, v in _ratios(c, fma).items():
                worst[k] = max(worst.get(k, 0.0), v)
        if C % 64 == 0:
            ref = lc.reference_resid(c)
            got, b = lc.emulate_resid(c), lc.column_bounds(c, ref, "resid")
            for name, v in got.items():
                worst[f"resid/{name}"] = max(worst.get(f"resid/{name}", 0.0), _ratio(v, getattr(ref, name), b[name]))
    print(f"{kind} C={C}: " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("rows,C,fused", [(4099, 64, False), (3075, 64, True)])
def test_column_sums_when_a_wave_walks_a_second_row(rows, C, fused):
    for kind in ("gaussian", "exact"):
        c = lc.case(kind, rows, C)
        got = lc.emulate_backward(c, fused)
        if kind == "exact":
            for name, v in got.items():
                assert np.array_equal(v.astype(F64), getattr(c.expect, name)), name
            continue
        ref = lc.reference(c)
        b = lc.column_bounds(c, ref, "fused" if fused else "bwd")
        r = {name: _ratio(v, getattr(ref, name), b[name]) for name, v in got.items()}
        print(rows, C, fused, r)
        assert max(r.values()) <= 1.0, r
    blocks, nwv = lc.bwd_grid(rows, C, fused)
    assert rows > blocks * nwv


@pytest.mark.parametrize("C", ALL_WIDTHS)
def test_the_bounds_catch_five_wrong_kernels(C):
    """Not vacuous: each deliberately wrong emulation exceeds a bound or breaks exactness, at every width."""
    off, gau, ex = lc.case("offset", ROWS, C), lc.case("gaussian", ROWS, C), lc.exact_case(ROWS, C)
    roff, rgau = lc.reference(off), lc.reference(gau)
    # variance as E[x^2] - mu^2: cancels at mean 1000
    assert _ratio(lc.emulate_forward(off, mutant="var_e2"), roff.y, lc.forward_bound(off, roff)) > 1.0
    assert _ratio(lc.emulate_backward(off, False, mutant="var_e2")["dh_out"], roff.dh_out, lc.backward_bounds(off, roff)[0]) > 1.0
    # one lane's vector dropped from the row sum
    assert _ratio(lc.emulate_forward(off, mutant="drop_lane"), roff.y, lc.forward_bound(off, roff)) > 1.0
    assert _ratio(lc.emulate_backward(off, True, mutant="drop_lane")["dh_out"], roff.dh_out, lc.backward_bounds(off, roff)[0]) > 1.0
    # gamma of channel c + 4 used for channel c
    assert not np.array_equal(lc.emulate_forward(ex, mutant="gamma_shift").astype(F64), ex.expect.y)
    assert not np.array_equal(lc.emulate_backward(ex, True, mutant="gamma_shift")["dh_out"].astype(F64), ex.expect.dh_out)
    assert _ratio(lc.emulate_forward(gau, mutant="gamma_shift"), rgau.y, lc.forward_bound(gau, rgau)) > 1.0
    # dgamma missing its last row
    assert not np.array_equal(lc.emulate_backward(ex, False, mutant="dgamma_last_row")["dgamma"].astype(F64), ex.expect.dgamma)
    assert _ratio(lc.emulate_backward(gau, False, mutant="dgamma_last_row")["dgamma"], rgau.dgamma, lc.column_bounds(gau, rgau, "bwd")["dgamma"]) > 1.0
    # m2 without the 1 / C
    assert _ratio(lc.emulate_backward(gau, False, mutant="m2_no_inv_c")["dh_out"], rgau.dh_out, lc.backward_bounds(gau, rgau)[0]) > 1.0
    # and the unmutated emulation passes the same checks
    assert _ratio(lc.emulate_forward(off), roff.y, lc.forward_bound(off, roff)) <= 1.0
    assert np.array_equal(lc.emulate_backward(ex, True)["dgamma"].astype(F64), ex.expect.dgamma)


def test_new_entries_size_their_scratch_and_refuse_bad_arguments_on_the_host():
    """ldit_layernorm_bwd_resid_f32 / ldit_resid_bwd_bf16: the partial rows the launchers write fit the scratch the sizing functions
    ask for, and every refusal happens before a launch (the pointers below are aligned numbers, nothing is dereferenced)."""
    lib = _lib.load()
    for rows, C in ((1, 64), (137, 192), (3075, 768), (4099, 1280), (20000, 4096)):
        blocks, _ = lc.bwd_grid(rows, C, True)
        assert lib.ldit_layernorm_bwd_resid_scratch_bytes(rows, C) == 4 * blocks * C * 4
        assert lib.ldit_resid_bwd_scratch_bytes(rows, C) == 2 * -(-rows // 64) * C * 4
    assert lib.ldit_layernorm_bwd_resid_scratch_bytes(0, 64) == 0 and lib.ldit_resid_bwd_scratch_bytes(5, 0) == 0
    p, n = 4096, 1 << 30
    err = lambda: lib.ldit_last_error().decode()                                                    # noqa: E731
    assert lib.ldit_layernorm_bwd_resid_f32(p, p, p, p, p, None, p, p, 4, 64, 1e-12, p, p, p, p, p, 16, None) == _lib.LDIT_EWORKSPACE
    assert lib.ldit_layernorm_bwd_resid_f32(p, p, p, p, p, None, p, p, 4, 8192, 1e-12, p, p, p, p, p, n, None) == _lib.LDIT_EINVAL
    assert lib.ldit_layernorm_bwd_resid_f32(p, p, p, p, p, None, p, p, 4, 66, 1e-12, p, p, p, p, p, n, None) == _lib.LDIT_EUNSUPPORTED
    assert "multiple of 4" in err()
    assert lib.ldit_layernorm_bwd_resid_f32(p, p, p, None, p, None, p, p, 4, 64, 1e-12, p, p, p, p, p, n, None) == _lib.LDIT_EINVAL
    assert lib.ldit_layernorm_bwd_resid_f32(p, p, p, p, p, None, p, p + 2, 4, 64, 1e-12, p, p, p, p, p, n, None) == _lib.LDIT_EINVAL
    assert lib.ldit_layernorm_bwd_resid_f32(p + 4, p, p, p, p, None, p, p, 4, 64, 1e-12, p, p, p, p, p, n, None) == _lib.LDIT_EINVAL
    assert "16-byte" in err()
    assert lib.ldit_layernorm_bwd_resid_f32(p, p, p, p, p, None, p, p, 4, 64, 1e-12, p, None, p, p, p, n, None) == _lib.LDIT_EINVAL
    assert lib.ldit_resid_bwd_bf16(p, p, p, None, p, 4, 96, p, p, p, n, None) == _lib.LDIT_EUNSUPPORTED and "multiple of 64" in err()
    assert lib.ldit_resid_bwd_bf16(p, p, p, None, p, 4, 64, p, p, p, 16, None) == _lib.LDIT_EWORKSPACE
    assert lib.ldit_resid_bwd_bf16(p, None, p, None, p, 4, 64, p, p, p, n, None) == _lib.LDIT_EINVAL
    assert lib.ldit_resid_bwd_bf16(p, p, p + 4, None, p, 4, 64, p, p, p, n, None) == _lib.LDIT_EINVAL and "aligned" in err()
    assert lib.ldit_resid_bwd_bf16(p, p, p, None, p, 0, 64, p, p, p, n, None) == _lib.LDIT_EINVAL
