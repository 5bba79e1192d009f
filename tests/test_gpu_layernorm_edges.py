"""Every LayerNorm entry point at its edges, against float64 on the same fp32 operands and against exact
expectations - never against another kernel of this library.

  forward    ldit_layernorm_f32, ldit_layernorm_f32_planes (2 / 3 planes), ldit_layernorm_mxfp8, ldit_layernorm_mxfp8_train
  backward   ldit_layernorm_bwd_f32, ldit_layernorm_bwd_resid_f32 (with and without rowscale), ldit_resid_bwd_bf16

Inputs, bounds and the count of additions behind every column-sum bound: tests/layernorm_cases.py, pinned on the CPU by
tests/test_layernorm_cases_cpu.py (the fp32 emulation there stays below 0.35 of the forward bound, 0.95 of dh_out's; dz reaches its
bound, which is half a bf16 ulp).  The reciprocal square root is taken as 2 u: division and square root are correctly rounded in the
compiled kernels (read from the device assembly, see that module's docstring).
  exact rows     bit equality: fp32 outputs as values, planes = the split of the exact y, MX codes and scales = the host pack of the
                 exact y, Yd = the dequantised codes, dz as bf16 values
  other kinds    finite, every element inside its bound; on `gaussian` the suite's tensor gates too (1e-5 max-rel forward, 2e-5
                 relative-L2 backward); planes: their sum inside the forward bound + 2^-17 |y| (2) / 2^-24 |y| (3); MX: the interval
                 check of tests/mx_checks.py with the interval y_ref +- bound
Widths and rows are paired so that each instantiation (forward 1 / 4 / 4 with two rows per wave / 16 vectors per lane; backward
1 / 3 / 4 / 16, plain and fused) meets each row regime once: 1; 3 (fewer rows than waves); 5, 33; 130 / 137 (17 / 18 partial rows of the
plain backward: the tall reduction's ragged tail); 1145; 3075 (a fused wave walks a second row); 4099 (a plain wave does); 8193
(forward: two rows per wave, ragged last wave).  Cases above 600k elements run the exact, gaussian and offset rows only.
The worst observed ratio to every bound is written to layernorm_edges.json in the directory tests/test_gpu_split_fp32.py records
its margins in."""
import functools
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from layoutdit_amd import _lib                                        # noqa: E402
from tests import layernorm_cases as lc                              # noqa: E402
from tests.mx_checks import check_mx_pack                            # noqa: E402
from tests.test_gpu_split_fp32 import OUT                             # noqa: E402  (the suite's directory for measured margins)
from tests.util import max_rel, rel_l2                                # noqa: E402

DEV = "cuda:0"
BF = torch.bfloat16
EPS = 1e-12
MARGINS = {}

FWD_CASES = [(1, 4), (3, 64), (5, 192), (33, 256), (130, 64), (137, 192), (1145, 256), (3075, 4), (4099, 64),                       # 1 vector
             (1, 260), (3, 384), (5, 512), (33, 768), (130, 772), (137, 1024), (1145, 384), (3075, 260), (4099, 512),               # 4 vectors
             (8193, 260), (8193, 768),                                                                                           # two rows per wave
             (1, 1028), (3, 4096), (5, 1028), (33, 4096), (130, 1028), (137, 4096), (1145, 1028), (3075, 1028), (4099, 1028)]      # 16 vectors
MX_CASES = [(r, c) for r, c in FWD_CASES if c % 32 == 0] + [(5, 288), (137, 288), (8193, 288), (33, 1056), (1145, 1056)]
BWD_CASES = [(1, 4), (3, 64), (5, 192), (33, 256), (130, 64), (137, 192), (1145, 256), (3075, 64), (4099, 64),                      # 1 vector
             (1, 260), (3, 384), (5, 512), (33, 768), (130, 384), (137, 512), (1145, 768), (3075, 260), (4099, 384),                # 3 vectors
             (1, 772), (3, 1024), (5, 772), (33, 1024), (130, 772), (137, 1024), (1145, 772), (3075, 1024), (4099, 772),            # 4 vectors
             (1, 1028), (3, 4096), (5, 1028), (33, 4096), (130, 1028), (137, 4096), (1145, 1028), (3075, 1028), (4099, 1028)]      # 16 vectors
RESID_CASES = [(1, 64), (3, 192), (5, 256), (33, 384), (130, 512), (137, 768), (1145, 1024), (3075, 64), (65, 4096), (4099, 192)]
_id = lambda rc: f"rows{rc[0]}-C{rc[1]}"                               # noqa: E731


@pytest.fixture(scope="module", autouse=True)
def _record_margins():
    assert torch.cuda.is_available(), "gpu-marked test running without a GPU"
    _lib.load()
    yield
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "layernorm_edges.json"), "w") as f:
        json.dump(dict(sorted(MARGINS.items())), f, indent=1)


def _kinds(rows, C):
    return ("exact",) + (lc.KINDS if rows * C <= 600_000 else ("gaussian", "offset"))


@functools.lru_cache(maxsize=8)
def _case(kind, rows, C, backward=True):
    """computed once, shared between the tests of a shape, never modified"""
    return lc.case(kind, rows, C, True, backward)


def _s():
    return torch.cuda.current_stream().cuda_stream


def _d(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _p(t):
    return None if t is None else t.data_ptr()


def _nan(shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _np(t):
    return t.float().cpu().numpy().astype(np.float64)


def _inside(name, got, ref, bound):
    """finite and every element inside its bound; the worst ratio is printed and recorded before anything is asserted"""
    finite = bool(np.isfinite(got).all())
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float(np.nan_to_num(np.where(err == 0, 0.0, err / bound), nan=np.inf).max())
    print(f"{name}: finite {finite}  worst element / bound {ratio:.3f}")
    if finite:
        MARGINS[name] = max(MARGINS.get(name, 0.0), ratio)
    assert finite, f"{name}: non-finite values in {int((~np.isfinite(got)).reshape(got.shape[0], -1).any(-1).sum())} rows / columns"
    assert ratio <= 1.0, (name, ratio)


def _same(name, got, expect):
    bad = got != expect
    assert not bool(bad.any()), (name, int(bad.sum()), "elements differ; first:", got[bad][:4].tolist(), expect[bad][:4].tolist())


def _split(y32: torch.Tensor, planes: int) -> torch.Tensor:
    """p0 = bf16(y), p1 = bf16(y - p0), ... side by side (y - p0 is exact in fp32)"""
    out, r = [], y32.clone()
    for _ in range(planes):
        p = r.to(BF)
        out.append(p)
        r = r - p.float()
    return torch.cat(out, dim=1)


# ================================================================================================================ forward
@pytest.mark.parametrize("rows,C", FWD_CASES, ids=map(_id, FWD_CASES))
def test_forward_f32_and_planes(rows, C):
    lib = _lib.load()
    for kind in _kinds(rows, C):
        c = _case(kind, rows, C, False)
        x, g, b = _d(c.x), _d(c.gamma), _d(c.beta)
        y = _nan((rows, C))
        _lib.check(lib.ldit_layernorm_f32(_p(x), _p(g), _p(b), _p(y), rows, C, EPS, _s()))
        yp = {}
        for planes in (2, 3):
            yp[planes] = _nan((rows, planes * C), BF)
            _lib.check(lib.ldit_layernorm_f32_planes(_p(x), _p(g), _p(b), _p(yp[planes]), rows, C, EPS, planes, _s()))
        torch.cuda.synchronize()
        tag = f"{kind}/V{lc.fwd_vpl(C)}{'x2' if rows >= 8192 and 256 < C <= 1024 else ''}"
        if c.exact:
            _same(f"f32 y {rows}x{C}", _np(y), c.expect.y)
            y32 = torch.from_numpy(c.expect.y.astype(np.float32))
            for planes in (2, 3):
                assert torch.equal(yp[planes].cpu(), _split(y32, planes)), (planes, rows, C)
            continue
        ref = lc.reference(c, backward=False)
        bound = lc.forward_bound(c, ref)
        _inside(f"f32/y/{tag}", _np(y), ref.y, bound)
        if kind == "gaussian":
            mr = max_rel(_np(y), ref.y)
            print(f"f32 y {rows}x{C}: max-rel {mr:.3e} (gate 1e-5)")
            MARGINS["f32/y/gaussian/max_rel_over_gate"] = max(MARGINS.get("f32/y/gaussian/max_rel_over_gate", 0.0), mr / 1e-5)
            assert mr < 1e-5
        for planes, rep in ((2, 2.0 ** -17), (3, 2.0 ** -24)):
            got = sum(_np(yp[planes][:, s * C:(s + 1) * C]) for s in range(planes))
            _inside(f"planes{planes}/y/{tag}", got, ref.y, bound + rep * np.abs(ref.y))


@pytest.mark.parametrize("rows,C", MX_CASES, ids=map(_id, MX_CASES))
def test_forward_mxfp8(rows, C):
    lib = _lib.load()
    for kind in _kinds(rows, C):
        c = _case(kind, rows, C, False)
        x, g, b = _d(c.x), _d(c.gamma), _d(c.beta)
        outs = {}
        for train in (False, True):
            codes = torch.full((rows, C), 0xFF, dtype=torch.uint8, device=DEV)
            scales = torch.full((rows, C // 32), 0xFF, dtype=torch.uint8, device=DEV)
            yd = _nan((rows, C), BF) if train else None
            if train:
                _lib.check(lib.ldit_layernorm_mxfp8_train(_p(x), _p(g), _p(b), _p(codes), _p(scales), _p(yd), rows, C, EPS, _s()))
            else:
                _lib.check(lib.ldit_layernorm_mxfp8(_p(x), _p(g), _p(b), _p(codes), _p(scales), rows, C, EPS, _s()))
            outs[train] = (codes, scales, yd)
        torch.cuda.synchronize()
        if c.exact:
            center, half = c.expect.y, None
        else:
            ref = lc.reference(c, backward=False)
            center, half = ref.y, lc.forward_bound(c, ref)
        for train, (codes, scales, yd) in outs.items():
            cn, sn = codes.cpu().numpy(), scales.cpu().numpy()
            assert not (sn == 0xFF).any(), "a block scale was not written"
            name = f"mxfp8{'_train' if train else ''}/{kind}/V{lc.fwd_vpl(C)}"
            check_mx_pack(name, cn, sn, center, None if yd is None else _np(yd), c.exact, MARGINS, half=half)
        assert torch.equal(outs[False][0], outs[True][0]) and torch.equal(outs[False][1], outs[True][1])


# ================================================================================================================ backward
def _gauss_gate(name, got, ref):
    e = rel_l2(got, ref)
    print(f"{name}: rel-L2 {e:.3e} (gate 2e-5)")
    MARGINS[name + "/rel_l2_over_gate"] = max(MARGINS.get(name + "/rel_l2_over_gate", 0.0), e / 2e-5)
    assert e < 2e-5, (name, e)


def _check_outputs(entry, tag, c, got, names):
    if c.exact:
        for n in names:
            _same(f"{entry} {n} {c.rows}x{c.C}", got[n], getattr(c.expect, n))
        return
    ref = lc.reference(c) if entry != "resid" else lc.reference_resid(c)
    bounds = lc.column_bounds(c, ref, entry)
    for n in names:
        _inside(f"{entry}/{n}/{tag}", got[n], getattr(ref, n), bounds[n])
        if c.kind == "gaussian" and n != "dz" and entry != "resid":
            _gauss_gate(f"{entry}/{n}/gaussian", got[n], getattr(ref, n))


@pytest.mark.parametrize("rows,C", BWD_CASES, ids=map(_id, BWD_CASES))
def test_backward_plain(rows, C):
    lib = _lib.load()
    need = int(lib.ldit_layernorm_bwd_scratch_bytes(rows, C))
    for kind in _kinds(rows, C):
        c = _case(kind, rows, C)
        dy, x, g, dh = _d(c.dy), _d(c.x), _d(c.gamma), _d(c.dh)
        dg, db = _nan((C,)), _nan((C,))
        scratch = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
        _lib.check(lib.ldit_layernorm_bwd_f32(_p(dy), _p(x), _p(g), _p(dh), rows, C, EPS, _p(dg), _p(db), _p(scratch), need, _s()))
        torch.cuda.synchronize()
        _check_outputs("bwd", f"{kind}/V{lc.bwd_vpl(C)}", c, {"dh_out": _np(dh), "dgamma": _np(dg), "dbeta": _np(db)},
                       ("dh_out", "dgamma", "dbeta"))


@pytest.mark.parametrize("rows,C", BWD_CASES, ids=map(_id, BWD_CASES))
@pytest.mark.parametrize("rowscale", [True, False], ids=["rowscale", "no-rowscale"])
def test_backward_fused_layerscale(rows, C, rowscale):
    lib = _lib.load()
    need = int(lib.ldit_layernorm_bwd_resid_scratch_bytes(rows, C))
    for kind in _kinds(rows, C):
        c = _case(kind, rows, C) if rowscale else lc.without_rowscale(_case(kind, rows, C))
        dy, x, g, dh = _d(c.dy), _d(c.x), _d(c.gamma), _d(c.dh)
        z, lam, rs = _d(c.z, BF), _d(c.lam), None if c.rs is None else _d(c.rs)
        dz = _nan((rows, C), BF)
        vec = {n: _nan((C,)) for n in ("dgamma", "dbeta", "dlam", "dzbias")}
        scratch = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
        _lib.check(lib.ldit_layernorm_bwd_resid_f32(_p(dy), _p(x), _p(g), _p(z), _p(lam), _p(rs), _p(dh), _p(dz), rows, C, EPS,
                                                    _p(vec["dgamma"]), _p(vec["dbeta"]), _p(vec["dlam"]), _p(vec["dzbias"]),
                                                    _p(scratch), need, _s()))
        torch.cuda.synchronize()
        got = {"dh_out": _np(dh), "dz": _np(dz), **{n: _np(v) for n, v in vec.items()}}
        _check_outputs("fused", f"{kind}/V{lc.bwd_vpl(C)}", c, got, ("dh_out", "dgamma", "dbeta", "dz", "dlam", "dzbias"))


@pytest.mark.parametrize("rows,C", RESID_CASES, ids=map(_id, RESID_CASES))
@pytest.mark.parametrize("rowscale", [True, False], ids=["rowscale", "no-rowscale"])
def test_resid_backward(rows, C, rowscale):
    lib = _lib.load()
    need = int(lib.ldit_resid_bwd_scratch_bytes(rows, C))
    for kind in _kinds(rows, C):
        c = lc.exact_resid_case(rows, C, rowscale) if kind == "exact" else _case(kind, rows, C)
        c = c if rowscale or c.exact else lc.without_rowscale(c)
        dh, z, lam, rs = _d(c.dh), _d(c.z, BF), _d(c.lam), None if c.rs is None else _d(c.rs)
        dz, dlam, dbias = _nan((rows, C), BF), _nan((C,)), _nan((C,))
        scratch = torch.full((need,), 0xFF, dtype=torch.uint8, device=DEV)
        _lib.check(lib.ldit_resid_bwd_bf16(_p(dh), _p(z), _p(lam), _p(rs), _p(dz), rows, C, _p(dlam), _p(dbias), _p(scratch), need, _s()))
        torch.cuda.synchronize()
        assert torch.equal(dh.cpu(), torch.from_numpy(c.dh)), "dh is an input"
        _check_outputs("resid", kind, c, {"dz": _np(dz), "dlam": _np(dlam), "dbias": _np(dbias)}, ("dz", "dlam", "dbias"))
