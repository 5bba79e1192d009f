"""Inputs that put the LayerNorm kernels at their edges, their float64 reference, the per-element error bounds derived from it and
an fp32 emulation in the kernels' own order.  numpy only: importable without a GPU;
tests/test_layernorm_cases_cpu.py pins every property the GPU tests (tests/test_gpu_layernorm_edges.py) rely on.

Rows (all from layoutdit_amd.synth, every case with a seed of its own):
  exact      every output has ONE correct bit pattern.  Each group of four channels holds (+a, +a, -a, -a) in a permutation drawn
             per row and group, a = 2^k, k per row in -3 .. 3: mu = 0, var = a^2, var + 1e-12 rounds to a^2, rstd = 2^-k, all exact
             in fp32 provided fl32(C) * fl32(1 / C) rounds to 1 (asserted per width; 137 multiples of 4 up to 4096 fail it, none of
             the widths used here).  gamma_c = 2^((c mod 17) - 8) and beta_c = (c - 2048) / 16 differ between a channel and its
             neighbours at every distance a kernel could confuse (1, 4 = the next lane, 256 = the next vector of the lane, 1024), so
             y = fl32(+-gamma + beta).  Backward: gy = dy gamma is (p, -p) on the group's two +a channels and (q, -q) on its two -a
             channels, p, q in +-{1, 2, 3}: sum gy = sum gy xhat = 0 in every order, dx = rstd gy, dh_out = dh + dx with dh an integer
             in -7 .. 7 (a multiple of 1/8 below 32: at most 8 significant bits), dgamma / dbeta integer sums times 1 / gamma_c.
             Fused LayerScale: z integers in -4 .. 4 (bf16), lam_c = 2^((c mod 13) - 6), rowscale in {0, 1, 2} or absent:
             dz = dh_out rs lam is bf16-representable, dlam and dzbias are sums of multiples of 1/8 far below 2^24.
  gaussian   the suite's usual rows: 0.5 + 2 n, row 0 times 50
  offset     1000 + 2 n        (the case the two-pass variance exists for)
  outlier    2 n with one channel at 3000   (BEiT's large-magnitude channels)
  flat       100 + 1e-3 n
  tiny       1e-4 n

Bounds, from the float64 reference of the same fp32 inputs.  u = 2^-24; V = float4 vectors per lane of the instantiation the
launcher picks for C (forward 1 / 4 / 16: layernorm.hip launch_ln; backward 1 / 3 / 4 / 16: train_ops.hip launch_layernorm_bwd_t);
S = 2 + (V - 1) + 6 + 1 additions of a row sum of lane quads plus the 1 / C product; S4 = 4 V + 7 for the element-wise sums:
  dmu   = S u mean|x|                      dd_i = dmu + u |d_i|
  rho   = 1/2 ((S4 + 3) u + 2 mean(dd |d|) / (var + eps)) + 2 u            (rstd's relative error)
  y:      |g_i| rstd dd_i + |g_i d_i rstd| (rho + 3 u) + u |y_i|
  dxh_i = rstd dd_i + |xh_i| (rho + u)
  dm1   = (S4 + 1) u mean|gy|              dm2 = (S4 + 2) u mean|gy xh| + mean(|gy| dxh)
  T_i   = |gy_i| + |m1| + |xh_i m2|
  dh_out: rstd (u |gy_i| + dm1 + |xh_i| dm2 + |m2| dxh_i + 3 u T_i) + (rho + u) rstd T_i + u |dh_out_i|
The 2 u of rho is the reciprocal square root as 1.0f / sqrtf(.), both correctly rounded: confirmed from the compiled objects - every
layernorm_rows / layernorm_bwd_rows instantiation carries the v_div_scale / v_div_fmas / v_div_fixup sequence and the refined
v_sqrt_f32, none a v_rsq_f32 (clang's default for HIP device code, -fhip-fp32-correctly-rounded-divide-sqrt).

Column sums (dgamma, dbeta, dlam, dzbias, dbias): sum_r (the term's own error) + n_add u sum_r |term|, n_add = the additions on the
longest path (n_add() below, read from train_ops.hip):
  layernorm_bwd_rows   a wave adds its rows one after the other (rows_per_wave), the workgroup adds its NWV waves in order from 0
                       (NWV; 8 for the plain form at C <= 1024, otherwise 4), reduce_jobs_kernel adds the P partial rows:
                       P > 16: 16 row groups of ceil(P / 16) rows each, then the 16 groups in order (ceil(P / 16) + 15);
                       P <= 16: four interleaved accumulators, (s0 + s1) + (s2 + s3)  (ceil(P / 4) + 2)
  resid_bwd_tile       the 64 rows of a tile in order (64), then the same second stage over ceil(rows / 64) partial rows
Own errors: dy xh: |dy| dxh + u |dy xh|;  dy: none;  gr = dh_out rs, a = gr lam, gr z: |rs lam| B(dh_out) + 2 u |a| and
|rs z| B(dh_out) + 2 u |gr z| (two fp32 products).  dz = bf16(a): half a bf16 ulp of the reference + |rs lam| B(dh_out) + 2 u |a|
(the last term - 2^-14 of the first - is what the two fp32 products may move a value that sits on a bf16 tie).  dzbias sums the
unrounded a, not the bf16 dz."""
from __future__ import annotations

import types

import numpy as np

from layoutdit_amd import synth

U = 2.0 ** -24
EPS = np.float32(1e-12)
F32, F64 = np.float32, np.float64
KINDS = ("gaussian", "offset", "outlier", "flat", "tiny")
WIDTHS = (4, 64, 192, 256, 260, 384, 512, 768, 772, 1024, 1028, 4096)
MX_WIDTHS = tuple(c for c in WIDTHS if c % 32 == 0) + (288, 1056)
RESID_WIDTHS = tuple(c for c in WIDTHS if c % 64 == 0)


# ---- which instantiation the launchers pick ----------------------------------------------------------------------------------------
def fwd_vpl(C: int) -> int:
    return 1 if C <= 256 else 4 if C <= 1024 else 16


def bwd_vpl(C: int) -> int:
    return 1 if C <= 256 else 3 if C <= 768 else 4 if C <= 1024 else 16


def bwd_grid(rows: int, C: int, fused: bool):
    """(workgroups, waves per workgroup) of layernorm_bwd_rows, as launch_layernorm_bwd_t sets them."""
    if fused and C <= 1024:
        return ((rows + 3) // 4 if rows < 4 * 768 else 768), 4
    return ((rows + 7) // 8 if rows < 8 * 512 else 512), (8 if C <= 1024 else 4)


def _second_stage_adds(P: int) -> int:
    return -(-P // 16) + 15 if P > 16 else -(-P // 4) + 2


def n_add(entry: str, rows: int, C: int) -> int:
    """Additions on the longest path of a column sum.  entry: "bwd", "fused" or "resid"."""
    if entry == "resid":
        return 64 + _second_stage_adds(-(-rows // 64))
    blocks, nwv = bwd_grid(rows, C, entry == "fused")
    return -(-rows // (blocks * nwv)) + nwv + _second_stage_adds(blocks)


def inv_c_is_exact(C: int) -> bool:
    return F32(C) * (F32(1.0) / F32(C)) == F32(1.0)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def _seed(kind: str, rows: int, C: int, what: int) -> int:
    return (synth._stream_of(kind) * 31 + rows * 7919 + C * 104729 + what) & 0x7FFFFFFF


def _n(kind, rows, C, what, shape):
    return synth.normal(_seed(kind, rows, C, what), 17, int(np.prod(shape))).reshape(shape)


def _ints(kind, rows, C, what, shape, lo, hi):
    """integers lo .. hi inclusive"""
    u = synth.uniform01(_seed(kind, rows, C, what), 19, int(np.prod(shape))).reshape(shape)
    return np.minimum(np.floor(u * (hi - lo + 1)), hi - lo).astype(np.int64) + lo


def bf16_round(a: np.ndarray) -> np.ndarray:
    """fp32 values rounded to the nearest bf16 (ties to even), as fp32."""
    b = np.ascontiguousarray(a, F32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(F32).reshape(np.shape(a))


def rows_of(kind: str, rows: int, C: int) -> np.ndarray:
    n = _n(kind, rows, C, 1, (rows, C))
    if kind == "gaussian":
        x = 0.5 + 2.0 * n
        x[0] *= 50.0
    elif kind == "offset":
        x = 1000.0 + 2.0 * n
    elif kind == "outlier":
        x = 2.0 * n
        x[np.arange(rows), _ints(kind, rows, C, 2, (rows,), 0, C - 1)] = 3000.0
    elif kind == "flat":
        x = 100.0 + 1e-3 * n
    elif kind == "tiny":
        x = 1e-4 * n
    else:
        raise ValueError(kind)
    return x.astype(F32)


def case(kind: str, rows: int, C: int, rowscale: bool = True, backward: bool = True):
    """Every operand of the forward, the backward and the fused LayerScale backward for one (kind, rows, C).  z is bf16-exact fp32.
    backward = False: the forward's operands only."""
    if kind == "exact":
        return exact_case(rows, C, rowscale)
    c = types.SimpleNamespace(kind=kind, rows=rows, C=C, exact=False)
    c.x = rows_of(kind, rows, C)
    c.gamma = (1.0 + 0.1 * _n(kind, rows, C, 3, (C,))).astype(F32)
    c.beta = (0.1 * _n(kind, rows, C, 4, (C,))).astype(F32)
    if not backward:
        return c
    c.dy = _n(kind, rows, C, 5, (rows, C)).astype(F32)
    c.dh = _n(kind, rows, C, 6, (rows, C)).astype(F32)
    c.z = bf16_round(_n(kind, rows, C, 7, (rows, C)).astype(F32))
    c.lam = (np.abs(_n(kind, rows, C, 8, (C,))) * 0.3 + 0.05).astype(F32)
    c.rs = ((np.arange(rows) % 3 != 0) / 0.9).astype(F32) if rowscale else None
    return c


def without_rowscale(c):
    """The same case with the stochastic-depth factors absent (the exact case's expectation is made again)."""
    if c.exact:
        return exact_case(c.rows, c.C, False)
    return types.SimpleNamespace(**{**vars(c), "rs": None})


_PATTERNS = np.array([[1, 1, -1, -1], [1, -1, 1, -1], [1, -1, -1, 1], [-1, 1, 1, -1], [-1, 1, -1, 1], [-1, -1, 1, 1]], F64)


def exact_gamma(C):
    return np.ldexp(1.0, (np.arange(C) % 17) - 8).astype(F32)


def exact_beta(C):
    return ((np.arange(C) - 2048) / 16.0).astype(F32)


def exact_lam(C):
    return np.ldexp(1.0, (np.arange(C) % 13) - 6).astype(F32)


def exact_case(rows: int, C: int, rowscale: bool = True):
    """The operands AND the expectation of every output (float64 arrays whose values are fp32- / bf16-representable)."""
    assert C % 4 == 0 and inv_c_is_exact(C), C
    c = types.SimpleNamespace(kind="exact", rows=rows, C=C, exact=True)
    G = C // 4
    k = _ints("exact", rows, C, 1, (rows,), -3, 3)
    a = np.ldexp(1.0, k)[:, None, None]
    sign = _PATTERNS[_ints("exact", rows, C, 2, (rows, G), 0, 5)]                      # [rows, G, 4]
    c.x = (sign * a).reshape(rows, C).astype(F32)
    c.gamma, c.beta, c.lam = exact_gamma(C), exact_beta(C), exact_lam(C)
    # gy: (p, -p) on the two +a channels of a group, in channel order, (q, -q) on the two -a channels
    mag = _ints("exact", rows, C, 3, (rows, G, 2), 1, 3) * (2 * _ints("exact", rows, C, 4, (rows, G, 2), 0, 1) - 1)
    plus = sign > 0
    first = np.where(plus, np.cumsum(plus, -1) == 1, np.cumsum(~plus, -1) == 1)         # the first of its sign inside the group
    gy = np.where(plus, mag[..., :1], mag[..., 1:]) * np.where(first, 1.0, -1.0)
    gy = gy.reshape(rows, C)
    c.dy = (gy / c.gamma.astype(F64)).astype(F32)
    c.dh = _ints("exact", rows, C, 5, (rows, C), -7, 7).astype(F32)
    c.z = _ints("exact", rows, C, 6, (rows, C), -4, 4).astype(F32)
    c.rs = _ints("exact", rows, C, 7, (rows,), 0, 2).astype(F32) if rowscale else None
    # expectations
    g64, xh = c.gamma.astype(F64), sign.reshape(rows, C)
    e = types.SimpleNamespace()
    e.y = (F32(1) * (xh * g64).astype(F32) + c.beta).astype(F64)                         # fl32(+-gamma + beta): ONE fp32 addition
    e.dh_out = c.dh.astype(F64) + gy * np.ldexp(1.0, -k)[:, None]
    e.dgamma = (c.dy.astype(F64) * xh).sum(0)
    e.dbeta = c.dy.astype(F64).sum(0)
    rs = np.ones(rows) if c.rs is None else c.rs.astype(F64)
    gr = e.dh_out * rs[:, None]
    e.dz = gr * c.lam.astype(F64)
    e.dlam = (gr * c.z.astype(F64)).sum(0)
    e.dzbias = e.dz.sum(0)
    c.expect = e
    return c


def exact_resid_case(rows: int, C: int, rowscale: bool = True):
    """ldit_resid_bwd_bf16 on its own: dh multiples of 1/8 up to 10, the other operands as in exact_case."""
    c = types.SimpleNamespace(kind="exact", rows=rows, C=C, exact=True)
    c.dh = (_ints("exact_resid", rows, C, 1, (rows, C), -80, 80) / 8.0).astype(F32)
    c.z = _ints("exact_resid", rows, C, 2, (rows, C), -4, 4).astype(F32)
    c.lam = exact_lam(C)
    c.rs = _ints("exact_resid", rows, C, 3, (rows,), 0, 2).astype(F32) if rowscale else None
    rs = np.ones(rows) if c.rs is None else c.rs.astype(F64)
    gr = c.dh.astype(F64) * rs[:, None]
    c.expect = types.SimpleNamespace(dz=gr * c.lam.astype(F64), dlam=(gr * c.z.astype(F64)).sum(0), dbias=(gr * c.lam.astype(F64)).sum(0))
    return c


# ---- float64 reference --------------------------------------------------------------------------------------------------------------
def reference(c, backward: bool = True, fused: bool = True):
    r = types.SimpleNamespace()
    x, g = c.x.astype(F64), c.gamma.astype(F64)
    r.mu = x.mean(1, keepdims=True)
    r.d = x - r.mu
    r.var = (r.d * r.d).mean(1, keepdims=True)
    r.rstd = 1.0 / np.sqrt(r.var + F64(EPS))
    r.xh = r.d * r.rstd
    r.y = r.xh * g + c.beta.astype(F64)
    r.absx = np.abs(x).mean(1, keepdims=True)
    if not backward:
        return r
    dy = c.dy.astype(F64)
    r.gy = dy * g
    r.m1 = r.gy.mean(1, keepdims=True)
    r.m2 = (r.gy * r.xh).mean(1, keepdims=True)
    r.dh_out = c.dh.astype(F64) + r.rstd * (r.gy - r.m1 - r.xh * r.m2)
    r.dgamma, r.dbeta = (dy * r.xh).sum(0), dy.sum(0)
    if fused:
        r.rs = np.ones((c.rows, 1)) if c.rs is None else c.rs.astype(F64)[:, None]
        r.gr = r.dh_out * r.rs
        r.dz = r.gr * c.lam.astype(F64)
        r.dlam, r.dzbias = (r.gr * c.z.astype(F64)).sum(0), r.dz.sum(0)
    return r


def reference_resid(c):
    r = types.SimpleNamespace()
    r.rs = np.ones((c.rows, 1)) if c.rs is None else c.rs.astype(F64)[:, None]
    r.gr = c.dh.astype(F64) * r.rs
    r.dz = r.gr * c.lam.astype(F64)
    r.dlam, r.dbias = (r.gr * c.z.astype(F64)).sum(0), r.dz.sum(0)
    return r


# ---- bounds -------------------------------------------------------------------------------------------------------------------------
def _stats_bounds(c, r, V):
    S, S4 = 2 + (V - 1) + 6 + 1, 4 * V + 7
    dmu = S * U * r.absx
    dd = dmu + U * np.abs(r.d)
    rho = 0.5 * ((S4 + 3) * U + 2 * (dd * np.abs(r.d)).mean(1, keepdims=True) / (r.var + F64(EPS))) + 2 * U
    return S4, dd, rho


def forward_bound(c, r) -> np.ndarray:
    _, dd, rho = _stats_bounds(c, r, fwd_vpl(c.C))
    g = np.abs(c.gamma.astype(F64))
    return g * r.rstd * dd + np.abs(g * r.d * r.rstd) * (rho + 3 * U) + U * np.abs(r.y)


def backward_bounds(c, r):
    """(bound of dh_out [rows, C], bound of xhat [rows, C])"""
    S4, dd, rho = _stats_bounds(c, r, bwd_vpl(c.C))
    dxh = r.rstd * dd + np.abs(r.xh) * (rho + U)
    agy = np.abs(r.gy)
    dm1 = (S4 + 1) * U * agy.mean(1, keepdims=True)
    dm2 = (S4 + 2) * U * np.abs(r.gy * r.xh).mean(1, keepdims=True) + (agy * dxh).mean(1, keepdims=True)
    T = agy + np.abs(r.m1) + np.abs(r.xh * r.m2)
    b = r.rstd * (U * agy + dm1 + np.abs(r.xh) * dm2 + np.abs(r.m2) * dxh + 3 * U * T) + (rho + U) * r.rstd * T + U * np.abs(r.dh_out)
    return b, dxh


def half_bf16_ulp(a: np.ndarray) -> np.ndarray:
    a = np.abs(np.asarray(a, F64))
    _, E = np.frexp(np.where(a > 0, a, 1.0))
    return np.where(a > 0, np.ldexp(1.0, E - 9), 0.0)


def column_bounds(c, r, entry: str):
    """dict name -> bound, for the column sums (and dz) of entry "bwd", "fused" or "resid"."""
    na = n_add(entry, c.rows, c.C) * U
    out = {}
    if entry == "resid":
        bdh = 0.0
    else:
        bdh, dxh = backward_bounds(c, r)
        dy = np.abs(c.dy.astype(F64))
        t = dy * np.abs(r.xh)
        out["dh_out"] = bdh
        out["dgamma"] = (dy * dxh + U * t).sum(0) + na * t.sum(0)
        out["dbeta"] = na * dy.sum(0)
        if entry == "bwd":
            return out
    rl, rz = np.abs(r.rs * c.lam.astype(F64)), np.abs(r.rs * c.z.astype(F64))
    a, q = np.abs(r.dz), np.abs(r.gr * c.z.astype(F64))
    own_a, own_q = rl * bdh + 2 * U * a, rz * bdh + 2 * U * q
    out["dz"] = half_bf16_ulp(r.dz) + own_a
    out["dlam"] = own_q.sum(0) + na * q.sum(0)
    out["dzbias" if entry == "fused" else "dbias"] = own_a.sum(0) + na * a.sum(0)
    return out


# ---- fp32 emulation in the kernels' own order ----------------------------------------------------------------------------------------
def _fma(a, b, c, fma):
    if fma:
        return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)
    return (np.asarray(a, F32) * np.asarray(b, F32)).astype(F32) + np.asarray(c, F32)


def _lanes(a: np.ndarray):
    """[rows, C] -> [rows, V, 64, 4]: vector idx = lane + 64 u holds channels 4 idx .. 4 idx + 3; zeros past C; and the mask."""
    rows, C = a.shape
    V = -(-C // 256)
    p = np.zeros((rows, V * 256), a.dtype)
    p[:, :C] = a
    m = np.zeros((rows, V * 256), bool)
    m[:, :C] = True
    return p.reshape(rows, V, 64, 4), m.reshape(rows, V, 64, 4)


def _wave_sum(s: np.ndarray) -> np.ndarray:
    """the xor butterfly over the last axis (64 lanes): every lane ends with the same fp32 value"""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[..., lane ^ o]
    return s[..., :1]


def _row_stats(x, fma, mutant):
    """mu, centred row (lane layout), rstd and the mask: sums of lane quads, two-pass variance, element by element."""
    C = x.shape[1]
    v, mask = _lanes(x)
    inv_c = F32(1.0) / F32(C)
    s = np.zeros(v.shape[:1] + (64,), F32)
    for u in range(v.shape[1]):
        quad = (v[:, u, :, 0] + v[:, u, :, 1]) + (v[:, u, :, 2] + v[:, u, :, 3])
        if mutant == "drop_lane" and u == 0:
            quad = quad.copy()
            quad[:, 0] = 0                                    # one lane's vector never reaches the row sum
        s = s + quad
    mu = (_wave_sum(s) * inv_c)[:, None, :, None]                # [rows, 1, 1, 1]
    d = np.where(mask, v - mu, F32(0))
    q = np.zeros_like(s)
    if mutant == "var_e2":                                    # E[x^2] - mu^2 with the same sums
        for u in range(v.shape[1]):
            for e in range(4):
                q = _fma(v[:, u, :, e], v[:, u, :, e], q, fma)
        var = _wave_sum(q) * inv_c - (mu * mu).reshape(-1, 1)
    else:
        for u in range(v.shape[1]):
            for e in range(4):
                q = _fma(d[:, u, :, e], d[:, u, :, e], q, fma)
        var = _wave_sum(q) * inv_c
    rstd = (F32(1.0) / np.sqrt((var + EPS).astype(F32))).astype(F32)
    return d, rstd[:, None, :, None], mask, inv_c


def _unlane(a, C):
    return a.reshape(a.shape[0], -1)[:, :C]


def _shift_gamma(g):
    return np.roll(g, -4 if g.size > 4 else -1)                 # channel c reads gamma of c + 4 (c + 1 inside a single vector)


def emulate_forward(c, fma: bool = True, mutant: str = None) -> np.ndarray:
    d, rstd, mask, _ = _row_stats(c.x, fma, mutant)
    g = _shift_gamma(c.gamma) if mutant == "gamma_shift" else c.gamma
    gl, bl = _lanes(g[None, :])[0], _lanes(c.beta[None, :])[0]
    return _unlane(_fma(d * rstd, gl, bl, fma), c.C)


def _wave_column_sums(term: np.ndarray, rows: int, blocks: int, nwv: int) -> np.ndarray:
    """[rows, C] -> [blocks, C]: wave w of workgroup b adds rows b nwv + w, + blocks nwv, ... in order; the workgroup adds its waves
    in order from 0."""
    C = term.shape[1]
    per = blocks * nwv
    K = -(-rows // per)
    p = np.zeros((K * per, C), F32)
    p[:rows] = term
    p = p.reshape(K, blocks, nwv, C)
    acc = np.zeros((blocks, nwv, C), F32)
    for k in range(K):
        acc = acc + p[k]
    out = np.zeros((blocks, C), F32)
    for w in range(nwv):
        out = out + acc[:, w]
    return out


def second_stage(part: np.ndarray) -> np.ndarray:
    """reduce_jobs_kernel over the P partial rows of one vector."""
    P = part.shape[0]
    if P > 16:
        groups = []
        for rg in range(16):
            s = np.zeros(part.shape[1], F32)
            for q in range(rg, P, 16):
                s = s + part[q]
            groups.append(s)
        t = groups[0]
        for g in groups[1:]:
            t = t + g
        return t
    s = [np.zeros(part.shape[1], F32) for _ in range(4)]
    for q in range(P):
        s[q % 4] = s[q % 4] + part[q]
    return (s[0] + s[1]) + (s[2] + s[3])


def emulate_backward(c, fused: bool, fma: bool = True, mutant: str = None):
    """dict of dh_out, dgamma, dbeta (+ dz (fp32 values rounded to bf16), dlam, dzbias when fused)."""
    rows, C = c.x.shape
    d, rstd, mask, inv_c = _row_stats(c.x, fma, mutant)
    g = _shift_gamma(c.gamma) if mutant == "gamma_shift" else c.gamma
    gl = _lanes(g[None, :])[0]
    dy, _ = _lanes(c.dy)
    xh = (d * rstd).astype(F32)
    gy = (dy * gl).astype(F32)
    s1 = np.zeros((rows, 64), F32)
    s2 = np.zeros((rows, 64), F32)
    for u in range(xh.shape[1]):
        for e in range(4):
            s1 = s1 + gy[:, u, :, e]
            s2 = _fma(gy[:, u, :, e], xh[:, u, :, e], s2, fma)
    m1 = (_wave_sum(s1) * inv_c)[:, None, :, None]
    m2 = _wave_sum(s2)
    m2 = (m2 if mutant == "m2_no_inv_c" else m2 * inv_c)[:, None, :, None]
    t = _fma(-xh, m2, _fma(dy, gl, -m1, fma), fma)
    out = {"dh_out": _unlane(_fma(rstd, t, _lanes(c.dh)[0], fma), C)}
    blocks, nwv = bwd_grid(rows, C, fused)
    tg = _unlane((dy * xh).astype(F32), C)                                 # sg += d * xh: the sum's own rounding is in the addition
    part_g = _wave_column_sums(tg, rows, blocks, nwv)
    if mutant == "dgamma_last_row":
        part_g = _wave_column_sums(np.concatenate([tg[:-1], np.zeros_like(tg[:1])]), rows, blocks, nwv)
    out["dgamma"] = second_stage(part_g)
    out["dbeta"] = second_stage(_wave_column_sums(c.dy, rows, blocks, nwv))
    if fused:
        rs = np.ones((rows, 1), F32) if c.rs is None else c.rs[:, None]
        gr = (out["dh_out"] * rs).astype(F32)
        a = (gr * c.lam[None, :]).astype(F32)
        out["dz"] = bf16_round(a)
        out["dzbias"] = second_stage(_wave_column_sums(a, rows, blocks, nwv))
        out["dlam"] = second_stage(_wave_column_sums((gr * c.z).astype(F32), rows, blocks, nwv))
    return out


def emulate_resid(c):
    """resid_bwd_tile + reduce_jobs_kernel: dz, dlam, dbias."""
    rows, C = c.dh.shape
    rs = np.ones((rows, 1), F32) if c.rs is None else c.rs[:, None]
    gr = (c.dh * rs).astype(F32)
    a, q = (gr * c.lam[None, :]).astype(F32), (gr * c.z).astype(F32)
    P = -(-rows // 64)

    def tiles(t):
        p = np.zeros((P * 64, C), F32)
        p[:rows] = t
        p = p.reshape(P, 64, C)
        s = np.zeros((P, C), F32)
        for r_ in range(64):
            s = s + p[:, r_]
        return s
    return {"dz": bf16_round(a), "dbias": second_stage(tiles(a)), "dlam": second_stage(tiles(q))}
