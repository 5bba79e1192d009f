"""Inputs that put the attention kernels at softmax's edges, their float64 reference and the error bounds derived from it
(DESIGN.md section 26).  numpy + CPU torch only: importable without a GPU; tests/test_attention_cases_cpu.py pins the properties
the GPU tests (tests/test_gpu_attention_edges.py) rely on.

  gaussian    q, k, v, dO ~ N(0, 1) rounded to bf16: logits ~ N(0, 1), every softmax row near uniform, level 0 (what the rest of
              the suite feeds attention)
  shifted     the same with channel 0 of every head overwritten: q[..., 0] = 64, k[..., 0] = t / 8 (both bf16-exact), so EVERY
              logit of a row moves by exactly t natural units (scale 1/8): softmax, o, dq, dk, dv are mathematically unchanged
              (dk[..., 0] is the one element that sees the 64), only the absolute level of the logits - and of the log-sum-exp the
              backward recomputes its probabilities from - moves.  `alternate`: q[i, 0] = +64 / -64 on even / odd query rows, so
              one wave holds rows at +t and at -t
  selecting   softmax rows that are EXACTLY one-hot or two-hot, so that every output has an exact expectation (below)
"""
from __future__ import annotations

import dataclasses
from typing import Optional

import numpy as np
import torch

D = 64
SCALE = D ** -0.5                         # 1/8
LOG2E = 1.4426950408889634
U = 2.0 ** -9                             # bf16 half-ulp, relative
SHIFTS = (-512, -128, -96, -64, 0, 64, 512)
SELECT_N = (17, 33, 197, 256, 257, 300, 600, 1025)
CODE_BITS, CODE_REP, CODE_DIMS, SPARE = 11, 5, 55, 9       # 11 label bits x 5 repeats = 55 code dims, 9 spare dims
QGAIN = 128.0                             # query = QGAIN * code: matching logit QGAIN * 55 / 8 = 880, next one <= 720
BF = torch.bfloat16


@dataclasses.dataclass
class Case:
    """qkv: bf16 [B, N, 3C] (q | k | v column blocks, head-major inside a block); do: bf16 [B, N, C]."""
    qkv: torch.Tensor
    do: torch.Tensor
    H: int
    target: Optional[np.ndarray] = None   # selecting: [B, H, N] pair index chosen by each query

    @property
    def C(self):
        return self.H * D

    def parts(self):
        C = self.C
        return self.qkv[..., :C], self.qkv[..., C:2 * C], self.qkv[..., 2 * C:]


def _bf(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(BF)


def gaussian(B: int, N: int, H: int, seed: int) -> Case:
    rng = np.random.default_rng([seed, B, N, H])
    C = H * D
    return Case(_bf(rng.standard_normal((B, N, 3 * C))), _bf(0.5 * rng.standard_normal((B, N, C))), H)


def shifted(B: int, N: int, H: int, t: float, seed: int, alternate: bool = False) -> Case:
    case = gaussian(B, N, H, seed)
    C = H * D
    k0 = t * 8.0 / 64.0
    assert float(_bf(np.array([k0]))[0]) == k0, "t / 8 must be bf16-exact"
    q0 = torch.full((N,), 64.0)
    if alternate:
        q0[1::2] = -64.0
    for h in range(H):
        case.qkv[:, :, h * D] = q0.to(BF)[None, :]
        case.qkv[:, :, C + h * D] = k0
    return case


def select_head(N: int, rng):
    """One (image, head) of `selecting`: q, k, v, dO [N, 64] float64 (small integers) and target [N] (pair index per query)."""
    npair = (N + 1) // 2
    label = rng.permutation(1 << CODE_BITS)[:npair]                       # distinct 11-bit labels: two pairs differ in >= 1 bit
    bits = ((label[:, None] >> np.arange(CODE_BITS)) & 1) * 2 - 1
    code = np.repeat(bits, CODE_REP, axis=1).astype(np.float64)           # [npair, 55], entries +-1
    pair = np.arange(N) // 2
    k = np.zeros((N, D))
    k[:, :CODE_DIMS] = code[pair]
    k[:, CODE_DIMS:] = rng.integers(-2, 3, (N, SPARE))
    same = (k[0:N - 1:2, CODE_DIMS:] == k[1:N:2, CODE_DIMS:]).all(1)      # twins must differ somewhere in the spare dims
    k[1:N:2, CODE_DIMS][same] += np.where(k[1:N:2, CODE_DIMS][same] < 2, 1, -1)
    perm = rng.permutation(npair)
    # the first query tile reaches into the last (partial) key tile and back: query 0 -> last pair, last query -> pair 0
    a, b = int(np.where(perm == npair - 1)[0][0]), 0
    perm[[a, b]] = perm[[b, a]]
    last = (N - 1) % npair
    a = int(np.where(perm == 0)[0][0])
    if last != 0:
        perm[[a, last]] = perm[[last, a]]
    target = perm[np.arange(N) % npair]                                   # every pair is chosen by at most two queries
    q = np.zeros((N, D))
    q[:, :CODE_DIMS] = QGAIN * code[target]
    v = rng.integers(-1, 2, (N, D)).astype(np.float64)
    do = rng.integers(-1, 2, (N, D)).astype(np.float64)
    return q, k, v, do, target


def selecting(B: int, N: int, H: int, seed: int) -> Case:
    """Keys come in twins (j, j ^ 1) that share an 11-bit label, each bit +-1 repeated 5 times over the 55 code dims, and differ
    only by small integers in the 9 spare dims; query i = 128 code(target(i)) on the code dims, 0 on the spare dims.  With scale 1/8
    the matching logit is 128 * 55 / 8 = 880 and any other pair disagrees in >= 1 bit = 5 dims: <= 128 * 45 / 8 = 720.  The gap of
    160 (231 in the exp2 domain) is past fp32's exp2 underflow (2^-149), so every unselected probability is exactly 0 in the
    kernels, twins tie exactly (identical arithmetic on identical code dims), and a row is {1/2, 1/2}, or {1} when N is odd and
    the last key has no twin.  v, dO take values in {-1, 0, 1}.  Different labels, targets and values per image and head."""
    C = H * D
    qkv, do = np.zeros((B, N, 3 * C)), np.zeros((B, N, C))
    target = np.zeros((B, H, N), dtype=np.int64)
    for b in range(B):
        for h in range(H):
            q, k, v, g, tg = select_head(N, np.random.default_rng([seed, N, b, h]))
            s = slice(h * D, (h + 1) * D)
            qkv[b, :, :C][:, s], qkv[b, :, C:2 * C][:, s], qkv[b, :, 2 * C:][:, s], do[b][:, s] = q, k, v, g
            target[b, h] = tg
    case = Case(_bf(qkv), _bf(do), H, target)
    assert np.array_equal(case.qkv.double().numpy(), qkv) and np.array_equal(case.do.double().numpy(), do)   # bf16-exact
    return case


def select_expectation(case: Case):
    """The exact results of a `selecting` case (scale 1/8) from the construction alone, no softmax: o, dq, dk, dv float64
    [B, N, C] and the log2-domain lse [B, H, N] (880 log2 e, + 1 for a two-hot row)."""
    B, N, _ = case.qkv.shape
    q, k, v = (t.double().numpy().reshape(B, N, case.H, D) for t in case.parts())
    g = case.do.double().numpy().reshape(B, N, case.H, D)
    o, dq, dk, dv = (np.zeros((B, N, case.H, D)) for _ in range(4))
    lse2 = np.zeros((B, case.H, N))
    for b in range(B):
        for h in range(case.H):
            for i in range(N):
                keys = [j for j in (2 * case.target[b, h, i], 2 * case.target[b, h, i] + 1) if j < N]
                p = 1.0 / len(keys)
                o[b, i, h] = p * sum(v[b, j, h] for j in keys)
                lse2[b, h, i] = QGAIN * CODE_DIMS * SCALE * LOG2E + np.log2(len(keys))
                dp = {j: float(g[b, i, h] @ v[b, j, h]) for j in keys}
                delta = p * sum(dp.values())
                for j in keys:
                    ds = p * (dp[j] - delta) * SCALE
                    dv[b, j, h] += p * g[b, i, h]
                    dq[b, i, h] += ds * k[b, j, h]
                    dk[b, j, h] += ds * q[b, i, h]
    C = case.C
    return tuple(a.reshape(B, N, C) for a in (o, dq, dk, dv)) + (lse2,)


@dataclasses.dataclass
class Ref:
    o: torch.Tensor        # [B, N, C]
    lse2: torch.Tensor     # [B, H, N]   log2-domain log-sum-exp of the scaled logits
    P: torch.Tensor        # [B, H, N, N]
    dP: torch.Tensor       # [B, H, N, N]  dO V^T
    delta: torch.Tensor    # [B, H, N]   rowsum(dO o O)
    dq: torch.Tensor
    dk: torch.Tensor
    dv: torch.Tensor
    absqk: torch.Tensor    # [B, H, N]   max_j sum_d |q_id k_jd|
    gap: float             # smallest distance, over rows, from the row's top logit to the next DIFFERENT logit (natural units)
    ln_scale: float


def _heads(t, H):
    B, N, C = t.shape
    return t.double().reshape(B, N, H, C // H).transpose(1, 2)          # [B, H, N, D]


def _tokens(t):
    B, H, N, d = t.shape
    return t.transpose(1, 2).reshape(B, N, H * d)


def reference(q, k, v, do, H: int, ln_scale: float = SCALE) -> Ref:
    """float64 attention forward and backward of the given (already rounded) operands, written out (no autograd: the bounds need
    P, dP and delta).  The natural-log logits are ln_scale * q . k: 1/8 for the plain entries, ln 2 for queries that arrive
    pre-multiplied by scale log2 e."""
    qh, kh, vh, gh = (_heads(t, H) for t in (q, k, v, do))
    s = (qh @ kh.transpose(-1, -2)) * ln_scale
    top = s.max(-1, keepdim=True).values
    below = torch.where(s < top, top - s, torch.full_like(s, float("inf")))
    P = torch.softmax(s, -1)
    oh = P @ vh
    dP = gh @ vh.transpose(-1, -2)
    delta = (gh * oh).sum(-1)
    dS = P * (dP - delta[..., None])
    absqk = (qh.abs() @ kh.abs().transpose(-1, -2)).max(-1).values
    return Ref(_tokens(oh), torch.logsumexp(s, -1) / np.log(2.0), P, dP, delta, _tokens(ln_scale * (dS @ kh)),
               _tokens(ln_scale * (dS.transpose(-1, -2) @ qh)), _tokens(P.transpose(-1, -2) @ gh), absqk, float(below.min()), ln_scale)


# ---- bounds: every one is computed from the inputs and the float64 reference, never from a kernel's result
def lse_bound(ref: Ref) -> torch.Tensor:
    """[B, H, N]: the existing absolute gate 2e-3 plus the fp32 accumulation bound of the largest logit of the row,
    D 2^-24 c max_j sum_d |q_id k_jd| (c = ln_scale log2 e: lse is in the log2 domain)."""
    return 2e-3 + D * 2.0 ** -24 * ref.ln_scale * LOG2E * ref.absqk


def fwd_bound_bf16(ref: Ref, v, H: int) -> torch.Tensor:
    """[B, N, C]: 1.25 * 2u * (P |V|).  P is rounded to bf16 before the second product and the output is rounded to bf16: each at
    most u sum_j p_ij |v_jd|; the 1.25 covers the fp32 accumulation and v_exp_f32."""
    return 1.25 * 2 * U * _tokens(ref.P @ _heads(v, H).abs())


def half_ulp(x: torch.Tensor) -> torch.Tensor:
    """What rounding x to bf16 (8 significant bits, nearest) can move it by: 2^(floor(log2 |x|) - 8), between u |x| (x just below a
    power of two) and 2u |x| (x just above one)."""
    a = x.abs()
    _, E = torch.frexp(torch.where(a > 0, a, torch.ones_like(a)))
    return torch.where(a > 0, torch.ldexp(torch.ones_like(a), E - 9), torch.zeros_like(a))


def dv_bound(ref: Ref, do, H: int, exact_half_ulp: bool = True) -> torch.Tensor:
    """[B, N, C]: 1.25 (h(P)^T |dO| + h(dv)): P to bf16, the result to bf16, h = half_ulp.  Written with u |x| in place of h(x)
    (exact_half_ulp = False) the bound understates a rounding by up to a factor 2, and the exact arithmetic of the kernel (P to bf16,
    fp32 sums, the result to bf16) exceeds it where few terms average: by 1.06 at N = 17 (tests/test_attention_cases_cpu.py)."""
    g = _heads(do, H).abs()
    if exact_half_ulp:
        return 1.25 * (_tokens(half_ulp(ref.P).transpose(-1, -2) @ g) + half_ulp(ref.dv))
    return 1.25 * (U * _tokens(ref.P.transpose(-1, -2) @ g) + U * ref.dv.abs())


def emulate_bf16_backward(case: Case, ref: Ref):
    """(o, dq, dk, dv) float64 [B, N, C] of a torch restatement of the bf16 kernels' roundings and nothing else: scores and every sum
    in fp32 or better, p = exp2(c s - L2) in fp32, P and dS rounded to bf16 before the second products, o and the gradients
    rounded to bf16, delta from the bf16 o.  What honest arithmetic of that design gives - the yardstick for a bound."""
    H = case.H
    qh, kh, vh, gh = (_heads(t, H) for t in case.parts() + (case.do,))
    s = (qh @ kh.transpose(-1, -2)).float()
    P = torch.exp2(s * np.float32(ref.ln_scale * LOG2E) - ref.lse2.float()[..., None])
    Pb = P.to(BF).double()
    o = (Pb @ vh).float().to(BF).double()
    delta = (gh * o).sum(-1).float()
    dS = (P * ((gh @ vh.transpose(-1, -2)).float() - delta[..., None]) * np.float32(ref.ln_scale)).to(BF).double()
    rnd = lambda t: _tokens(t.float().to(BF).double())                 # noqa: E731
    return _tokens(o), rnd(dS @ kh), rnd(dS.transpose(-1, -2) @ qh), rnd(Pb.transpose(-1, -2) @ gh)


def dqdk_bounds(ref: Ref, q, k, do, H: int):
    """([B, N, C], [B, N, C]).  E_ij = scale p_ij ((2u + 2^-22 |L2_i|) |dP_ij - delta_i| + u sum_d |dO_id o_id|): P and dS rounded
    to bf16 (2u), the fp32 exponent c s - L2 of the recomputed p (2^-22 |L2|: a few ulps of a number of L2's size), and the bf16 O
    inside delta.  |err dq_i| <= 1.25 (sum_j E_ij |k_j| + u |dq_i|), |err dk_j| <= 1.25 (sum_i E_ij |q_i| + u |dk_j|)."""
    gh, oh = _heads(do, H), _heads(ref.o, H)
    ddelta = U * (gh.abs() * oh.abs()).sum(-1)
    rel = 2 * U + 2.0 ** -22 * ref.lse2.abs()
    E = ref.ln_scale * ref.P * (rel[..., None] * (ref.dP - ref.delta[..., None]).abs() + ddelta[..., None])
    bq = 1.25 * (_tokens(E @ _heads(k, H).abs()) + U * ref.dq.abs())
    bk = 1.25 * (_tokens(E.transpose(-1, -2) @ _heads(q, H).abs()) + U * ref.dk.abs())
    return bq, bk


def drop_channel0(t: torch.Tensor, H: int) -> torch.Tensor:
    """[B, N, C] without channel 0 of every head (the shifted cases' offset channel must not carry a norm)."""
    B, N, C = t.shape
    return t.reshape(B, N, H, C // H)[..., 1:].reshape(B, N, -1)


def padded_key_backward_standin(q, k, do, ref: Ref, H: int, mask: bool) -> torch.Tensor:
    """float32 torch stand-in of the ONE thing the one-block backward did to a padded key before it was masked: the key's row in
    LDS is zero, so its score is 0, its recomputed probability is p = exp2(-L2) and its dS = p (0 - delta) scale is multiplied by
    the zero K row and summed into dq of a real query.  Returns that padded contribution to dq, [B, H, N, D] (all zeros in exact
    arithmetic; inf * 0 = NaN once p overflows).  mask = True selects the padded probability away first, as the kernels do now."""
    L2 = ref.lse2.float()
    p = torch.exp2(-L2)
    if mask:
        p = torch.zeros_like(p)
    ds = (p * (0.0 - ref.delta.float()) * np.float32(ref.ln_scale)).to(BF).float()
    return ds[..., None] * torch.zeros(D, dtype=torch.float32)
