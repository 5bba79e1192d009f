"""The MX (block-scaled e4m3) format of the ``"mxfp8"`` build, pinned on the CPU (include/ldit.h, LDIT_MXFP8):

  codes [rows, K] e4m3fn + scales [rows, K / 32] bytes; block exponent e = the smallest integer with amax <= 448 * 2^e, clamped
  to [-127, 127], byte = e + 127; code = e4m3_RNE(x * 2^-e); all-zero block -> byte 0, codes 0; Inf / NaN in the block -> byte 0xFF.

``mx_quant_ref`` is the numpy reference every GPU test of the build (tests/test_gpu_mxfp8.py) checks against.  Also here: the C
header and the binding declare the new entry points, the encoder constructs, and the block-scaled GEMM instantiations really
issue the VGPR-scaled MFMA (device assembly, cross-compiled)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- numpy reference ------------------------------------------------------------------------------------------------------
def mx_exponent(amax: np.ndarray) -> np.ndarray:
    """Block exponent of the scale rule: amax = m 2^E, m in [0.5, 1) -> E - 9 if m <= 0.875 else E - 8 (448 = 0.875 2^9),
    clamped to [-127, 127]; -127 (byte 0) for an all-zero block."""
    amax = np.asarray(amax, np.float64)
    m, E = np.frexp(amax)
    e = np.where(m <= 0.875, E - 9, E - 8)
    e = np.where(amax == 0, -127, e)
    return np.clip(e, -127, 127).astype(np.int64)


def e4m3_bits(y: np.ndarray) -> np.ndarray:
    """OCP e4m3fn bit patterns of float64 values with |y| <= 448, rounded to nearest even (min normal 2^-6, subnormal step 2^-9)."""
    y = np.asarray(y, np.float64)
    sign = np.signbit(y).astype(np.uint8) << 7
    a = np.abs(y)
    _, E = np.frexp(np.where(a > 0, a, 1.0))
    ex = np.maximum(E - 1, -6)                       # exponent of the binade (subnormals share 2^-6's step)
    step = np.ldexp(1.0, ex - 3)
    q = np.round(a / step) * step                     # np.round: half to even
    assert np.all(q <= 448), "e4m3_bits: value above 448"
    _, Eq = np.frexp(np.where(q > 0, q, 1.0))
    eq = Eq - 1
    normal = (q > 0) & (eq >= -6)
    biased = np.where(normal, eq + 7, 0)
    mant = np.where(normal, np.round((q / np.ldexp(1.0, eq) - 1.0) * 8), np.round(q / 2.0 ** -9))
    return (sign | (biased.astype(np.uint8) << 3) | mant.astype(np.uint8)).astype(np.uint8)


def mx_quant_ref(x: np.ndarray):
    """(codes uint8 [rows, K], scales uint8 [rows, K / 32], finite-block mask [rows, K / 32]) of fp32 ``x`` [rows, K].
    The codes of a block holding Inf / NaN are unspecified (mask False there)."""
    x = np.asarray(x, np.float32)
    rows, K = x.shape
    b = x.reshape(rows, K // 32, 32).astype(np.float64)
    finite = np.isfinite(b).all(-1)
    amax = np.where(finite, np.abs(np.where(np.isfinite(b), b, 0)).max(-1), 0.0)
    e = mx_exponent(amax)
    scales = np.where(finite, e + 127, 255).astype(np.uint8)
    y = np.where(finite[..., None], b * np.ldexp(1.0, -e)[..., None], 0.0)
    return e4m3_bits(y).reshape(rows, K), scales, finite


def mx_dequant(codes: np.ndarray, scales: np.ndarray) -> np.ndarray:
    """float64 value of an MX operand: code * 2^(byte - 127)."""
    lut = e4m3_values()
    v = lut[np.asarray(codes, np.uint8)].reshape(codes.shape[0], -1, 32)
    return (v * np.ldexp(1.0, scales.astype(np.int64) - 127)[..., None]).reshape(codes.shape)


def e4m3_values() -> np.ndarray:
    """float64 value of each of the 256 e4m3fn codes (NaN for 0x7F / 0xFF)."""
    out = np.empty(256)
    for c in range(256):
        s, ex, mt = c >> 7, (c >> 3) & 15, c & 7
        v = (mt / 8.0) * 2.0 ** -6 if ex == 0 else (1 + mt / 8.0) * 2.0 ** (ex - 7)
        out[c] = np.nan if (ex == 15 and mt == 7) else (-v if s else v)
    return out


def edge_blocks() -> np.ndarray:
    """[rows, 64] fp32 rows of edge blocks (two blocks per row)."""
    rng = np.random.default_rng(5)
    rows = []
    def blk(vals):
        b = np.zeros(32, np.float32)
        b[:len(vals)] = vals
        return b
    f = np.float32
    rows.append(np.concatenate([blk([]), blk([1.0, -2.0])]))                               # all-zero block
    for e in (-20, 0, 3, 40):                                                                # amax exactly 448 2^e, and the next float
        a = f(448.0 * 2.0 ** e)
        rows.append(np.concatenate([blk([a, -a / 3, a / 1000]), blk([np.nextafter(a, f(np.inf)), -a / 7])]))
        rows.append(np.concatenate([blk([-a, a * f(0.999)]), blk([np.nextafter(a, f(0)), a / 5])]))
    rows.append(np.concatenate([blk([448.0, 2.0 ** -7, 2.0 ** -8, 2.0 ** -9, 3 * 2.0 ** -10, 2.0 ** -10, 2.0 ** -11, -2.0 ** -9]),
                                blk([1.0, 2.0 ** -16, 1.5 * 2.0 ** -16, 2.0 ** -17])]))       # e4m3 subnormal codes and their rounding
    rows.append(np.concatenate([blk([f(2.0 ** 100), f(-3 * 2.0 ** 97)]), blk([f(2.0 ** -100), f(-2.0 ** -103)])]))
    rows.append(np.concatenate([blk([f(1e-40), f(-3e-41)]), blk([f(2.0 ** -126), f(2.0 ** -130)])]))   # fp32 subnormal amax: clamped
    rows.append(np.concatenate([blk([1.0, np.nan]), blk([np.inf, 1.0])]))                     # Inf / NaN blocks
    rows.append(np.concatenate([blk([0.875 * 2.0 ** 5]), blk([0.875 * 2.0 ** 5 * (1 + 2.0 ** -23)])]))  # m on the 0.875 boundary
    for _ in range(6):
        rows.append((rng.standard_normal(64) * np.exp2(rng.integers(-30, 30))).astype(np.float32))
    return np.stack(rows).astype(np.float32)


# ---- the reference itself ---------------------------------------------------------------------------------------------------
def test_scale_rule_is_the_smallest_exponent_that_does_not_clip():
    rng = np.random.default_rng(0)
    amax = np.concatenate([np.exp2(rng.uniform(-120, 120, 20000)), 448.0 * np.exp2(np.arange(-100, 100, dtype=np.float64)),
                           np.nextafter(448.0 * np.exp2(np.arange(-100, 100, dtype=np.float64)), np.inf)])
    e = mx_exponent(amax)
    assert np.all(amax <= 448.0 * np.exp2(e.astype(np.float64)))
    inside = e > -127                                    # (below 448 2^-128 the clamp decides)
    assert inside.sum() > 19000
    assert np.all(amax[inside] > 448.0 * np.exp2(e[inside].astype(np.float64) - 1))
    assert mx_exponent(np.array([0.0]))[0] == -127 and mx_exponent(np.array([1e300]))[0] == 127


def test_numpy_reference_agrees_with_torch_casts_on_edge_blocks():
    torch = pytest.importorskip("torch")
    if not hasattr(torch, "float8_e8m0fnu"):
        pytest.skip("this torch has no float8_e8m0fnu")
    x = edge_blocks()
    codes, scales, finite = mx_quant_ref(x)
    rows, K = x.shape
    assert scales.shape == (rows, K // 32) and codes.shape == (rows, K)
    e = scales.astype(np.int64) - 127
    # codes: a multiply by an exact power of two in fp32, then torch's e4m3fn cast
    mul = np.repeat(np.ldexp(np.float32(1.0), -np.where(finite, e, 0)).astype(np.float32), 32, axis=1)
    xt = torch.from_numpy(np.where(np.repeat(finite, 32, axis=1), x, 0).astype(np.float32))
    tcodes = (xt * torch.from_numpy(mul)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    np.testing.assert_array_equal(codes[np.repeat(finite, 32, axis=1)], tcodes[np.repeat(finite, 32, axis=1)])
    # scales: 2^e as E8M0
    tsc = torch.from_numpy(np.ldexp(1.0, e[finite]).astype(np.float32)).to(torch.float8_e8m0fnu).view(torch.uint8).numpy()
    np.testing.assert_array_equal(scales[finite], tsc)
    # the edges themselves
    assert scales[0, 0] == 0 and not codes[0, :32].any()                        # zero block: byte 0, codes 0
    assert scales[1, 0] == 127 - 20 and codes[1, 0] == 0x7E                     # 448 2^-20 -> e = -20, code 448
    assert scales[1, 1] == 127 - 19                                             # the next float up needs e + 1
    assert not finite[-8, 0] and not finite[-8, 1] and scales[-8, 0] == 0xFF and scales[-8, 1] == 0xFF
    assert scales[-7, 0] == 127 + 5 - 9 and scales[-7, 1] == 127 + 5 - 8      # m = 0.875 exactly vs just above
    assert scales[-9, 0] == 0 and scales[-9, 1] == 0                            # fp32-subnormal amax: clamped to -127
    assert set(codes[9, :8].tolist()) & {1, 2, 4, 0x81}                        # e4m3 subnormal codes present
    # dequantisation never exceeds the block's amax by more than the rounding of its largest element
    deq = mx_dequant(codes, scales)
    fin = np.repeat(finite, 32, axis=1)
    assert np.all(np.abs(deq[fin]) <= np.abs(x[fin]) * (1 + 2.0 ** -4) + 2.0 ** -9 * np.repeat(np.ldexp(1.0, e), 32, axis=1)[fin])


# ---- header, binding, module surface --------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_mxfp8_build():
    hdr = open(os.path.join(ROOT, "include", "ldit.h")).read()
    assert re.search(r"\bLDIT_MXFP8\s*=\s*6\b", hdr)
    for fn in ("ldit_quant_mx_f32_fp8", "ldit_linear_mxfp8", "ldit_layernorm_mxfp8"):
        assert re.search(r"\bint\s+" + fn + r"\s*\(", hdr), fn
    from layoutdit_amd import _lib
    assert _lib.DTYPE_MXFP8 == 6
    for fn in ("ldit_quant_mx_f32_fp8", "ldit_linear_mxfp8", "ldit_layernorm_mxfp8"):
        assert fn in _lib.SIGNATURES, fn
    from layoutdit_amd import ops
    assert callable(ops.quant_mxfp8) and callable(ops.linear_mxfp8)


def test_encoder_constructs_on_the_mxfp8_build_and_needs_no_calibration():
    import torch
    from layoutdit_amd import config
    from layoutdit_amd.modeling import DiTBackbone, DiTEncoder
    enc = DiTEncoder(config.vit_tiny(), compute_dtype="mxfp8")
    assert enc.compute_dtype == "mxfp8"
    with pytest.raises(RuntimeError, match="not needed"):
        enc.calibrate_fp8(torch.zeros(1, 3, 224, 224))
    assert DiTBackbone(config=config.vit_tiny(), compute_dtype="mxfp8").dit.compute_dtype == "mxfp8"


# ---- device assembly of the block-scaled GEMM ----------------------------------------------------------------------------
def _kernels(asm: str):
    """kernel name -> text from its label to the next kernel's label (the metadata comments, ScratchSize included)"""
    labels = [(m.start(), m.group(1)) for m in re.finditer(r"^(_Z\S+):", asm, re.M)]
    return {name: asm[s:(labels[i + 1][0] if i + 1 < len(labels) else len(asm))] for i, (s, name) in enumerate(labels)}


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc (cross-compiles without a GPU)")
def test_mx_gemm_instantiations_issue_the_vgpr_scaled_mfma(tmp_path):
    """Every MX instantiation of the fp8 GEMM, inference and train step, issues the VGPR-scaled MFMA and uses no scratch memory."""
    out = os.path.join(str(tmp_path), "gemm_fp8.s")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-Wno-unused-function",
                        "-S", "--cuda-device-only", "-o", out, os.path.join(ROOT, "layoutdit_amd", "csrc", "gemm_fp8.hip")],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    ks = _kernels(open(out).read())
    vgpr_scaled = re.compile(r"v_mfma_scale_f32_32x32x64_f8f6f4\s+\S+,\s*\S+,\s*\S+,\s*\S+,\s*v\d+,\s*v\d+")
    # template arguments end in <MX, TR>; a TR (mxfp8 train step) instantiation is an MX one with its own argument struct
    mx = {n: t for n, t in ks.items() if re.search(r"gemm_fp8_(mfma|tail)I.*ELb1ELb0EEEv", n)}
    plain = {n: t for n, t in ks.items() if re.search(r"gemm_fp8_(mfma|tail)I.*ELb0ELb0EEEv", n)}
    train = {n: t for n, t in ks.items() if re.search(r"gemm_fp8_(mfma|tail)I.*ELb1ELb1EEEv", n)}
    assert len(mx) + len(plain) + len(train) == sum("gemm_fp8_" in n for n in ks), sorted(ks)
    # three epilogues x (five tiles + the tail)
    assert len(mx) == 3 * 6 - 1, sorted(mx)        # (the scale+residual epilogue has no 320-row tile)
    assert len(plain) == 3 * 6 - 1, sorted(plain)
    # the two train epilogues x (five tiles + the tail), no 320-row scale+residual tile
    assert len(train) == 2 * 6 - 1, sorted(train)
    for n, t in plain.items():
        assert not vgpr_scaled.search(t), n
    for n, t in {**mx, **train}.items():
        assert vgpr_scaled.search(t), n
        assert re.search(r"ScratchSize:\s*0\b", t), (n, re.search(r"ScratchSize:\s*\d+", t).group(0))
