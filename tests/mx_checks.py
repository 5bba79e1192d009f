"""The check of an MX operand (e4m3 codes + E8M0 block scales) that a kernel quantised from values it does not hand out exactly:
shared by tests/test_gpu_attention_edges.py and tests/test_gpu_layernorm_edges.py."""
import numpy as np

from tests.test_mxfp8_format import e4m3_bits, mx_dequant, mx_exponent, mx_quant_ref


def half_bf16_ulp(a: np.ndarray) -> np.ndarray:
    """a = m 2^E, m in [0.5, 1): bf16 ulp 2^(E-8); 0 for a = 0"""
    a = np.abs(np.asarray(a, np.float64))
    _, E = np.frexp(np.where(a > 0, a, 1.0))
    return np.where(a > 0, np.ldexp(1.0, E - 9), 0.0)


def check_mx_pack(name, codes, scales, ob, od, exact, margins, half=None):
    """od (when the entry writes one) is the exact dequantisation of (codes, scales).  exact: codes and scales EQUAL the host MX pack
    of ob.  Otherwise the kernel quantised a value it did not hand out, known to lie in [ob - half, ob + half]; `half` defaults to half a
    bf16 ulp of ob - the attention kernel quantises its fp32 o, of which ob is the bf16 rounding (attention_flash.hip, OUT_MX epilogue:
    amax and pack_fp8x4 read o[dt][e], Ob stores (bf16)o[dt][e]), so the pack of ob is a SECOND rounding of o and may differ from the codes
    wherever ob landed on an e4m3 tie (1 in 16 bf16 values is one).  What must hold: the block's scale byte is the scale rule's byte
    for an amax inside the interval, and each code lies between the e4m3 roundings of the two ends of its element's interval
    [|ob| - h, |ob| + h], with ob's sign (unless the interval holds 0)."""
    rows = codes.shape[0]
    obn = np.asarray(ob, np.float64).reshape(rows, -1)
    if od is not None:
        assert np.array_equal(np.asarray(od, np.float64).reshape(rows, -1), mx_dequant(codes, scales)), name
    rc, rs, finite = mx_quant_ref(obn.astype(np.float32))
    assert finite.all()
    same = float((rc == codes).mean())
    print(f"{name}: codes equal to the host pack of ob: {same:.4f} of the elements, scales: {float((rs == scales).mean()):.4f}")
    key = name + "/fraction_of_codes_equal_to_pack_of_ob"
    margins[key] = min(margins.get(key, 1.0), same)
    if exact:
        assert np.array_equal(rc, codes) and np.array_equal(rs, scales), name
        return
    a = np.abs(obn)
    hulp = half_bf16_ulp(a) if half is None else np.asarray(half, np.float64).reshape(rows, -1)
    lo, hi = np.maximum(a - hulp, 0.0), a + hulp
    blo, bhi = (x.reshape(rows, -1, 32).max(-1) for x in (lo, hi))
    e = scales.astype(np.int64) - 127
    assert ((mx_exponent(blo) <= e) & (e <= mx_exponent(bhi))).all(), name
    inv = np.repeat(np.ldexp(1.0, -e), 32, axis=1)
    clo, chi = e4m3_bits(np.minimum(lo * inv, 448.0)) & 0x7F, e4m3_bits(np.minimum(hi * inv, 448.0)) & 0x7F
    mag = codes & 0x7F
    assert ((clo <= mag) & (mag <= chi)).all(), name
    assert (((codes >> 7) == np.signbit(obn)) | (mag == 0) | (a <= hulp)).all(), name
