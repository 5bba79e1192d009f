"""No kernel may depend on, or touch, memory outside its operands: every device-pointer entry of include/ldit.h, called through
ctypes, with its operands placed inside guard bands (tests/guarded.py).

Each case runs TWICE with the same geometry (offsets, strides, tiling switch): what surrounds the inputs - gap columns of strided
operands, the rows in front of and behind them, a scratch buffer's previous contents - is 0x00 in the first run and 0xFF (NaN in
every float format, -1 as an integer) in the second.  Asserted:
  (a) the outputs' parents are equal bit for bit between the two runs (no tolerance: the geometry is identical);
  (b) the second output is finite wherever the contract defines a finite value;
  (c) what surrounds an output (0xA5 before the call) and every byte of an input's parent are untouched;
  (d) the first output meets the entry's parity gate against its float64 / exact oracle, with the tolerance of the entry's
      own test (named at each gate), so that (a) does not compare two wrong results.
What the header promises the kernel is kept: a zero page is zeros (of the documented 128 bytes, poison around it), a `+=`
destination and an in-place residual hold their values, alignments are those the header asks for.

Read before run (one line per kernel: is a padding row turned into an address before the count test?):
  rpn_topk_kernel / rpn_topk_chunked_kernel   no count; a level's slots i >= n get the key ~0 without a load (proposals.hip:70, :94)
  rpn_decode_kernel                           idx is range-checked as unsigned BEFORE it indexes anything (proposals.hip:113)
  nms_batched_kernel                          ids come from sort keys clamped to [0, N) (proposals.hip:202-203); -inf / NaN rows never alive
  roi_align_levels_kernel                     r < count[b] is tested first; boxes[row] is loaded after it (roi_heads.hip:78-84)
  box_postprocess_kernel                      reads head / proposals of a padding row BY ROW INDEX (in bounds) and writes a box from them
                                              (roi_heads.hip:156-178); no address is formed from their values
  rpn_targets_kernel / _chunked_kernel        G is clamped to [0, Gmax]; only gt_boxes[g], g < G, is loaded (rpn_train.hip:102-108, :178-184)
  rpn_loss_kernel                             the label is read first; logits only for label 0 / 1, deltas and targets for label 1 (:276-287)
  roi_targets_kernel                          count and gt_count clamped; a candidate is loaded after `valid` (roi_train.hip:50-71)
  roi_align_levels_bwd_kernel                 r < valid_rows && levels[r] == l before boxes[r] (roi_train.hip:231-232)
  box_loss_kernel                             a label >= NC becomes -1 before it indexes a column (roi_train.hip:308-309)
  coco_match_kernel                           tid < Dv / tid < Gv before every load of a row (coco_eval.hip:99, :109)
  coco_keys_kernel                            rank is read first; scores / labels only for rank >= 0 (coco_eval.hip:209-213)
  coco_accumulate_kernel                      sorted_index only inside the category's run of present keys (coco_eval.hip:276-283)

Padding rows about which the header is silent (the twin run asserts only that they do not change):
  ldit_box_postprocess_f32   boxes_out of a row r >= count[b]: "the box is still written", its value is not defined.  The kernel
                             decodes it from the padding row of head / proposals (roi_heads.hip:156-178); 0x00 and 0xFF rows both
                             decode to the box (0, 0, 0, 0) because fmaxf / fminf drop a NaN operand in the clamp to the image.
Every other padding row has a documented value (-1, zeros, -inf, ABSENT) and is compared with the oracle.

Coverage: every entry of include/ldit.h that takes a device pointer (72).  "here": this module, with the shapes; "fresh": through
the whole path in tests/test_gpu_fresh_memory.py; "exempt": with the reason (7 of 72).
  entry                          where   shapes / reason
  ldit_linear_f32                here    tiles 0..7 + auto + persistent panel; M 17..321 around each tile height, N 50 / 96 / 200 / 257, K 64 / 96
  ldit_linear_bf16               here    tiles 1..5 + auto; M 37 / 528 / 1040, the peeled tail at 16400 x 1024 (riding and own launch); K 64 / 192
  ldit_linear_bf16_ex            here    EPI_F32 (splits 1 and 3), GELU + Ypre, SCALE_RESID + rowscale + Ypre, GELU_BWD with ldaux > N
  ldit_reduce_slabs_f32          here    3 slabs of 136 x 96 (bf16_ex) and of 136 x 96 (wgrad)
                                         (the slab buffers of ldit_linear_bf16_ex and ldit_linear_bf16_tr are treated as SCRATCH: their own
                                         footprint holds 0x00 / 0xFF before the call, the 0xA5 canary stays around them)
  ldit_linear_bf16_tr            here    dgrad tiles 2..5 + auto, three epilogues; wgrad tiles 2 / 3 / 6 + auto, K 37 / 197 / 325, splits 1 and 3
  ldit_linear_fp8                here    tiles 0..4 + auto, M 37 (tail kernel) / 528 / 1040, K 128 / 384, per-tensor and per-channel scales
  ldit_linear_mxfp8              here    tiles 0..4 + auto, M 37 / 528, K 128 / 384, three epilogues (MX output with its scales)
  ldit_linear_mxfp8_train        here    tiles 0 / 2 + auto; GELU (Ypre, Yd), SCALE_RESID in place and with a separate R, rowscale
  ldit_linear_planes             here    planes 2 and 3; M 37 / 528, three epilogues
  ldit_attention_f32             here    N 1 / 33 / 225, B = H = 2; the dominant last key at N = 449
  ldit_attention_bf16            here    N 33 / 257, scale given and prescaled
  ldit_attention_planes          here    planes 2 and 3, N 33 / 130
  ldit_attention_fwd_lse_bf16    here    N 33 / 257
  ldit_attention_bwd_bf16        here    N 33 / 257 (one workgroup per head, and the blocked form), fused dq | dk | dv
  ldit_attention_mxfp8_train     here    N 17 / 257
  ldit_layernorm_f32             here    rows 1 / 5 / 65, C 64 / 192 / 768
  ldit_layernorm_f32_planes      here    the same, planes 2 and 3
  ldit_layernorm_mxfp8           here    the same
  ldit_layernorm_mxfp8_train     here    the same
  ldit_layernorm_bwd_f32         here    the same; dh a += destination; scratch 0x00 / 0xFF
  ldit_layernorm_bwd_resid_f32   here    the same, with and without rowscale; dh a += destination; scratch 0x00 / 0xFF
  ldit_resid_bwd_bf16            here    the same, with and without rowscale; dh an input; scratch 0x00 / 0xFF
  ldit_colsum_f32                here    M 1 / 5 / 65 / 513, ldx > N; scratch 0x00 / 0xFF
  ldit_colamax_f32               here    the same
  ldit_split_f32_planes          here    rows 1 / 5 / 65, lds > cols
  ldit_quant_rows_f32_fp8        here    the same shapes, dense
  ldit_quant_mx_f32_fp8          here    the same shapes, lds > K
  ldit_quant_f32_fp8             here    n 1 / 4 / 1027
  ldit_amax_f32                  here    n 1 / 4 / 1027
  ldit_cast_f32_bf16             here    n 1 / 4 / 1027
  ldit_cast_f16_f32              here    n 1 / 4 / 1027
  ldit_cast_f32_f16              here    n 1 / 4 / 1027
  ldit_pad_nhwc_f32_bf16         here    1 x 1, 5 x 9, 7 x 7; C 32 / 64 / 96
  ldit_embed_f32                 here    grids 1 x 1, 5 x 9, 7 x 7; C 32 / 64 / 96
  ldit_embed_bf16                here    the same; im2col scratch 0x00 / 0xFF
  ldit_embed_bf16_images         here    images 33 x 17 and 64 x 64, fp32 and fp16; im2col scratch 0x00 / 0xFF
  ldit_preprocess_f32            here    images 33 x 17 and 64 x 64
  ldit_preprocess_f16            here    the same
  ldit_tap_to_map_f32            here    grids 1 x 1, 5 x 9, 7 x 7; scales 4 / 2 / 1 / 0.5
  ldit_tap_to_map_bwd_f32        here    the same
  ldit_fpn_merge_f32             here    the same, with and without a top map
  ldit_fpn_merge_bwd_f32         here    the same; d_top a += destination
  ldit_conv3x3_nhwc_f32          here    1 x 1, 5 x 9, 7 x 7; the zero page is 128 bytes
  ldit_roi_align_levels_f32      here    R 1 / 63 / 65, count 0 / 1 / R, C 32 / 64; strided maps, `pool` a view of p5
  ldit_roi_align_levels_bf16     here    the same
  ldit_roi_align_levels_bwd_f32  here    the same; strided gradient maps
  ldit_rpn_topk_f32              here    levels 63 / 65 / 1
  ldit_rpn_topk_chunked_f32      here    the same, and a level of 17000
  ldit_rpn_decode_f32            here    K 1 / 63 / 65, valid slots 0 / 1 / 40 / K
  ldit_nms_batched_f32           here    N 1 / 63 / 65, valid 0 / 1 / 40 / N, three groups
  ldit_box_postprocess_f32       here    R 1 / 63 / 65, count (R, R / 2)
  ldit_rpn_targets_f32           here    N 1 / 63 / 65, gt_count 0 / 1 / 7
  ldit_rpn_targets_chunked_f32   here    the same, and N = 16500
  ldit_rpn_loss_f32              here    N 1 / 63 / 65 / 2500; workspace 0x00 / 0xFF
  ldit_roi_targets_f32           here    R 1 / 63 / 65, count (R, R / 2), gt_count 0 / 1 / 7 / 40
  ldit_box_loss_f32              here    M = 32 rows of those targets; workspace 0x00 / 0xFF
  ldit_coco_match                here    D 1 / 63 / 65, count 0 / 1 / D, a store with rows in front of and behind the batch's
  ldit_coco_keys                 here    the stored rows of that batch
  ldit_coco_accumulate           here    the same
  ldit_vit_forward               fresh   six builds, micro and tiny at batch 2, two lanes at batch 4: workspace 0xFF / 0x00
  ldit_vit_forward_images        fresh   six builds, a ragged image list
  ldit_vit_forward_train         fresh   bf16 micro / tiny, mxfp8 micro: saved block 0xFF / 0x00
  ldit_vit_backward              fresh   the same: workspace and gradient block 0xFF / 0x00, full and staged
  ldit_vit_forward_timed         exempt  ldit_vit_forward's launches between host-side events (a measurement aid that blocks the host)
  ldit_pack_weights              exempt  reads the caller's parameter tensors through HOST structs of pointers; its output block is checked
                                         by every whole-path parity test
  ldit_set_fp8_act_scales        exempt  a memcpy of HOST floats into the packed block
  ldit_pack_train                here    the bf16 mirror of ViT-micro's flat block
  ldit_adamw_step                here    n 4 / 1028; parameters and moments in place, the bf16 mirror an output
  ldit_adamw_step_mxfp8          exempt  ldit_adamw_step, then the MX launch of ldit_pack_train's mxfp8 form; tests/test_gpu_mxfp8_qat.py compares master,
                                         moments and mirror with those two bit for bit
  ldit_grads_check_multi_f32     exempt  tests/test_gpu_detector_step.py already surrounds its segments with sentinels
  ldit_opt_advance               exempt  the same
  ldit_adamw_multi_f32           exempt  the same
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import torch.nn.functional as F                     # noqa: E402

from layoutdit_amd import _lib, ops                 # noqa: E402
from tests import guarded                           # noqa: E402
from tests.guarded import In, Out, Scratch          # noqa: E402
from tests.test_mxfp8_format import mx_dequant, mx_exponent, mx_quant_ref   # noqa: E402
from tests.util import max_rel, rel_l2              # noqa: E402

DEV = "cuda:0"
BF, F8, F32, I32 = torch.bfloat16, torch.float8_e4m3fn, torch.float32, torch.int32
BIAS, GELU, RESID, EF32, GELU_BWD, RELU = (_lib.EPI_BIAS, _lib.EPI_BIAS_GELU, _lib.EPI_SCALE_RESID, _lib.EPI_F32, _lib.EPI_GELU_BWD,
                                           _lib.EPI_BIAS_RELU)
SWITCHES = ("LDIT_GEMM_TILE", "LDIT_GEMM_PERSIST", "LDIT_GEMM_BF16_TILE", "LDIT_GEMM_BF16_TAIL_LAUNCH", "LDIT_GEMM_FP8_TILE",
            "LDIT_GEMM_BF16_TR_TILE")


@pytest.fixture(autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "gpu-marked test running without a GPU"
    _lib.load()
    yield
    for s in SWITCHES:
        _lib.set_switch(s, None)


def _f32(seed, *shape, scale=1.0):
    return torch.from_numpy((scale * np.random.default_rng(seed).standard_normal(shape)).astype(np.float32))


def _bf(seed, *shape, scale=1.0):
    return _f32(seed, *shape, scale=scale).to(BF)


def _p(t):
    return None if t is None else t.data_ptr()


def _s():
    return torch.cuda.current_stream().cuda_stream


def _twin(specs, call):
    return guarded.twin_run(specs, call, device=DEV, sync=torch.cuda.synchronize)


def _rel(got, ref):
    return rel_l2(got.double().numpy(), ref.double().numpy())


def _mrel(got, ref):
    return max_rel(got.double().numpy(), ref.double().numpy())


def _done(res, *names):
    """(b) and completeness for outputs that are finite numbers everywhere."""
    for n in names:
        guarded.assert_written(res.poisoned[n], n)
        guarded.assert_finite(res.poisoned[n], n)


def _up(n, m):
    return (n + m - 1) // m * m


# =============================================================================================================== GEMMs
def _gelu(z):
    return F.gelu(z)                                     # exact erf-GELU (float64 input)


def _lin_common(M, N, epi, mode, ydt, ldy, seed):
    """bias / lam / residual / outputs, each in a parent of its own.  mode "inplace": R aliases Y; "separate": a poisoned R."""
    s, r = {"b": In(_f32(seed + 2, N, scale=0.1))}, None
    if epi == RESID:
        r = _f32(seed + 4, M, N)
        s["lam"] = In(_f32(seed + 3, N).abs() * 0.3 + 0.05)
        if mode == "inplace":
            s["y"] = Out((M, N), F32, ld=ldy, init=r)
        else:
            s["r"] = In(r, ld=ldy)
            s["y"] = Out((M, N), F32, ld=ldy)
        s["y2"] = Out((M, N), F32, ld=ldy)
    else:
        s["y"] = Out((M, N), ydt, ld=ldy)
    return s, r


def _lin_ref(x, w, s, epi, r, mul=None):
    z = x.double() @ w.double().T
    if mul is not None:
        z = z * mul
    z = z + s["b"].data.double()
    if epi == GELU:
        z = _gelu(z)
    if epi == RELU:
        z = torch.relu(z)
    if epi == RESID:
        z = r.double() + s["lam"].data.double() * z
    return z


def _resid_args(t, epi, mode):
    if epi != RESID:
        return None, None, None
    return _p(t["lam"]), _p(t["y"] if mode == "inplace" else t["r"]), _p(t["y2"])


# ---- fp32: every LDIT_GEMM_TILE.  Rows per tile (gemm_f32.hip launch_tiled, gemm_thin_f32.hip): 0: 320, 1: 128, 2: 64, 3: 304,
# 4: 32, 5: 144, 6: 80, 7: 48 - one M below the height and one a row past a multiple of it
F32_TILE_M = {"auto": (37, 305), "0": (17, 321), "1": (37, 129), "2": (17, 65), "3": (37, 305), "4": (17, 33), "5": (65, 145),
              "6": (37, 81), "7": (17, 49)}


def _linear_f32_case(M, N, K, epi, mode, seed=100):
    lib = _lib.load()
    lda, ldy = K + 32, _up(N, 4) + 8
    x, w = _f32(seed, M, K), _f32(seed + 1, N, K, scale=0.1)
    s, r = _lin_common(M, N, epi, mode, F32, ldy, seed)
    s.update(x=In(x, ld=lda), w=In(w))

    def call(t):
        lam, R, y2 = _resid_args(t, epi, mode)
        _lib.check(lib.ldit_linear_f32(_p(t["x"]), lda, _p(t["w"]), _p(t["b"]), _p(t["y"]), ldy, M, N, K, epi, lam, R, y2, _s()))

    res = _twin(s, call)
    ref = _lin_ref(x, w, s, epi, r)
    got = res.clean["y"]
    if epi == GELU:        # test_gpu_ops.py::test_linear_gelu_epilogue
        np.testing.assert_allclose(got.numpy(), ref.float().numpy(), rtol=1e-5, atol=2e-6)
    else:                  # test_gpu_ops.py::test_linear_row_strides_through_the_c_abi, test_linear_bias
        assert _rel(got, ref) < 1e-5 and _mrel(got, ref) < 1e-5, (M, N, K, epi, _rel(got, ref))
    _done(res, "y")
    if epi == RESID:
        assert torch.equal(res.poisoned["y2"], res.poisoned["y"])


@pytest.mark.parametrize("tile", list(F32_TILE_M))
def test_linear_f32(tile):
    if tile != "auto":
        _lib.set_switch("LDIT_GEMM_TILE", tile)
    lo, hi = F32_TILE_M[tile]
    _linear_f32_case(lo, 50, 64, GELU, None)
    _linear_f32_case(hi, 96, 96, RESID, "inplace")
    _linear_f32_case(hi, 200, 64, RESID, "separate")
    _linear_f32_case(lo, 257, 96, BIAS, None)


def test_linear_f32_persistent_panel():
    _lib.set_switch("LDIT_GEMM_TILE", "3")
    _lib.set_switch("LDIT_GEMM_PERSIST", "1")
    _linear_f32_case(305, 200, 96, RESID, "inplace")
    _linear_f32_case(305, 50, 64, GELU, None)


# ---- bf16: LDIT_GEMM_BF16_TILE 1..5 and auto (tiles of 128 / 256 / 192 / 320 rows; <= 64 rows: gemm_bf16_tail unless a tile is forced)
def _bf16_gate(got, ref, epi):
    if epi in (RESID, EF32):   # test_gpu_bf16.py::test_linear_bf16_gelu_and_residual, test_gpu_train.py::test_linear_bf16_training_epilogues
        assert _rel(got, ref) < 1e-5, _rel(got, ref)
    else:                      # test_gpu_bf16.py::test_linear_bf16_bias
        assert _rel(got, ref) < 3e-3 and _mrel(got, ref) < 1.6e-2, (_rel(got, ref), _mrel(got, ref))


def _linear_bf16_case(M, N, K, epi, mode, seed=200):
    lib = _lib.load()
    f32_out = epi == RESID
    lda, ldy = K + 32, (_up(N, 4) + 8) if f32_out else (_up(N, 8) + 16)
    x, w = _bf(seed, M, K), _bf(seed + 1, N, K, scale=0.1)
    s, r = _lin_common(M, N, epi, mode, BF, ldy, seed)
    s.update(x=In(x, ld=lda), w=In(w))

    def call(t):
        lam, R, y2 = _resid_args(t, epi, mode)
        _lib.check(lib.ldit_linear_bf16(_p(t["x"]), lda, _p(t["w"]), _p(t["b"]), _p(t["y"]), ldy, M, N, K, epi, lam, R, y2, _s()))

    res = _twin(s, call)
    _bf16_gate(res.clean["y"], _lin_ref(x, w, s, epi, r), epi)
    _done(res, "y")
    if epi == RESID:
        assert torch.equal(res.poisoned["y2"], res.poisoned["y"])


@pytest.mark.parametrize("tile", ["auto", "1", "2", "3", "4", "5"])
def test_linear_bf16(tile):
    if tile != "auto":
        _lib.set_switch("LDIT_GEMM_BF16_TILE", tile)
    _linear_bf16_case(37, 50, 64, BIAS, None)
    _linear_bf16_case(528, 96, 192, RESID, "inplace")
    _linear_bf16_case(528, 200, 64, GELU, None)
    if tile == "auto":
        _linear_bf16_case(1040, 96, 64, RELU, None)
        _linear_bf16_case(37, 257, 192, RESID, "separate")


@pytest.mark.parametrize("own_launch", [False, True])
def test_linear_bf16_peeled_tail(own_launch):
    """M = 64 x 256 + 16 against N = 1024: the 16 rows past the last full tile row are peeled (launch_gemm_bf16_ex peels only where
    that saves a round of the machine, which needs this many tiles), riding in the main launch or as a launch of their own."""
    if own_launch:
        _lib.set_switch("LDIT_GEMM_BF16_TAIL_LAUNCH", "1")
    _linear_bf16_case(64 * 256 + 16, 1024, 64, BIAS, None)


def _linear_bf16_ex_case(M, N, K, epi, splits=1, seed=300):
    """The train step's extras: Ypre, rowscale, aux (row stride ldaux > N), split-K slabs summed by ldit_reduce_slabs_f32."""
    lib = _lib.load()
    f32_out = epi in (RESID, EF32)
    lda, ldy, ldaux = K + 32, (_up(N, 4) + 8) if f32_out else (_up(N, 8) + 16), _up(N, 8) + 24
    x, w = _bf(seed, M, K, scale=0.5), _bf(seed + 1, N, K, scale=0.1)
    s = {"x": In(x, ld=lda), "w": In(w), "b": In(_f32(seed + 2, N, scale=0.1))}
    ref = x.double() @ w.double().T
    r = rs = aux = None
    if epi == EF32:
        s["y"] = Out((splits * M, N), F32, ld=ldy, scratch=True)      # slab s at Y + s M ldy: scratch, 0x00 / 0xFF before the call
        if splits == 1:
            ref = ref + s["b"].data.double()
    elif epi == GELU:
        s["y"], s["ypre"] = Out((M, N), BF, ld=ldy), Out((M, N), BF, ld=ldy)
    elif epi == RESID:
        r = _f32(seed + 4, M, N)
        rs = torch.from_numpy((np.arange(M) % 3 != 0).astype(np.float32) / 0.9)
        s.update(lam=In(_f32(seed + 3, N).abs() * 0.3 + 0.05), rs=In(rs), y=Out((M, N), F32, ld=ldy, init=r),
                 ypre=Out((M, N), BF, ld=ldy))
    elif epi == GELU_BWD:
        aux = _bf(seed + 5, M, N, scale=0.5) + 0.5
        s.update(aux=In(aux, ld=ldaux), y=Out((M, N), BF, ld=ldy))

    def call(t):
        _lib.check(lib.ldit_linear_bf16_ex(_p(t["x"]), lda, _p(t["w"]), None if epi == GELU_BWD or splits > 1 else _p(t["b"]), _p(t["y"]),
                                           ldy, M, N, K, epi, _p(t.get("lam")), _p(t["y"]) if epi == RESID else None, None,
                                           _p(t.get("ypre")), _p(t.get("rs")), _p(t.get("aux")), ldaux, splits, _s()))

    res = _twin(s, call)
    got = res.clean["y"]
    _done(res, "y")
    if epi == EF32:
        if splits > 1:
            # the slabs of both runs are bit-equal (twin_run); their fixed-order sum, from a poisoned dense copy
            slabs = got.reshape(splits, M * N)
            red = {"slabs": In(slabs.reshape(-1)), "out": Out((M * N,), F32)}
            rr = _twin(red, lambda t: _lib.check(lib.ldit_reduce_slabs_f32(_p(t["slabs"]), _p(t["out"]), M * N, splits, _s())))
            _done(rr, "out")
            got = rr.clean["out"].reshape(M, N)
        _bf16_gate(got, ref, EF32)                       # test_gpu_train.py::test_linear_bf16_split_k_slabs / _training_epilogues
    elif epi == GELU:      # test_gpu_train.py::test_linear_bf16_training_epilogues
        z = (ref + s["b"].data.double()).requires_grad_(True)
        F.gelu(z).sum().backward()
        assert _rel(res.clean["ypre"], z.grad) < 3e-3 and _rel(got, F.gelu(z.detach())) < 3e-3
        _done(res, "ypre")
    elif epi == RESID:
        z = ref + s["b"].data.double()
        assert _rel(got, r.double() + rs.double()[:, None] * s["lam"].data.double() * z) < 1e-5
        assert _rel(res.clean["ypre"], z) < 3e-3
        _done(res, "ypre")
    else:
        assert _rel(got, ref * aux.double()) < 3e-3


def test_linear_bf16_ex():
    _linear_bf16_ex_case(37, 50, 64, EF32)
    _linear_bf16_ex_case(528, 200, 192, GELU)
    _linear_bf16_ex_case(528, 96, 64, RESID)
    _linear_bf16_ex_case(300, 200, 64, GELU_BWD)
    _linear_bf16_ex_case(136, 96, 192, EF32, splits=3)


# ---- the reduction-major GEMMs of the backward (gemm_bf16_tr.hip): rows past K of the wgrad operands come from the zero page
def _zero_page():
    return In(torch.zeros(64, dtype=BF))                 # the documented 128 bytes of zeros, poison around them


@pytest.mark.parametrize("tile", [None, "2", "3", "4", "5"])
def test_linear_bf16_tr_dgrad(tile):
    lib = _lib.load()
    _lib.set_switch("LDIT_GEMM_BF16_TR_TILE", tile)
    for (M, N, K, epi) in ((37, 56, 64, EF32), (321, 96, 192, BIAS), (300, 200, 64, GELU_BWD)):
        lda, ldw = K + 32, N + 24
        ldy = N + 8 if epi == EF32 else N + 16
        a, w = _bf(400, M, K, scale=0.5), _bf(401, K, N, scale=0.1)
        s = {"a": In(a, ld=lda), "w": In(w, ld=ldw), "zeros": _zero_page(), "y": Out((M, N), F32 if epi == EF32 else BF, ld=ldy)}
        ref = a.double() @ w.double()
        if epi == GELU_BWD:
            aux = _bf(402, M, N, scale=0.5) + 0.5
            s["aux"] = In(aux)                           # row stride N (header)
            ref = ref * aux.double()

        def call(t):
            _lib.check(lib.ldit_linear_bf16_tr(_p(t["a"]), lda, 0, _p(t["w"]), ldw, _p(t["y"]), ldy, M, N, K, epi, _p(t.get("aux")), 1,
                                               _p(t["zeros"]), _s()))

        res = _twin(s, call)
        # test_gpu_train.py::test_dgrad_reads_the_weight_as_stored
        assert _rel(res.clean["y"], ref) < (1e-5 if epi == EF32 else 3e-3), (tile, M, N, K, epi)
        _done(res, "y")


@pytest.mark.parametrize("tile", [None, "2", "3", "6"])
def test_linear_bf16_tr_wgrad(tile):
    """dW[M, N] = A[K, M]^T . W[K, N] with K (tokens) no multiple of the 64-row k-tile: the rows behind the last token are 0xFF."""
    lib = _lib.load()
    _lib.set_switch("LDIT_GEMM_BF16_TR_TILE", tile)
    for (M, N, K, splits) in ((40, 56, 37, 1), (136, 264, 197, 1), (136, 96, 325, 3)):
        lda, ldw, ldy = M + 24, N + 32, N + 8
        a, w = _bf(410, K, M, scale=0.3), _bf(411, K, N, scale=0.3)
        s = {"a": In(a, ld=lda), "w": In(w, ld=ldw), "zeros": _zero_page(),
             "y": Out((splits * M, N), F32, ld=ldy, scratch=True)}       # the slab buffer is scratch: 0x00 / 0xFF before the call

        def call(t):
            _lib.check(lib.ldit_linear_bf16_tr(_p(t["a"]), lda, 1, _p(t["w"]), ldw, _p(t["y"]), ldy, M, N, K, EF32, None, splits,
                                               _p(t["zeros"]), _s()))

        res = _twin(s, call)
        _done(res, "y")
        got = res.clean["y"]
        if splits > 1:
            red = {"slabs": In(got.reshape(-1)), "out": Out((M * N,), F32)}
            rr = _twin(red, lambda t: _lib.check(lib.ldit_reduce_slabs_f32(_p(t["slabs"]), _p(t["out"]), M * N, splits, _s())))
            _done(rr, "out")
            got = rr.clean["out"].reshape(M, N)
        # test_gpu_train.py::test_wgrad_reads_both_operands_token_major
        assert _rel(got, a.double().T @ w.double()) < 1e-5, (tile, M, N, K, splits)


# ---- fp8 (per-tensor / per-channel scales): LDIT_GEMM_FP8_TILE 0..4 and auto; <= 64 rows run on gemm_fp8_tail
def _fp8_codes(x, scale):
    """tests/test_gpu_fp8.py::_torch_quant"""
    return (x * torch.tensor(np.float32(1.0 / float(scale)))).clamp(-448.0, 448.0).to(F8)


def _gelu_lp(z):
    """The logistic form the low-precision epilogues evaluate (csrc/ldit_common.h gelu_lp), float64."""
    return z / (1.0 + torch.exp(-(1.5957691216 * z + 0.0713548163 * z ** 3)))


def _linear_fp8_case(M, N, K, epi, mode, per_channel, seed=500):
    lib = _lib.load()
    ydt = {BIAS: BF, GELU: F8, RESID: F32}[epi]
    lda = K + 32
    ldy = {BIAS: _up(N, 8) + 16, GELU: _up(N, 16) + 32, RESID: _up(N, 4) + 8}[epi]
    # operands as tests/test_gpu_fp8.py makes them: x ~ N(0, 1), w ~ N(0, 0.05), each quantised with scale = amax / 448
    xf, wf = _f32(seed, M, K), _f32(seed + 1, N, K, scale=0.05)
    sx, sw = float(xf.abs().max()) / 448.0, float(wf.abs().max()) / 448.0
    x, w = _fp8_codes(xf, sx), _fp8_codes(wf, sw)
    ab = sx * sw
    s, r = _lin_common(M, N, epi, mode, ydt, ldy, seed)
    s.update(x=In(x, ld=lda), w=In(w))
    mul = torch.tensor(float(np.float32(ab)), dtype=torch.float64)
    if per_channel:
        ws = _f32(seed + 6, N).abs() + 0.5
        s["ws"] = In(ws)
        mul = mul * ws.double()
    pre = _lin_ref(x.float(), w.float(), s, BIAS, None, mul=mul)
    so = float(_gelu_lp(pre).abs().max()) / 448.0 * 0.5      # half the range: the top values saturate (test_gpu_fp8.py)

    def call(t):
        lam, R, y2 = _resid_args(t, epi, mode)
        _lib.check(lib.ldit_linear_fp8(_p(t["x"]), lda, _p(t["w"]), _p(t["b"]), _p(t["y"]), ldy, M, N, K, epi, lam, R, y2, ab, 1.0 / so,
                                       _p(t.get("ws")), _s()))

    res = _twin(s, call)
    got = res.clean["y"]
    _done(res, "y")
    if epi == BIAS:        # test_gpu_fp8.py::test_linear_fp8_bias
        assert _rel(got, pre) < 3e-3 and _mrel(got, pre) < 1.6e-2
    elif epi == RESID:     # test_gpu_fp8.py::test_linear_fp8_scale_residual_fp32
        ref = r.double() + s["lam"].data.double() * pre
        assert _rel(got, ref) < 1e-4 and _mrel(got, ref) < 1e-3
        assert torch.equal(res.poisoned["y2"], res.poisoned["y"])
    else:                  # test_gpu_fp8.py::test_linear_fp8_gelu_requantised
        ref = _gelu_lp(pre).float()
        want = _fp8_codes(ref, so).float().numpy()
        gv = got.float().numpy()
        assert np.isfinite(gv).all() and np.abs(gv).max() == 448.0          # the top values saturate, they do not turn NaN
        differ = gv != want                                                  # by value: +0 and -0 are the same number
        print(f"fp8 GELU {M}x{N}x{K}: {differ.mean():.2e} of the codes differ from the torch quantisation")
        assert differ.mean() < 1e-2, differ.mean()                           # rounding-boundary cases only
        bad = np.abs(gv - want) > np.maximum(np.abs(want) * 0.125, 2.0 ** -9) + 1.2e-3 / so
        assert not bad.any(), int(bad.sum())


@pytest.mark.parametrize("tile", ["auto", "0", "1", "2", "3", "4"])
def test_linear_fp8(tile):
    if tile != "auto":
        _lib.set_switch("LDIT_GEMM_FP8_TILE", tile)
    _linear_fp8_case(37, 50, 128, BIAS, None, per_channel=True)
    _linear_fp8_case(528, 200, 384, GELU, None, per_channel=False)
    if tile != "4":        # the 320-row tile has no scale + residual instantiation (tests/test_gpu_mxfp8.py::_check_exact)
        _linear_fp8_case(528, 96, 128, RESID, "inplace", per_channel=True)
    if tile == "auto":
        _linear_fp8_case(37, 257, 384, RESID, "separate", per_channel=False)
        _linear_fp8_case(1040, 96, 128, BIAS, None, per_channel=False)


# ---- mxfp8 (block scales in the MFMA): K, lda % 128 == 0, so the gap columns lie behind the operand's own
def _mx_operand(seed, rows, K, scale):
    x = _f32(seed, rows, K, scale=scale).numpy()
    codes, scales, _ = mx_quant_ref(x)
    return torch.from_numpy(codes).view(F8), torch.from_numpy(scales), torch.from_numpy(mx_dequant(codes, scales))


def _mx_gate_gelu(codes, scales, pre):
    """tests/test_gpu_mxfp8.py::test_linear_mxfp8_gelu_writes_mx, every clause: block scales equal except where an amax sits on a
    power-of-two boundary within the MFMA's error, codes equal except a small fraction one step away, all within the envelope."""
    M, N = pre.shape
    ref32 = _gelu_lp(pre).float().numpy()
    ref = ref32.astype(np.float64)
    gs = scales.numpy()
    gc = codes.view(torch.uint8).numpy()
    wc, wsc, _ = mx_quant_ref(ref32)
    amax = np.abs(ref32.reshape(M, N // 32, 32)).max(-1).astype(np.float64)
    tol = 1e-3 * np.maximum(np.abs(pre.numpy()).reshape(M, N // 32, 32).max(-1), 1.0)
    boundary = mx_exponent(amax - tol) != mx_exponent(amax + tol)
    assert np.all((gs == wsc) | boundary), int(((gs != wsc) & ~boundary).sum())
    assert (gs != wsc).mean() < 1e-2
    gv = mx_dequant(gc, gs)
    differ = (gv != mx_dequant(wc, wsc)) & np.repeat(gs == wsc, 32, axis=1)
    print(f"mx GELU {M}x{N}: scales differ {(gs != wsc).mean():.2e}, codes differ {differ.mean():.2e}")
    assert differ.mean() < 1e-2, differ.mean()
    step = np.repeat(np.ldexp(1.0, gs.astype(np.int64) - 127), 32, axis=1)
    bad = np.abs(gv - ref) > np.maximum(np.abs(ref) * 0.0625, 2.0 ** -9 * step) + 1.2e-3 * np.maximum(np.abs(pre.numpy()), 1.0)
    assert not bad.any(), int(bad.sum())


def _linear_mxfp8_case(M, N, K, epi, mode, train, seed=600):
    lib = _lib.load()
    ydt = {BIAS: BF, GELU: F8, RESID: F32}[epi]
    lda = K + 128
    ldy = {BIAS: _up(N, 8) + 16, GELU: N + 32, RESID: _up(N, 4) + 8}[epi]
    xc, xs, xv = _mx_operand(seed, M, K, 1.0)
    wc, ws, wv = _mx_operand(seed + 1, N, K, 0.05)
    s, r = _lin_common(M, N, epi, mode, ydt, ldy, seed)
    s.update(x=In(xc, ld=lda, col0=0), xs=In(xs, ld=lda // 32, col0=0), w=In(wc), ws=In(ws))
    rs = None
    if epi == GELU:
        s["y"] = Out((M, N), F8, ld=ldy, col0=0)
        s["ys"] = Out((M, N // 32), torch.uint8, ld=ldy // 32, col0=0)
    if train:
        s["ypre"] = Out((M, N), BF, ld=ldy, col0=0 if epi == GELU else None)
        if epi == GELU:
            s["yd"] = Out((M, N), BF, ld=ldy, col0=0)
        else:
            rs = torch.from_numpy((np.arange(M) % 3 != 0).astype(np.float32) / 0.9)
            s["rs"] = In(rs)
    pre = xv @ wv.T + s["b"].data.double()

    def call(t):
        lam, R, y2 = _resid_args(t, epi, mode)
        if train:
            _lib.check(lib.ldit_linear_mxfp8_train(_p(t["x"]), lda, _p(t["xs"]), _p(t["w"]), _p(t["ws"]), _p(t["b"]), _p(t["y"]), ldy,
                                                   _p(t.get("ys")), M, N, K, epi, lam, R, y2, _p(t["ypre"]), _p(t.get("rs")),
                                                   _p(t.get("yd")), _s()))
        else:
            _lib.check(lib.ldit_linear_mxfp8(_p(t["x"]), lda, _p(t["xs"]), _p(t["w"]), _p(t["ws"]), _p(t["b"]), _p(t["y"]), ldy,
                                             _p(t.get("ys")), M, N, K, epi, lam, R, y2, _s()))

    res = _twin(s, call)
    got = res.clean["y"]
    guarded.assert_written(res.poisoned["y"], "y")
    if epi == BIAS:        # tests/test_gpu_mxfp8.py::test_linear_mxfp8_bias_and_scale_residual
        assert _rel(got, pre) < 3e-3 and _mrel(got, pre) < 1.6e-2
        _done(res, "y")
    elif epi == RESID:
        lam = s["lam"].data.double() if rs is None else rs.double()[:, None] * s["lam"].data.double()
        ref = r.double() + lam * pre
        assert _rel(got, ref) < 1e-4 and _mrel(got, ref) < 1e-3
        assert torch.equal(res.poisoned["y2"], res.poisoned["y"])
        _done(res, "y")
        if train:          # tests/test_gpu_mxfp8_qat.py::test_linear_mxfp8_train_epilogues: the branch output before LayerScale
            assert float((res.clean["ypre"].double() - pre).abs().max()) <= 1e-2 * max(1.0, float(pre.abs().max()))
            _done(res, "ypre")
    else:
        _mx_gate_gelu(got, res.clean["ys"], pre)
        assert not bool((res.poisoned["ys"] == 0xFF).any())           # (b): no block reports Inf / NaN
        if train:          # tests/test_gpu_mxfp8_qat.py::test_linear_mxfp8_train_epilogues: Yd is the dequantised output, exactly
            deq = mx_dequant(got.view(torch.uint8).numpy(), res.clean["ys"].numpy())
            assert np.array_equal(res.clean["yd"].double().numpy(), deq)
            z = pre.clone().requires_grad_(True)
            _gelu_lp(z).sum().backward()
            assert float((res.clean["ypre"].double() - z.grad).abs().max()) < 2e-2
            _done(res, "ypre", "yd")


@pytest.mark.parametrize("tile", ["auto", "0", "1", "2", "3", "4"])
def test_linear_mxfp8(tile):
    if tile != "auto":
        _lib.set_switch("LDIT_GEMM_FP8_TILE", tile)
    _linear_mxfp8_case(37, 50, 128, BIAS, None, train=False)
    _linear_mxfp8_case(528, 96, 384, GELU, None, train=False)
    if tile != "4":
        _linear_mxfp8_case(528, 200, 128, RESID, "inplace", train=False)
    if tile == "auto":
        _linear_mxfp8_case(37, 257, 384, RESID, "separate", train=False)


@pytest.mark.parametrize("tile", ["auto", "0", "2"])
def test_linear_mxfp8_train(tile):
    if tile != "auto":
        _lib.set_switch("LDIT_GEMM_FP8_TILE", tile)
    _linear_mxfp8_case(37, 96, 128, GELU, None, train=True)
    _linear_mxfp8_case(528, 200, 384, RESID, "inplace", train=True)
    _linear_mxfp8_case(528, 64, 128, RESID, "separate", train=True)


# ---- split-fp32 (2 / 3 bf16 planes per value)
def _split(x, planes):
    """The planes of include/ldit.h: p0 = bf16(x), p1 = bf16(x - p0), p2 = bf16(x - p0 - p1), side by side."""
    p0 = x.to(BF)
    r1 = x - p0.float()
    p1 = r1.to(BF)
    p2 = (r1 - p1.float()).to(BF)
    return torch.cat([p0, p1, p2][:planes], dim=-1)


def _planes_sum(p, planes):
    c = p.shape[-1] // planes
    return sum(p[..., i * c:(i + 1) * c].double() for i in range(planes))


@pytest.mark.parametrize("planes", [2, 3])
def test_linear_planes(planes):
    lib = _lib.load()
    for (M, N, K, epi, mode) in ((37, 50, 64, BIAS, None), (528, 96, 192, RESID, "inplace"), (528, 200, 64, GELU, None),
                                 (37, 257, 192, RESID, "separate")):
        seed = 700
        lda = planes * K + 32
        ldy = planes * N if epi == GELU else _up(N, 4) + 8          # the GELU epilogue writes planes: ldy = planes * N (header)
        x, w = _f32(seed, M, K), _f32(seed + 1, N, K, scale=0.1)
        s, r = _lin_common(M, N, epi, mode, F32, ldy, seed)
        if epi == GELU:
            s["y"] = Out((M, planes * N), BF)
        s.update(x=In(_split(x, planes), ld=lda), w=In(_split(w, planes)))

        def call(t):
            lam, R, y2 = _resid_args(t, epi, mode)
            _lib.check(lib.ldit_linear_planes(_p(t["x"]), lda, _p(t["w"]), _p(t["b"]), _p(t["y"]), ldy, M, N, K, epi, lam, R, y2, planes, _s()))

        res = _twin(s, call)
        ref = _lin_ref(x, w, s, epi, r)
        got = res.clean["y"]
        _done(res, "y")
        # tests/test_gpu_split_fp32.py::test_linear_planes_vs_float64
        if epi == GELU:
            assert _rel(_planes_sum(got, planes), ref) < (2e-5 if planes == 2 else 2e-6)
        else:
            assert _rel(got, ref) < (1.5e-5 if planes == 2 else 1.5e-6)


# =========================================================================================================== attention
# q, k and v are column slices of ONE fused tensor whose row stride exceeds 3C: poison in the gap columns, in front of token 0 and
# behind the last token of the last image.  B = 2, H = 2, D = 64.
AB, AH, AD = 2, 2, 64
AC = AH * AD


def _qkv(seed, B, N, Cc=AC, dtype=F32, dominant=None):
    t = _f32(seed, B, N, 3 * Cc)
    if dominant is not None:                             # test_attention_large_logits_force_rescale: a dominant LAST-chunk key
        key, query = dominant
        t[0, key, Cc:2 * Cc] = 6.0 * t[0, query, :Cc]
        t[0, query, :Cc] *= 3.0
    return t.to(dtype)


def _attn_ref(qkv, H, scale=None, log2_domain=False):
    B, N, C3 = qkv.shape
    Cc = C3 // 3
    D = Cc // H
    q, k, v = (qkv[..., i * Cc:(i + 1) * Cc].double().view(B, N, H, D).transpose(1, 2) for i in range(3))
    sc = q @ k.transpose(-1, -2) * (np.log(2.0) if log2_domain else (D ** -0.5 if scale is None else scale))
    o = (torch.softmax(sc, -1) @ v).transpose(1, 2).reshape(B, N, Cc)
    return o, torch.logsumexp(sc, -1) / np.log(2.0)


def _slices(t, Cc=AC):
    return t[..., :Cc], t[..., Cc:2 * Cc], t[..., 2 * Cc:3 * Cc]


@pytest.mark.parametrize("B,N,H,dominant", [(AB, 1, AH, None), (AB, 33, AH, None), (AB, 225, AH, None), (1, 449, 1, (440, 7))])
def test_attention_f32(B, N, H, dominant):
    lib = _lib.load()
    Cc = H * AD
    qkv = _qkv(800 + N, B, N, Cc, dominant=dominant)
    ld, ldo = 3 * Cc + 32, Cc + 16
    s = {"qkv": In(qkv, ld=ld), "o": Out((B, N, Cc), F32, ld=ldo)}

    def call(t):
        q, k, v = _slices(t["qkv"], Cc)
        _lib.check(lib.ldit_attention_f32(_p(q), _p(k), _p(v), _p(t["o"]), B, N, H, AD, ld, ld, ld, ldo, AD ** -0.5, _s()))

    res = _twin(s, call)
    ref, _ = _attn_ref(qkv, H)
    if dominant:           # test_gpu_ops.py::test_attention_large_logits_force_rescale
        assert _mrel(res.clean["o"], ref) < 1e-5
    else:                  # test_gpu_ops.py::test_attention_ragged_lengths
        assert _rel(res.clean["o"], ref) < 1e-5
    _done(res, "o")


@pytest.mark.parametrize("N,prescaled", [(33, False), (257, False), (257, True)])
def test_attention_bf16(N, prescaled):
    lib = _lib.load()
    qkv = _qkv(810 + N, AB, N)
    if prescaled:
        qkv[..., :AC] *= AD ** -0.5 * np.log2(np.e)
    qkv = qkv.to(BF)
    ld, ldo = 3 * AC + 32, AC + 16
    s = {"qkv": In(qkv, ld=ld), "o": Out((AB, N, AC), BF, ld=ldo)}

    def call(t):
        q, k, v = _slices(t["qkv"])
        _lib.check(lib.ldit_attention_bf16(_p(q), _p(k), _p(v), _p(t["o"]), AB, N, AH, AD, ld, ld, ld, ldo,
                                           0.0 if prescaled else AD ** -0.5, _s()))

    res = _twin(s, call)
    ref, _ = _attn_ref(qkv.float(), AH, log2_domain=prescaled)
    assert _rel(res.clean["o"], ref) < 6e-3              # test_gpu_bf16.py::test_attention_bf16, _prescaled_queries
    _done(res, "o")


@pytest.mark.parametrize("N", [33, 257])
def test_attention_fwd_lse_and_bwd_bf16(N):
    lib = _lib.load()
    qkv = _qkv(820 + N, AB, N, dtype=BF)
    do = _bf(821 + N, AB, N, AC, scale=0.5)
    ld, ldo, lddo, ldd = 3 * AC + 32, AC + 16, AC + 24, 3 * AC + 40
    s = {"qkv": In(qkv, ld=ld), "o": Out((AB, N, AC), BF, ld=ldo), "lse": Out((AB, AH, N), F32)}

    def fwd(t):
        q, k, v = _slices(t["qkv"])
        _lib.check(lib.ldit_attention_fwd_lse_bf16(_p(q), _p(k), _p(v), _p(t["o"]), _p(t["lse"]), AB, N, AH, AD, ld, ld, ld, ldo,
                                                   AD ** -0.5, _s()))

    res = _twin(s, fwd)
    _done(res, "o", "lse")
    q64 = qkv.double().requires_grad_(True)
    ro, rl = _attn_ref(q64, AH)
    (ro * do.double()).sum().backward()
    # test_gpu_train.py::test_attention_forward_lse_and_backward
    assert _rel(res.clean["o"], ro.detach()) < 6e-3
    np.testing.assert_allclose(res.clean["lse"].numpy(), rl.detach().numpy(), atol=2e-3)
    # the backward reads the forward's own O and lse, each from a poisoned parent; dq | dk | dv are slices of one fused gradient
    b = {"qkv": In(qkv, ld=ld), "o": In(res.clean["o"], ld=ldo), "do": In(do, ld=lddo), "lse": In(res.clean["lse"]),
         "d": Out((AB, N, 3 * AC), BF, ld=ldd)}

    def bwd(t):
        q, k, v = _slices(t["qkv"])
        dq, dk, dv = _slices(t["d"])
        _lib.check(lib.ldit_attention_bwd_bf16(_p(q), _p(k), _p(v), _p(t["o"]), _p(t["do"]), _p(t["lse"]), _p(dq), _p(dk), _p(dv), AB, N,
                                               AH, AD, ld, ldo, lddo, ldd, AD ** -0.5, _s()))

    rb = _twin(b, bwd)
    _done(rb, "d")
    for i, name in enumerate(("dq", "dk", "dv")):
        sl = slice(i * AC, (i + 1) * AC)
        assert _rel(rb.clean["d"][..., sl], q64.grad[..., sl]) < 1.5e-2, name


@pytest.mark.parametrize("planes", [2, 3])
@pytest.mark.parametrize("N", [33, 130])
def test_attention_planes(planes, N):
    lib = _lib.load()
    qkv = _qkv(830 + N, AB, N)
    qkv[0, :, :AD] *= 6.0                                # scores of +-50: the deferred rescale (test_attention_planes_vs_float64)
    qkv[..., :AC] *= np.float32(AD ** -0.5 * 1.4426950408889634)
    xp = _split(qkv.reshape(AB * N, 3 * AC), planes)     # [rows, planes * 3C]: plane s of a row 3C elements further
    ld_in, ldo = planes * 3 * AC + 32, planes * AC + 16
    s = {"qkv": In(xp, ld=ld_in), "o": Out((AB * N, planes * AC), BF, ld=ldo)}

    def call(t):
        q, k, v = _slices(t["qkv"])
        _lib.check(lib.ldit_attention_planes(_p(q), _p(k), _p(v), _p(t["o"]), AB, N, AH, AD, ld_in, 3 * AC, ldo, planes, _s()))

    res = _twin(s, call)
    ref, _ = _attn_ref(qkv, AH, log2_domain=True)
    got = _planes_sum(res.clean["o"], planes).reshape(AB, N, AC)
    assert _rel(got, ref) < (2e-5 if planes == 2 else 2e-6)           # tests/test_gpu_split_fp32.py::test_attention_planes_vs_float64
    _done(res, "o")


@pytest.mark.parametrize("N", [17, 257])
def test_attention_mxfp8_train(N):
    lib = _lib.load()
    qkv = _qkv(840 + N, AB, N)
    qkv[..., :AC] *= AD ** -0.5 * np.log2(np.e)          # the packed builds' fold: scale = 0
    qkv = qkv.to(BF)
    ld, ldo = 3 * AC + 32, AC + 32                       # ldo % 32 == 0
    rows = AB * N
    s = {"qkv": In(qkv, ld=ld), "o": Out((rows, AC), F8, ld=ldo, col0=0), "os": Out((rows, AC // 32), torch.uint8, ld=ldo // 32, col0=0),
         "lse": Out((AB, AH, N), F32), "ob": Out((rows, AC), BF, ld=ldo, col0=0), "od": Out((rows, AC), BF, ld=ldo, col0=0)}

    def call(t):
        q, k, v = _slices(t["qkv"])
        _lib.check(lib.ldit_attention_mxfp8_train(_p(q), _p(k), _p(v), _p(t["o"]), _p(t["os"]), _p(t["lse"]), _p(t["ob"]), _p(t["od"]),
                                                  AB, N, AH, AD, ld, ld, ld, ldo, 0.0, _s()))

    res = _twin(s, call)
    ref, rl = _attn_ref(qkv.float(), AH, log2_domain=True)
    # Ob and lse against an independent float64 reference with the bf16 attention's own gates (test_gpu_bf16.py::test_attention_bf16:
    # rel-L2 6e-3; test_gpu_train.py::test_attention_forward_lse_and_backward: lse to 2e-3) - the qat test compares them with the bf16
    # kernel instead, which is no independent oracle.  From tests/test_gpu_mxfp8_qat.py::test_attention_mxfp8_train_outputs: Od is the
    # codes' exact values, and the codes quantise O to within 0.07 of its peak
    assert _rel(res.clean["ob"].reshape(AB, N, AC), ref) < 6e-3
    np.testing.assert_allclose(res.clean["lse"].numpy(), rl.numpy(), atol=2e-3)
    deq = mx_dequant(res.clean["o"].view(torch.uint8).numpy(), res.clean["os"].numpy())
    assert np.array_equal(res.clean["od"].double().numpy(), deq)
    ob = res.clean["ob"].double().numpy()
    assert np.abs(deq - ob).max() <= 0.07 * np.abs(ob).max()
    _done(res, "lse", "ob", "od")
    guarded.assert_written(res.poisoned["o"], "o")
    assert not bool((res.poisoned["os"] == 0xFF).any())


# ============================================================================================== row and column kernels
LN_SHAPES = [(1, 64), (5, 192), (65, 64), (65, 768)]


def _ln_inputs(rows, Cc):
    x = _f32(900 + rows + Cc, rows, Cc, scale=3.0) + 1.5
    return x, 1.0 + 0.1 * _f32(901, Cc), 0.1 * _f32(902, Cc)


def _ln_ref(x, g, b, eps=1e-12):
    return F.layer_norm(x.double(), (x.shape[-1],), g.double(), b.double(), eps)


def _ln_kernel(x, g, b):
    """The fp32 kernel's own rows, which the planes / MX variants are defined to split / quantise (their tests' gates)."""
    return ops.layernorm(x.to(DEV), g.to(DEV), b.to(DEV), eps=1e-12).cpu()


@pytest.mark.parametrize("rows,Cc", LN_SHAPES)
def test_layernorm_f32_and_planes(rows, Cc):
    lib = _lib.load()
    x, g, b = _ln_inputs(rows, Cc)
    s = {"x": In(x), "g": In(g), "b": In(b), "y": Out((rows, Cc), F32)}
    res = _twin(s, lambda t: _lib.check(lib.ldit_layernorm_f32(_p(t["x"]), _p(t["g"]), _p(t["b"]), _p(t["y"]), rows, Cc, 1e-12, _s())))
    assert _mrel(res.clean["y"], _ln_ref(x, g, b)) < 1e-5            # test_gpu_ops.py::test_layernorm_shapes
    _done(res, "y")
    for planes in (2, 3):  # tests/test_gpu_split_fp32.py::test_layernorm_planes_are_the_planes_of_the_fp32_layernorm
        s["y"] = Out((rows, planes * Cc), BF)
        rp = _twin(s, lambda t: _lib.check(lib.ldit_layernorm_f32_planes(_p(t["x"]), _p(t["g"]), _p(t["b"]), _p(t["y"]), rows, Cc, 1e-12,
                                                                         planes, _s())))
        assert torch.equal(rp.clean["y"], _split(res.clean["y"], planes))
        _done(rp, "y")


@pytest.mark.parametrize("rows,Cc", LN_SHAPES)
@pytest.mark.parametrize("train", [False, True])
def test_layernorm_mxfp8(rows, Cc, train):
    lib = _lib.load()
    x, g, b = _ln_inputs(rows, Cc)
    s = {"x": In(x), "g": In(g), "b": In(b), "y": Out((rows, Cc), F8), "ys": Out((rows, Cc // 32), torch.uint8)}
    if train:
        s["yd"] = Out((rows, Cc), BF)

    def call(t):
        if train:
            _lib.check(lib.ldit_layernorm_mxfp8_train(_p(t["x"]), _p(t["g"]), _p(t["b"]), _p(t["y"]), _p(t["ys"]), _p(t["yd"]), rows, Cc,
                                                      1e-12, _s()))
        else:
            _lib.check(lib.ldit_layernorm_mxfp8(_p(t["x"]), _p(t["g"]), _p(t["b"]), _p(t["y"]), _p(t["ys"]), rows, Cc, 1e-12, _s()))

    res = _twin(s, call)
    # tests/test_gpu_mxfp8.py::test_layernorm_mxfp8_is_the_mx_operand_of_the_fp32_layernorm
    wc, ws, _ = mx_quant_ref(_ln_kernel(x, g, b).numpy())
    assert np.array_equal(res.clean["ys"].numpy(), ws) and np.array_equal(res.clean["y"].view(torch.uint8).numpy(), wc)
    guarded.assert_written(res.poisoned["y"], "y")
    assert not bool((res.poisoned["ys"] == 0xFF).any())
    if train:              # tests/test_gpu_mxfp8_qat.py::test_layernorm_train_variant_is_the_inference_operand_plus_its_dequantised_copy
        assert np.array_equal(res.clean["yd"].double().numpy(), mx_dequant(wc, ws))
        _done(res, "yd")


@pytest.mark.parametrize("rows,Cc", LN_SHAPES)
def test_layernorm_bwd_f32(rows, Cc):
    """dh is a documented += destination: it keeps its values; the scratch is 0x00 / 0xFF."""
    lib = _lib.load()
    x, g, _ = _ln_inputs(rows, Cc)
    dy, dh0 = _f32(910, rows, Cc), _f32(911, rows, Cc)
    need = int(lib.ldit_layernorm_bwd_scratch_bytes(rows, Cc))
    s = {"dy": In(dy), "x": In(x), "g": In(g), "dh": Out((rows, Cc), F32, init=dh0), "dg": Out((Cc,), F32), "db": Out((Cc,), F32),
         "scratch": Scratch(need)}

    def call(t):
        _lib.check(lib.ldit_layernorm_bwd_f32(_p(t["dy"]), _p(t["x"]), _p(t["g"]), _p(t["dh"]), rows, Cc, 1e-12, _p(t["dg"]), _p(t["db"]),
                                              _p(t["scratch"]), need, _s()))

    res = _twin(s, call)
    xt, gt = x.double().requires_grad_(True), g.double().requires_grad_(True)
    bt = torch.zeros(Cc, dtype=torch.float64, requires_grad=True)
    (F.layer_norm(xt, (Cc,), gt, bt, 1e-12) * dy.double()).sum().backward()
    # test_gpu_train.py::test_layernorm_backward
    assert _rel(res.clean["dh"], dh0.double() + xt.grad) < 2e-5
    assert _rel(res.clean["dg"], gt.grad) < 2e-5 and _rel(res.clean["db"], bt.grad) < 2e-5
    _done(res, "dh", "dg", "db")


def _resid_ref(dh, z, lam, rs):
    gr = dh.double() * (1.0 if rs is None else rs.double()[:, None])
    return gr * lam.double(), (gr * z.double()).sum(0), (gr * lam.double()).sum(0)


def _resid_inputs(rows, Cc, rowscale):
    z, lam = _bf(912, rows, Cc), _f32(913, Cc).abs() * 0.3 + 0.05
    rs = ((torch.arange(rows) % 3 != 1).float() / 0.9) if rowscale else None
    return z, lam, rs


@pytest.mark.parametrize("rows,Cc", LN_SHAPES)
@pytest.mark.parametrize("rowscale", [False, True])
def test_layernorm_bwd_resid_f32(rows, Cc, rowscale):
    """The fused LayerNorm + LayerScale backward: dh is a documented += destination, dz and the four vectors are overwritten, the
    scratch is 0x00 / 0xFF.  C = 64 and 192 leave lanes of the wave without a vector (the gamma registers of those lanes)."""
    lib = _lib.load()
    x, g, _ = _ln_inputs(rows, Cc)
    dy, dh0 = _f32(910, rows, Cc), _f32(911, rows, Cc)
    z, lam, rs = _resid_inputs(rows, Cc, rowscale)
    need = int(lib.ldit_layernorm_bwd_resid_scratch_bytes(rows, Cc))
    s = {"dy": In(dy), "x": In(x), "g": In(g), "z": In(z), "lam": In(lam), "dh": Out((rows, Cc), F32, init=dh0),
         "dz": Out((rows, Cc), BF), "dg": Out((Cc,), F32), "db": Out((Cc,), F32), "dlam": Out((Cc,), F32), "dzb": Out((Cc,), F32),
         "scratch": Scratch(need)}
    if rowscale:
        s["rs"] = In(rs)

    def call(t):
        _lib.check(lib.ldit_layernorm_bwd_resid_f32(_p(t["dy"]), _p(t["x"]), _p(t["g"]), _p(t["z"]), _p(t["lam"]), _p(t.get("rs")),
                                                    _p(t["dh"]), _p(t["dz"]), rows, Cc, 1e-12, _p(t["dg"]), _p(t["db"]), _p(t["dlam"]),
                                                    _p(t["dzb"]), _p(t["scratch"]), need, _s()))

    res = _twin(s, call)
    xt, gt = x.double().requires_grad_(True), g.double().requires_grad_(True)
    bt = torch.zeros(Cc, dtype=torch.float64, requires_grad=True)
    (F.layer_norm(xt, (Cc,), gt, bt, 1e-12) * dy.double()).sum().backward()
    dh_ref = dh0.double() + xt.grad
    rdz, rdlam, rdzb = _resid_ref(dh_ref, z, lam, rs)
    # test_gpu_train.py::test_layernorm_backward (fp32 outputs); dz is one bf16 rounding of an fp32-grade value
    assert _rel(res.clean["dh"], dh_ref) < 2e-5
    assert _rel(res.clean["dg"], gt.grad) < 2e-5 and _rel(res.clean["db"], bt.grad) < 2e-5
    assert _rel(res.clean["dlam"], rdlam) < 2e-5 and _rel(res.clean["dzb"], rdzb) < 2e-5
    assert _rel(res.clean["dz"], rdz) < 3e-3
    _done(res, "dh", "dz", "dg", "db", "dlam", "dzb")


@pytest.mark.parametrize("rows,Cc", LN_SHAPES)
@pytest.mark.parametrize("rowscale", [False, True])
def test_resid_bwd_bf16(rows, Cc, rowscale):
    """The LayerScale / residual backward on its own: dh is only read; the scratch is 0x00 / 0xFF."""
    lib = _lib.load()
    dh = _f32(914, rows, Cc)
    z, lam, rs = _resid_inputs(rows, Cc, rowscale)
    need = int(lib.ldit_resid_bwd_scratch_bytes(rows, Cc))
    s = {"dh": In(dh), "z": In(z), "lam": In(lam), "dz": Out((rows, Cc), BF), "dlam": Out((Cc,), F32), "db": Out((Cc,), F32),
         "scratch": Scratch(need)}
    if rowscale:
        s["rs"] = In(rs)

    def call(t):
        _lib.check(lib.ldit_resid_bwd_bf16(_p(t["dh"]), _p(t["z"]), _p(t["lam"]), _p(t.get("rs")), _p(t["dz"]), rows, Cc, _p(t["dlam"]),
                                           _p(t["db"]), _p(t["scratch"]), need, _s()))

    res = _twin(s, call)
    rdz, rdlam, rdb = _resid_ref(dh, z, lam, rs)
    assert _rel(res.clean["dlam"], rdlam) < 2e-5 and _rel(res.clean["db"], rdb) < 2e-5
    assert _rel(res.clean["dz"], rdz) < 3e-3
    _done(res, "dz", "dlam", "db")


@pytest.mark.parametrize("M,N", [(1, 64), (5, 192), (65, 64), (513, 96)])
def test_colsum_and_colamax_f32(M, N):
    lib = _lib.load()
    x = _f32(920 + M, M, N)
    ldx = N + 16
    need = int(lib.ldit_colsum_scratch_bytes(M, N))
    s = {"x": In(x, ld=ldx), "out": Out((N,), F32), "scratch": Scratch(max(need, 16))}
    for fn, ref, gate in ((lib.ldit_colsum_f32, x.double().sum(0), 1e-6), (lib.ldit_colamax_f32, x.double().abs().amax(0), 0.0)):
        res = _twin(s, lambda t: _lib.check(fn(_p(t["x"]), M, N, ldx, _p(t["out"]), _p(t["scratch"]), need, _s())))
        # tests/test_gpu_fpn.py::test_fpn_backward_building_blocks (sum); a maximum of fp32 values is exact
        assert _rel(res.clean["out"], ref) <= gate
        _done(res, "out")


@pytest.mark.parametrize("rows,cols", [(1, 64), (5, 192), (65, 64)])
def test_split_and_quantisers(rows, cols):
    lib = _lib.load()
    x = _f32(930 + rows, rows, cols, scale=3.0)
    lds = cols + 36
    for planes in (2, 3):  # tests/test_gpu_split_fp32.py::test_split_planes_reconstruct_the_value (the planes' definition, bit for bit)
        s = {"x": In(x, ld=lds), "y": Out((rows, planes * cols), BF)}
        res = _twin(s, lambda t: _lib.check(lib.ldit_split_f32_planes(_p(t["x"]), lds, _p(t["y"]), rows, cols, planes, _s())))
        assert torch.equal(res.clean["y"], _split(x, planes))
        _done(res, "y")
    # ldit_quant_mx_f32_fp8 (lds > K): tests/test_gpu_mxfp8.py::test_quant_mx_bit_exact
    s = {"x": In(x, ld=lds), "y": Out((rows, cols), F8), "ys": Out((rows, cols // 32), torch.uint8)}
    res = _twin(s, lambda t: _lib.check(lib.ldit_quant_mx_f32_fp8(_p(t["x"]), lds, _p(t["y"]), _p(t["ys"]), rows, cols, _s())))
    wc, ws, _ = mx_quant_ref(x.numpy())
    assert np.array_equal(res.clean["ys"].numpy(), ws) and np.array_equal(res.clean["y"].view(torch.uint8).numpy(), wc)
    # ldit_quant_rows_f32_fp8: scales[n] = max|W[n, :]| / 448, codes = fp8(W / scale) (header; per-channel test in test_gpu_fp8.py)
    s = {"x": In(x), "y": Out((rows, cols), F8), "sc": Out((rows,), F32)}
    res = _twin(s, lambda t: _lib.check(lib.ldit_quant_rows_f32_fp8(_p(t["x"]), _p(t["y"]), _p(t["sc"]), rows, cols, _s())))
    sc = res.clean["sc"]
    # tests/test_gpu_fp8.py::test_per_channel_weight_scales_rescue_small_rows: the scales to 1e-6, the codes those of torch's cast
    # of w * (1 / scale) except at ties of the reciprocal's rounding (below 1e-3 of them)
    np.testing.assert_allclose(sc.numpy(), (x.abs().amax(1) / np.float32(448.0)).numpy(), rtol=1e-6)
    want = (x * (1.0 / sc)[:, None]).clamp(-448.0, 448.0).to(F8)
    differ = (res.clean["y"].view(torch.uint8) != want.view(torch.uint8)).float().mean().item()
    print(f"quant_rows {rows}x{cols}: {differ:.2e} of the codes differ from torch's cast")
    assert differ < 1e-3
    _done(res, "y", "sc")


@pytest.mark.parametrize("n", [1, 4, 1027])
def test_flat_kernels(n):
    lib = _lib.load()
    x = _f32(940 + n, n, scale=30.0)
    x[: min(n, 4)] = torch.tensor([447.9, -500.0, 0.0, 1.00390625])[: min(n, 4)]
    # the three casts: round to nearest even, torch's own conversion (test_gpu_bf16.py::test_cast_matches_torch_round_to_nearest_even)
    for fn, src, ydt in ((lib.ldit_cast_f32_bf16, x, BF), (lib.ldit_cast_f32_f16, x, torch.float16), (lib.ldit_cast_f16_f32, x.half(), F32)):
        s = {"x": In(src), "y": Out((n,), ydt)}
        res = _twin(s, lambda t: _lib.check(fn(_p(t["x"]), _p(t["y"]), n, _s())))
        assert torch.equal(res.clean["y"], src.to(ydt))
        _done(res, "y")
    # ldit_quant_f32_fp8: test_gpu_fp8.py::test_quant_matches_torch_bit_for_bit
    inv = np.float32(1.0 / 0.37)
    s = {"x": In(x), "y": Out((n,), F8)}
    res = _twin(s, lambda t: _lib.check(lib.ldit_quant_f32_fp8(_p(t["x"]), _p(t["y"]), n, float(inv), _s())))
    want = (x * torch.tensor(inv)).clamp(-448.0, 448.0).to(F8)
    assert torch.equal(res.clean["y"].view(torch.uint8), want.view(torch.uint8))
    _done(res, "y")
    # ldit_amax_f32: test_gpu_fp8.py::test_amax
    s = {"x": In(x), "out": Out((1,), F32)}
    res = _twin(s, lambda t: _lib.check(lib.ldit_amax_f32(_p(t["x"]), n, _p(t["out"]), _s())))
    assert float(res.clean["out"][0]) == float(x.abs().max())
    _done(res, "out")


@pytest.mark.parametrize("B,H,W,Cc", [(2, 1, 1, 32), (2, 5, 9, 64), (1, 7, 7, 96)])
def test_pad_nhwc_f32_bf16(B, H, W, Cc):
    lib = _lib.load()
    x = _f32(950, B, H, W, Cc)
    s = {"x": In(x), "y": Out((B, H + 2, W + 2, Cc), BF)}
    res = _twin(s, lambda t: _lib.check(lib.ldit_pad_nhwc_f32_bf16(_p(t["x"]), _p(t["y"]), B, H, W, Cc, _s())))
    assert torch.equal(res.clean["y"], F.pad(x, (0, 0, 1, 1, 1, 1)).to(BF))     # tests/test_gpu_fpn.py::test_fpn_backward_building_blocks
    _done(res, "y")


# ================================================================================================================ maps
def _embed_ref(x, pw, pb, cls, pos, p):
    B, Cc = x.shape[0], pw.shape[0]
    t = F.conv2d(x.double(), pw.double().reshape(Cc, x.shape[1], p, p), pb.double(), stride=p).flatten(2).transpose(1, 2)
    return torch.cat([(cls.double() + pos.double()[0]).expand(B, 1, Cc), t + pos.double()[1:]], dim=1)


EMBED_CASES = [(2, 16, 16, 32), (2, 80, 144, 64), (1, 112, 112, 96)]      # grids 1 x 1, 5 x 9, 7 x 7 at patch 16


def _embed_inputs(B, H, W, Cc):
    T = (H // 16) * (W // 16) + 1
    x = torch.from_numpy(np.random.default_rng(1000 + H).uniform(0, 1, (B, 3, H, W)).astype(np.float32))
    return x, _f32(1001, Cc, 3 * 256, scale=0.02), _f32(1002, Cc, scale=0.02), _f32(1003, Cc, scale=0.02), _f32(1004, T, Cc, scale=0.02), T


@pytest.mark.parametrize("B,H,W,Cc", EMBED_CASES)
def test_embed_f32_and_bf16(B, H, W, Cc):
    lib = _lib.load()
    x, pw, pb, cls, pos, T = _embed_inputs(B, H, W, Cc)
    s = {"x": In(x), "pw": In(pw), "pb": In(pb), "cls": In(cls), "pos": In(pos), "out": Out((B, T, Cc), F32)}
    res = _twin(s, lambda t: _lib.check(lib.ldit_embed_f32(_p(t["x"]), _p(t["pw"]), _p(t["pb"]), _p(t["cls"]), _p(t["pos"]), _p(t["out"]),
                                                           B, 3, H, W, 16, Cc, _s())))
    ref = _embed_ref(x, pw, pb, cls, pos, 16)
    assert _rel(res.clean["out"], ref) < 1e-5 and _mrel(res.clean["out"], ref) < 1e-5        # test_gpu_ops.py::test_embed
    _done(res, "out")
    # the bf16 embedding: its im2col scratch is 0x00 / 0xFF before the call
    s.update(pw=In(pw.to(BF)), scratch=Scratch(B * (T - 1) * 768 * 2))
    res = _twin(s, lambda t: _lib.check(lib.ldit_embed_bf16(_p(t["x"]), _p(t["pw"]), _p(t["pb"]), _p(t["cls"]), _p(t["pos"]), _p(t["out"]),
                                                            _p(t["scratch"]), B, 3, H, W, 16, Cc, _s())))
    ref = _embed_ref(x.to(BF), pw.to(BF), pb, cls, pos, 16)
    # test_gpu_ops.py::test_embed_bf16_is_the_oracle_embedding_of_the_bf16_rounded_operands
    assert _rel(res.clean["out"], ref) < 1e-5 and _mrel(res.clean["out"], ref) < 1e-5
    _done(res, "out")


def _image_list(t, names):
    n = len(names)
    return ((C.c_void_p * n)(*[t[k].data_ptr() for k in names]), (C.c_int32 * n)(*[t[k].shape[1] for k in names]),
            (C.c_int32 * n)(*[t[k].shape[2] for k in names]))


@pytest.mark.parametrize("half", [False, True])
def test_preprocess_and_embed_bf16_images(half):
    """Ragged images 33 x 17 and 64 x 64, each in a parent of its own, resized to 64 x 64."""
    lib = _lib.load()
    rng = np.random.default_rng(1010)
    imgs = [torch.from_numpy(rng.uniform(0, 1, (3, h, w)).astype(np.float32)) for h, w in ((33, 17), (64, 64))]
    if half:
        imgs = [a.half() for a in imgs]
    names = ["img0", "img1"]
    s = {k: In(a) for k, a in zip(names, imgs)}
    s["out"] = Out((2, 3, 64, 64), F32)
    fn = lib.ldit_preprocess_f16 if half else lib.ldit_preprocess_f32

    def call(t):
        ptrs, hs, ws = _image_list(t, names)
        _lib.check(fn(ptrs, hs, ws, 2, 3, 0.5, 0.5, 64, 64, _p(t["out"]), _s()))

    res = _twin(s, call)
    for i, a in enumerate(imgs):       # test_gpu_ops.py::test_preprocess_variable_sizes_vs_oracle_and_torch
        ref = F.interpolate(((a.float() - 0.5) / 0.5)[None], size=(64, 64), mode="bilinear", align_corners=False)[0]
        assert float((res.clean["out"][i] - ref).abs().max()) < 2e-5
    _done(res, "out")
    # the same transform fused into the bf16 patch-embedding load
    Cc, T = 32, 17
    _, pw, pb, cls, pos, _ = _embed_inputs(2, 64, 64, Cc)
    s = {k: In(a) for k, a in zip(names, imgs)}
    s.update(pw=In(pw.to(BF)), pb=In(pb), cls=In(cls), pos=In(pos), out=Out((2, T, Cc), F32), scratch=Scratch(2 * 16 * 768 * 2))

    def call2(t):
        ptrs, hs, ws = _image_list(t, names)
        _lib.check(lib.ldit_embed_bf16_images(ptrs, hs, ws, int(half), 0.5, 0.5, _p(t["pw"]), _p(t["pb"]), _p(t["cls"]), _p(t["pos"]),
                                              _p(t["out"]), _p(t["scratch"]), 2, 3, 64, 64, 16, Cc, _s()))

    res2 = _twin(s, call2)
    # tests/test_gpu_fpn.py::test_input_transform_fused_into_the_patch_embedding_load: the bits of transform-then-embed
    two_step = _embed_ref(res.clean["out"].to(BF), pw.to(BF), pb, cls, pos, 16)
    assert _rel(res2.clean["out"], two_step) < 1e-5 and _mrel(res2.clean["out"], two_step) < 1e-5
    plain = ops.embed_bf16(res.clean["out"].to(DEV), pw.to(BF).to(DEV), pb.to(DEV), cls.to(DEV), pos.to(DEV), 16).cpu()
    assert torch.equal(res2.clean["out"], plain)
    _done(res2, "out")


def _interp(m, scale):
    return m if scale == 1.0 else F.interpolate(m, scale_factor=scale, mode="bilinear", align_corners=False)


MAP_CASES = [(1, 1, 4.0, 32), (5, 9, 2.0, 64), (7, 7, 0.5, 96), (5, 9, 1.0, 32)]


@pytest.mark.parametrize("gh,gw,scale,Cc", MAP_CASES)
def test_tap_to_map_and_adjoint(gh, gw, scale, Cc):
    lib = _lib.load()
    B, oh, ow = 2, int(gh * scale), int(gw * scale)
    tap, g = _f32(1020, B, gh * gw + 1, Cc), _f32(1021, B, Cc, oh, ow)
    s = {"tap": In(tap), "out": Out((B, Cc, oh, ow), F32)}
    res = _twin(s, lambda t: _lib.check(lib.ldit_tap_to_map_f32(_p(t["tap"]), _p(t["out"]), B, gh, gw, Cc, scale, _s())))
    r = tap.double().requires_grad_(True)
    rm = _interp(r[:, 1:, :].permute(0, 2, 1).reshape(B, Cc, gh, gw), scale)
    (rm * g.double()).sum().backward()
    assert _mrel(res.clean["out"], rm.detach()) < 1e-6              # test_gpu_ops.py::test_tap_to_map_vs_oracle
    _done(res, "out")
    s = {"dmap": In(g), "dtap": Out((B, gh * gw + 1, Cc), F32)}
    res = _twin(s, lambda t: _lib.check(lib.ldit_tap_to_map_bwd_f32(_p(t["dmap"]), _p(t["dtap"]), B, gh, gw, Cc, scale, _s())))
    assert _rel(res.clean["dtap"], r.grad) < 1e-6                   # tests/test_gpu_fpn.py::test_tap_to_map_adjoint
    assert float(res.clean["dtap"][:, 0].abs().max()) == 0.0        # the CLS row is written as zeros
    _done(res, "dtap")


@pytest.mark.parametrize("gh,gw,scale,Ch", MAP_CASES)
@pytest.mark.parametrize("with_top", [True, False])
def test_fpn_merge_and_adjoint(gh, gw, scale, Ch, with_top):
    lib = _lib.load()
    B, oh, ow = 2, int(gh * scale), int(gw * scale)
    th, tw = (max(oh // 2, 1), max(ow // 2, 1)) if with_top else (0, 0)
    lat, g = _f32(1030, B, gh * gw + 1, Ch), _f32(1031, B, oh, ow, Ch)
    s = {"lat": In(lat), "out": Out((B, oh, ow, Ch), F32)}
    top = None
    if with_top:
        top = _f32(1032, B, th, tw, Ch)
        s["top"] = In(top)
    res = _twin(s, lambda t: _lib.check(lib.ldit_fpn_merge_f32(_p(t["lat"]), _p(t.get("top")), _p(t["out"]), B, gh, gw, Ch, scale, th, tw, _s())))
    rl = lat.double().requires_grad_(True)
    m = _interp(rl[:, 1:, :].permute(0, 2, 1).reshape(B, Ch, gh, gw), scale)
    rt = None
    if with_top:
        rt = top.double().requires_grad_(True)
        m = m + F.interpolate(rt.permute(0, 3, 1, 2), size=(oh, ow), mode="nearest")
    (m.permute(0, 2, 3, 1) * g.double()).sum().backward()
    assert _rel(res.clean["out"], m.detach().permute(0, 2, 3, 1)) < 1e-6         # tests/test_gpu_fpn.py::test_fpn_merge_level
    _done(res, "out")
    # the adjoint: d_lat is written (CLS row zero), d_top is a documented += destination and keeps its values
    s = {"g": In(g), "d_lat": Out((B, gh * gw + 1, Ch), F32)}
    seed = None
    if with_top:
        seed = _f32(1033, B, th, tw, Ch)
        s["d_top"] = Out((B, th, tw, Ch), F32, init=seed)
    res = _twin(s, lambda t: _lib.check(lib.ldit_fpn_merge_bwd_f32(_p(t["g"]), _p(t["d_lat"]), _p(t.get("d_top")), B, gh, gw, Ch, scale, th, tw, _s())))
    # tests/test_gpu_fpn.py::test_fpn_merge_adjoint
    assert _rel(res.clean["d_lat"], rl.grad) < 1e-6 and float(res.clean["d_lat"][:, 0].abs().max()) == 0.0
    _done(res, "d_lat")
    if with_top:
        assert _rel(res.clean["d_top"].double() - seed.double(), rt.grad) < 1e-5
        _done(res, "d_top")


@pytest.mark.parametrize("B,H,W,Cin,Cout", [(2, 1, 1, 32, 32), (2, 5, 9, 64, 96), (1, 7, 7, 32, 64)])
def test_conv3x3_nhwc_f32(B, H, W, Cin, Cout):
    """The padding taps read the zero page: the documented 128 bytes of zeros, poison around them."""
    lib = _lib.load()
    x, w, b = _f32(1040, B, H, W, Cin), _f32(1041, Cout, Cin, 3, 3, scale=0.05), _f32(1042, Cout, scale=0.1)
    s = {"x": In(x), "w": In(w.permute(0, 2, 3, 1).contiguous()), "b": In(b), "zeros": In(torch.zeros(32)), "y": Out((B, H, W, Cout), F32)}
    res = _twin(s, lambda t: _lib.check(lib.ldit_conv3x3_nhwc_f32(_p(t["x"]), _p(t["w"]), _p(t["b"]), _p(t["y"]), B, H, W, Cin, Cout,
                                                                  _p(t["zeros"]), _s())))
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), padding=1).permute(0, 2, 3, 1)
    assert _rel(res.clean["y"], ref) < 1e-5                         # tests/test_gpu_fpn.py::test_conv3x3_nhwc_implicit_gemm
    _done(res, "y")


# ============================================================================================================ RoIAlign
from tests import roi_oracle as roi                  # noqa: E402
from tests import roi_train_oracle as bo             # noqa: E402

ROI_IMAGE = (96, 160)
ROI_SIZES = [(24, 40), (12, 20), (6, 10), (3, 5)]    # p2 .. p5; `pool` = p5[:, ::2, ::2] is a strided view of p5's parent
ROI_COUNTS = {1: (1, 0), 63: (63, 1), 65: (0, 65)}


def _map_strides(h, w, Cc):
    """Element strides of a channels-last map with poison between pixels, between rows and between images (multiples of 4)."""
    sx = Cc + 4
    sy = w * sx + 8
    return (h * sy + 16, sy, sx, 1)


def _level_args(maps):
    L = len(maps)
    return ((C.c_void_p * L)(*[m.data_ptr() for m in maps]), (C.c_int32 * L)(*[m.shape[1] for m in maps]),
            (C.c_int32 * L)(*[m.shape[2] for m in maps]), (C.c_int64 * L)(*[m.stride(0) for m in maps]),
            (C.c_int64 * L)(*[m.stride(1) for m in maps]), (C.c_int64 * L)(*[m.stride(2) for m in maps]))


def _row_pad(count, R):
    """[B, R] mask of the rows at or past count[b]."""
    return torch.arange(R)[None, :] >= torch.as_tensor(count)[:, None]


@pytest.mark.parametrize("R", [1, 63, 65])
@pytest.mark.parametrize("Cc", [32, 64])
def test_roi_align_levels_forward_and_backward(R, Cc):
    """Boxes touch and cross the map border (roi_oracle.make_boxes); rows past count are 0x00 / 0xFF in boxes, d_out and levels."""
    lib = _lib.load()
    B, count = 2, np.asarray(ROI_COUNTS[R], dtype=np.int32)
    maps = [_f32(1100 + l, B, h, w, Cc, scale=1.5) for l, (h, w) in enumerate(ROI_SIZES)]
    sizes = ROI_SIZES + [(2, 3)]
    boxes = torch.from_numpy(np.stack([roi.make_boxes(100 * R + b, R, ROI_IMAGE, sizes)[0] for b in range(B)]))
    pad = _row_pad(count, R)
    scales = roi.infer_scales(sizes, ROI_IMAGE)
    k_min, k_max = roi.level_range(scales)
    s = {f"m{l}": In(m, strides=_map_strides(m.shape[1], m.shape[2], Cc)) for l, m in enumerate(maps)}
    s.update(boxes=In(boxes, pad=pad[:, :, None]), count=In(torch.from_numpy(count)), out=Out((B * R, 7, 7, Cc), F32),
             levels=Out((B, R), I32))
    outs = {}
    for name, fn, dt in (("f32", lib.ldit_roi_align_levels_f32, F32), ("bf16", lib.ldit_roi_align_levels_bf16, BF)):
        s["out"] = Out((B * R, 7, 7, Cc), dt)

        def call(t):
            views = [t[f"m{l}"] for l in range(4)] + [t["m3"][:, ::2, ::2]]
            ptrs, hs, ws, sb, sy, sx = _level_args(views)
            _lib.check(fn(ptrs, hs, ws, (C.c_float * 5)(*scales), sb, sy, sx, 5, Cc, _p(t["boxes"]), _p(t["count"]), B, R, 7, 2, k_min, k_max,
                          224.0, 4.0, _p(t["out"]), _p(t["levels"]), _s()))

        outs[name] = _twin(s, call)
        _done(outs[name], "out")
    res = outs["f32"]
    host = [m.numpy() for m in maps] + [maps[3][:, ::2, ::2].numpy()]
    ref, ref_levels = roi.roi_align_levels(host, boxes.numpy(), count, ROI_IMAGE)
    # tests/test_gpu_roi.py::test_roi_align_levels_matches_the_float64_oracle (padding rows: zeros, level -1 - in the oracle too)
    assert np.array_equal(res.clean["levels"].numpy(), ref_levels)
    peak = max(float(np.abs(m).max()) for m in host)
    assert float(np.abs(res.clean["out"].numpy() - ref).max()) <= 2.0 ** -13 * peak
    assert not bool(res.clean["out"].reshape(B, R, -1)[pad].any())
    # include/ldit.h: every element of the bf16 entry is the fp32 entry's value rounded to nearest even
    assert torch.equal(outs["bf16"].clean["out"], res.clean["out"].to(BF)) and torch.equal(outs["bf16"].clean["levels"], res.clean["levels"])

    # ---- backward: every element of every gradient map written exactly once, strided maps with canaries in the gaps
    d_out = _f32(1110, B * R, 7, 7, Cc)
    b = {"d_out": In(d_out, pad=pad.reshape(B * R)[:, None, None, None]), "boxes": In(boxes, pad=pad[:, :, None]),
         "count": In(torch.from_numpy(count)), "levels": In(res.clean["levels"], pad=pad)}
    for l, (h, w) in enumerate(sizes):
        b[f"g{l}"] = Out((B, h, w, Cc), F32, strides=_map_strides(h, w, Cc))

    def bwd(t):
        views = [t[f"g{l}"] for l in range(5)]
        ptrs, hs, ws, sb, sy, sx = _level_args(views)
        _lib.check(lib.ldit_roi_align_levels_bwd_f32(_p(t["d_out"]), _p(t["boxes"]), _p(t["count"]), _p(t["levels"]), B, R, ptrs, hs, ws,
                                                     (C.c_float * 5)(*scales), sb, sy, sx, 5, Cc, 7, 2, _s()))

    rb = _twin(b, bwd)
    refs, touch = bo.roi_align_levels_bwd(d_out.numpy(), boxes.numpy(), count, ref_levels, sizes, ROI_IMAGE)
    peak = float(d_out.abs().max())
    for l in range(5):     # tests/test_gpu_roi_train.py::_bwd_case
        got = rb.clean[f"g{l}"].numpy()
        _done(rb, f"g{l}")
        assert not got[touch[l] == 0].any()
        err = np.abs(got.astype(np.float64) - refs[l]).max(axis=-1)
        assert (err <= 2.0 ** -15 * peak * touch[l]).all(), l


# ============================================================================================== padded-result kernels
from tests import coco_oracle as co                  # noqa: E402
from tests import rpn_oracle as ro                   # noqa: E402
from tests import rpn_train_oracle as to             # noqa: E402

EPS32 = 2.0 ** -23


@pytest.mark.parametrize("entry", ["topk", "chunked"])
def test_rpn_topk(entry):
    lib = _lib.load()
    fn = lib.ldit_rpn_topk_f32 if entry == "topk" else lib.ldit_rpn_topk_chunked_f32
    cases = [((63, 65, 1), 40)] + ([((17000, 65), 100)] if entry == "chunked" else [])
    for sizes, k in cases:
        B, Ntot = 2, sum(sizes)
        v = _f32(1200, B, Ntot, scale=2.0)
        v[:, ::11] = 0.5                                 # ties: ascending index
        v[0, 3], v[1, 7] = float("-inf"), float("nan")   # -inf sorts last, NaN behind it
        ksum = sum(min(k, n) for n in sizes)
        s = {"logits": In(v), "idx": Out((B, ksum), I32)}
        res = _twin(s, lambda t: _lib.check(fn(_p(t["logits"]), (C.c_int64 * len(sizes))(*sizes), len(sizes), B, k, _p(t["idx"]), _s())))
        for b in range(B):     # tests/test_gpu_rpn.py::test_topk_per_level_is_a_stable_descending_argsort
            np.testing.assert_array_equal(res.clean["idx"][b].numpy(), ro.topk_indices(v[b].numpy(), sizes, k))
        guarded.assert_written(res.poisoned["idx"], "idx")


@pytest.mark.parametrize("K,valid", [(1, 0), (1, 1), (63, 1), (65, 65), (65, 40)])
def test_rpn_decode(K, valid):
    """Slots past `valid` hold the index -1 (what a poisoned padding slot is): box 0, score -inf (include/ldit.h)."""
    lib = _lib.load()
    B, Ntot = 2, 129
    rng = np.random.default_rng(1210)
    xy = rng.integers(0, 160, (Ntot, 2)).astype(np.float32)
    wh = rng.integers(8, 64, (Ntot, 2)).astype(np.float32)
    anchors = torch.from_numpy(np.concatenate([xy, xy + wh], axis=1))
    logits, deltas = _f32(1211, B, Ntot, scale=2.0), _f32(1212, B, Ntot, 4, scale=0.2)
    idx = torch.full((B, K), -1, dtype=I32)
    idx[:, :valid] = torch.from_numpy(rng.integers(0, Ntot, (B, valid)).astype(np.int32))
    if valid > 2:
        idx[0, 1] = Ntot                                 # one past the last anchor: outside as well
    s = {"logits": In(logits), "deltas": In(deltas), "anchors": In(anchors), "idx": In(idx), "boxes": Out((B, K, 4), F32),
         "scores": Out((B, K), F32)}
    res = _twin(s, lambda t: _lib.check(lib.ldit_rpn_decode_f32(_p(t["logits"]), _p(t["deltas"]), _p(t["anchors"]), _p(t["idx"]), B, Ntot, K,
                                                                224.0, 224.0, 1e-3, 0.0, _p(t["boxes"]), _p(t["scores"]), _s())))
    guarded.assert_written(res.poisoned["boxes"], "boxes")
    guarded.assert_finite(res.poisoned["boxes"], "boxes")
    for b in range(B):         # tests/test_gpu_rpn.py::_check_decode, extended to the slots that hold no anchor
        ok = ((idx[b] >= 0) & (idx[b] < Ntot)).numpy()
        boxes, scores = res.clean["boxes"][b].numpy(), res.clean["scores"][b].numpy()
        assert not boxes[~ok].any() and np.isneginf(scores[~ok]).all()
        if ok.any():
            ref_box, ref_score, (pcx, pcy, pw, ph) = ro.decode(logits[b].numpy(), deltas[b].numpy(), anchors.numpy(), idx[b].numpy()[ok],
                                                               224, 224, 1e-3, 0.0)
            bx = 8 * EPS32 * np.maximum(np.maximum(np.abs(pcx), pw), 1.0)
            by = 8 * EPS32 * np.maximum(np.maximum(np.abs(pcy), ph), 1.0)
            assert (np.abs(boxes[ok].astype(np.float64) - ref_box) <= np.stack([bx, by, bx, by], axis=1)).all()
            fin = np.isfinite(ref_score)
            np.testing.assert_array_equal(np.isneginf(scores[ok]), ~fin)
            assert (np.abs(scores[ok][fin] - ref_score[fin]) <= 8 * EPS32 * ref_score[fin] + 1e-38).all()


@pytest.mark.parametrize("N,valid", [(1, 0), (1, 1), (63, 1), (63, 63), (65, 65), (65, 40)])
def test_nms_batched(N, valid):
    """Candidates past `valid` have the score -inf (dropped: never kept, never suppressing); their boxes and groups are 0x00 / 0xFF."""
    lib = _lib.load()
    P, max_out = 2, 24
    probs = [ro.clustered_problem(1220 + p, N, n_clusters=6, n_groups=3, tie_frac=0.1) for p in range(P)]
    boxes = torch.from_numpy(np.stack([q[0] for q in probs]))
    scores = torch.from_numpy(np.stack([q[1] for q in probs]))
    groups = torch.from_numpy(np.stack([q[2] for q in probs]))
    pad = torch.arange(N)[None, :].expand(P, N) >= valid
    scores[pad] = float("-inf")
    s = {"boxes": In(boxes, pad=pad[:, :, None]), "scores": In(scores), "groups": In(groups, pad=pad), "keep": Out((P, max_out), I32),
         "count": Out((P,), I32), "ob": Out((P, max_out, 4), F32), "os": Out((P, max_out), F32)}
    res = _twin(s, lambda t: _lib.check(lib.ldit_nms_batched_f32(_p(t["boxes"]), _p(t["scores"]), _p(t["groups"]), P, N, 0.5, max_out,
                                                                 _p(t["keep"]), _p(t["count"]), _p(t["ob"]), _p(t["os"]), None, 0, _s())))
    _done(res, "keep", "count", "ob", "os")
    for p in range(P):         # tests/test_gpu_rpn.py::_run_nms: keep padded with -1, the gathered rows with zeros
        ref_keep, ref_count = ro.nms(boxes[p].numpy()[:valid], scores[p].numpy()[:valid], groups[p].numpy()[:valid], 0.5, max_out)
        assert int(res.clean["count"][p]) == ref_count
        np.testing.assert_array_equal(res.clean["keep"][p].numpy(), ref_keep)
        k = ref_keep[:ref_count]
        assert torch.equal(res.clean["ob"][p, :ref_count], boxes[p][k]) and torch.equal(res.clean["os"][p, :ref_count], scores[p][k])
        assert not res.clean["ob"][p, ref_count:].any() and not res.clean["os"][p, ref_count:].any()


def _target_problem(N, gts, Gmax=7):
    """Quarter-pixel boxes (every IoU term exact in fp32, tests/rpn_train_oracle.scene): N anchors, a few of them shifted GT boxes."""
    gt_list = [to.scene(40 + g, g, ROI_IMAGE) for g in gts]
    gt_boxes, gt_count = to.pad_gt(gt_list, gmax=Gmax, fill=0.0)
    anchors = to.scene(1230 + N, N, ROI_IMAGE)
    allg = np.concatenate([g for g in gt_list if len(g)] or [np.zeros((0, 4), np.float32)])
    for i in range(min(N, len(allg))):
        anchors[i] = allg[i] + np.float32(0.25 * (i % 3))
    keys = np.random.default_rng(1231).integers(0, 2 ** 31 - 1, (2, N)).astype(np.int32)
    keys[1] = keys[1] % 8                                # ties: by ascending index
    return anchors, gt_boxes, gt_count, keys


@pytest.mark.parametrize("N,gts", [(1, (0, 1)), (63, (1, 7)), (65, (7, 0)), (16500, (7, 1))])
def test_rpn_targets_both_entries(N, gts):
    lib = _lib.load()
    B, Gmax, bs = 2, 7, 16
    anchors, gt_boxes, gt_count, keys = _target_problem(N, gts)
    gpad = _row_pad(gt_count, Gmax)
    s = {"anchors": In(torch.from_numpy(anchors)), "gt": In(torch.from_numpy(gt_boxes), pad=gpad[:, :, None]),
         "gtc": In(torch.from_numpy(gt_count)), "keys": In(torch.from_numpy(keys)), "labels": Out((B, N), I32), "matched": Out((B, N), I32),
         "reg": Out((B, N, 4), F32), "sampled": Out((B, 2), I32)}
    ref_lab, ref_mat, ref_reg, ref_smp = to.targets(anchors, gt_boxes, gt_count, keys, 0.7, 0.3, bs, 0.5)
    got = {}
    for name, fn in (("plain", lib.ldit_rpn_targets_f32), ("chunked", lib.ldit_rpn_targets_chunked_f32)):
        if name == "plain" and N > 16384:
            continue
        res = _twin(s, lambda t: _lib.check(fn(_p(t["anchors"]), _p(t["gt"]), _p(t["gtc"]), _p(t["keys"]), B, N, Gmax, 0.7, 0.3, bs, 0.5,
                                               _p(t["labels"]), _p(t["matched"]), _p(t["reg"]), _p(t["sampled"]), _s())))
        _done(res, "labels", "matched", "reg", "sampled")
        got[name] = res
        # tests/test_gpu_rpn_train.py::test_targets_equal_the_oracle
        np.testing.assert_array_equal(res.clean["matched"].numpy(), ref_mat)
        np.testing.assert_array_equal(res.clean["sampled"].numpy(), ref_smp)
        np.testing.assert_array_equal(res.clean["labels"].numpy(), ref_lab)
        reg = res.clean["reg"].numpy()
        assert (np.abs(reg.astype(np.float64) - ref_reg) <= 8 * EPS32 * np.maximum(np.abs(ref_reg), 1.0)).all()
        assert not reg[ref_mat < 0].any()
    if len(got) == 2:          # include/ldit.h: where both entry points apply, all four outputs are bit-identical
        for k in ("labels", "matched", "reg", "sampled"):
            assert torch.equal(got["plain"].clean[k], got["chunked"].clean[k]), k


@pytest.mark.parametrize("N", [1, 63, 65, 2500])
def test_rpn_loss(N):
    """Anchors that are not in the loss (label -1) carry 0x00 / 0xFF logits; deltas and targets are 0x00 / 0xFF wherever the label is not 1."""
    lib = _lib.load()
    B = 2
    rng = np.random.default_rng(1240 + N)
    lab = rng.integers(-1, 2, (B, N)).astype(np.int32)
    if N == 1:
        lab[:] = [[1], [-1]]
    reg = (rng.standard_normal((B, N, 4)) * 0.5).astype(np.float32)
    logits = (rng.standard_normal((B, N)) * 2.5).astype(np.float32)
    deltas = (reg + rng.standard_normal((B, N, 4)) * 0.12).astype(np.float32)      # both branches of smooth-L1 (beta 1 / 9)
    smp = np.stack([(lab == 1).sum(1), (lab == 0).sum(1)], axis=1).astype(np.int32)
    out, notpos = torch.from_numpy(lab < 0), torch.from_numpy(lab != 1)
    need = int(lib.ldit_rpn_loss_workspace_bytes(B, N))
    s = {"logits": In(logits, pad=out), "deltas": In(deltas, pad=notpos[:, :, None]), "labels": In(lab), "reg": In(reg, pad=notpos[:, :, None]),
         "smp": In(smp), "loss": Out((2,), F32), "dl": Out((B, N), F32), "dd": Out((B, N, 4), F32), "ws": Scratch(max(need, 16))}
    res = _twin(s, lambda t: _lib.check(lib.ldit_rpn_loss_f32(_p(t["logits"]), _p(t["deltas"]), _p(t["labels"]), _p(t["reg"]), _p(t["smp"]), B, N,
                                                              1.0 / 9.0, _p(t["loss"]), _p(t["dl"]), _p(t["dd"]), _p(t["ws"]), need, _s())))
    _done(res, "loss", "dl", "dd")
    ref, ref_dl, ref_dd = to.loss(logits, np.where(notpos[:, :, None].numpy(), 0, deltas), lab, np.where(notpos[:, :, None].numpy(), 0, reg))
    # tests/test_gpu_rpn_train.py::_check_loss
    for a, w in zip(res.clean["loss"].double().numpy(), ref):
        assert abs(a - w) <= 2e-5 * abs(w)
    dl, dd = res.clean["dl"].numpy(), res.clean["dd"].numpy()
    assert rel_l2(dl, ref_dl) < 2e-5 and not dl[lab < 0].any() and not dd[lab != 1].any()
    if (lab == 1).any():
        assert rel_l2(dd, ref_dd) < 2e-5


from tests.test_gpu_roi import _check_postprocess, _post_inputs             # noqa: E402
from tests.test_gpu_roi_train import target_problem                         # noqa: E402

NC = 6
BOX_W = np.asarray([10.0, 10.0, 5.0, 5.0])


@pytest.mark.parametrize("R", [1, 63, 65])
def test_box_postprocess(R):
    """Rows at or past count[b] of head and proposals, and the head's columns past 5 NC, are 0x00 / 0xFF.  The header defines a padding
    row's score (-inf) and label; about its box it says only that it is written: the twin run asserts that it does not change."""
    lib = _lib.load()
    head, props, count = _post_inputs(1250 + R, R)
    pad = _row_pad(count, R)
    hpad = pad.reshape(2 * R)[:, None] | (torch.arange(32) >= 5 * NC)[None, :]
    N = R * (NC - 1)
    s = {"head": In(head, pad=hpad), "props": In(props, pad=pad[:, :, None]), "count": In(count), "boxes": Out((2, N, 4), F32),
         "scores": Out((2, N), F32), "labels": Out((2, N), I32)}
    res = _twin(s, lambda t: _lib.check(lib.ldit_box_postprocess_f32(_p(t["head"]), 32, _p(t["props"]), _p(t["count"]), 2, R, NC, 224.0, 224.0,
                                                                     (C.c_float * 4)(*BOX_W), 0.05, 1e-2, _p(t["boxes"]), _p(t["scores"]),
                                                                     _p(t["labels"]), _s())))
    guarded.assert_written(res.poisoned["boxes"], "boxes")
    guarded.assert_written(res.poisoned["scores"], "scores")
    guarded.assert_finite(res.poisoned["boxes"], "boxes")
    # tests/test_gpu_roi.py::_check_postprocess on the operands of the clean run (its padding rows hold zeros)
    head0, props0 = np.where(hpad.numpy(), np.float32(0), head), np.where(pad[:, :, None].numpy(), np.float32(0), props)
    _check_postprocess(head0, props0, count, res.clean["boxes"].numpy(), res.clean["scores"].numpy(), res.clean["labels"].numpy(), R)
    assert bool(torch.isneginf(res.clean["scores"].reshape(2, R, NC - 1)[pad]).all())


@pytest.mark.parametrize("R,gts", [(1, (0, 7)), (63, (1, 40)), (65, (0, 7)), (65, (1, 40))])
def test_roi_targets_and_box_loss(R, gts):
    lib = _lib.load()
    B, S = 2, 16
    props, count, gt_boxes, gt_labels, gt_count, keys = target_problem(R, gts)
    Gmax = gt_boxes.shape[1]
    ppad, gpad = _row_pad(count, R), _row_pad(gt_count, Gmax)
    s = {"props": In(props, pad=ppad[:, :, None]), "count": In(count), "gt": In(gt_boxes, pad=gpad[:, :, None]), "gtl": In(gt_labels, pad=gpad),
         "gtc": In(gt_count), "keys": In(keys, pad=torch.cat([ppad, gpad], dim=1)), "rois": Out((B, S, 4), F32), "labels": Out((B, S), I32),
         "reg": Out((B, S, 4), F32), "matched": Out((B, S), I32), "sampled": Out((B, 2), I32)}
    res = _twin(s, lambda t: _lib.check(lib.ldit_roi_targets_f32(_p(t["props"]), _p(t["count"]), _p(t["gt"]), _p(t["gtl"]), _p(t["gtc"]),
                                                                 _p(t["keys"]), B, R, Gmax, 0.5, 0.5, S, 0.25, (C.c_float * 4)(*BOX_W),
                                                                 _p(t["rois"]), _p(t["labels"]), _p(t["reg"]), _p(t["matched"]),
                                                                 _p(t["sampled"]), _s())))
    _done(res, "rois", "labels", "reg", "matched", "sampled")
    ref_rois, ref_lab, ref_reg, ref_mat, ref_smp = bo.targets(props, count, gt_boxes, gt_labels, gt_count, keys, 0.5, 0.5, S, 0.25)
    # tests/test_gpu_roi_train.py::test_targets_equal_the_oracle (padding rows: rois and targets zero, label and match -1)
    np.testing.assert_array_equal(res.clean["sampled"].numpy(), ref_smp)
    np.testing.assert_array_equal(res.clean["labels"].numpy(), ref_lab)
    np.testing.assert_array_equal(res.clean["matched"].numpy(), ref_mat)
    assert res.clean["rois"].numpy().tobytes() == ref_rois.tobytes()
    reg = res.clean["reg"].numpy()
    assert (np.abs(reg.astype(np.float64) - ref_reg) <= 8 * EPS32 * np.maximum(np.abs(ref_reg), BOX_W[None, None, :])).all()
    assert not reg[ref_lab < 1].any()

    # ---- fastrcnn_loss on these rows: padding rows (label -1) and the columns past 5 NC of head_out are 0x00 / 0xFF
    M, ld = B * S, 32
    lab = ref_lab.reshape(M)
    rng = np.random.default_rng(1260 + R)
    head = np.zeros((M, ld), dtype=np.float32)
    head[:, :NC] = rng.standard_normal((M, NC)) * 2.5
    head[:, NC:5 * NC] = rng.standard_normal((M, 4 * NC)) * 0.6
    tgt = reg.reshape(M, 4)
    for r in np.flatnonzero(lab >= 1):
        head[r, NC + 4 * lab[r]:NC + 4 * lab[r] + 4] = tgt[r] + rng.standard_normal(4) * 0.12
    hpad = torch.from_numpy(lab < 0)[:, None] | (torch.arange(ld) >= 5 * NC)[None, :]
    need = int(lib.ldit_box_loss_workspace_bytes(M))
    s = {"head": In(head, pad=hpad), "labels": In(lab), "reg": In(tgt, pad=torch.from_numpy(lab < 1)[:, None]), "smp": In(ref_smp),
         "loss": Out((2,), F32), "dh": Out((M, ld), F32), "ws": Scratch(max(need, 16))}
    rl = _twin(s, lambda t: _lib.check(lib.ldit_box_loss_f32(_p(t["head"]), ld, _p(t["labels"]), _p(t["reg"]), _p(t["smp"]), B, M, NC, 1.0 / 9.0,
                                                             _p(t["loss"]), _p(t["dh"]), _p(t["ws"]), need, _s())))
    _done(rl, "loss", "dh")
    ref, ref_d = bo.loss(np.where(hpad.numpy(), np.float32(0), head), lab, np.where((lab < 1)[:, None], np.float32(0), tgt), NC)
    # tests/test_gpu_roi_train.py::_check_loss (d_head written in full: padding rows / columns and the other classes exactly zero)
    for a, w in zip(rl.clean["loss"].double().numpy(), ref):
        assert abs(a - w) <= 2e-5 * abs(w)
    dh = rl.clean["dh"].numpy()
    assert rel_l2(dh[:, :NC], ref_d[:, :NC]) < 2e-5 and not dh[ref_d == 0].any() and not dh[lab < 0].any() and not dh[:, 5 * NC:].any()
    if (lab >= 1).any():
        assert rel_l2(dh[:, NC:], ref_d[:, NC:]) < 2e-5


@pytest.mark.parametrize("D,nd,ng", [(1, (1, 0), (3, 2)), (63, (63, 1), (9, 0)), (65, (0, 65), (1, 9))])
def test_coco_match_keys_accumulate(D, nd, ng):
    """Rows at or past count / gt_count are 0x00 / 0xFF in every input; the store has a row in front of and one behind the batch's."""
    lib = _lib.load()
    B, G, K, cap, Ds, off = 2, 9, 3, 4, D + 3, 1
    boxes, scores, labels, count, gtb, gtl, gtc, crowd, area = co.scene(1270 + D, nd, ng, D, G, K)
    dpad, gpad = _row_pad(count, D), _row_pad(gtc, G)
    s = {"boxes": In(boxes, pad=dpad[:, :, None]), "scores": In(scores, pad=dpad), "labels": In(labels, pad=dpad), "count": In(count),
         "gtb": In(gtb, pad=gpad[:, :, None]), "gtl": In(gtl, pad=gpad), "crowd": In(crowd, pad=gpad), "area": In(area, pad=gpad), "gtc": In(gtc),
         "code": Out((cap, Ds, 4, 10), torch.uint8), "rank": Out((cap, Ds), I32), "npig": Out((cap, K, 4), I32), "so": Out((cap, Ds), F32),
         "lo": Out((cap, Ds), I32)}
    thr, rng_ = (C.c_double * 10)(*co.IOU_THRS.tolist()), (C.c_double * 8)(*[x for pr in co.AREA_RNG for x in pr])
    res = _twin(s, lambda t: _lib.check(lib.ldit_coco_match(_p(t["boxes"]), _p(t["scores"]), _p(t["labels"]), _p(t["count"]), _p(t["gtb"]),
                                                            _p(t["gtl"]), _p(t["crowd"]), _p(t["area"]), _p(t["gtc"]), B, D, G, K, thr, rng_,
                                                            _p(t["code"]), _p(t["rank"]), _p(t["npig"]), _p(t["so"]), _p(t["lo"]), cap, Ds, off, _s())))
    ref_code, ref_rank, ref_npig = co.match(boxes, scores, labels, count, gtb, gtl, gtc, crowd, area, K)
    rows = slice(off, off + B)
    code, rank, npig = res.clean["code"].numpy(), res.clean["rank"].numpy(), res.clean["npig"].numpy()
    # tests/test_gpu_coco_eval.py::test_match_equals_the_oracle_exactly; the rows of the batch are written IN FULL, no other row is touched
    np.testing.assert_array_equal(code[rows, :D], ref_code)
    np.testing.assert_array_equal(rank[rows, :D], ref_rank)
    np.testing.assert_array_equal(npig[rows], ref_npig)
    assert (code[rows, D:] == co.ABSENT).all() and (rank[rows, D:] == -1).all()
    present = ref_rank >= 0
    so, lo = res.clean["so"].numpy()[rows, :D], res.clean["lo"].numpy()[rows, :D]
    np.testing.assert_array_equal(so[present], scores[present])
    np.testing.assert_array_equal(lo[present], labels[present])
    assert not so[~present].any() and not lo[~present].any() and not res.clean["so"].numpy()[rows, D:].any()
    for k in ("code", "rank", "npig", "so", "lo"):
        raw = res.poisoned[k].contiguous().view(torch.uint8).reshape(cap, -1)
        assert bool((raw[:off] == guarded.CANARY).all()) and bool((raw[off + B:] == guarded.CANARY).all()), k
        guarded.assert_written(res.poisoned[k][rows], k)
    guarded.assert_finite(res.poisoned["so"][rows], "scores_out")

    # ---- keys of the batch's rows: scores and labels of absent slots are not read
    rk, sc, lb = (torch.from_numpy(np.ascontiguousarray(a[rows])) for a in (rank, res.clean["so"].numpy(), res.clean["lo"].numpy()))
    absent = rk < 0
    s = {"rank": In(rk), "scores": In(sc, pad=absent), "labels": In(lb, pad=absent), "keys": Out((B * Ds,), torch.int64)}
    rk_ = _twin(s, lambda t: _lib.check(lib.ldit_coco_keys(_p(t["rank"]), _p(t["scores"]), _p(t["labels"]), B, Ds, _p(t["keys"]), _s())))
    keys = rk_.clean["keys"].numpy().reshape(B, Ds)
    guarded.assert_written(rk_.poisoned["keys"], "keys")
    # include/ldit.h: (category << 56) | (inverted ordered score bits << 24) | (image * store_D + rank); absent: INT64_MAX
    assert (keys[absent.numpy()] == np.iinfo(np.int64).max).all()
    img, slot = np.nonzero(~absent.numpy())
    kk = keys[img, slot]
    assert ((kk >> 56) == lb.numpy()[img, slot]).all() and ((kk & 0xffffff) == img * Ds + rk.numpy()[img, slot]).all()
    want = np.lexsort((rk.numpy()[img, slot], img, -sc.numpy()[img, slot].astype(np.float64), lb.numpy()[img, slot]))
    assert np.array_equal(np.argsort(kk, kind="stable"), want)

    # ---- accumulation over the two stored rows
    skeys, sidx = torch.sort(rk_.clean["keys"])
    codeb, npigb = torch.from_numpy(np.ascontiguousarray(code[rows])), torch.from_numpy(np.ascontiguousarray(npig[rows]))
    s = {"skeys": In(skeys), "sidx": In(sidx), "code": In(codeb), "rank": In(rk), "npig": In(npigb),
         "precision": Out((10, 101, K, 4, 3), torch.float64), "recall": Out((10, K, 4, 3), torch.float64)}
    rec, md = (C.c_double * 101)(*co.REC_THRS.tolist()), (C.c_int32 * 3)(*co.MAX_DETS)
    ra = _twin(s, lambda t: _lib.check(lib.ldit_coco_accumulate(_p(t["skeys"]), _p(t["sidx"]), _p(t["code"]), _p(t["rank"]), _p(t["npig"]), B, Ds,
                                                                K, rec, md, _p(t["precision"]), _p(t["recall"]), _s())))
    _done(ra, "precision", "recall")
    rp, rr = co.accumulate(code[rows], rank[rows], npig[rows], sc.numpy(), lb.numpy(), K)
    # tests/test_gpu_coco_eval.py::test_accumulation_matches_the_oracle
    assert np.abs(ra.clean["precision"].numpy() - rp).max() <= 1e-12 and np.abs(ra.clean["recall"].numpy() - rr).max() <= 1e-12


# ================================================================================= the train step's two elementwise passes
@pytest.mark.parametrize("n", [4, 1028])
def test_adamw_step(n):
    """params and the two moments are updated in place (they keep their values); the bf16 mirror is an output."""
    lib = _lib.load()
    lr, b1, b2, eps, wd, step, gs = 1e-2, 0.9, 0.999, 1e-8, 0.01, 3, 0.5
    p0, g, m0, v0 = _f32(1300, n), _f32(1301, n, scale=0.1), _f32(1302, n, scale=0.01), _f32(1303, n).abs() * 1e-3
    s = {"p": Out((n,), F32, init=p0), "g": In(g), "m": Out((n,), F32, init=m0), "v": Out((n,), F32, init=v0), "mirror": Out((n,), BF)}
    res = _twin(s, lambda t: _lib.check(lib.ldit_adamw_step(_p(t["p"]), _p(t["g"]), _p(t["m"]), _p(t["v"]), n, lr, b1, b2, eps, wd, step, gs,
                                                            _p(t["mirror"]), _s())))
    gg = g.double() * gs
    m, v = b1 * m0.double() + (1 - b1) * gg, b2 * v0.double() + (1 - b2) * gg * gg
    p = p0.double() * (1 - lr * wd) - lr / (1 - b1 ** step) * m / (v.sqrt() / np.sqrt(1 - b2 ** step) + eps)
    # test_gpu_train.py::test_fused_adamw_matches_torch
    assert _rel(res.clean["p"], p) < 1e-6 and _rel(res.clean["m"], m) < 1e-6 and _rel(res.clean["v"], v) < 1e-6
    assert torch.equal(res.clean["mirror"], res.clean["p"].to(BF))
    _done(res, "p", "m", "v", "mirror")


def test_pack_train_bf16():
    """The bf16 mirror of the flat parameter block of ViT-micro: element i = bf16(flat[i]) (include/ldit.h)."""
    lib = _lib.load()
    lcfg = _lib.LditCfg(hidden=128, layers=3, heads=2, mlp=512, patch=16, in_ch=3, img_h=64, img_w=64, n_taps=0, ln_eps=1e-12,
                        dtype=_lib.DTYPE_BF16, flags=0)
    nb, mb = int(lib.ldit_flat_param_bytes(C.byref(lcfg))), int(lib.ldit_train_mirror_bytes(C.byref(lcfg)))
    assert nb > 0 and mb >= nb // 2
    offs = (C.c_int64 * (4 + 14 * 3 + 1))()
    _lib.check(lib.ldit_flat_param_layout(C.byref(lcfg), offs, len(offs)))
    flat = _f32(1310, nb // 4)
    for l in range(3):                                   # the key-bias third of bqkv stays zero (no key bias)
        o = offs[4 + 14 * l + 3]
        flat[o + 128:o + 256] = 0.0
    s = {"flat": In(flat), "mirror": Out((mb,), torch.uint8)}
    res = _twin(s, lambda t: _lib.check(lib.ldit_pack_train(C.byref(lcfg), _p(t["flat"]), _p(t["mirror"]), mb, _s())))
    assert torch.equal(res.clean["mirror"][:nb // 2].view(BF), flat.to(BF))
