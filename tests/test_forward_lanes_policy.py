"""Host-side policy of the two-lane fp32 forward (csrc/api.hip: forward_lanes), through ldit_forward_lanes: no GPU, no launch."""
import ctypes as C

import pytest

from layoutdit_amd import _lib, config as cfgs


def _cfg(c, size=224, dtype=_lib.DTYPE_F32):
    return _lib.LditCfg(hidden=c.hidden_size, layers=c.num_hidden_layers, heads=c.num_attention_heads, mlp=c.intermediate_size,
                        patch=c.patch_size, in_ch=3, img_h=size, img_w=size, n_taps=0, ln_eps=1e-12, dtype=dtype, flags=0)


def _lanes(lc, batch, switch=None):
    _lib.set_switch("LDIT_FWD_LANES", switch)
    try:
        return _lib.load().ldit_forward_lanes(C.byref(lc), batch)
    finally:
        _lib.set_switch("LDIT_FWD_LANES", None)


OTHER_DTYPES = [_lib.DTYPE_BF16, _lib.DTYPE_FP8, _lib.DTYPE_MXFP8, _lib.DTYPE_F32X3, _lib.DTYPE_F32X6]


@pytest.mark.parametrize("dtype", OTHER_DTYPES)
def test_every_other_build_keeps_one_lane(dtype):
    lc = _cfg(cfgs.vit_base(), dtype=dtype)
    for batch in (1, 2, 64, 256):
        for switch in (None, "1", "2"):
            assert _lanes(lc, batch, switch) == 1, (dtype, batch, switch)


def test_batch_one_and_bad_arguments():
    lc = _cfg(cfgs.vit_base())
    for switch in (None, "1", "2"):
        assert _lanes(lc, 1, switch) == 1
    assert _lanes(lc, 0) == 0 and _lanes(lc, -3) == 0
    lc.heads = 7
    assert _lanes(lc, 64) == 0 and "divisible" in _lib.load().ldit_last_error().decode()


def test_small_batches_stay_below_the_threshold():
    for c, size in ((cfgs.vit_micro(), 64), (cfgs.vit_tiny(), 224), (cfgs.vit_base(), 224)):
        for batch in (2, 3, 5, 8):
            assert _lanes(_cfg(c, size), batch) == 1


def test_config_1_runs_two_lanes_and_smaller_batches_do_not():
    """ViT-B/16 224^2 fp32: two lanes from batch 48, the smallest batch that won all three alternations (profiles/forward_lanes_ab.txt:
    batch 32 ties, batch 16 loses).  The bound is in token rows, so ViT-L/16 512^2 reaches it at batch 10."""
    lc = _cfg(cfgs.vit_base())
    assert _lanes(lc, 64) == 2 and _lanes(lc, 128) == 2 and _lanes(lc, 48) == 2
    assert _lanes(lc, 47) == 1 and _lanes(lc, 32) == 1 and _lanes(lc, 16) == 1
    big = _cfg(cfgs.vit_large(), 512)
    assert _lanes(big, 16) == 2 and _lanes(big, 9) == 1


def test_switch_overrides_the_policy_both_ways():
    lc = _cfg(cfgs.vit_base())
    assert _lanes(lc, 64, "1") == 1 and _lanes(lc, 256, "1") == 1
    assert _lanes(lc, 2, "2") == 2 and _lanes(lc, 3, "2") == 2 and _lanes(_cfg(cfgs.vit_micro(), 64), 2, "2") == 2
    assert _lanes(lc, 2) == 1                      # and the switch is gone again
