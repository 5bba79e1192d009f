"""The guard-band helper (tests/guarded.py) has teeth: three deliberately sloppy torch stand-ins for a kernel, each with one of
the faults the GPU footprint tests look for, must be reported, and a correct stand-in must pass.  CPU tensors only; no
library code is involved."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import guarded                                           # noqa: E402
from tests.guarded import GuardError, In, Out, Scratch, twin_run    # noqa: E402

ROWS, COLS, LD, PAD = 5, 12, 24, 16     # a row-sum "kernel" that works on tiles of PAD columns


def _x():
    return np.arange(ROWS * COLS, dtype=np.float32).reshape(ROWS, COLS) / 7.0 - 3.0


def _specs(with_scratch=False):
    s = {"x": In(_x(), ld=LD), "y": Out((ROWS, 4), torch.float32, ld=8)}
    if with_scratch:
        s["scratch"] = Scratch(ROWS * 4)
    return s


def _tile(x):
    """The PAD-column tile a tiled kernel would load: the row's COLS columns and PAD - COLS more from whatever follows."""
    return torch.as_strided(x, (ROWS, PAD), (x.stride(0), 1), x.storage_offset())


def rowsum_correct(t):
    t["y"][:, 0] = t["x"].sum(dim=1)
    t["y"][:, 1:] = 0.0


def rowsum_masks_by_multiplying(t):
    tile = _tile(t["x"])
    mask = (torch.arange(PAD) < COLS).to(tile.dtype)
    t["y"][:, 0] = (tile * mask).sum(dim=1)           # 0 * NaN = NaN: the padding is multiplied away, not selected away
    t["y"][:, 1:] = 0.0


def rowsum_masks_by_select(t):
    tile = _tile(t["x"])
    keep = torch.arange(PAD) < COLS
    t["y"][:, 0] = torch.where(keep, tile, torch.zeros_like(tile)).sum(dim=1)
    t["y"][:, 1:] = 0.0


def rowsum_writes_past_its_row(t):
    y = t["y"]
    wide = torch.as_strided(y, (ROWS, 5), (y.stride(0), 1), y.storage_offset())
    wide[:, 0] = t["x"].sum(dim=1)
    wide[:, 1:] = 0.0                                 # one element past the 4 columns of every output row


def rowsum_trusts_its_scratch(t):
    acc = t["scratch"].view(torch.float32)            # assumed to arrive zeroed
    acc += t["x"].sum(dim=1)
    t["y"][:, 0] = acc
    t["y"][:, 1:] = 0.0


def rowsum_clears_its_scratch(t):
    acc = t["scratch"].view(torch.float32)
    acc.zero_()
    acc += t["x"].sum(dim=1)
    t["y"][:, 0] = acc
    t["y"][:, 1:] = 0.0


def _check(res):
    ref = torch.from_numpy(_x().astype(np.float64).sum(axis=1).astype(np.float32))
    torch.testing.assert_close(res.clean["y"][:, 0], ref, rtol=1e-6, atol=0)     # 12 fp32 additions: a few ulp
    guarded.assert_finite(res.poisoned["y"])
    guarded.assert_written(res.poisoned["y"])


def test_geometry_of_a_guarded_operand():
    g = guarded.Guarded((ROWS, COLS), torch.float32, ld=LD, fill=guarded.POISON, data=_x(), name="x")
    assert g.view.shape == (ROWS, COLS) and g.view.stride() == (LD, 1)
    assert g.view.data_ptr() % 16 == 0 and (g.view.data_ptr() - g.parent.data_ptr()) == g.start
    assert g.start >= max(256, LD * 4) and g.nbytes - (g.start + ((ROWS - 1) * LD + COLS) * 4) >= max(256, LD * 4)
    assert int(g.footprint.sum()) == ROWS * COLS * 4
    outside = torch.from_numpy(g.bytes()[~g.footprint])
    assert bool((outside == 0xFF).all())
    assert torch.equal(g.value(), torch.from_numpy(_x()))
    # 0xFF in every byte is NaN in each float format the library reads
    raw = torch.full((16,), 0xFF, dtype=torch.uint8)
    for dt in (torch.float32, torch.bfloat16, torch.float16, torch.float8_e4m3fn):
        assert bool(torch.isnan(raw.view(dt).float()).all()), dt
    assert bool((raw.view(torch.int32) == -1).all())
    g.check_surroundings()
    g.check_unchanged()


@pytest.mark.parametrize("fn", [rowsum_correct, rowsum_masks_by_select])
def test_a_correct_stand_in_passes(fn):
    _check(twin_run(_specs(), fn))


def test_a_correct_stand_in_with_scratch_passes():
    _check(twin_run(_specs(with_scratch=True), rowsum_clears_its_scratch))


def test_mask_by_multiplication_is_reported():
    with pytest.raises(GuardError, match="depends on memory outside"):
        twin_run(_specs(), rowsum_masks_by_multiplying)


def test_write_past_the_output_row_is_reported():
    with pytest.raises(GuardError, match="outside the operand were written"):
        twin_run(_specs(), rowsum_writes_past_its_row)


def test_trusting_the_scratch_is_reported():
    with pytest.raises(GuardError, match="depends on memory outside"):
        twin_run(_specs(with_scratch=True), rowsum_trusts_its_scratch)


def test_accumulating_into_an_output_slab_is_reported_only_when_the_slab_is_scratch():
    """An output pre-filled with the canary in both runs cannot show a `+=` into it; one marked as scratch holds the run's fill."""
    def accumulates(t):
        t["y"][:, 0] += t["x"].sum(dim=1)              # a slab assumed to arrive zeroed
        t["y"][:, 1:] = 0.0
    twin_run(_specs(), accumulates)                                                   # the same 0xA5 prefill twice: invisible
    slab = dict(_specs(), y=Out((ROWS, 4), torch.float32, ld=8, scratch=True))
    with pytest.raises(GuardError, match="depends on memory outside"):
        twin_run(slab, accumulates)
    _check(twin_run(slab, rowsum_correct))
    g = guarded.build(slab, guarded.POISON, "cpu")["y"]
    assert bool(torch.isnan(g.view).all()) and bool((torch.from_numpy(g.bytes()[~g.footprint]) == guarded.CANARY).all())


def test_a_written_input_is_reported():
    def scribbles(t):
        rowsum_correct(t)
        t["x"][0, 0] = 1.0
    with pytest.raises(GuardError, match="const operand changed"):
        twin_run(_specs(), scribbles)


def test_an_unwritten_element_is_reported():
    def lazy(t):
        t["y"][:, 0] = t["x"].sum(dim=1)              # columns 1.. never written
    res = twin_run(_specs(), lazy)
    with pytest.raises(GuardError, match="never written"):
        guarded.assert_written(res.poisoned["y"])


def test_one_byte_outputs_are_left_to_the_oracle():
    guarded.assert_written(torch.full((4,), 0xA5, dtype=torch.uint8))            # an ordinary byte value: not judged
    with pytest.raises(GuardError, match="never written"):
        guarded.assert_written(torch.full((4,), 0xA5, dtype=torch.uint8).view(torch.int16))


def test_padding_inside_an_operand_takes_the_fill_of_the_run():
    x = In(_x(), ld=LD, pad=(torch.arange(ROWS) >= 3)[:, None])
    for fill, bad in ((guarded.CLEAN, 0.0), (guarded.POISON, float("nan"))):
        g = guarded.build({"x": x}, fill, "cpu")["x"]
        assert torch.equal(g.view[:3], torch.from_numpy(_x())[:3])
        assert bool(torch.isnan(g.view[3:]).all()) if fill else bool((g.view[3:] == bad).all())
        raw = g.view[3:].contiguous().view(torch.uint8)
        assert bool((raw == fill).all())


def test_fresh_memory_fills_new_tensors(monkeypatch):
    with guarded.fresh_memory(monkeypatch, 0xFF):
        a = torch.empty(3, 5)
        b = torch.empty_like(torch.zeros(2, 3, 4, 5).contiguous(memory_format=torch.channels_last))
        c = torch.zeros(2, dtype=torch.int32).new_empty((4,))
    assert bool(torch.isnan(a).all()) and bool(torch.isnan(b).all()) and bool((c == -1).all())
    with guarded.fresh_memory(monkeypatch, 0x00):
        assert bool((torch.empty(7) == 0).all())
    assert torch.empty is not None and torch.empty.__module__ != __name__     # restored
