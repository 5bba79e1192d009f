"""The two-lane fp32 forward (csrc/api.hip: enqueue_lanes): images [0, (B + 1) / 2) on the caller's stream, the rest on the library's
side stream, both in disjoint row ranges of one workspace.  Every tap must EQUAL the one-lane forward bit for bit - rows never mix in
LayerNorm and the GEMMs, images never mix in attention, and every GEMM tiling keeps the per-row product order - and the call must stay
ordered against the caller's stream on both sides (fork after the producer of the input, join before whatever follows).

Lanes are forced with LDIT_FWD_LANES=2 (the policy only turns them on for large batches); the reference is LDIT_FWD_LANES=1."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from layoutdit_amd import _lib, config as cfgs, synth                                  # noqa: E402
from layoutdit_amd.modeling import DiTEncoder                                          # noqa: E402
from layoutdit_amd.modeling.detector_input import DetectorInputTransform               # noqa: E402

DEV = "cuda:0"
GEOMS = {"micro": (cfgs.vit_micro, 64), "tiny": (cfgs.vit_tiny, 224)}
BATCHES = (2, 3, 5)


class _switches:
    """LDIT_* switches for the duration of a block; removed again whatever happens inside."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        for k, v in self.kv.items():
            _lib.set_switch(k, v)

    def __exit__(self, *exc):
        for k in self.kv:
            _lib.set_switch(k, None)


@functools.lru_cache(maxsize=None)
def _model(geom, wseed=1):
    cfg = GEOMS[geom][0]()
    return DiTEncoder(cfg).load_numpy(synth.synth_weights(cfg, wseed)).to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _images(geom, batch, seed=0):
    size = GEOMS[geom][1]
    return torch.from_numpy(synth.synth_images(batch, size, size, seed=500 + 10 * batch + seed)).to(DEV)


def _all_taps(m, x):
    """every hidden state 0 .. L (at most LDIT_MAX_TAPS per call), cloned, after a full synchronisation"""
    L = m.config.num_hidden_layers
    out = []
    with torch.no_grad():
        for lo in range(0, L + 1, _lib.LDIT_MAX_TAPS):
            idx = list(range(lo, min(L + 1, lo + _lib.LDIT_MAX_TAPS)))
            hs = m(x, taps=idx).hidden_states
            out += [hs[i].clone() for i in idx]
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _one_lane(geom, batch):
    """the reference: one lane, the picker's own tiling; computed once per shape and shared"""
    with _switches(LDIT_FWD_LANES="1"):
        return _all_taps(_model(geom), _images(geom, batch))


@pytest.mark.parametrize("tile", [None, 3, 5, 6, 7], ids=lambda t: "picker" if t is None else f"tile{t}")
@pytest.mark.parametrize("geom", ["micro", "tiny"])
def test_two_lanes_equal_one_lane_bit_for_bit(geom, tile):
    """Batches 2, 3 (odd: 2 + 1) and 5, every hidden state: with the picker choosing each lane's tiling from the lane's own row count
    (serving-size lanes take the thin kernel), and with LDIT_GEMM_TILE forcing the 304-row panel (3) and its 144 / 80 / 48-row variants
    (5, 6, 7) on both lanes."""
    m = _model(geom)
    for batch in BATCHES:
        want = _one_lane(geom, batch)
        kv = {"LDIT_FWD_LANES": "2"}
        if tile is not None:
            kv["LDIT_GEMM_TILE"] = str(tile)
        with _switches(**kv):
            got = _all_taps(m, _images(geom, batch))
        assert len(got) == m.config.num_hidden_layers + 1
        for l, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a, b), (geom, tile, batch, l)


@pytest.mark.parametrize("geom", ["micro", "tiny"])
def test_batch_one_runs_on_one_lane(geom):
    m = _model(geom)
    want = _one_lane(geom, 1)
    with _switches(LDIT_FWD_LANES="2"):
        got = _all_taps(m, _images(geom, 1))
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_call_is_ordered_against_the_callers_stream():
    """On a non-default stream: the input is written by a kernel enqueued right before the call (the side stream must not start
    before it: fork), a reduction of the last tap is enqueued right after it (it must see lane B's rows: join), and the input buffer
    is overwritten right after the call."""
    geom = "tiny"
    m = _model(geom)
    L = m.config.num_hidden_layers
    src = _images(geom, 5)
    want = _one_lane(geom, 5)[L]
    want_sum = want.double().sum(dim=(1, 2))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with _switches(LDIT_FWD_LANES="2"), torch.no_grad(), torch.cuda.stream(s):
        for _ in range(3):
            x = torch.empty_like(src)
            x.copy_(src * 0.5).mul_(2.0)                  # produced on `s` immediately before the call (exact: powers of two)
            last = m(x).hidden_states[L]
            red = last.double().sum(dim=(1, 2))           # consumer on `s` immediately after
            x.fill_(float("nan"))                         # and the input is gone
            s.synchronize()
            assert torch.equal(last, want)
            assert torch.equal(red, want_sum)


def test_consecutive_calls_share_one_workspace():
    """batch 5 then batch 4 through one module, nothing in between: the second call's embedding overwrites rows the first call's
    lane B was working in, so it must be ordered behind the first call's join."""
    geom = "tiny"
    m = _model(geom)
    L = m.config.num_hidden_layers
    want5, want4 = _one_lane(geom, 5)[L], _one_lane(geom, 4)[L]
    x5, x4 = _images(geom, 5), _images(geom, 4)
    torch.cuda.synchronize()
    with _switches(LDIT_FWD_LANES="2"), torch.no_grad():
        for _ in range(3):
            a = m(x5).hidden_states[L]
            b = m(x4).hidden_states[L]
            torch.cuda.synchronize()
            assert torch.equal(a, want5) and torch.equal(b, want4)


def test_image_list_forward_under_lanes():
    """forward_image_list: the fp32 build writes the transformed batch into the workspace before the embedding - both before the fork."""
    cfg = cfgs.vit_micro()
    m = _model("micro")
    rng = np.random.default_rng(7)
    sizes = [(80, 50), (64, 64), (33, 129)]
    imgs = [torch.from_numpy(np.clip(0.5 + 0.3 * rng.standard_normal((3, h, w)), 0, 1).astype(np.float32)).to(DEV) for h, w in sizes]
    t = DetectorInputTransform(fixed_size=(64, 64))
    with torch.no_grad():
        with _switches(LDIT_FWD_LANES="1"):
            want = m(t(imgs)[0].tensors).hidden_states
            torch.cuda.synchronize()
        with _switches(LDIT_FWD_LANES="2"):
            got = m.forward_image_list(imgs, size=(64, 64)).hidden_states
            torch.cuda.synchronize()
    for tp in cfg.taps:
        assert torch.equal(got[tp], want[tp]), tp


def test_capture_with_lanes_forced_replays_bit_exact():
    """A capturing stream gets the one-lane schedule whatever the switch says (a captured forward is a linear graph); the replay
    equals the eager two-lane forward."""
    geom = "tiny"
    m = _model(geom)
    xs = [_images(geom, 2, seed=i) for i in range(3)]
    with _switches(LDIT_FWD_LANES="2"), torch.no_grad():
        eager = [[h.clone() for h in m(x).hidden_states if h is not None] for x in xs]
        static_x = xs[0].clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            m(static_x)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_out = [h for h in m(static_x).hidden_states if h is not None]
        for x, ref in zip(xs, eager):
            static_x.copy_(x)
            graph.replay()
            torch.cuda.synchronize()
            for a, b in zip(static_out, ref):
                assert torch.equal(a, b)


def test_two_modules_on_two_streams_with_lanes_forced():
    """Two modules, two caller streams, one side stream between them: both stay correct."""
    geom = "tiny"
    m1, m2 = _model(geom, 1), _model(geom, 2)
    L = m1.config.num_hidden_layers
    x1, x2 = _images(geom, 2), _images(geom, 3)
    with torch.no_grad():
        with _switches(LDIT_FWD_LANES="1"):
            r1 = m1(x1).hidden_states[L].clone()
            r2 = m2(x2).hidden_states[L].clone()
            torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        outs = []
        with _switches(LDIT_FWD_LANES="2"):
            for _ in range(5):
                with torch.cuda.stream(s1):
                    a = m1(x1).hidden_states[L]
                with torch.cuda.stream(s2):
                    b = m2(x2).hidden_states[L]
                outs.append((a, b))
            torch.cuda.synchronize()
    for a, b in outs:
        assert torch.equal(a, r1) and torch.equal(b, r2)
