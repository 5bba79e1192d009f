"""Guard bands around kernel operands: does a kernel depend on, or touch, memory outside its operands?

A test helper (not a conftest, no fixtures), device-agnostic: it works on CPU tensors exactly as on ``cuda`` ones.

An operand is placed inside a larger byte parent and handed to the code under test as a strided view of the wanted shape:

    parent:  | margin | row 0: gap . operand . gap | row 1: gap . operand . gap | ... | margin |

- each margin is at least one full operand row and at least 256 bytes; the view starts 16-byte aligned;
- a row stride ``ld > cols`` leaves gap columns on both sides of the operand's columns (the front gap a multiple of 16 bytes);
- what surrounds an INPUT is ``0xFF`` in every byte (NaN as fp32, bf16, fp16, fp8 e4m3 and E8M0, -1 as any integer) or, for the
  clean twin with IDENTICAL geometry, ``0x00``;
- what surrounds an OUTPUT is ``0xA5`` in every byte, and so is the output's own footprint before the call (a kernel that
  leaves an element unwritten shows as ``0xA5`` bytes there);
- after the call every byte outside an output's footprint must still hold ``0xA5``, gap columns included, and every byte of an
  input's parent must be what it was (inputs are ``const``).

Padding INSIDE an operand - the rows past a ``count`` of the padded, fixed-size results - is marked with ``In(..., pad=mask)`` and
holds the run's fill byte as well.

``twin_run`` runs one call twice - input surroundings and scratch ``0x00``, then ``0xFF`` - and asserts that the outputs'
parents are equal bit for bit: with identical geometry no tolerance is needed.  The caller adds its parity gate on the first
result and its finiteness claim on the second.
"""
from __future__ import annotations

import contextlib
from typing import Callable, Dict, Optional, Sequence

import numpy as np
import torch

POISON, CLEAN, CANARY = 0xFF, 0x00, 0xA5
MIN_MARGIN = 256


class GuardError(AssertionError):
    """A guard band was violated, or two runs that may differ only outside their operands disagree."""


def _round_up(n: int, m: int) -> int:
    return (n + m - 1) // m * m


def _contiguous_strides(shape: Sequence[int]):
    st, acc = [], 1
    for s in reversed(shape):
        st.append(acc)
        acc *= max(int(s), 1)
    return tuple(reversed(st))


class Guarded:
    """One operand inside its parent.  ``view``: the tensor the code under test gets; ``parent``: all bytes (uint8, 1-D)."""

    def __init__(self, shape, dtype: torch.dtype, *, ld: Optional[int] = None, strides=None, fill: int = POISON, data=None,
                 device="cpu", name: str = "operand", col0: Optional[int] = None, pad=None, pad_fill: Optional[int] = None):
        shape = tuple(int(s) for s in shape)
        isz = torch.empty((), dtype=dtype).element_size()
        if strides is None:
            strides = list(_contiguous_strides(shape))
            if ld is not None:
                assert len(shape) >= 2 and ld >= shape[-1], "ld is the stride of the second-to-last axis and at least cols"
                inner = strides[-2]
                strides = [s // inner * ld if i < len(shape) - 1 else s for i, s in enumerate(strides)]
        strides = tuple(int(s) for s in strides)
        assert len(strides) == len(shape)
        # element offsets of the footprint (relative to the view's first element)
        # (runs of `run` consecutive elements when the last axis has unit stride: one offset per run)
        unit = len(shape) >= 1 and strides[-1] == 1
        run = shape[-1] if unit else 1
        lead = list(zip(shape[:-1], strides[:-1])) if unit else list(zip(shape, strides))
        offs = np.zeros((1,) * max(len(lead), 1), dtype=np.int64)
        for ax, (n, st) in enumerate(lead):
            idx = (np.arange(n, dtype=np.int64) * st).reshape([n if a == ax else 1 for a in range(len(lead))])
            offs = offs + idx
        offs = offs.reshape(-1) if run and all(s > 0 for s in shape) else np.zeros(0, dtype=np.int64)
        extent = int(offs.max()) + run if offs.size else 0
        row_elems = strides[-2] if len(shape) >= 2 else max(extent, 1)
        # gap columns: the operand's columns sit inside their row, the front gap a multiple of 16 bytes
        gap = row_elems - shape[-1] if len(shape) >= 2 and strides[-1] == 1 else 0
        if col0 is None:
            col0 = (gap // 2) * isz // 16 * 16 // isz
        assert 0 <= col0 <= max(gap, 0) and (col0 * isz) % 16 == 0
        margin = _round_up(max(MIN_MARGIN, row_elems * isz), 16)
        start = margin + col0 * isz
        body = _round_up(max(extent, 1) * isz + (gap * isz if gap else 0), 16)
        total = margin + body + margin
        self.name, self.fill, self.dtype, self.shape, self.strides = name, int(fill), dtype, shape, strides
        self.nbytes, self.start, self.itemsize = total, start, isz
        self.parent = torch.full((total,), self.fill, dtype=torch.uint8, device=device)
        typed = self.parent.view(dtype)
        self.view = torch.as_strided(typed, shape, strides, start // isz)
        delta = np.zeros(total + 1, dtype=np.int32)        # +1 where a run of operand bytes starts, -1 behind its end
        if offs.size:
            b0 = start + offs * isz
            np.add.at(delta, b0, 1)
            np.add.at(delta, b0 + run * isz, -1)
        self.footprint = np.cumsum(delta[:-1]) > 0
        if data is not None:
            if isinstance(data, np.ndarray):
                data = torch.from_numpy(np.ascontiguousarray(data))
            assert tuple(data.shape) == shape, (name, tuple(data.shape), shape)
            self.view.copy_(data.to(dtype).to(device))
        if pad is not None:
            # padding elements INSIDE the operand (rows past a count): every byte of them holds pad_fill
            idt = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[isz]
            word = int.from_bytes(bytes([self.fill if pad_fill is None else pad_fill]) * isz, "little", signed=idt != torch.uint8)
            ints = torch.as_strided(self.parent.view(idt), shape, strides, start // isz)
            ints.masked_fill_(torch.as_tensor(pad, dtype=torch.bool).expand(shape).to(device), word)
        self._before = self.bytes()

    def bytes(self) -> np.ndarray:
        return self.parent.cpu().numpy().copy()

    def value(self) -> torch.Tensor:
        """A dense CPU copy of the operand."""
        return self.view.detach().cpu().contiguous().clone()

    def check_surroundings(self) -> None:
        """Every byte outside the footprint still holds the fill."""
        now = self.bytes()
        bad = np.flatnonzero((now != self.fill) & ~self.footprint)
        if bad.size:
            raise GuardError(f"{self.name}: {bad.size} byte(s) outside the operand were written, first at byte offset "
                             f"{int(bad[0]) - self.start} relative to the operand's start (parent of {self.nbytes} bytes)")

    def check_unchanged(self) -> None:
        """Every byte of the parent, operand included, is what it was (a const input)."""
        bad = np.flatnonzero(self.bytes() != self._before)
        if bad.size:
            raise GuardError(f"{self.name}: const operand changed, {bad.size} byte(s), first at byte offset "
                             f"{int(bad[0]) - self.start} relative to the operand's start")


class In:
    """Spec of an input: ``data`` (numpy array or CPU tensor; its dtype unless ``dtype`` is given).  ``pad``: a boolean mask
    (broadcastable to the data) of padding elements inside the operand - rows past a count - that get the run's fill byte too."""

    def __init__(self, data, ld: Optional[int] = None, strides=None, dtype: Optional[torch.dtype] = None, col0: Optional[int] = None,
                 pad=None):
        if isinstance(data, np.ndarray):
            data = torch.from_numpy(np.ascontiguousarray(data))
        self.data, self.ld, self.strides, self.dtype, self.col0 = data, ld, strides, dtype or data.dtype, col0
        self.pad = pad


class Out:
    """Spec of an output.  ``init``: contents the contract defines before the call (an in-place residual, a ``+=`` destination).
    ``scratch``: the output is a buffer whose previous contents the callee may not rely on (split-K slabs): its own footprint holds
    the run's fill (``0x00`` / ``0xFF``) before the call instead of the canary, which stays around it."""

    def __init__(self, shape, dtype: torch.dtype = torch.float32, ld: Optional[int] = None, strides=None, init=None,
                 col0: Optional[int] = None, scratch: bool = False):
        self.shape, self.dtype, self.ld, self.strides, self.init, self.col0 = tuple(shape), dtype, ld, strides, init, col0
        self.scratch = scratch


class Scratch:
    """Spec of a workspace of ``nbytes`` whose previous contents the callee may not rely on: ``0x00`` in one run, ``0xFF`` in the other."""

    def __init__(self, nbytes: int):
        self.nbytes = int(nbytes)


class TwinResult:
    def __init__(self):
        self.clean: Dict[str, torch.Tensor] = {}      # outputs of the run with 0x00 around the inputs (dense CPU copies)
        self.poisoned: Dict[str, torch.Tensor] = {}   # outputs of the run with 0xFF around the inputs


def build(specs: Dict[str, object], fill: int, device) -> Dict[str, Guarded]:
    made = {}
    for name, s in specs.items():
        if isinstance(s, In):
            made[name] = Guarded(s.data.shape, s.dtype, ld=s.ld, strides=s.strides, fill=fill, data=s.data,
                                 device=device, name=name, col0=s.col0, pad=s.pad, pad_fill=fill)
        elif isinstance(s, Out):
            made[name] = Guarded(s.shape, s.dtype, ld=s.ld, strides=s.strides, fill=CANARY, data=s.init, device=device, name=name,
                                 col0=s.col0, pad=torch.ones(1, dtype=torch.bool) if s.scratch else None, pad_fill=fill)
        elif isinstance(s, Scratch):
            g = Guarded((max(s.nbytes, 1),), torch.uint8, fill=CANARY, device=device, name=name)
            g.view.fill_(fill)
            made[name] = g
        else:
            raise TypeError(f"{name}: not an In / Out / Scratch spec")
    return made


def twin_run(specs: Dict[str, object], call: Callable[[Dict[str, torch.Tensor]], None], device="cpu",
             sync: Optional[Callable[[], None]] = None) -> TwinResult:
    """Run ``call(views)`` with ``0x00`` and then with ``0xFF`` around every input and inside every scratch, identical geometry.
    Asserts (c) output surroundings and input bytes untouched in both runs and (a) output parents bit-equal between the runs."""
    res, parents = TwinResult(), []
    for fill, store in ((CLEAN, res.clean), (POISON, res.poisoned)):
        made = build(specs, fill, device)
        call({k: g.view for k, g in made.items()})
        if sync is not None:
            sync()
        snap = {}
        for name, g in made.items():
            s = specs[name]
            if isinstance(s, In):
                g.check_unchanged()
            else:
                g.check_surroundings()
            if isinstance(s, Out):
                snap[name] = g.bytes()
                store[name] = g.value()
        parents.append(snap)
    for name in parents[0]:
        a, b = parents[0][name], parents[1][name]
        if not np.array_equal(a, b):
            bad = np.flatnonzero(a != b)
            raise GuardError(f"{name}: the result depends on memory outside the operands: {bad.size} byte(s) differ between the "
                             f"0x00 and the 0xFF run, first at parent byte {int(bad[0])}")
    return res


def assert_finite(t: torch.Tensor, what: str = "output") -> None:
    if not bool(torch.isfinite(t.float()).all()):
        raise GuardError(f"{what}: non-finite values under poisoned surroundings "
                         f"({int((~torch.isfinite(t.float())).sum())} of {t.numel()})")


def assert_written(t: torch.Tensor, what: str = "output") -> None:
    """No element still holds the ``0xA5`` canary in every byte (an element the kernel never wrote).  One-byte elements are not
    judged: 0xA5 is an ordinary fp8 code (-0.203125) and an ordinary byte, so only the caller's exact oracle can tell."""
    if t.element_size() == 1:
        return
    raw = t.contiguous().view(torch.uint8).reshape(-1, t.element_size())
    left = int((raw == CANARY).all(dim=1).sum())
    if left:
        raise GuardError(f"{what}: {left} of {t.numel()} element(s) were never written (still 0xA5 in every byte)")


@contextlib.contextmanager
def fresh_memory(monkeypatch, fill: int):
    """While active, ``torch.empty``, ``torch.empty_like`` and ``Tensor.new_empty`` return tensors whose bytes are all ``fill``:
    what a fresh allocation may hold is then chosen by the test rather than by the caching allocator's history."""
    real_empty, real_like, real_new = torch.empty, torch.empty_like, torch.Tensor.new_empty

    def _filled(t):
        if isinstance(t, torch.Tensor) and t.numel():
            # a fresh tensor is dense whatever its memory format: its elements are one run of storage
            flat = torch.as_strided(t, (t.numel(),), (1,), t.storage_offset())
            if t.dtype == torch.bool:
                flat.fill_(bool(fill))
            else:
                flat.view(torch.uint8).fill_(fill)
        return t

    def empty(*a, **k):
        return _filled(real_empty(*a, **k))

    def empty_like(*a, **k):
        return _filled(real_like(*a, **k))

    def new_empty(self, *a, **k):
        return _filled(real_new(self, *a, **k))

    with monkeypatch.context() as m:
        m.setattr(torch, "empty", empty)
        m.setattr(torch, "empty_like", empty_like)
        m.setattr(torch.Tensor, "new_empty", new_empty)
        yield
