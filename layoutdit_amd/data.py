"""Getting decoded pages onto the GPU: one pinned host buffer, one copy, uint8 all the way.

A decoder hands over uint8 pages, usually interleaved ``[h, w, C]``.  The image-list entries read those codes as they are
(``ops.image_list_args``: planar or interleaved uint8, any byte alignment, ``c`` standing for ``c / 255``), so nothing has to be
widened, divided or transposed on the CPU, and a batch crosses the link at a quarter of its fp32 size.  ``stage_images`` is the
remaining step: it packs a ragged batch back to back into ONE pinned buffer and moves it with ONE non-blocking copy instead of
one small copy per page.  The kernels do the rest.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

LAYOUTS = ("hwc", "chw")


class StagingBuffer:
    """The host side of ``stage_images``, kept by the caller and passed back in so that the next batch reuses it: a uint8 buffer
    (pinned when the destination is a GPU) that grows to the largest batch seen, and the event that says when the last copy out
    of it has finished - the buffer is not overwritten before that."""

    def __init__(self):
        self.host: Optional[torch.Tensor] = None
        self.event = None

    def reserve(self, nbytes: int, pin: bool) -> torch.Tensor:
        if self.event is not None:
            self.event.synchronize()            # the previous batch has left the buffer
            self.event = None
        if self.host is None or self.host.numel() < nbytes or self.host.is_pinned() != pin:
            self.host = torch.empty(max(nbytes, 1), dtype=torch.uint8, pin_memory=pin)
        return self.host


def _as_array(img, i: int) -> np.ndarray:
    if isinstance(img, torch.Tensor):
        if img.device.type != "cpu":
            raise ValueError(f"images[{i}]: stage_images takes CPU images (this one is on {img.device})")
        if img.dtype != torch.uint8:
            raise ValueError(f"images[{i}]: expected uint8, got {img.dtype}")
        a = img.detach().numpy()
    else:
        a = np.asarray(img)
        if a.dtype != np.uint8:
            raise ValueError(f"images[{i}]: expected uint8, got {a.dtype}")
    if a.ndim != 3 or 0 in a.shape:
        raise ValueError(f"images[{i}]: expected a non-empty 3-d image, got shape {tuple(a.shape)}")
    return a


def stage_images(images: Sequence, device, pinned: Optional[StagingBuffer] = None, *, layout: str) -> List[torch.Tensor]:
    """CPU uint8 images (numpy arrays or tensors, ragged) -> ``[C, h, w]`` uint8 views of ONE buffer on ``device``, ready for
    ``ops.preprocess``, ``DiTEncoder.forward_image_list`` and the detector.

    ``layout`` says how every input is stored and is never guessed from the shapes: ``"hwc"`` (``[h, w, C]``, a decoder's array; the
    views returned are interleaved, strides ``(1, w*C, C)``) or ``"chw"`` (``[C, h, w]``; the views are contiguous).  The bytes are
    packed back to back - the kernels need no alignment - into ``pinned``'s host buffer and cross in one non-blocking copy on the
    current stream of ``device``.  ``pinned``: a ``StagingBuffer`` to reuse across batches (``None``: a buffer for this call only)."""
    if layout not in LAYOUTS:
        raise ValueError(f"layout must be one of {LAYOUTS} (it is stated, not guessed), got {layout!r}")
    if len(images) == 0:
        raise ValueError("empty image list")
    device = torch.device(device)
    arrays = [_as_array(img, i) for i, img in enumerate(images)]
    ch = arrays[0].shape[2 if layout == "hwc" else 0]
    for i, a in enumerate(arrays):
        if a.shape[2 if layout == "hwc" else 0] != ch:
            raise ValueError(f"images[{i}]: {a.shape[2 if layout == 'hwc' else 0]} channels in a list of {ch}-channel images "
                             f"(layout {layout!r})")
    sizes = [a.size for a in arrays]
    total = sum(sizes)
    stage = pinned if pinned is not None else StagingBuffer()
    gpu = device.type == "cuda"
    host = stage.reserve(total, pin=gpu)
    flat = host.numpy()
    off = 0
    for a, n in zip(arrays, sizes):
        flat[off:off + n].reshape(a.shape)[...] = a
        off += n
    dev = torch.empty(total, dtype=torch.uint8, device=device)
    dev.copy_(host[:total], non_blocking=True)
    if gpu:
        stage.event = torch.cuda.Event()
        stage.event.record(torch.cuda.current_stream(device))
    out, off = [], 0
    for a, n in zip(arrays, sizes):
        v = dev[off:off + n].view(a.shape)
        out.append(v.permute(2, 0, 1) if layout == "hwc" else v)
        off += n
    return out
