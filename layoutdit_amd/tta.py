"""Test-time augmentation of the detector: the page is run through several VIEWS - other sizes, a horizontal
mirror - each view's detections are mapped back to the page, the pooled boxes go through one class-wise NMS and, optionally, each
surviving box is refined from the boxes that agree with it ("box voting").  :class:`TestTimeAugment` is the description of the
views and of the merge; ``LayoutDetectionModel.forward_padded_tta(images, tta)``, ``model(images, tta=tta)`` and ``evaluate(...,
tta=tta)`` consume it.  A view costs no copy of a page (``ops.preprocess(..., size=, windows=)`` mirrors and resizes from the page
itself) and the merge is three device launches without a synchronisation (``ops.tta_merge``).

What it does to the accuracy of a trained detector is not measured here: there are no trained weights beside this package.
"""
from __future__ import annotations

import operator
from typing import List, NamedTuple, Optional, Sequence, Tuple

from . import ops

MAX_VIEWS = ops.TTA_MAX_VIEWS


class TTAView(NamedTuple):
    """One view: the batch at ``width`` x ``height``, mirrored left-right where ``flip`` is 1."""
    width: int
    height: int
    flip: int


def _thresh(name: str, value) -> Optional[float]:
    if value is None:
        return None
    value = float(value)
    if not 0.0 <= value <= 1.0:                          # NaN fails both comparisons
        raise ValueError(f"TestTimeAugment: {name} = {value} is outside [0, 1]")
    return value


class TestTimeAugment:
    """``sizes``: a sequence of ``(width, height)`` in the input transform's ``fixed_size`` convention, each side a positive multiple
    of 32 (``None``: the model's own size).  ``flip``: every size is also run mirrored left-right.  The views, in the FIXED order that
    decides ties between equal scores (the pool is indexed view-major): every size plain, in the order given, then every size
    mirrored, in the same order.  At most 16 views.  ``nms_thresh`` / ``detections_per_img``: the class-wise NMS over the pooled
    detections and the number of rows of the result; ``vote_thresh``: a kept box becomes the score-weighted mean of the pooled boxes of
    its class whose IoU with it is at least this (``None``: no voting, the kept boxes' own bits).  ``None`` for the NMS threshold and
    the cap means the model's own ``roi_heads`` values.  Everything is checked here, at construction."""

    __test__ = False                                     # not a test class, whatever its name says to a collector

    def __init__(self, sizes: Optional[Sequence[Sequence[int]]] = None, flip: bool = True, nms_thresh: Optional[float] = None,
                 vote_thresh: Optional[float] = None, detections_per_img: Optional[int] = None):
        self.flip = bool(flip)
        self.sizes: Optional[Tuple[Tuple[int, int], ...]] = None
        if sizes is not None:
            checked = []
            for i, s in enumerate(sizes):
                try:
                    s = tuple(operator.index(x) for x in s)
                except TypeError:
                    s = ()
                if len(s) != 2 or min(s) < 32 or s[0] % 32 or s[1] % 32:
                    raise ValueError(f"TestTimeAugment: sizes[{i}] must be (width, height), each a positive multiple of 32, got {list(sizes)[i]!r}")
                checked.append(s)
            if not checked:
                raise ValueError("TestTimeAugment: sizes is empty (None means the model's own size)")
            self.sizes = tuple(checked)
        n_views = (len(self.sizes) if self.sizes is not None else 1) * (2 if self.flip else 1)
        if n_views > MAX_VIEWS:
            raise ValueError(f"TestTimeAugment: {n_views} views, at most {MAX_VIEWS} are handled")
        self.nms_thresh = _thresh("nms_thresh", nms_thresh)
        self.vote_thresh = _thresh("vote_thresh", vote_thresh)
        self.detections_per_img = None
        if detections_per_img is not None:
            self.detections_per_img = operator.index(detections_per_img)
            if self.detections_per_img < 1:
                raise ValueError(f"TestTimeAugment: detections_per_img = {detections_per_img} must be positive")

    def views(self, model=None) -> List[TTAView]:
        """The resolved views in pool order.  ``model`` (a ``LayoutDetectionModel``) supplies the size where ``sizes`` is ``None``."""
        sizes = self.sizes
        if sizes is None:
            if model is None:
                raise ValueError("TestTimeAugment.views: sizes=None means the model's own size - pass the model")
            t = model.model.transform
            sizes = ((t.out_w, t.out_h),)
        out = [TTAView(w, h, 0) for w, h in sizes]
        if self.flip:
            out += [TTAView(w, h, 1) for w, h in sizes]
        return out

    def merge_args(self, model) -> Tuple[float, int, Optional[float]]:
        """``(nms_thresh, detections_per_img, vote_thresh)`` with the model's ``roi_heads`` values where this object holds ``None``."""
        rh = model.model.roi_heads
        return (rh.nms_thresh if self.nms_thresh is None else self.nms_thresh,
                rh.detections_per_img if self.detections_per_img is None else self.detections_per_img, self.vote_thresh)

    def __repr__(self) -> str:
        return (f"TestTimeAugment(sizes={None if self.sizes is None else list(self.sizes)}, flip={self.flip}, nms_thresh={self.nms_thresh}, "
                f"vote_thresh={self.vote_thresh}, detections_per_img={self.detections_per_img})")
