"""Train-time augmentation of the detector's input: which WINDOW of each page the input transform resizes to the batch.

DiT's published layout-detection recipe trains with a random crop, scale jitter and a flip.  Here all three are one window per image,
five host integers ``(x0, y0, cw, ch, flip)``: the crop is the window, the scale jitter is its size against the fixed batch size, the
flip its last entry.  The pixels of the window are resized straight from the page by the windowed input-transform kernel
(``ops.preprocess(..., windows=)``) and the boxes follow in one launch (``ops.augment_targets``) - no cropped copy, no boolean
indexing, no synchronisation.

:class:`DetectorAugment` only DRAWS the windows, on the host, from its own CPU generator: the pages' sizes are shapes, so nothing is
read from the device.  ``DetectorInputTransform.forward(images, targets, windows)``, ``LayoutDetectionModel.losses(..., windows=)`` and
``DetectorTrainStep(model, augment=)`` take them from there.
"""
from __future__ import annotations

import math
from typing import List, Sequence, Tuple

import torch


def whole_page_windows(sizes: Sequence[Sequence[int]]) -> List[Tuple[int, int, int, int, int]]:
    """The windows that change nothing: every ``(h, w)`` page whole, not flipped."""
    return [(0, 0, int(w), int(h), 0) for h, w in sizes]


class DetectorAugment:
    """Random crop / scale jitter / flip as windows.  ``scale``: the window's share of the page's area, uniform in the range;
    ``ratio``: the window's aspect as a multiple of the page's own, log-uniform in the range; ``crop_prob``: with probability
    ``1 - crop_prob`` the window is the whole page; ``flip_prob``: probability of a left-right mirror (default 0: text is not
    mirror-invariant).  ``min_visibility`` / ``min_size`` are what ``ops.augment_targets`` keeps a box by: its visible share of its own
    area, and its sides in the batch's pixels.  ``seed`` starts the object's own CPU generator.

    :meth:`sample` is a pure function of the generator's state and the sizes; ``state_dict`` / ``load_state_dict`` carry that state, so
    a resumed run draws the windows the uninterrupted one would."""

    def __init__(self, scale: Tuple[float, float] = (0.5, 1.0), ratio: Tuple[float, float] = (3.0 / 4.0, 4.0 / 3.0), crop_prob: float = 1.0,
                 flip_prob: float = 0.0, min_visibility: float = 0.3, min_size: float = 1.0, seed: int = 0):
        scale, ratio = (float(scale[0]), float(scale[1])), (float(ratio[0]), float(ratio[1]))
        if not 0.0 < scale[0] <= scale[1] <= 1.0:
            raise ValueError(f"DetectorAugment: scale {scale} must satisfy 0 < low <= high <= 1 (no zoom-out: a window lies inside its page)")
        if not 0.0 < ratio[0] <= ratio[1]:
            raise ValueError(f"DetectorAugment: ratio {ratio} must satisfy 0 < low <= high")
        if not 0.0 <= float(crop_prob) <= 1.0 or not 0.0 <= float(flip_prob) <= 1.0:
            raise ValueError("DetectorAugment: crop_prob and flip_prob are probabilities")
        if not float(min_visibility) >= 0.0 or not float(min_size) >= 0.0:
            raise ValueError("DetectorAugment: min_visibility and min_size must not be negative")
        self.scale, self.ratio = scale, ratio
        self.crop_prob, self.flip_prob = float(crop_prob), float(flip_prob)
        self.min_visibility, self.min_size = float(min_visibility), float(min_size)
        self.seed = int(seed)
        self.generator = torch.Generator(device="cpu")
        self.generator.manual_seed(self.seed)

    def sample(self, sizes: Sequence[Sequence[int]]) -> List[Tuple[int, int, int, int, int]]:
        """One window ``(x0, y0, cw, ch, flip)`` per ``(h, w)`` page.  Six uniform doubles are drawn per page whatever they decide, so
        the stream's position depends on the number of pages alone.  Area ``s * h * w`` and aspect ``r * w / h`` give ``cw = sqrt(s * r)
        * w`` and ``ch = sqrt(s / r) * h``, rounded to integers and clamped to ``[1, w]`` / ``[1, h]``; the origin is uniform over the
        positions at which the window lies inside the page."""
        sizes = [(int(h), int(w)) for h, w in sizes]
        for i, (h, w) in enumerate(sizes):
            if h < 1 or w < 1:
                raise ValueError(f"DetectorAugment.sample: page {i} is {w} x {h} (width x height)")
        if not sizes:
            return []
        u = torch.rand((len(sizes), 6), generator=self.generator, dtype=torch.float64).tolist()
        out = []
        for (h, w), (u_crop, u_scale, u_ratio, u_x, u_y, u_flip) in zip(sizes, u):
            cw, ch, x0, y0 = w, h, 0, 0
            if u_crop < self.crop_prob:
                s = self.scale[0] + (self.scale[1] - self.scale[0]) * u_scale
                r = math.exp(math.log(self.ratio[0]) + (math.log(self.ratio[1]) - math.log(self.ratio[0])) * u_ratio)
                cw = min(max(int(round(math.sqrt(s * r) * w)), 1), w)
                ch = min(max(int(round(math.sqrt(s / r) * h)), 1), h)
                x0 = min(int(u_x * (w - cw + 1)), w - cw)
                y0 = min(int(u_y * (h - ch + 1)), h - ch)
            out.append((x0, y0, cw, ch, int(u_flip < self.flip_prob)))
        return out

    def state_dict(self) -> dict:
        return {"generator": self.generator.get_state().clone()}

    def load_state_dict(self, sd: dict) -> None:
        self.generator.set_state(sd["generator"].to(device="cpu", dtype=torch.uint8))
