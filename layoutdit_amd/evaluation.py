"""COCO box evaluation on the device: the scoring arithmetic of the reference's ``Evaluator.score()`` (ref
``src/layoutdit/evaluation/evaluator.py:219-286``), which copies every box to the host, writes a JSON file and hands it to
``pycocotools.COCOeval``.  Here the padded detections that ``LayoutDetectionModel.forward_padded`` delivers are matched to the GT
boxes per image as they arrive (``csrc/coco_eval.hip``: one launch per batch, results kept in a store allocated once), and
``compute()`` turns the store into COCO's precision / recall table and its 12 summary numbers with one key launch, one
``torch.sort`` and one accumulation launch - nothing is read back until the caller asks for the numbers (``summary()``).  The
dataset, the JSON files and the visualisations of the reference's evaluator stay outside this package.
"""
from __future__ import annotations

from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops

COCO_KEYS = ("mAP", "AP50", "AP75", "AP_s", "AP_m", "AP_l", "AR1", "AR10", "AR100", "AR_s", "AR_m", "AR_l")
# COCO's defaults, as numpy forms them: the kernels get these very doubles
IOU_THRS = tuple(float(x) for x in np.linspace(.5, .95, 10))
REC_THRS = tuple(float(x) for x in np.linspace(0, 1, 101))
MAX_DETS = (1, 10, 100)
AREA_RNG = ((0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))      # all, small, medium, large


def _masked_mean(x: torch.Tensor) -> torch.Tensor:
    """Mean over the entries ``> -1``, or ``-1`` when there is none; device arithmetic only."""
    valid = x > -1
    n = valid.sum()
    total = torch.where(valid, x, torch.zeros_like(x)).sum()
    return torch.where(n > 0, total / n.clamp(min=1).to(x.dtype), torch.full_like(total, -1.0))


class CocoBoxEvaluator:
    """COCO ``bbox`` evaluation of up to ``capacity`` images with categories ``1 .. num_classes``, at most ``max_dets`` detection slots
    and ``max_gt`` GT boxes per image (each at most 128; at most 64 categories).  ``update`` queues one launch per batch and keeps a
    host-side image count; ``compute`` queues the accumulation and returns device tensors; only ``summary`` synchronises."""

    def __init__(self, num_classes: int, capacity: int, max_dets: int = 128, max_gt: int = 128, device="cuda"):
        K, N, D, G = int(num_classes), int(capacity), int(max_dets), int(max_gt)
        ops._coco_caps(D, G, K)
        if N < 1 or N * D > ops.COCO_MAX_SLOTS:
            raise ValueError(f"CocoBoxEvaluator: capacity {N} x {D} slots: between 1 and 2^24 slots are handled")
        self.num_classes, self.capacity, self.max_dets, self.max_gt = K, N, D, G
        self.device = torch.device(device)
        dev = self.device
        self.code = torch.full((N, D, 4, 10), 3, device=dev, dtype=torch.uint8)
        self.rank = torch.full((N, D), -1, device=dev, dtype=torch.int32)
        self.npig = torch.zeros((N, K, 4), device=dev, dtype=torch.int32)
        self.scores = torch.zeros((N, D), device=dev, dtype=torch.float32)
        self.labels = torch.zeros((N, D), device=dev, dtype=torch.int32)
        self.precision = torch.full((10, 101, K, 4, 3), -1.0, device=dev, dtype=torch.float64)
        self.recall = torch.full((10, K, 4, 3), -1.0, device=dev, dtype=torch.float64)
        self.num_images = 0

    def reset(self) -> None:
        """Forget every image (device-side fills, no synchronisation)."""
        self.code.fill_(3)
        self.rank.fill_(-1)
        self.npig.zero_()
        self.scores.zero_()
        self.labels.zero_()
        self.precision.fill_(-1.0)
        self.recall.fill_(-1.0)
        self.num_images = 0

    def update(self, boxes: torch.Tensor, scores: torch.Tensor, labels: torch.Tensor, count: torch.Tensor, gt_boxes: torch.Tensor,
               gt_labels: torch.Tensor, gt_count: torch.Tensor, gt_crowd: Optional[torch.Tensor] = None,
               gt_area: Optional[torch.Tensor] = None) -> None:
        """Append a batch: ``boxes`` fp32 [B, D, 4] (xyxy), ``scores`` fp32 [B, D], ``labels`` int32 [B, D], ``count`` int32 [B] as
        ``forward_padded`` returns them (``D <= max_dets``); ``gt_boxes`` fp32 [B, G, 4], ``gt_labels`` int32 [B, G], ``gt_count`` int32
        [B] (``G <= max_gt``), ``gt_crowd`` uint8 [B, G] and ``gt_area`` fp32 [B, G] optional (no crowd; the box's own area).  Detections
        and GT boxes share one coordinate system.  One launch, no synchronisation; a batch that does not fit raises before it."""
        if not isinstance(scores, torch.Tensor) or scores.dim() != 2:
            raise ValueError("CocoBoxEvaluator.update: scores: expected a [B, D] tensor")
        B = int(scores.shape[0])
        if self.num_images + B > self.capacity:
            raise ValueError(f"CocoBoxEvaluator.update: {self.num_images} + {B} images overflow the capacity of {self.capacity}")
        if isinstance(gt_labels, torch.Tensor) and gt_labels.dim() == 2 and gt_labels.shape[1] > self.max_gt:
            raise ValueError(f"CocoBoxEvaluator.update: {gt_labels.shape[1]} GT boxes per image, max_gt is {self.max_gt}")
        ops.coco_match(boxes, scores, labels, count, gt_boxes, gt_labels, gt_count, gt_crowd, gt_area, self.num_classes, self.code, self.rank,
                       self.npig, self.scores, self.labels, self.num_images, IOU_THRS, AREA_RNG)
        self.num_images += B

    def update_lists(self, outputs: Sequence[Dict[str, torch.Tensor]], targets: Sequence[Dict[str, torch.Tensor]]) -> None:
        """Append the reference's lists: ``outputs`` as ``model.forward`` returns them (``{boxes [n, 4], labels [n], scores [n]}`` per
        image) and its target dicts (``{boxes [g, 4], labels [g]}`` with optional ``iscrowd`` [g] and ``area`` [g]).  They are padded
        to ``max_dets`` / ``max_gt`` rows with device-side copies (the lengths are shapes: no synchronisation) and go through
        :meth:`update`.  When some target carries ``area``, one that does not gets its boxes' area in float32."""
        if len(outputs) != len(targets) or len(outputs) == 0:
            raise ValueError("CocoBoxEvaluator.update_lists: one target per output, at least one image")
        B, D, G, dev = len(outputs), self.max_dets, self.max_gt, self.device
        f32, i32 = torch.float32, torch.int32
        boxes, scores = torch.zeros((B, D, 4), device=dev, dtype=f32), torch.zeros((B, D), device=dev, dtype=f32)
        labels = torch.zeros((B, D), device=dev, dtype=i32)
        counts = []
        for i, o in enumerate(outputs):
            n = int(o["scores"].shape[0])
            if n > D:
                raise ValueError(f"CocoBoxEvaluator.update_lists: image {i} has {n} detections, max_dets is {D}")
            if tuple(o["boxes"].shape) != (n, 4) or tuple(o["labels"].shape) != (n,):
                raise ValueError(f"CocoBoxEvaluator.update_lists: image {i}: boxes / labels / scores do not fit together")
            counts.append(n)
            if n:
                boxes[i, :n], scores[i, :n] = o["boxes"].detach().to(device=dev, dtype=f32), o["scores"].detach().to(device=dev, dtype=f32)
                labels[i, :n] = o["labels"].detach().to(device=dev, dtype=i32)
        count = _to_device(torch.tensor(counts, dtype=i32), dev)
        self.update(boxes, scores, labels, count, *_pad_targets(targets, G, dev))

    def compute(self) -> torch.Tensor:
        """Accumulate the images so far: fills ``.precision`` fp64 [10, 101, K, 4, 3] and ``.recall`` fp64 [10, K, 4, 3] (``-1``: a cell
        without GT) and returns the 12 numbers in ``COCO_KEYS`` order as a float64 device tensor.  No synchronisation; capturable."""
        ops.coco_accumulate(self.code, self.rank, self.npig, self.scores, self.labels, self.num_images, self.num_classes, REC_THRS, MAX_DETS,
                            self.precision, self.recall)
        p, r = self.precision, self.recall
        last = len(MAX_DETS) - 1
        parts = [p[:, :, :, 0, last], p[0, :, :, 0, last], p[5, :, :, 0, last], p[:, :, :, 1, last], p[:, :, :, 2, last], p[:, :, :, 3, last],
                 r[:, :, 0, 0], r[:, :, 0, 1], r[:, :, 0, 2], r[:, :, 1, last], r[:, :, 2, last], r[:, :, 3, last]]
        return torch.stack([_masked_mean(x) for x in parts])

    def summary(self) -> Dict[str, float]:
        """``compute()`` as the reference's dict: its 12 key names in its order.  This reads the numbers back: it SYNCHRONISES."""
        return dict(zip(COCO_KEYS, self.compute().tolist()))


def _to_device(host: torch.Tensor, device: torch.device) -> torch.Tensor:
    """A small host tensor on the device through pinned memory: the copy is queued, the host does not wait for the device."""
    if device.type != "cuda":
        return host.to(device)
    return host.pin_memory().to(device, non_blocking=True)


def evaluate(model, batches: Iterable[Tuple[List[torch.Tensor], List[Dict[str, torch.Tensor]]]], capacity: Optional[int] = None,
             max_gt: int = 128, evaluator: Optional[CocoBoxEvaluator] = None, tta=None) -> Dict[str, float]:
    """The loop of the reference's ``Evaluator.score()``: ``batches`` yields ``(images, targets)`` - a list of ``[3, h, w]`` images and
    the reference's target dicts in the ORIGINAL images' coordinates.  Per batch: the input transform, ``forward_padded``, the boxes
    times each image's ``(rw, rh, rw, rh)`` (formed on the host from the shapes exactly as ``resize_boxes`` forms them, so the boxes
    scored are bit for bit those of ``model.forward(images)``), then ``CocoBoxEvaluator.update``.  Nothing is read back before the
    end; returns the 12 numbers as a dict.  ``capacity``: the number of images (``None``: ``batches`` is listed first and counted).

    ``tta`` (a ``layoutdit_amd.TestTimeAugment``): per batch ``model.forward_padded_tta(images, tta)`` instead - its
    detections are already in the pages' coordinates and go to ``CocoBoxEvaluator.update`` as they are, still without a
    synchronisation.  ``head_dtype``, ``neck_dtype`` and ``compute_dtype`` need nothing, and under ``with step.ema_weights():`` the
    averaged weights are evaluated either way.  None: nothing changes."""
    if model.training:
        raise RuntimeError("evaluate: inference only - call .eval() first")
    m = model.model
    dev = next(model.parameters()).device
    d_out = m.roi_heads.detections_per_img if tta is None else tta.merge_args(model)[1]
    if evaluator is None:
        if capacity is None:
            batches = list(batches)
            capacity = sum(len(images) for images, _ in batches)
        evaluator = CocoBoxEvaluator(m.roi_heads.box_predictor.num_classes - 1, max(int(capacity), 1), d_out, max_gt, device=dev)
    elif tta is not None and evaluator.max_dets < d_out:
        raise ValueError(f"evaluate: the evaluator's max_dets = {evaluator.max_dets} does not cover the {d_out} detections per image of tta")
    for images, targets in batches:
        if len(images) != len(targets):
            raise ValueError("evaluate: one target per image")
        if tta is not None:
            boxes, scores, labels, count = model.forward_padded_tta(images, tta)
            evaluator.update(boxes, scores, labels, count, *_pad_targets(targets, evaluator.max_gt, boxes.device))
            continue
        image_list, _ = m.transform(images)
        boxes, scores, labels, count = model.forward_padded(image_list.tensors)
        ratios = []
        for img, (nh, nw) in zip(images, image_list.image_sizes):       # DetectorInputTransform.postprocess -> resize_boxes(boxes, new, orig)
            oh, ow = img.shape[-2:]
            rh, rw = float(oh) / float(nh), float(ow) / float(nw)
            ratios.append([rw, rh, rw, rh])
        scale = _to_device(torch.tensor(ratios, dtype=boxes.dtype), boxes.device)
        boxes = boxes * scale[:, None, :]
        gt = _pad_targets(targets, evaluator.max_gt, boxes.device)
        evaluator.update(boxes, scores, labels, count, *gt)
    return evaluator.summary()


def _pad_targets(targets, G: int, dev):
    """The reference's target dicts -> ``(gt_boxes, gt_labels, gt_count, gt_crowd, gt_area)`` padded to ``G`` rows on ``dev``, the last
    two ``None`` when no target carries ``iscrowd`` / ``area``.  The lengths are shapes: device-side copies, no synchronisation."""
    B, f32, i32 = len(targets), torch.float32, torch.int32
    gt_boxes, gt_labels = torch.zeros((B, G, 4), device=dev, dtype=f32), torch.zeros((B, G), device=dev, dtype=i32)
    any_crowd, any_area = any("iscrowd" in t for t in targets), any("area" in t for t in targets)
    gt_crowd = torch.zeros((B, G), device=dev, dtype=torch.uint8) if any_crowd else None
    gt_area = torch.zeros((B, G), device=dev, dtype=f32) if any_area else None
    counts = []
    for i, t in enumerate(targets):
        g = int(t["labels"].shape[0])
        if g > G:
            raise ValueError(f"image {i} has {g} GT boxes, max_gt is {G}")
        if tuple(t["boxes"].shape) != (g, 4):
            raise ValueError(f"image {i}: target boxes {tuple(t['boxes'].shape)} / labels {tuple(t['labels'].shape)} are not [G, 4] / [G]")
        counts.append(g)
        if g:
            gb = t["boxes"].detach().to(device=dev, dtype=f32)
            gt_boxes[i, :g], gt_labels[i, :g] = gb, t["labels"].detach().to(device=dev, dtype=i32)
            if "iscrowd" in t:
                gt_crowd[i, :g] = t["iscrowd"].detach().to(device=dev).ne(0).to(torch.uint8)
            if any_area:
                gt_area[i, :g] = t["area"].detach().to(device=dev, dtype=f32) if "area" in t else (gb[:, 2] - gb[:, 0]) * (gb[:, 3] - gb[:, 1])
    return gt_boxes, gt_labels, _to_device(torch.tensor(counts, dtype=i32), dev), gt_crowd, gt_area
