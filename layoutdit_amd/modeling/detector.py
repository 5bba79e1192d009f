"""``LayoutDetectionModel`` (ref ``src/layoutdit/modeling/model.py:20-88``): the reference's
``FasterRCNN(DiTWithFPN, num_classes + 1, rpn_anchor_generator=AnchorGenerator(...), box_roi_pool=MultiScaleRoIAlign(["p2", "p3",
"p4", "p5", "pool"], 7, 2), fixed_size=(224, 224), image_mean / std 0.5)`` assembled from this package's stages: input transform,
``DiTWithFPN``, ``RegionProposalNetwork``, ``RoIHeads``.  ``forward(images)`` has torchvision's surface (a list of ``[3, h, w]``
images in, a list of ``{boxes, labels, scores}`` in each image's own coordinates out, one synchronisation);
``forward_padded(batch)`` is the fixed-size path from pixels to padded detections without any - it can sit in one graph.

The ``state_dict`` keys are the reference's (``model.backbone.*``, ``model.rpn.head.*``, ``model.roi_heads.box_head.fc6.*`` ...).
Training: ``rpn_losses(images, targets)`` is the RPN half of the reference's ``loss_dict = model(images, targets)``
(ref ``training/trainer.py:164-183``) - ``loss_objectness`` and ``loss_rpn_box_reg``; ``losses(images, targets)`` is the whole dict,
with the box head's ``loss_classifier`` and ``loss_box_reg`` on the RPN's (detached) train-mode proposals - all four differentiable
down to the encoder.  ``forward`` and ``forward_padded`` keep torchvision's eval surface and stay refused in train mode.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from ..config import DiTConfig
from .detector_input import DetectorInputTransform
from .dit_fpn import DiTWithFPN
from .grad_ops import check_dtype
from .roi_heads import FastRCNNPredictor, MultiScaleRoIAlign, RoIHeads, TwoMLPHead, _nhwc_f32
from .rpn import AnchorGenerator, RegionProposalNetwork, RPNHead

FEATMAP_NAMES = ("p2", "p3", "p4", "p5", "pool")


class _FasterRCNN(nn.Module):
    """The container whose attribute names give the parameters torchvision's keys: ``backbone``, ``rpn``, ``roi_heads``
    (``transform`` holds no parameter)."""

    def __init__(self, backbone: DiTWithFPN, num_classes: int, anchor_generator: AnchorGenerator, fixed_size=(224, 224),
                 head_dtype: str = "f32", neck_dtype: str = "f32", grad_dtype: str = "f32", train_dtype: str = "f32"):
        super().__init__()
        self.transform = DetectorInputTransform(fixed_size=tuple(fixed_size), image_mean=(0.5, 0.5, 0.5), image_std=(0.5, 0.5, 0.5))
        self.backbone = backbone
        c = backbone.out_channels
        self.rpn = RegionProposalNetwork(anchor_generator, RPNHead(c, anchor_generator.num_anchors_per_location()[0], neck_dtype=neck_dtype,
                                                                           grad_dtype=grad_dtype, train_dtype=train_dtype))
        pool = MultiScaleRoIAlign(FEATMAP_NAMES, output_size=7, sampling_ratio=2)
        self.roi_heads = RoIHeads(pool, TwoMLPHead(c * 7 * 7, 1024, grad_dtype=grad_dtype, train_dtype=train_dtype),
                                  FastRCNNPredictor(1024, num_classes), head_dtype=head_dtype)


class LayoutDetectionModel(nn.Module):
    def __init__(self, num_classes: int = 5, anchor_sizes=((32,), (64,), (128,), (256,), (512,)),
                 aspect_ratios=((0.5, 1.0, 2.0),) * 5, config: Optional[DiTConfig] = None, compute_dtype: str = "f32",
                 fixed_size: Tuple[int, int] = (224, 224), head_dtype: str = "f32", neck_dtype: str = "f32", grad_dtype: str = "f32",
                 train_dtype: str = "f32", qat: bool = False):
        """``num_classes`` counts the foreground classes (the reference adds the background itself, ref model.py:47); the anchor
        defaults are the reference's ``ModelConfig``.  ``compute_dtype`` selects the encoder build; the box head is fp32 in every build
        unless ``head_dtype="bf16"`` (eval mode only: bf16 pooled rows and bf16 GEMMs with fp32 accumulation behind the fp32 maps; the
        losses stay fp32), and so is the neck - the FPN and the RPN head - unless ``neck_dtype="bf16"`` (only where no gradient is
        wanted: their eight 3x3 convolutions and the RPN head's 1x1 pair on the bf16 MFMA GEMM with fp32 accumulation; laterals,
        merges, the fp32 maps the heads read and every loss stay as they are).  ``fixed_size`` is the input transform's ``(width, height)``, the
        reference's 224 x 224 by default: a multiple of 32 (the transform's check) whose sides the encoder's patch size divides
        (the encoder's own check).  ``grad_dtype="bf16"`` (default ``"f32"``) concerns the backward alone: the input-gradient GEMMs of the
        FPN, the RPN head and the box head run on the bf16 MFMA GEMM (bf16 operand rounding, fp32 accumulation - what every weight
        gradient of the detector has under either setting); every forward, hence every loss, sampled anchor and proposal, keeps its
        bits, and eval mode and ``no_grad`` never read it.  ``train_dtype="bf16"`` (default ``"f32"``) concerns the forward where a
        gradient is wanted - ``losses`` / ``rpn_losses`` in train mode: the FPN's and the RPN head's 3x3 convolutions, the RPN head's
        1x1 pair, fc6, fc7 and the box predictor run as ``neck_dtype`` / ``head_dtype="bf16"`` run them in eval mode (bf16 operand
        rounding, fp32 accumulation), and the backward reads the bf16 tensors that forward saved; eval mode and ``no_grad`` never read
        it, and it is independent of the other three options.  ``qat=True`` (``compute_dtype="mxfp8"`` only; anything else is the
        encoder's ``ValueError``): the encoder is the quantisation-aware training build of the mxfp8 inference build - ``losses`` runs
        the inference arithmetic in the forward and a straight-through backward against fp32 masters, and ``DetectorTrainStep`` trains
        it.  The parameters and ``state_dict`` keys are those of every other build."""
        super().__init__()
        for option, value in (("head_dtype", head_dtype), ("neck_dtype", neck_dtype), ("grad_dtype", grad_dtype), ("train_dtype", train_dtype)):
            check_dtype(option, value)
        if len(set(len(s) * len(r) for s, r in zip(anchor_sizes, aspect_ratios))) != 1:
            raise ValueError("LayoutDetectionModel: every level must have the same number of anchors per location (one RPN head)")
        backbone = DiTWithFPN(pretrained=False, config=config, compute_dtype=compute_dtype, qat=qat, neck_dtype=neck_dtype,
                              grad_dtype=grad_dtype, train_dtype=train_dtype)
        self.model = _FasterRCNN(backbone, int(num_classes) + 1, AnchorGenerator(sizes=anchor_sizes, aspect_ratios=aspect_ratios),
                                 fixed_size=fixed_size, head_dtype=head_dtype, neck_dtype=neck_dtype, grad_dtype=grad_dtype,
                                 train_dtype=train_dtype)

    def _set(self, option: str, value: str, *stages) -> "LayoutDetectionModel":
        check_dtype(option, value)                                    # refused before any stage changes
        for stage in stages:
            getattr(stage, "set_" + option)(value)
        return self

    @property
    def qat(self) -> bool:
        """Whether the encoder is the quantisation-aware training build of ``compute_dtype="mxfp8"`` (fixed at construction)."""
        return self.model.backbone.backbone.dit.qat

    @property
    def head_dtype(self) -> str:
        return self.model.roi_heads.head_dtype

    def set_head_dtype(self, head_dtype: str) -> "LayoutDetectionModel":
        """``"f32"`` or ``"bf16"``: how the box head of ``forward`` / ``forward_padded`` runs from now on, on the same weights."""
        return self._set("head_dtype", head_dtype, self.model.roi_heads)

    @property
    def neck_dtype(self) -> str:
        return self.model.backbone.neck_dtype

    def set_neck_dtype(self, neck_dtype: str) -> "LayoutDetectionModel":
        """``"f32"`` or ``"bf16"``: how the FPN's and the RPN head's convolutions of ``forward`` / ``forward_padded`` run from now on,
        on the same weights."""
        return self._set("neck_dtype", neck_dtype, self.model.backbone, self.model.rpn.head)

    @property
    def grad_dtype(self) -> str:
        return self.model.backbone.grad_dtype

    def set_grad_dtype(self, grad_dtype: str) -> "LayoutDetectionModel":
        """``"f32"`` or ``"bf16"``: the matrix pipe of the dgrad GEMMs of the FPN's, the RPN head's and the box head's backward from now
        on, on the same weights.  No forward changes."""
        return self._set("grad_dtype", grad_dtype, self.model.backbone, self.model.rpn.head, self.model.roi_heads)

    @property
    def train_dtype(self) -> str:
        return self.model.backbone.train_dtype

    def set_train_dtype(self, train_dtype: str) -> "LayoutDetectionModel":
        """``"f32"`` or ``"bf16"``: the matrix pipe of the FPN's, the RPN head's and the box head's forward from now on where a gradient
        is wanted, on the same weights.  Eval mode and ``no_grad`` do not change."""
        return self._set("train_dtype", train_dtype, self.model.backbone, self.model.rpn.head, self.model.roi_heads)

    def forward_padded(self, batch: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """``batch`` [B, 3, H, W] (already transformed) -> ``(boxes [B, D, 4], scores [B, D], labels int32 [B, D], count int32 [B])``
        in the coordinates of the batch, zero padding, no synchronisation."""
        m = self.model
        if self.training:
            raise RuntimeError("LayoutDetectionModel: forward_padded is inference only (the four losses are losses(images, targets)) - "
                               "call .eval() first")
        image_size = tuple(batch.shape[-2:])
        with torch.no_grad():
            feats = m.backbone(batch)
            feats = {k: _nhwc_f32(v) for k, v in feats.items()}      # low-precision inputs: the heads stay fp32
            proposals, _, count = m.rpn(feats, image_size, padded=True)
            return m.roi_heads(feats, proposals, count, image_size, padded=True)

    def rpn_losses(self, images: List[torch.Tensor], targets: List[Dict[str, torch.Tensor]],
                   generator: Optional[torch.Generator] = None, windows=None) -> Dict[str, torch.Tensor]:
        """The RPN half of the reference's loss dict: ``{"loss_objectness", "loss_rpn_box_reg"}`` for a list of ``[3, h, w]`` images
        and the reference's targets (``{"boxes": [G, 4] in the image's own coordinates, ...}`` per image).  Train mode only.  The
        transform rescales the boxes with the images, the backbone runs with gradients, the RPN in train mode; ``backward()`` on
        the losses reaches ``rpn.head``, the FPN and the encoder.  :meth:`losses` adds the box head's two.  ``generator`` seeds the
        sampler's keys.  ``windows``: as for :meth:`losses`."""
        if not self.training:
            raise RuntimeError("LayoutDetectionModel.rpn_losses: train mode only - call .train() first")
        if targets is None:
            raise ValueError("LayoutDetectionModel.rpn_losses: targets are required")
        m = self.model
        image_list, targets = m.transform(images, targets, windows=windows)
        if windows is not None:
            targets = (targets[0], targets[2])                       # the RPN's pair of the padded triple
        batch = image_list.tensors
        feats = {k: _nhwc_f32(v) for k, v in m.backbone(batch).items()}
        _, losses = m.rpn(feats, tuple(batch.shape[-2:]), targets=targets, padded=True, generator=generator)
        return losses

    def losses(self, images: List[torch.Tensor], targets: List[Dict[str, torch.Tensor]],
               generator: Optional[torch.Generator] = None, windows=None) -> Dict[str, torch.Tensor]:
        """The reference's ``loss_dict = model(images, targets)``: ``{"loss_classifier", "loss_box_reg", "loss_objectness",
        "loss_rpn_box_reg"}`` for a list of ``[3, h, w]`` images and targets ``{"boxes": [G, 4] in the image's own coordinates,
        "labels": [G] in [1, num_classes]}``.  Train mode only.  The transform and the backbone run once; the RPN in train mode gives
        its two losses and its proposals (detached), the box head samples from them and gives the other two.  ``backward()`` on the
        sum reaches the box head, ``rpn.head``, the FPN and the encoder.  ``generator`` seeds both samplers' keys.

        ``windows`` (train-time crop, scale jitter and flip; one ``(x0, y0, cw, ch, flip)`` per image, e.g. from
        ``augment.DetectorAugment.sample``): the losses of the cropped (mirrored) pages and of the targets those still show - bit for
        bit ``losses(crops, crop_targets)`` where the padded width of the targets is the same - without copying a page and without a
        synchronisation.  None: nothing changes."""
        if not self.training:
            raise RuntimeError("LayoutDetectionModel.losses: train mode only - call .train() first")
        if targets is None:
            raise ValueError("LayoutDetectionModel.losses: targets are required")
        m = self.model
        image_list, targets = m.transform(images, targets, windows=windows)
        batch = image_list.tensors
        image_size = tuple(batch.shape[-2:])
        feats = {k: _nhwc_f32(v) for k, v in m.backbone(batch).items()}
        rpn_targets = targets if windows is None else (targets[0], targets[2])    # the RPN takes the pair, the box head the triple
        (proposals, _, count), rpn_losses = m.rpn(feats, image_size, targets=rpn_targets, padded=True, generator=generator)
        out = m.roi_heads(feats, proposals.detach(), count, image_size, targets=targets, padded=True, generator=generator)
        out.update(rpn_losses)
        return out

    def forward_padded_tta(self, images: List[torch.Tensor], tta) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """Test-time augmentation (``tta``: a ``layoutdit_amd.TestTimeAugment``): a list of ``[3, h, w]`` pages ->
        ``(boxes [B, D_out, 4], scores [B, D_out], labels int32 [B, D_out], count int32 [B])`` in the PAGES' coordinates, zero padding, no
        synchronisation.  Per view of ``tta.views(self)`` one ``ops.preprocess`` of the list at the view's size - a mirrored view through
        the whole-page window ``(0, 0, w, h, 1)``: no mirrored or resized copy, every image format the transform takes, uint8
        included - then :meth:`forward_padded`; ``ops.tta_merge`` maps every view back to its page, pools them, runs one class-wise NMS
        and, where ``tta.vote_thresh`` is set, box voting.  ``head_dtype``, ``neck_dtype`` and ``compute_dtype`` act through
        :meth:`forward_padded` as they stand, and under ``with step.ema_weights():`` the views are those of the averaged weights."""
        if self.training:
            raise RuntimeError("LayoutDetectionModel: forward_padded_tta is inference only (the four losses are losses(images, targets)) - "
                               "call .eval() first")
        from .. import ops
        t = self.model.transform
        if len(images) == 0:
            raise ValueError("empty image list")
        for img in images:
            if img.dim() != 3:
                raise ValueError(f"images is expected to be a list of 3d tensors of shape [C, H, W], got {tuple(img.shape)}")
        views = tta.views(self)
        nms_thresh, detections_per_img, vote_thresh = tta.merge_args(self)
        original = [tuple(img.shape[-2:]) for img in images]
        operands = t._operands(images)
        mirror = [(0, 0, w, h, 1) for h, w in original]
        outs = []
        for view in views:
            batch = ops.preprocess(operands, size=(view.height, view.width), mean=t.mean, std=t.std, windows=mirror if view.flip else None)
            outs.append(self.forward_padded(batch))
        return ops.tta_merge(outs, views, original, nms_thresh, detections_per_img, vote_thresh)

    def forward(self, images: List[torch.Tensor], targets=None, tta=None) -> List[Dict[str, torch.Tensor]]:
        """``tta`` (a ``layoutdit_amd.TestTimeAugment``): the detections of :meth:`forward_padded_tta` as the list of dicts - they are
        already in the pages' coordinates, so ``transform.postprocess`` is not applied to them.  ``head_dtype``, ``neck_dtype`` and
        ``compute_dtype`` need nothing, and ``with step.ema_weights():`` evaluates the averaged weights either way.  None: nothing
        changes."""
        if self.training or targets is not None:
            raise RuntimeError("LayoutDetectionModel: forward is inference only (the four losses are losses(images, targets)) - call "
                               ".eval() first and pass no targets")
        if tta is not None:
            boxes, scores, labels, count = self.forward_padded_tta(images, tta)
            return [{"boxes": boxes[i, :n], "labels": labels[i, :n].to(torch.int64), "scores": scores[i, :n]}
                    for i, n in enumerate(count.tolist())]
        m = self.model
        original = [tuple(img.shape[-2:]) for img in images]
        image_list, _ = m.transform(images)
        boxes, scores, labels, count = self.forward_padded(image_list.tensors)
        result = [{"boxes": boxes[i, :n], "labels": labels[i, :n].to(torch.int64), "scores": scores[i, :n]}
                  for i, n in enumerate(count.tolist())]
        return m.transform.postprocess(result, image_list.image_sizes, original)
