"""numpy float32 restatement of ``ldit_augment_targets_f32`` (include/ldit.h, "train-time augmentation"), one rounding
per operation: every intermediate is a ``np.float32`` array, so each ``+ - *`` and each comparison is the kernel's.  Shared by
tests/test_augment_cpu.py and tests/test_gpu_augment.py.  Also the host-side helpers the tests cut crops with."""
import numpy as np

F = np.float32


def ratios(window, size):
    """``(rw, rh)``: the double quotients ``out_w / cw`` and ``out_h / ch`` rounded once to fp32 (what ``resize_boxes`` forms)."""
    out_h, out_w = size
    return F(float(out_w) / float(window[2])), F(float(out_h) / float(window[3]))


def kept_rows(boxes, window, size, min_visibility=0.3, min_size=1.0):
    """Boxes ``[G, 4]`` fp32 of one image (valid rows only) -> ``(keep bool [G], b fp32 [G, 4])``: the decision and the box in the batch's
    coordinates for every row, in the kernel's order of operations."""
    b = np.ascontiguousarray(boxes, dtype=F).reshape(-1, 4)
    x0, y0, cw, ch, flip = (int(v) for v in window)
    X0, Y0, X1, Y1, CW = F(x0), F(y0), F(x0 + cw), F(y0 + ch), F(cw)
    rw, rh = ratios(window, size)
    mv, ms = F(min_visibility), F(min_size)
    x1, y1, x2, y2 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    with np.errstate(invalid="ignore", over="ignore"):
        ax1, ax2 = np.minimum(np.maximum(x1, X0), X1), np.minimum(np.maximum(x2, X0), X1)
        ay1, ay2 = np.minimum(np.maximum(y1, Y0), Y1), np.minimum(np.maximum(y2, Y0), Y1)
        iw, ih = ax2 - ax1, ay2 - ay1
        keep = (iw > 0) & (ih > 0) & (iw * ih >= mv * ((x2 - x1) * (y2 - y1)))
        lx1, lx2 = ax1 - X0, ax2 - X0
        if flip:
            lx1, lx2 = CW - lx2, CW - lx1
        ly1, ly2 = ay1 - Y0, ay2 - Y0
        out = np.stack([lx1 * rw, ly1 * rh, lx2 * rw, ly2 * rh], axis=1).astype(F)
        keep &= ((out[:, 2] - out[:, 0]) >= ms) & ((out[:, 3] - out[:, 1]) >= ms)
    assert out.dtype == F and iw.dtype == F
    return keep, out


def augment_targets(gt_boxes, gt_labels, gt_count, windows, size, min_visibility=0.3, min_size=1.0):
    """Padded ``gt_boxes [B, Gmax, 4]``, ``gt_labels [B, Gmax]`` (or None), ``gt_count [B]`` -> ``(out_boxes, out_labels, out_count)`` of
    the same shapes: kept rows in their original order, zeros behind them.  Rows at or beyond the count are never read."""
    gt_boxes = np.asarray(gt_boxes, dtype=F)
    B, Gmax = gt_boxes.shape[:2]
    out_boxes = np.zeros((B, Gmax, 4), dtype=F)
    out_labels = np.zeros((B, Gmax), dtype=np.int32)
    out_count = np.zeros((B,), dtype=np.int32)
    for i in range(B):
        G = min(max(int(gt_count[i]), 0), Gmax)
        keep, out = kept_rows(gt_boxes[i, :G], windows[i], size, min_visibility, min_size)
        n = int(keep.sum())
        out_boxes[i, :n] = out[keep]
        if gt_labels is not None:
            out_labels[i, :n] = np.asarray(gt_labels[i][:G], dtype=np.int32)[keep]
        out_count[i] = n
    return out_boxes, out_labels, out_count


def crop_boxes(boxes, window, size, min_visibility=0.3, min_size=1.0):
    """The boxes of one image in the coordinates of its crop, BEFORE the scaling to the batch: ``(keep [G], [G, 4] fp32)`` with the
    decisions of :func:`kept_rows` - what a user would hand ``losses(crops, crop_targets)``; scaling them with ``resize_boxes`` is
    the kernel's last multiplication."""
    keep, _ = kept_rows(boxes, window, size, min_visibility, min_size)
    b = np.ascontiguousarray(boxes, dtype=F).reshape(-1, 4)
    x0, y0, cw, ch, flip = (int(v) for v in window)
    X0, Y0, X1, Y1, CW = F(x0), F(y0), F(x0 + cw), F(y0 + ch), F(cw)
    lx1 = np.minimum(np.maximum(b[:, 0], X0), X1) - X0
    lx2 = np.minimum(np.maximum(b[:, 2], X0), X1) - X0
    if flip:
        lx1, lx2 = CW - lx2, CW - lx1
    ly1 = np.minimum(np.maximum(b[:, 1], Y0), Y1) - Y0
    ly2 = np.minimum(np.maximum(b[:, 3], Y0), Y1) - Y0
    return keep, np.stack([lx1, ly1, lx2, ly2], axis=1).astype(F)


def crop_image(img, window):
    """``img[..., y0:y0+ch, x0:x0+cw]``, mirrored where flip is set: a numpy array or a torch tensor ``[C, h, w]``; the caller makes
    the copy contiguous."""
    x0, y0, cw, ch, flip = (int(v) for v in window)
    c = img[..., y0:y0 + ch, x0:x0 + cw]
    if flip:
        c = c[..., ::-1] if isinstance(c, np.ndarray) else c.flip(-1)
    return c
