"""numpy oracle of the box head's two kernels, written from the definitions in include/ldit.h ("box head"): torchvision's LevelMapper
and roi_align(aligned=False, sampling_ratio=2) on channels-last maps (float64), the softmax / BoxCoder(10, 10, 5, 5) decode / clip /
filters in front of the NMS (float64), and a generator of boxes that stay away from every discontinuity of the definition (level
boundaries in sqrt(area), samples at -1 or at the map's far edge) apart from hand-placed exact cases."""
import math

import numpy as np

CANONICAL_SCALE, CANONICAL_LEVEL, LEVEL_EPS = 224.0, 4.0, 1e-6
BBOX_XFORM_CLIP = math.log(1000.0 / 16.0)


def infer_scales(map_sizes, image_size):
    """torchvision's scale inference: 2 ** round(log2(map / image)) per axis, both axes must agree."""
    out = []
    for h, w in map_sizes:
        sh = 2.0 ** round(math.log2(h / image_size[0]))
        sw = 2.0 ** round(math.log2(w / image_size[1]))
        assert sh == sw, (h, w, image_size)
        out.append(sh)
    return out


def level_range(scales):
    return int(-math.log2(scales[0])), int(-math.log2(scales[-1]))


def box_levels(boxes, k_min, k_max):
    """boxes [n, 4] -> level index (k - k_min) of each box, float64 on the float32 coordinates."""
    b = np.asarray(boxes, dtype=np.float32).astype(np.float64)
    s = np.sqrt((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]))
    with np.errstate(divide="ignore"):
        k = np.floor(CANONICAL_LEVEL + np.log2(s / CANONICAL_SCALE) + LEVEL_EPS)
    return (np.clip(k, k_min, k_max) - k_min).astype(np.int64)


def sample_coords(lo, hi, scale, P=7, S=2):
    """The P * S sample coordinates of one axis of one box: start + p bin + (i + 0.5) bin / S, float64."""
    start = float(lo) * scale
    extent = max(float(hi) * scale - start, 1.0)
    bin_ = extent / P
    p = np.repeat(np.arange(P), S).astype(np.float64)
    i = np.tile(np.arange(S), P).astype(np.float64)
    return start + p * bin_ + (i + 0.5) * bin_ / S


def axis_terms(v, n):
    """torchvision's bilinear_interpolate along one axis of n cells: (low index, high index, low weight, high weight), the weights
    zero for a coordinate outside [-1, n]."""
    inside = ~((v < -1.0) | (v > n))
    v = np.maximum(v, 0.0)
    lo = np.floor(v).astype(np.int64)
    edge = lo >= n - 1
    lo = np.where(edge, n - 1, lo)
    hi = np.where(edge, n - 1, lo + 1)
    v = np.where(edge, lo.astype(np.float64), v)
    whi = v - lo
    wlo = 1.0 - whi
    lo, hi = np.clip(lo, 0, n - 1), np.clip(hi, 0, n - 1)                # (only coordinates outside, whose weights are zeroed)
    return lo, hi, np.where(inside, wlo, 0.0), np.where(inside, whi, 0.0)


def roi_align_row(fmap, box, scale, P=7, S=2):
    """One box on one map [h, w, C] (float64) -> [P, P, C]."""
    h, w, _ = fmap.shape
    ylo, yhi, wylo, wyhi = axis_terms(sample_coords(box[1], box[3], scale, P, S), h)
    xlo, xhi, wxlo, wxhi = axis_terms(sample_coords(box[0], box[2], scale, P, S), w)
    rows_lo, rows_hi = fmap[ylo], fmap[yhi]                              # [P S, w, C]
    val = ((wylo[:, None] * wxlo[None, :])[:, :, None] * rows_lo[:, xlo] + (wylo[:, None] * wxhi[None, :])[:, :, None] * rows_lo[:, xhi]
           + (wyhi[:, None] * wxlo[None, :])[:, :, None] * rows_hi[:, xlo] + (wyhi[:, None] * wxhi[None, :])[:, :, None] * rows_hi[:, xhi])
    return val.reshape(P, S, P, S, -1).sum(axis=(1, 3)) / (S * S)


def roi_align_levels(maps, boxes, count, image_size, P=7, S=2, levels=None):
    """maps: list of [B, h, w, C] arrays, finest first; boxes [B, R, 4]; count [B] or None.  Returns (out [B R, P, P, C] float64 with
    zero padding rows, levels int [B, R] with -1 for padding rows).  `levels` overrides the level decision (valid rows only)."""
    maps = [np.asarray(m, dtype=np.float64) for m in maps]
    boxes = np.asarray(boxes, dtype=np.float32)
    B, R = boxes.shape[:2]
    scales = infer_scales([m.shape[1:3] for m in maps], image_size)
    k_min, k_max = level_range(scales)
    out = np.zeros((B * R, P, P, maps[0].shape[3]))
    lv = np.full((B, R), -1, dtype=np.int64)
    for b in range(B):
        n = R if count is None else int(count[b])
        lv[b, :n] = box_levels(boxes[b, :n], k_min, k_max) if levels is None else np.asarray(levels)[b, :n]
        for r in range(n):
            l = lv[b, r]
            out[b * R + r] = roi_align_row(maps[l][b], boxes[b, r].astype(np.float64), scales[l], P, S)
    return out, lv


def level_margin(boxes):
    """Relative distance of sqrt(area) from the nearest level boundary 224 * 2^j (inf for an empty box)."""
    b = np.asarray(boxes, dtype=np.float32).astype(np.float64)
    s = np.sqrt((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]))
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.log2(s / CANONICAL_SCALE)
        frac = np.abs(t - np.round(t))
    return np.where(np.isfinite(t), np.abs(2.0 ** frac - 1.0), np.inf)


def edge_margin(boxes, levels, map_sizes, scales, P=7, S=2):
    """Smallest distance of any sample of each box from the two discontinuities of its axis: -1 and the number of cells."""
    out = np.empty(len(boxes))
    for i, (bx, l) in enumerate(zip(np.asarray(boxes, dtype=np.float32).astype(np.float64), levels)):
        h, w = map_sizes[l]
        y, x = sample_coords(bx[1], bx[3], scales[l], P, S), sample_coords(bx[0], bx[2], scales[l], P, S)
        out[i] = min(np.abs(y + 1).min(), np.abs(y - h).min(), np.abs(x + 1).min(), np.abs(x - w).min())
    return out


EXACT_SQRT_AREAS = (56.0, 112.0, 224.0)


def exact_boundary_boxes(img_h, img_w):
    """Boxes whose sqrt(area) is exactly 56, 112 or 224 in float32 (those that fit the image): they belong to the UPPER level."""
    cands = [[0, 0, 56, 56], [8, 4, 72, 53], [0, 0, 112, 112], [10, 20, 122, 132], [16, 0, 144, 98], [0, 0, 224, 224]]
    out = [c for c in cands if c[2] <= img_w and c[3] <= img_h]
    for c in out:
        assert math.sqrt((c[2] - c[0]) * (c[3] - c[1])) in EXACT_SQRT_AREAS
    return np.asarray(out, dtype=np.float32)


def make_boxes(seed, R, image_size, map_sizes):
    """R boxes, all but two inside the image: the hand-placed cases first (as many as fit in R) - the exact level boundaries, the full image, one
    box touching each edge, tiny boxes, the degenerate box x1 = x2 = width on the right edge, two boxes far larger than the image (the
    only way to the two coarsest levels at these image sizes) - then random ones.  Every box but the
    exact-boundary ones is at least 1e-4 (relative, in sqrt(area)) from a level boundary, and no sample of any box lies within 1e-3
    of -1 or of the far edge of its map: both are asserted."""
    img_h, img_w = image_size
    rng = np.random.RandomState(seed)
    exact = exact_boundary_boxes(img_h, img_w)
    hand = [
        [0, 0, img_w, img_h],                                            # the full image
        [0, 30.5, 40.25, 70.75], [img_w - 50.5, 10, img_w, 61.25],       # touching the left / right edge
        [20.5, 0, 90, 33.25], [11, img_h - 40.5, 77.5, img_h],           # top / bottom
        [30.3, 40.7, 31.1, 41.2], [5.25, 60.5, 5.75, 80.0], [100.1, 7.3, 100.1, 7.3],    # tiny (extent forced to one cell), empty
        [img_w, 20, img_w, 60],                                          # degenerate on the right edge: every sample beyond the map
        [0, 0, 55.9, 55.9], [0, 0, 112.1, 112.1] if img_h >= 113 else [0, 0, 140.0, 90.0],
        [-200.5, -150, 420, 400.25], [-600, -500.5, 800.75, 700],        # larger than the image: the two coarsest levels
    ]
    fixed = np.concatenate([exact, np.asarray(hand, dtype=np.float32)])[:R]
    scales = infer_scales(map_sizes, image_size)
    k_min, k_max = level_range(scales)

    def edge_ok(b):
        return (edge_margin(b, box_levels(b, k_min, k_max), map_sizes, scales) > 1e-3).all()

    boxes = []
    while len(boxes) < R - len(fixed):
        size = np.exp(rng.uniform(math.log(2.0), math.log(min(img_h, img_w)), size=2))
        if rng.rand() < 0.4:                                             # large boxes: the levels above the finest
            size = np.exp(rng.uniform(math.log(60.0), np.log([img_w, img_h])))
        x1, y1 = rng.uniform(0, img_w - size[0]), rng.uniform(0, img_h - size[1])
        bx = np.asarray([[x1, y1, x1 + size[0], y1 + size[1]]], dtype=np.float32)
        if level_margin(bx)[0] > 1e-4 and edge_ok(bx):
            boxes.append(bx[0])
    out = np.concatenate([fixed, np.asarray(boxes, dtype=np.float32).reshape(-1, 4)]).astype(np.float32)
    d = out.astype(np.float64)
    is_exact = np.isin(np.sqrt((d[:, 2] - d[:, 0]) * (d[:, 3] - d[:, 1])), EXACT_SQRT_AREAS)
    assert (level_margin(out)[~is_exact] > 1e-4).all()
    assert edge_ok(out)
    return out, is_exact


# ---- postprocess_detections in front of the NMS ---------------------------------------------------------------------------------
def softmax64(logits):
    lg = np.asarray(logits, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        e = np.exp(lg - lg.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def postprocess(head, proposals, count, img_h, img_w, num_classes, score_thresh=0.05, min_size=1e-2, weights=(10.0, 10.0, 5.0, 5.0)):
    """One image.  head [R, >= 5 NC] (logits | deltas), proposals [R, 4], count = valid rows (or None).  float64.  Returns boxes
    [R (NC - 1), 4], scores [R (NC - 1)] with -inf for dropped candidates, labels, the plain softmax scores and the unclipped centre
    / size terms (for the error bound).  The threshold is the float32 one the device compares with; the comparison is STRICT."""
    NC = num_classes
    head = np.asarray(head, dtype=np.float64)
    R = head.shape[0]
    prob = softmax64(head[:, :NC])[:, 1:]                                                        # [R, NC - 1]
    d = head[:, NC:5 * NC].reshape(R, NC, 4)[:, 1:]                                              # [R, NC - 1, 4]
    a = np.asarray(proposals, dtype=np.float64)[:, None, :]
    w, h = a[..., 2] - a[..., 0], a[..., 3] - a[..., 1]
    cx, cy = a[..., 0] + 0.5 * w, a[..., 1] + 0.5 * h
    dx, dy = d[..., 0] / weights[0], d[..., 1] / weights[1]
    dw, dh = np.minimum(d[..., 2] / weights[2], BBOX_XFORM_CLIP), np.minimum(d[..., 3] / weights[3], BBOX_XFORM_CLIP)
    pcx, pcy = dx * w + cx, dy * h + cy
    pw, ph = np.exp(dw) * w, np.exp(dh) * h
    box = np.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph], axis=-1)
    box[..., 0::2] = np.clip(box[..., 0::2], 0.0, img_w)
    box[..., 1::2] = np.clip(box[..., 1::2], 0.0, img_h)
    thr = float(np.float32(score_thresh))
    ms = float(np.float32(min_size))
    bad = ~(prob > thr) | ~((box[..., 2] - box[..., 0]) >= ms) | ~((box[..., 3] - box[..., 1]) >= ms)
    if count is not None:
        bad[int(count):] = True
    labels = np.tile(np.arange(1, NC, dtype=np.int32), (R, 1))
    score = np.where(bad, -np.inf, prob)
    flat = lambda t: t.reshape(R * (NC - 1), *t.shape[2:])                                       # noqa: E731
    return flat(box), flat(score), flat(labels), flat(prob), tuple(flat(t) for t in (pcx, pcy, pw, ph))
