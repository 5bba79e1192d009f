"""numpy oracle of the region-proposal stage, written from the definitions in include/ldit.h ("region proposals"):
per-level top-k, BoxCoder decoding + clipping + filters (float64), greedy batched NMS (IoU in float32, in the header's order of
operations, so that keep / suppress decisions are comparable exactly), and a generator of NMS problems whose IoU arithmetic
is exact in fp32 up to the one division."""
import math

import numpy as np

NEG_INF = np.float32(-np.inf)


def topk_indices(logits, level_sizes, k):
    """logits [Ntot] -> concatenated per-level indices: descending logit, ties by ascending index, -inf last, NaN after -inf."""
    out, off = [], 0
    for n in level_sizes:
        v = np.asarray(logits[off:off + n], dtype=np.float64)
        rank = np.where(np.isnan(v), np.inf, -v)           # ascending rank: NaN behind -inf (rank +inf; stable keeps index order)
        nan_last = np.isnan(v).astype(np.int64)            # ... and strictly behind: -(-inf) is +inf too
        order = np.lexsort((np.arange(n), rank, nan_last))
        out.append(off + order[:min(k, n)])
        off += n
    return np.concatenate(out).astype(np.int32)


def decode(logits, deltas, anchors, idx, img_h, img_w, min_size, score_thresh):
    """float64 decode of the candidates idx: boxes [K, 4] (unclipped centre / size terms returned too, for the error bound),
    scores [K] with -inf for filtered candidates."""
    a = np.asarray(anchors, dtype=np.float64)[idx]
    d = np.asarray(deltas, dtype=np.float64)[idx]
    lg = np.asarray(logits, dtype=np.float64)[idx]
    w, h = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
    cx, cy = a[:, 0] + 0.5 * w, a[:, 1] + 0.5 * h
    clip = math.log(1000.0 / 16.0)
    dw, dh = np.minimum(d[:, 2], clip), np.minimum(d[:, 3], clip)
    pcx, pcy = d[:, 0] * w + cx, d[:, 1] * h + cy
    pw, ph = np.exp(dw) * w, np.exp(dh) * h
    box = np.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph], axis=1)
    box[:, 0::2] = np.clip(box[:, 0::2], 0.0, img_w)
    box[:, 1::2] = np.clip(box[:, 1::2], 0.0, img_h)
    score = 1.0 / (1.0 + np.exp(-lg))
    bad = ((box[:, 2] - box[:, 0]) < min_size) | ((box[:, 3] - box[:, 1]) < min_size) | (score < score_thresh)
    score = np.where(bad, -np.inf, score)
    return box, score, (pcx, pcy, pw, ph)


def iou_f32(a, b):
    """IoU of box a [4] with boxes b [n, 4], float32, exactly: area = (x2-x1)*(y2-y1); iw = max(min(ax2,bx2) - max(ax1,bx1), 0);
    inter = iw*ih; iou = inter / ((areaA + areaB) - inter)."""
    a = np.asarray(a, dtype=np.float32)
    b = np.asarray(b, dtype=np.float32).reshape(-1, 4)
    zero = np.float32(0)
    area_a = (a[2] - a[0]) * (a[3] - a[1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    iw = np.maximum(np.minimum(a[2], b[:, 2]) - np.maximum(a[0], b[:, 0]), zero)
    ih = np.maximum(np.minimum(a[3], b[:, 3]) - np.maximum(a[1], b[:, 1]), zero)
    inter = iw * ih
    with np.errstate(divide="ignore", invalid="ignore"):
        return (inter / ((area_a + area_b) - inter)).astype(np.float32)


def nms(boxes, scores, groups, thr, max_out):
    """One problem.  Returns (keep int32 [max_out] padded with -1, count)."""
    boxes = np.asarray(boxes, dtype=np.float32)
    scores = np.asarray(scores, dtype=np.float32)
    n = scores.shape[0]
    groups = np.zeros(n, dtype=np.int32) if groups is None else np.asarray(groups)
    valid = np.flatnonzero(~(np.isnan(scores) | (scores == NEG_INF)))
    order = valid[np.argsort(-scores[valid].astype(np.float64), kind="stable")]
    thr = np.float32(thr)
    alive = np.ones(order.shape[0], dtype=bool)
    kept = []
    for pos, i in enumerate(order):
        if not alive[pos]:
            continue
        kept.append(i)
        rest = order[pos + 1:]
        if rest.size:
            sup = (iou_f32(boxes[i], boxes[rest]) > thr) & (groups[rest] == groups[i])
            alive[pos + 1:] &= ~sup
    keep = np.full(max_out, -1, dtype=np.int32)
    count = min(len(kept), max_out)
    keep[:count] = kept[:count]
    return keep, count


def clustered_problem(seed, n, n_clusters=40, n_groups=1, invalid_frac=0.0, tie_frac=0.0):
    """Boxes snapped to a quarter-pixel grid inside [0, 224]: every coordinate is k / 4 with k <= 896, so differences, areas (<= 2^20
    in units of 1/16), intersections and unions are exact in fp32 and the ONE rounding of an IoU is its division.  Clusters of
    jittered copies (centre sigma 3, log-size sigma 0.15); scores a permutation of distinct values (optionally with ties and
    -inf entries)."""
    rng = np.random.RandomState(seed)
    c = rng.uniform(20, 204, size=(n_clusters, 2))
    s = rng.uniform(16, 80, size=(n_clusters, 2))
    which = rng.randint(0, n_clusters, size=n)
    ctr = c[which] + rng.normal(0, 3.0, size=(n, 2))
    size = s[which] * np.exp(rng.normal(0, 0.15, size=(n, 2)))
    b = np.concatenate([ctr - 0.5 * size, ctr + 0.5 * size], axis=1)
    b = np.clip(np.round(b * 4.0) / 4.0, 0.0, 224.0)
    b[:, 2:] = np.maximum(b[:, 2:], b[:, :2] + 0.25)                   # no degenerate box
    b[:, 2:] = np.minimum(b[:, 2:], 224.0)
    b[:, :2] = np.minimum(b[:, :2], b[:, 2:] - 0.25)
    scores = (rng.permutation(n).astype(np.float32) + 1.0) / np.float32(n + 1)
    if tie_frac > 0:
        m = min(max(int(n * tie_frac), 2), n)
        scores[rng.choice(n, m, replace=False)] = np.float32(0.5)
    if invalid_frac > 0:
        scores[rng.rand(n) < invalid_frac] = NEG_INF
    groups = rng.randint(0, n_groups, size=n).astype(np.int32) if n_groups > 1 else None
    return b.astype(np.float32), scores.astype(np.float32), groups


def random_problem_away_from_threshold(seed, n, thr, n_groups=1, margin=1e-6):
    """Unsnapped random float boxes; the seed is stepped until no same-group pair has a float64 IoU within `margin` of thr."""
    while True:
        rng = np.random.RandomState(seed)
        ctr = rng.uniform(10, 214, size=(n, 2))
        # a few dense neighbourhoods so that suppression happens at all
        ctr[: n // 2] = ctr[rng.randint(0, 12, size=n // 2)] + rng.normal(0, 4.0, size=(n // 2, 2))
        size = rng.uniform(12, 70, size=(n, 2))
        b = np.concatenate([ctr - 0.5 * size, ctr + 0.5 * size], axis=1).astype(np.float32)
        groups = rng.randint(0, n_groups, size=n).astype(np.int32) if n_groups > 1 else np.zeros(n, dtype=np.int32)
        scores = rng.permutation(n).astype(np.float32)
        d = b.astype(np.float64)
        area = (d[:, 2] - d[:, 0]) * (d[:, 3] - d[:, 1])
        iw = np.maximum(np.minimum(d[:, None, 2], d[None, :, 2]) - np.maximum(d[:, None, 0], d[None, :, 0]), 0)
        ih = np.maximum(np.minimum(d[:, None, 3], d[None, :, 3]) - np.maximum(d[:, None, 1], d[None, :, 1]), 0)
        inter = iw * ih
        iou = inter / (area[:, None] + area[None, :] - inter)
        near = (np.abs(iou - float(np.float32(thr))) < margin) & (groups[:, None] == groups[None, :])
        np.fill_diagonal(near, False)
        if not near.any():
            return b, scores, (groups if n_groups > 1 else None), seed
        seed += 1
