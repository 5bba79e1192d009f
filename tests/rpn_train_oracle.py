"""numpy oracle of the RPN's training side, written from the definitions in include/ldit.h ("RPN training"): anchor matching with
torchvision's literal low-quality promotion, the key-driven balanced sampler, BoxCoder(1, 1, 1, 1).encode, and the two losses
with their gradients.  Two halves: the IoU is float32 in the kernel's order of operations (``rpn_oracle.iou_f32``), so labels,
matches and the sampler compare EXACTLY; encode and the losses are float64."""
import numpy as np

from tests import rpn_oracle as ro


def iou_matrix_f32(anchors, gt):
    """float32 [G, N]; a quotient that is not > 0 (disjoint boxes, NaN) counts as +0."""
    anchors = np.asarray(anchors, dtype=np.float32)
    gt = np.asarray(gt, dtype=np.float32).reshape(-1, 4)
    m = np.zeros((gt.shape[0], anchors.shape[0]), dtype=np.float32)
    for g in range(gt.shape[0]):
        v = ro.iou_f32(gt[g], anchors)
        m[g] = np.where(v > 0, v, np.float32(0))
    return m


def match(anchors, gt, fg_thr=0.7, bg_thr=0.3):
    """matched int32 [N]: GT index of a positive anchor, -1 negative, -2 ignored; also the IoU matrix."""
    n = np.asarray(anchors).shape[0]
    gt = np.asarray(gt, dtype=np.float32).reshape(-1, 4)
    if gt.shape[0] == 0:
        return np.full(n, -1, dtype=np.int32), np.zeros((0, n), dtype=np.float32)
    m = iou_matrix_f32(anchors, gt)
    best, arg = m.max(axis=0), m.argmax(axis=0)                       # argmax: the FIRST maximum, i.e. the lowest GT index
    out = np.where(best >= np.float32(fg_thr), arg, np.where(best < np.float32(bg_thr), -1, -2)).astype(np.int32)
    promoted = (m == m.max(axis=1, keepdims=True)).any(axis=0)        # holds SOME GT's best: gets its OWN argmax back
    out[promoted] = arg[promoted]
    return out, m


def encode(anchors, gt, matched):
    """float64 [N, 4]: BoxCoder(1, 1, 1, 1).encode of the matched GT for positive anchors, zero elsewhere."""
    a = np.asarray(anchors, dtype=np.float64)
    t = np.zeros((a.shape[0], 4))
    pos = np.flatnonzero(matched >= 0)
    if pos.size:
        g = np.asarray(gt, dtype=np.float64).reshape(-1, 4)[matched[pos]]
        a = a[pos]
        aw, ah = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
        gw, gh = g[:, 2] - g[:, 0], g[:, 3] - g[:, 1]
        t[pos] = np.stack([((g[:, 0] + 0.5 * gw) - (a[:, 0] + 0.5 * aw)) / aw, ((g[:, 1] + 0.5 * gh) - (a[:, 1] + 0.5 * ah)) / ah,
                           np.log(gw / aw), np.log(gh / ah)], axis=1)
    return t


def sample(matched, keys, batch_size=256, positive_fraction=0.5):
    """labels int32 [N] (1 / 0 / -1) and (positives, negatives) taken: the smallest (key, index) of each class."""
    matched, keys = np.asarray(matched), np.asarray(keys, dtype=np.int64) & 0x7fffffff
    labels = np.full(matched.shape[0], -1, dtype=np.int32)
    pos, neg = np.flatnonzero(matched >= 0), np.flatnonzero(matched == -1)
    take_pos = min(int(float(batch_size) * float(np.float32(positive_fraction))), pos.size)
    take_neg = min(batch_size - take_pos, neg.size)
    labels[pos[np.lexsort((pos, keys[pos]))][:take_pos]] = 1
    labels[neg[np.lexsort((neg, keys[neg]))][:take_neg]] = 0
    return labels, (take_pos, take_neg)


def targets(anchors, gt_boxes, gt_count, keys, fg_thr=0.7, bg_thr=0.3, batch_size=256, positive_fraction=0.5):
    """The batch: labels [B, N], matched [B, N], reg_targets float64 [B, N, 4], sampled [B, 2].  GT rows past the count are cut
    off before anything looks at them."""
    out = [[], [], [], []]
    for b in range(len(gt_count)):
        gt = np.asarray(gt_boxes[b])[:int(gt_count[b])]
        m, _ = match(anchors, gt, fg_thr, bg_thr)
        lab, taken = sample(m, keys[b], batch_size, positive_fraction)
        for o, v in zip(out, (lab, m, encode(anchors, gt, m), np.asarray(taken, dtype=np.int32))):
            o.append(v)
    return tuple(np.stack(o) for o in out)


def loss(logits, deltas, labels, reg_targets, beta=1.0 / 9.0):
    """float64: (loss [2], d_logits, d_deltas).  n = the anchors with label 0 or 1 over the whole batch; objectness = mean of
    max(x, 0) - x y + log1p(exp(-|x|)); box = sum over label 1 of smooth_l1(beta) / n.  n == 0: zeros."""
    x = np.asarray(logits, dtype=np.float64)
    d = np.asarray(deltas, dtype=np.float64) - np.asarray(reg_targets, dtype=np.float64)
    labels = np.asarray(labels)
    used, pos = labels >= 0, labels == 1
    n = int(used.sum())
    dl, dd = np.zeros_like(x), np.zeros_like(d)
    if n == 0:
        return np.zeros(2), dl, dd
    y = pos.astype(np.float64)
    bce = np.maximum(x, 0) - x * y + np.log1p(np.exp(-np.abs(x)))
    en = np.exp(-np.abs(x))
    sig = np.where(x >= 0, 1 / (1 + en), en / (1 + en))
    dl[used] = (sig - y)[used] / n
    ad = np.abs(d)
    quad = ad < beta
    with np.errstate(divide="ignore", invalid="ignore"):
        sl1 = np.where(quad, 0.5 * d * d / beta, ad - 0.5 * beta)
        g = np.where(quad, d / beta, np.sign(d))
    dd[pos] = g[pos] / n
    return np.asarray([bce[used].sum() / n, sl1[pos].sum() / n]), dl, dd


def pad_gt(gt_list, gmax=None, fill=np.nan):
    """list of [G_i, 4] -> (gt_boxes float32 [B, Gmax, 4] with `fill` in the rows past the count, gt_count int32 [B])."""
    gmax = max(max((len(g) for g in gt_list), default=0), 1) if gmax is None else gmax
    out = np.full((len(gt_list), gmax, 4), fill, dtype=np.float32)
    for b, g in enumerate(gt_list):
        if len(g):
            out[b, :len(g)] = g
    return out, np.asarray([len(g) for g in gt_list], dtype=np.int32)


def scene(seed, g, size=(224, 224)):
    """g GT boxes snapped to the quarter-pixel grid inside the image, width and height at least 4: with integer anchors every
    difference, area, intersection and area sum is exact in fp32, and the ONE rounding of an IoU is its division."""
    rng = np.random.RandomState(seed)
    h, w = size
    wh = np.exp(rng.uniform(np.log(8.0), np.log(0.8 * min(h, w)), size=(g, 2)))
    wh[:, 0], wh[:, 1] = np.minimum(wh[:, 0], w - 1), np.minimum(wh[:, 1], h - 1)
    x1 = rng.uniform(0, 1, size=g) * (w - wh[:, 0])
    y1 = rng.uniform(0, 1, size=g) * (h - wh[:, 1])
    b = np.stack([x1, y1, x1 + wh[:, 0], y1 + wh[:, 1]], axis=1)
    b = np.round(b * 4.0) / 4.0
    b[:, 0::2] = np.clip(b[:, 0::2], 0, w)
    b[:, 1::2] = np.clip(b[:, 1::2], 0, h)
    b[:, 2:] = np.maximum(b[:, 2:], b[:, :2] + 4.0)
    return b.astype(np.float32)
