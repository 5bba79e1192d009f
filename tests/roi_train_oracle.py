"""numpy oracle of the box head's training side, written from the definitions in include/ldit.h ("box head training"): proposal
matching and sampling (the GT boxes join the candidates; IoU float32 in the kernel's order of operations, so labels, matches, the
sampler and the row order compare EXACTLY; the encoding is float64), fastrcnn_loss with its gradient (float64), and the transposed
multi-scale RoIAlign (float64) together with s(e), the number of (row, sample) pairs whose bilinear footprint includes a map
element - the unit of the backward's error bound."""
import numpy as np

from tests import roi_oracle as ro
from tests import rpn_train_oracle as rto

WEIGHTS = (10.0, 10.0, 5.0, 5.0)


def targets_image(proposals, count, gt, gt_labels, keys, fg_thr=0.5, bg_thr=0.5, batch_size=512, positive_fraction=0.25, weights=WEIGHTS):
    """One image.  proposals [R, 4] (rows past `count` ignored), gt [G, 4], gt_labels [G], keys [R + Gmax] (key R + g belongs to GT g).
    Returns rois float32 [S, 4], labels [S], reg_targets float64 [S, 4], matched [S], (positives, negatives)."""
    proposals = np.asarray(proposals, dtype=np.float32)
    gt = np.asarray(gt, dtype=np.float32).reshape(-1, 4)
    R, G, S = proposals.shape[0], gt.shape[0], int(batch_size)
    cand = np.concatenate([proposals[:count], gt])
    index = np.concatenate([np.arange(count), R + np.arange(G)]).astype(np.int64)
    key = (np.asarray(keys, dtype=np.int64) & 0x7fffffff)[index]
    if G:
        iou = rto.iou_matrix_f32(cand, gt)                                  # [G, n]
        best, arg = iou.max(axis=0), iou.argmax(axis=0)                     # the FIRST maximum: the lowest GT index
        pos = np.flatnonzero(best >= np.float32(fg_thr))
        neg = np.flatnonzero(best < np.float32(bg_thr))
    else:
        arg = np.zeros(len(cand), dtype=np.int64)
        pos, neg = np.zeros(0, dtype=np.int64), np.arange(len(cand))
    take_pos = min(int(float(S) * float(np.float32(positive_fraction))), pos.size)
    take_neg = min(S - take_pos, neg.size)
    pos = pos[np.lexsort((index[pos], key[pos]))][:take_pos]
    neg = neg[np.lexsort((index[neg], key[neg]))][:take_neg]
    rois, labels = np.zeros((S, 4), dtype=np.float32), np.full(S, -1, dtype=np.int32)
    reg, matched = np.zeros((S, 4)), np.full(S, -1, dtype=np.int32)
    rois[:take_pos], rois[take_pos:take_pos + take_neg] = cand[pos], cand[neg]
    labels[:take_pos], labels[take_pos:take_pos + take_neg] = np.asarray(gt_labels)[arg[pos]] if take_pos else 0, 0
    matched[:take_pos] = arg[pos]
    if take_pos:
        a, g = cand[pos].astype(np.float64), gt[arg[pos]].astype(np.float64)
        aw, ah = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
        gw, gh = g[:, 2] - g[:, 0], g[:, 3] - g[:, 1]
        reg[:take_pos] = np.stack([weights[0] * ((g[:, 0] + 0.5 * gw) - (a[:, 0] + 0.5 * aw)) / aw,
                                   weights[1] * ((g[:, 1] + 0.5 * gh) - (a[:, 1] + 0.5 * ah)) / ah,
                                   weights[2] * np.log(gw / aw), weights[3] * np.log(gh / ah)], axis=1)
    return rois, labels, reg, matched, (take_pos, take_neg)


def targets(proposals, count, gt_boxes, gt_labels, gt_count, keys, fg_thr=0.5, bg_thr=0.5, batch_size=512, positive_fraction=0.25,
            weights=WEIGHTS):
    """The batch: rois [B, S, 4], labels [B, S], reg_targets float64 [B, S, 4], matched [B, S], sampled [B, 2].  Rows past the counts
    are cut off before anything looks at them."""
    out = [[], [], [], [], []]
    for b in range(len(gt_count)):
        g = int(gt_count[b])
        res = targets_image(proposals[b], int(count[b]), np.asarray(gt_boxes[b])[:g], np.asarray(gt_labels[b])[:g], keys[b], fg_thr, bg_thr,
                            batch_size, positive_fraction, weights)
        for o, v in zip(out, res[:4] + (np.asarray(res[4], dtype=np.int32),)):
            o.append(v)
    return tuple(np.stack(o) for o in out)


def loss(head, labels, reg_targets, num_classes, beta=1.0 / 9.0):
    """float64: (loss [2], d_head [M, ld]).  n = the rows with label >= 0; classifier = sum of logsumexp(logits) - logit[label] over
    them / n; box = sum over label >= 1 of smooth_l1(beta) of the row's own class / n.  d_head holds d loss[0] in columns [0, NC) and
    d loss[1] in [NC, 5 NC).  n == 0: zeros."""
    head = np.asarray(head, dtype=np.float64)
    labels = np.asarray(labels).reshape(-1)
    t = np.asarray(reg_targets, dtype=np.float64).reshape(-1, 4)
    NC, M = int(num_classes), head.shape[0]
    d = np.zeros_like(head)
    used, pos = np.flatnonzero(labels >= 0), np.flatnonzero(labels >= 1)
    n = used.size
    if n == 0:
        return np.zeros(2), d
    lg = head[used, :NC]
    mx = lg.max(axis=1, keepdims=True)
    e = np.exp(lg - mx)
    lse = mx[:, 0] + np.log(e.sum(axis=1))
    cls = (lse - lg[np.arange(n), labels[used]]).sum() / n
    p = e / e.sum(axis=1, keepdims=True)
    p[np.arange(n), labels[used]] -= 1.0
    d[used, :NC] = p / n
    box = 0.0
    if pos.size:
        cols = NC + 4 * labels[pos][:, None] + np.arange(4)[None, :]
        diff = head[pos[:, None], cols] - t[pos]
        ad = np.abs(diff)
        quad = ad < beta
        with np.errstate(divide="ignore", invalid="ignore"):
            box = np.where(quad, 0.5 * diff * diff / beta, ad - 0.5 * beta).sum() / n
            d[pos[:, None], cols] = np.where(quad, diff / beta, np.sign(diff)) / n
    assert M == labels.shape[0]
    return np.asarray([cls, box]), d


def axis_matrices(lo, hi, scale, n, P=7, S=2, dtype=np.float64):
    """One axis of one box on n cells: A [P, n] = the weight bin p puts on each cell (summed over its S samples) and F [P S, n] = 1
    where a sample's footprint (its low and high cell, if the sample is inside) includes the cell.  `dtype` float32 evaluates the
    coordinates and weights in float32 in the kernel's order of operations (the measurement of the gate)."""
    if dtype == np.float32:
        f = np.float32
        start = f(lo) * f(scale)
        extent = np.maximum(f(hi) * f(scale) - start, f(1))
        bin_ = extent / f(P)
        p, i = np.repeat(np.arange(P), S).astype(f), np.tile(np.arange(S), P).astype(f)
        v = (start + p * bin_ + (i + f(0.5)) * bin_ / f(S)).astype(f)
    else:
        v = ro.sample_coords(lo, hi, scale, P, S)
    inside = ~((v < -1.0) | (v > n))
    vc = np.maximum(v, dtype(0))
    l = np.floor(vc).astype(np.int64)
    edge = l >= n - 1
    l = np.where(edge, n - 1, l)
    h = np.where(edge, n - 1, l + 1)
    vc = np.where(edge, l.astype(dtype), vc).astype(dtype)
    whi = (vc - l.astype(dtype)).astype(dtype)
    wlo = (dtype(1) - whi).astype(dtype)
    W, F = np.zeros((P * S, n), dtype=dtype), np.zeros((P * S, n), dtype=np.int64)
    for s in np.flatnonzero(inside):
        W[s, l[s]] += wlo[s]
        W[s, h[s]] += whi[s]
        F[s, l[s]] = F[s, h[s]] = 1
    return W.reshape(P, S, n).sum(axis=1, dtype=dtype), F


def roi_align_levels_bwd(d_out, boxes, count, levels, map_sizes, image_size, P=7, S=2, dtype=np.float64):
    """The transposed forward.  d_out [B R, P, P, C], boxes [B, R, 4], count [B] or None, levels [B, R] (as the forward decided them),
    map_sizes: (h, w) per level.  Returns (grads: list of [B, h, w, C], s: list of int [B, h, w]) - s counts the (row, sample) pairs
    that touch the element."""
    boxes = np.asarray(boxes, dtype=np.float32)
    B, R = boxes.shape[:2]
    d_out = np.asarray(d_out, dtype=dtype).reshape(B, R, P, P, -1)
    scales = ro.infer_scales(map_sizes, image_size)
    grads = [np.zeros((B, h, w, d_out.shape[-1]), dtype=dtype) for h, w in map_sizes]
    touch = [np.zeros((B, h, w), dtype=np.int64) for h, w in map_sizes]
    for b in range(B):
        n = R if count is None else int(count[b])
        for r in range(n):
            l = int(levels[b][r])
            if not 0 <= l < len(map_sizes):
                continue
            h, w = map_sizes[l]
            bx = boxes[b, r] if dtype == np.float32 else boxes[b, r].astype(np.float64)
            Ay, Fy = axis_matrices(bx[1], bx[3], scales[l], h, P, S, dtype)
            Ax, Fx = axis_matrices(bx[0], bx[2], scales[l], w, P, S, dtype)
            ys, xs = np.flatnonzero(Fy.any(axis=0)), np.flatnonzero(Fx.any(axis=0))
            if ys.size == 0 or xs.size == 0:
                continue
            g = np.einsum("py,qx,pqc->yxc", Ay[:, ys], Ax[:, xs], d_out[b, r]).astype(dtype) * dtype(1.0 / (S * S))
            grads[l][b][np.ix_(ys, xs)] += g
            touch[l][b][np.ix_(ys, xs)] += np.outer(Fy[:, ys].sum(axis=0), Fx[:, xs].sum(axis=0))
    return grads, touch
