"""numpy restatement of the test-time-augmentation merge (``layoutdit_amd/csrc/tta_merge.hip`` + the NMS of ``proposals.hip``):
float32 for unmirror, scale and IoU in the kernels' operation order, float64 for the vote, a greedy class-wise NMS under the NMS
kernel's total order (descending score, ascending pool index, invalid entries last and never candidates), and the smallest
``|IoU - thresh|`` over every pair a threshold decided - the input condition under which exact comparison means something.

numpy evaluates every float32 operation with one rounding and never contracts, which is what the kernels are built to do.
"""
import numpy as np

F32 = np.float32
NEG_INF = F32(-np.inf)


def ratios(view_w, view_h, page_hw):
    """``(rw, rh)`` for one page ``(h, w)``: double quotients rounded to float32 once (``resize_boxes``)."""
    oh, ow = page_hw
    return F32(float(ow) / float(view_w)), F32(float(oh) / float(view_h))


def unmirror(boxes, view_w):
    """``(W - x2, y1, W - x1, y2)`` in float32."""
    b = np.asarray(boxes, dtype=F32)
    W = F32(view_w)
    out = b.copy()
    out[..., 0] = W - b[..., 2]
    out[..., 2] = W - b[..., 0]
    return out


def pool(views, view_specs, page_sizes):
    """``views``: V tuples ``(boxes [B, D, 4], scores [B, D], labels [B, D], count [B])``; ``view_specs``: V ``(W, H, flip)``;
    ``page_sizes``: B ``(h, w)``.  Returns ``(pool_boxes [B, V*D, 4] f32, pool_scores [B, V*D] f32, pool_labels [B, V*D] i32)``.  The
    rows at or beyond a count are never read."""
    V = len(views)
    B, D = np.asarray(views[0][1]).shape
    pb = np.zeros((B, V * D, 4), dtype=F32)
    ps = np.full((B, V * D), NEG_INF, dtype=F32)
    pl = np.zeros((B, V * D), dtype=np.int32)
    for v, ((boxes, scores, labels, count), (W, H, flip)) in enumerate(zip(views, view_specs)):
        boxes, scores, labels = np.asarray(boxes, dtype=F32), np.asarray(scores, dtype=F32), np.asarray(labels)
        for b in range(B):
            n = int(min(max(int(count[b]), 0), D))
            if n == 0:
                continue
            bx = boxes[b, :n]
            if flip:
                bx = unmirror(bx, W)
            rw, rh = ratios(W, H, page_sizes[b])
            pb[b, v * D:v * D + n] = bx * np.array([rw, rh, rw, rh], dtype=F32)
            ps[b, v * D:v * D + n] = scores[b, :n]
            pl[b, v * D:v * D + n] = labels[b, :n]
    return pb, ps, pl


def iou_f32(a, b):
    """IoU of box ``a`` [4] with boxes ``b`` [n, 4] in float32, in the order of ``iou_exceeds``: area = (x2-x1)*(y2-y1); iw =
    max(min(ax2,bx2) - max(ax1,bx1), 0); inter = iw*ih; inter / ((area_a + area_b) - inter)."""
    a = np.asarray(a, dtype=F32)
    b = np.asarray(b, dtype=F32).reshape(-1, 4)
    zero = F32(0)
    area_a = (a[2] - a[0]) * (a[3] - a[1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    iw = np.maximum(np.minimum(a[2], b[:, 2]) - np.maximum(a[0], b[:, 0]), zero)
    ih = np.maximum(np.minimum(a[3], b[:, 3]) - np.maximum(a[1], b[:, 1]), zero)
    inter = iw * ih
    with np.errstate(divide="ignore", invalid="ignore"):
        return (inter / ((area_a + area_b) - inter)).astype(F32)


def _margin(iou, thr, margins):
    """Record the smallest finite ``|IoU - thr|`` of the decisions just taken (float64 of the float32 quotient)."""
    d = np.abs(iou.astype(np.float64) - float(F32(thr)))
    d = d[np.isfinite(d)]
    if d.size:
        margins.append(float(d.min()))


def nms(boxes, scores, labels, thr, max_out, margins=None):
    """One image.  Greedy class-wise NMS: candidates are the entries whose score is neither ``-inf`` nor NaN, in descending score,
    ties by ascending index; a kept entry suppresses every later one of its label whose IoU with it is ``> thr``.  Returns ``(keep
    int32 [max_out] padded with -1, count)``; the walk stops at ``max_out`` kept entries."""
    boxes, scores, labels = np.asarray(boxes, dtype=F32), np.asarray(scores, dtype=F32), np.asarray(labels)
    valid = np.flatnonzero(~(np.isnan(scores) | (scores == NEG_INF)))
    order = valid[np.argsort(-scores[valid].astype(np.float64), kind="stable")]
    alive = np.ones(order.shape[0], dtype=bool)
    kept = []
    for pos, i in enumerate(order):
        if not alive[pos]:
            continue
        kept.append(int(i))
        if len(kept) == max_out:
            break
        rest = order[pos + 1:]
        same = (labels[rest] == labels[i]) & alive[pos + 1:]
        if same.any():
            iou = iou_f32(boxes[i], boxes[rest[same]])
            if margins is not None:
                _margin(iou, thr, margins)
            sup = np.zeros(rest.shape[0], dtype=bool)
            sup[same] = iou > F32(thr)
            alive[pos + 1:] &= ~sup
    keep = np.full(max_out, -1, dtype=np.int32)
    keep[:len(kept)] = kept
    return keep, len(kept)


def vote(boxes, scores, labels, i, thr, margins=None):
    """The voted box of pool entry ``i`` of one image: float64 ``sum(s_j b_j) / sum(s_j)`` over the entries with ``i``'s label, a score
    ``> -inf`` and a float32 IoU ``>= thr`` with ``i`` (``i`` itself always).  Returns float64 [4]."""
    boxes, scores, labels = np.asarray(boxes, dtype=F32), np.asarray(scores, dtype=F32), np.asarray(labels)
    with np.errstate(invalid="ignore"):
        cand = np.flatnonzero((labels == labels[i]) & (scores > NEG_INF))
    cand = cand[cand != i]
    member = np.zeros(cand.shape[0], dtype=bool)
    if cand.size:
        iou = iou_f32(boxes[i], boxes[cand])
        if margins is not None:
            _margin(iou, thr, margins)
        member = iou >= F32(thr)
    idx = np.sort(np.concatenate([cand[member], [i]])).astype(np.int64)
    s = scores[idx].astype(np.float64)
    return (s[:, None] * boxes[idx].astype(np.float64)).sum(axis=0) / s.sum()


def merge(views, view_specs, page_sizes, nms_thresh=0.5, detections_per_img=100, vote_thresh=None):
    """The whole merge.  Returns ``(boxes, scores f32 [B, D_out], labels i32 [B, D_out], count i32 [B], margin)``.  ``boxes`` [B, D_out,
    4] is float32 (the kept entries' own bits) without voting and FLOAT64 (unrounded) with it; ``margin`` is the smallest ``|IoU -
    thresh|`` over every pair the NMS threshold or the voting threshold decided (``inf`` when none was)."""
    pb, ps, pl = pool(views, view_specs, page_sizes)
    B, Dout = pb.shape[0], int(detections_per_img)
    boxes = np.zeros((B, Dout, 4), dtype=F32 if vote_thresh is None else np.float64)
    scores, labels = np.zeros((B, Dout), dtype=F32), np.zeros((B, Dout), dtype=np.int32)
    count = np.zeros((B,), dtype=np.int32)
    margins = []
    for b in range(B):
        keep, n = nms(pb[b], ps[b], pl[b], nms_thresh, Dout, margins)
        count[b] = n
        for k in range(n):
            i = int(keep[k])
            scores[b, k], labels[b, k] = ps[b, i], pl[b, i]
            boxes[b, k] = pb[b, i] if vote_thresh is None else vote(pb[b], ps[b], pl[b], i, vote_thresh, margins)
    return boxes, scores, labels, count, (min(margins) if margins else float("inf"))


def brute_force(views, view_specs, page_sizes, nms_thresh, detections_per_img, vote_thresh):
    """The definition stated again in float64 and without any of the above: per-entry Python loops, no sorting routine shared.  Agrees
    with :func:`merge` on inputs whose margin is large against float32 rounding.  Returns ``(boxes f64, scores, labels, count)``."""
    V = len(views)
    B, D = np.asarray(views[0][1]).shape
    Dout = int(detections_per_img)
    out_b, out_s = np.zeros((B, Dout, 4)), np.zeros((B, Dout))
    out_l, out_n = np.zeros((B, Dout), dtype=np.int64), np.zeros((B,), dtype=np.int64)

    def iou(p, q):
        iw = max(min(p[2], q[2]) - max(p[0], q[0]), 0.0)
        ih = max(min(p[3], q[3]) - max(p[1], q[1]), 0.0)
        uni = (p[2] - p[0]) * (p[3] - p[1]) + (q[2] - q[0]) * (q[3] - q[1]) - iw * ih
        return iw * ih / uni if uni != 0 else float("nan")

    for b in range(B):
        oh, ow = page_sizes[b]
        entries = []                                             # (pool index, box, score, label)
        for v in range(V):
            bx, sc, lb, cn = views[v]
            W, H, flip = view_specs[v]
            for d in range(min(max(int(cn[b]), 0), D)):
                x1, y1, x2, y2 = (float(t) for t in bx[b][d])
                if flip:
                    x1, x2 = W - x2, W - x1
                rw, rh = ow / W, oh / H
                entries.append((v * D + d, (x1 * rw, y1 * rh, x2 * rw, y2 * rh), float(sc[b][d]), int(lb[b][d])))
        entries = [e for e in entries if e[2] == e[2] and e[2] != float("-inf")]
        remaining = sorted(entries, key=lambda e: (-e[2], e[0]))
        kept = []
        while remaining and len(kept) < Dout:
            top = remaining.pop(0)
            kept.append(top)
            remaining = [e for e in remaining if not (e[3] == top[3] and iou(top[1], e[1]) > nms_thresh)]
        out_n[b] = len(kept)
        for k, top in enumerate(kept):
            out_s[b, k], out_l[b, k] = top[2], top[3]
            if vote_thresh is None:
                out_b[b, k] = top[1]
                continue
            members = [e for e in entries if e[3] == top[3] and (e[0] == top[0] or iou(top[1], e[1]) >= vote_thresh)]
            sw = sum(e[2] for e in members)
            out_b[b, k] = [sum(e[2] * e[1][c] for e in members) / sw for c in range(4)]
    return out_b, out_s, out_l, out_n


def relabel_near_ties(views, view_specs, page_sizes, thresholds, margin, first_label=1000):
    """Inputs with a margin: every same-label pair of valid pool entries of an image whose float32 IoU lies within ``margin`` of one of
    ``thresholds`` loses its higher-indexed member to a label of its own (``first_label``, ``first_label + 1``, ...), so that no pair
    any threshold could decide is left near it - whichever pairs a walk then visits.  One pass suffices: an entry alone in its class
    is in no pair.  Returns new views (copies) and the number of entries relabelled."""
    pb, ps, pl = pool(views, view_specs, page_sizes)
    B, N = ps.shape
    D = N // len(views)
    views = [tuple(np.array(t, copy=True) for t in view) for view in views]
    nxt = first_label
    for b in range(B):
        valid = np.flatnonzero(ps[b] > NEG_INF)
        x = pb[b, valid]
        area = (x[:, 2] - x[:, 0]) * (x[:, 3] - x[:, 1])
        iw = np.maximum(np.minimum(x[:, None, 2], x[None, :, 2]) - np.maximum(x[:, None, 0], x[None, :, 0]), F32(0))
        ih = np.maximum(np.minimum(x[:, None, 3], x[None, :, 3]) - np.maximum(x[:, None, 1], x[None, :, 1]), F32(0))
        inter = iw * ih
        with np.errstate(divide="ignore", invalid="ignore"):
            iou = (inter / ((area[:, None] + area[None, :]) - inter)).astype(np.float64)
        near = np.zeros(iou.shape, dtype=bool)
        for t in thresholds:
            near |= np.abs(iou - float(F32(t))) < margin
        near &= pl[b, valid][:, None] == pl[b, valid][None, :]
        near = np.triu(near, 1)                                  # (i, j), i < j: j goes - unless i went before it
        gone = np.zeros(valid.shape[0], dtype=bool)
        for j in np.flatnonzero(near.any(axis=0)):
            if (near[:, j] & ~gone).any():
                gone[j] = True
                v, d = divmod(int(valid[j]), D)
                views[v][2][b, d] = nxt
                nxt += 1
    return views, nxt - first_label


def random_views(seed, B=3, K=3, V=2, D=20, sizes=((224, 224), (160, 192)), pages=None, n_objects=6, jitter=1.5, empty_views=(),
                 poison=False):
    """Synthetic views of ``n_objects`` objects per page: every view sees a random subset of the objects, each a few times, with the
    page box carried into the view's coordinates (mirrored where the view is), jittered, and a random score in (0.05, 1).  Counts are
    ragged; a view listed in ``empty_views`` has count 0 everywhere.  ``poison``: the rows at or beyond a count hold NaN boxes, huge
    scores and labels instead of zeros.  Returns ``(views, view_specs, pages)`` as numpy arrays / lists."""
    rng = np.random.RandomState(seed)
    pages = list(pages) if pages is not None else [(int(rng.randint(120, 400)), int(rng.randint(120, 400))) for _ in range(B)]
    specs = [(sizes[v % len(sizes)][0], sizes[v % len(sizes)][1], int(v >= (V + 1) // 2)) for v in range(V)]
    objects = []
    for (oh, ow) in pages:
        c = rng.uniform(0.15, 0.85, size=(n_objects, 2)) * [ow, oh]
        s = rng.uniform(0.08, 0.3, size=(n_objects, 2)) * [ow, oh]
        objects.append((np.concatenate([c - s / 2, c + s / 2], axis=1), rng.randint(1, K + 1, size=n_objects)))
    views = []
    for v, (W, H, flip) in enumerate(specs):
        boxes = np.zeros((B, D, 4), dtype=F32)
        scores, labels = np.zeros((B, D), dtype=F32), np.zeros((B, D), dtype=np.int32)
        count = np.zeros((B,), dtype=np.int32)
        for b, (oh, ow) in enumerate(pages):
            n = 0 if v in empty_views else int(rng.randint(max(D // 2, 1), D + 1))
            count[b] = n
            obj, lab = objects[b]
            which = rng.randint(0, n_objects, size=n)
            bx = obj[which] * [W / ow, H / oh, W / ow, H / oh] + rng.normal(0, jitter, size=(n, 4))
            bx = np.clip(bx, 0, [W, H, W, H])
            bx[:, 2:] = np.maximum(bx[:, 2:], bx[:, :2] + 1.0)
            if flip:
                bx = np.stack([W - bx[:, 2], bx[:, 1], W - bx[:, 0], bx[:, 3]], axis=1)
            boxes[b, :n], labels[b, :n] = bx.astype(F32), lab[which]
            scores[b, :n] = np.sort(rng.uniform(0.05, 1.0, size=n).astype(F32))[::-1]
            if poison:
                boxes[b, n:], scores[b, n:], labels[b, n:] = np.nan, F32(3e38), 0x7FFFFFFF
        views.append((boxes, scores, labels, count))
    return views, specs, pages
