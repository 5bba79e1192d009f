"""COCO box evaluation restated in float64 numpy: the definition the kernels of csrc/coco_eval.hip are compared with (DESIGN
section 22).  Per (image, category, area range): the greedy matching of score-ordered detections to GT boxes at ten IoU thresholds,
giving one code per detection (0 false positive, 1 true positive, 2 ignored, 3 absent); per (category, area range, maxDet): the
cumulative precision / recall curve sampled at 101 recall thresholds; then the 12 summary numbers.  Written from the published
definition of the metric; plain loops, no attempt at speed."""
import numpy as np

IOU_THRS = np.linspace(.5, .95, 10)
REC_THRS = np.linspace(0, 1, 101)
MAX_DETS = (1, 10, 100)
AREA_RNG = ((0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))
KEYS = ("mAP", "AP50", "AP75", "AP_s", "AP_m", "AP_l", "AR1", "AR10", "AR100", "AR_s", "AR_m", "AR_l")
EPS = 2.220446049250313e-16
ABSENT = 3


def iou(d, g, crowd):
    """IoU of two xyxy boxes (float64 arrays of 4) in the [x, y, w, h] form; ``crowd``: the union is the detection's area."""
    xd, yd, wd, hd = d[0], d[1], d[2] - d[0], d[3] - d[1]
    xg, yg, wg, hg = g[0], g[1], g[2] - g[0], g[3] - g[1]
    iw = min(xd + wd, xg + wg) - max(xd, xg)
    if iw <= 0:
        return 0.0
    ih = min(yd + hd, yg + hg) - max(yd, yg)
    if ih <= 0:
        return 0.0
    i = iw * ih
    u = wd * hd if crowd else wd * hd + wg * hg - i
    return i / u


def match(boxes, scores, labels, count, gt_boxes, gt_labels, gt_count, gt_crowd=None, gt_area=None, num_classes=1, margin=None, both_forms=True):
    """Padded batch in, ``(code uint8 [B, D, 4, 10], rank int32 [B, D], npig int32 [B, K, 4])`` out.  Rows at or past a count are
    never looked at.  ``margin``: assert that every IoU a decision rests on (plain and crowd form of every detection / GT pair of one
    category; ``both_forms=False``: only the form the GT box calls for) is at least that far from every threshold."""
    boxes, scores = np.asarray(boxes), np.asarray(scores)
    B, D = scores.shape
    K = int(num_classes)
    code = np.full((B, D, 4, 10), ABSENT, dtype=np.uint8)
    rank = np.full((B, D), -1, dtype=np.int32)
    npig = np.zeros((B, K, 4), dtype=np.int32)
    for b in range(B):
        nd, ng = int(count[b]), int(gt_count[b])
        dl = np.asarray(labels[b][:nd])
        gl = np.asarray(gt_labels[b][:ng])
        gb = np.asarray(gt_boxes[b][:ng], dtype=np.float64).reshape(-1, 4)
        crowd = np.zeros(ng, dtype=bool) if gt_crowd is None else np.asarray(gt_crowd[b][:ng]).astype(bool)
        area = (gb[:, 2] - gb[:, 0]) * (gb[:, 3] - gb[:, 1]) if gt_area is None else np.asarray(gt_area[b][:ng], dtype=np.float64)
        for k in range(1, K + 1):
            slots = np.nonzero(dl == k)[0]
            slots = slots[np.argsort(-np.asarray(scores[b][slots]), kind="stable")][:MAX_DETS[-1]]
            gts = np.nonzero(gl == k)[0]
            if len(slots) == 0 and len(gts) == 0:
                continue
            rank[b, slots] = np.arange(len(slots))
            db = np.asarray(boxes[b][slots], dtype=np.float64).reshape(-1, 4)
            darea = (db[:, 2] - db[:, 0]) * (db[:, 3] - db[:, 1])
            if margin is not None:
                for d in db:
                    for gi in gts:
                        for c in ((False, True) if both_forms else (bool(crowd[gi]),)):
                            g = gb[gi]
                            assert np.abs(iou(d, g, c) - IOU_THRS).min() >= margin, "an IoU sits on a threshold"
            for a, (lo, hi) in enumerate(AREA_RNG):
                ign = crowd[gts] | (area[gts] < lo) | (area[gts] > hi)
                order = np.argsort(ign, kind="stable")                       # ignored GT last
                g_idx, g_ign = gts[order], ign[order]
                npig[b, k - 1, a] = int((~ign).sum())
                for t, thr in enumerate(IOU_THRS):
                    taken = np.zeros(len(g_idx), dtype=bool)
                    for j in range(len(slots)):
                        best, m = min(thr, 1 - 1e-10), -1
                        for gi, g in enumerate(g_idx):
                            if taken[gi] and not crowd[g]:
                                continue
                            if m >= 0 and not g_ign[m] and g_ign[gi]:
                                break
                            v = iou(db[j], gb[g], crowd[g])
                            if v < best:
                                continue
                            best, m = v, gi
                        if m >= 0:
                            taken[m] = True
                            c = 2 if g_ign[m] else 1
                        else:
                            c = 2 if (darea[j] < lo or darea[j] > hi) else 0
                        code[b, slots[j], a, t] = c
    return code, rank, npig


def accumulate(code, rank, npig, scores, labels, num_classes):
    """The stored per-detection results of ``n`` images -> ``(precision [10, 101, K, 4, 3], recall [10, K, 4, 3])``."""
    code, rank, npig = np.asarray(code), np.asarray(rank), np.asarray(npig)
    scores, labels = np.asarray(scores), np.asarray(labels)
    N, D = rank.shape
    K = int(num_classes)
    precision = -np.ones((10, 101, K, 4, 3))
    recall = -np.ones((10, K, 4, 3))
    for k in range(1, K + 1):
        for a in range(4):
            total = int(npig[:, k - 1, a].sum())
            if total == 0:
                continue
            for mi, M in enumerate(MAX_DETS):
                img, slot = np.nonzero((rank >= 0) & (rank < M) & (labels == k))
                # (score descending, image ascending, rank ascending): lexsort's last key is the primary one
                order = np.lexsort((rank[img, slot], img, -scores[img, slot].astype(np.float64)))
                c = code[img[order], slot[order], a, :]                      # [n, 10]
                for t in range(10):
                    tp = np.cumsum(c[:, t] == 1).astype(np.float64)
                    fp = np.cumsum(c[:, t] == 0).astype(np.float64)
                    rc = tp / total
                    pr = tp / (tp + fp + EPS)
                    recall[t, k - 1, a, mi] = rc[-1] if len(rc) else 0.0
                    pr = pr.tolist()
                    for i in range(len(pr) - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    idx = np.searchsorted(rc, REC_THRS, side="left")
                    precision[t, :, k - 1, a, mi] = [pr[i] if i < len(pr) else 0.0 for i in idx]
    return precision, recall


def _mean(x):
    x = x[x > -1]
    return float(np.mean(x)) if x.size else -1.0


def stats(precision, recall):
    """The 12 numbers, in ``KEYS`` order."""
    p = lambda a, t=slice(None): _mean(precision[t, :, :, a, 2])             # noqa: E731
    r = lambda a, m: _mean(recall[:, :, a, m])                               # noqa: E731
    return np.asarray([p(0), p(0, 0), p(0, 5), p(1), p(2), p(3), r(0, 0), r(0, 1), r(0, 2), r(1, 2), r(2, 2), r(3, 2)])


def evaluate(boxes, scores, labels, count, gt_boxes, gt_labels, gt_count, gt_crowd=None, gt_area=None, num_classes=1, margin=None, both_forms=True):
    """Everything at once: a dict with ``code``, ``rank``, ``npig``, ``precision``, ``recall`` and ``stats``."""
    code, rank, npig = match(boxes, scores, labels, count, gt_boxes, gt_labels, gt_count, gt_crowd, gt_area, num_classes, margin, both_forms)
    lab = np.where(rank >= 0, np.asarray(labels), 0)
    precision, recall = accumulate(code, rank, npig, np.asarray(scores), lab, num_classes)
    return {"code": code, "rank": rank, "npig": npig, "precision": precision, "recall": recall, "stats": stats(precision, recall)}


def pad_lists(outputs, targets, D=None, G=None):
    """The reference's lists (``{boxes, labels, scores}`` per image; targets ``{boxes, labels[, iscrowd][, area]}``) as the padded
    arrays of :func:`match`, rows past the counts NaN / -7."""
    B = len(outputs)
    D = D or max(1, max(len(o["scores"]) for o in outputs))
    G = G or max(1, max(len(t["labels"]) for t in targets))
    boxes, scores = np.full((B, D, 4), np.nan, dtype=np.float32), np.full((B, D), np.nan, dtype=np.float32)
    labels, count = np.full((B, D), -7, dtype=np.int32), np.zeros(B, dtype=np.int32)
    gtb, gtl = np.full((B, G, 4), np.nan, dtype=np.float32), np.full((B, G), -7, dtype=np.int32)
    crowd, area, gtc = np.zeros((B, G), dtype=np.uint8), np.full((B, G), np.nan, dtype=np.float32), np.zeros(B, dtype=np.int32)
    for b, (o, t) in enumerate(zip(outputs, targets)):
        n, g = len(o["scores"]), len(t["labels"])
        count[b], gtc[b] = n, g
        boxes[b, :n], scores[b, :n], labels[b, :n] = np.asarray(o["boxes"]).reshape(-1, 4), o["scores"], o["labels"]
        gb = np.asarray(t["boxes"], dtype=np.float32).reshape(-1, 4)
        gtb[b, :g], gtl[b, :g] = gb, t["labels"]
        if "iscrowd" in t:
            crowd[b, :g] = t["iscrowd"]
        area[b, :g] = t["area"] if "area" in t else (gb[:, 2] - gb[:, 0]) * (gb[:, 3] - gb[:, 1])
    return boxes, scores, labels, count, gtb, gtl, gtc, crowd, area


def scene(seed, nd, ng, D, G, K, tie_images=(0,), stray_labels=True):
    """A padded random batch for the GPU tests: image b has ``nd[b]`` detections and ``ng[b]`` GT boxes.  About 70 % of the detections
    are jittered copies of a GT box of the image (with its label), the rest random boxes; 15 % of the GT are crowds; the area field is
    0.6 - 1 x the box's area; box sizes span the three area ranges.  The scores of ``tie_images`` are quantised to eighths (ties);
    ``stray_labels`` puts a few labels 0 and K + 1 among the detections.  Rows at or past a count hold NaN and garbage labels."""
    rng = np.random.RandomState(seed)
    B = len(nd)
    boxes, scores = np.full((B, D, 4), np.nan, dtype=np.float32), np.full((B, D), np.nan, dtype=np.float32)
    labels = rng.randint(-5, K + 5, size=(B, D)).astype(np.int32)
    gtb, gtl = np.full((B, G, 4), np.nan, dtype=np.float32), rng.randint(-5, K + 5, size=(B, G)).astype(np.int32)
    crowd, area = rng.randint(0, 2, size=(B, G)).astype(np.uint8), np.full((B, G), np.nan, dtype=np.float32)

    def rand_boxes(n):
        side = np.exp(rng.uniform(np.log(6.0), np.log(260.0), size=(n, 2)))
        xy = rng.uniform(0, 640, size=(n, 2))
        return np.concatenate([xy, xy + side], axis=1)

    for b in range(B):
        n, g = int(nd[b]), int(ng[b])
        gb = rand_boxes(g)
        gtb[b, :g], gtl[b, :g] = gb, rng.randint(1, K + 1, size=g)
        crowd[b, :g] = rng.uniform(size=g) < 0.15
        gb32 = gtb[b, :g].astype(np.float64)
        area[b, :g] = (gb32[:, 2] - gb32[:, 0]) * (gb32[:, 3] - gb32[:, 1]) * rng.uniform(0.6, 1.0, size=g)
        db, dl = rand_boxes(n), rng.randint(1, K + 1, size=n)
        if g:
            for i in range(n):
                if rng.uniform() < 0.7:
                    j = rng.randint(g)
                    wh = gb[j, 2:] - gb[j, :2]
                    db[i] = gb[j] + rng.normal(0, 0.12, size=4) * np.concatenate([wh, wh])
                    db[i, 2:] = np.maximum(db[i, 2:], db[i, :2] + 1.0)
                    dl[i] = gtl[b, j]
        if stray_labels and n:
            dl[rng.uniform(size=n) < 0.08] = 0
            dl[rng.uniform(size=n) < 0.08] = K + 1
        s = rng.uniform(0.05, 1.0, size=n)
        if b in tie_images:
            s = np.ceil(s * 8) / 8
        boxes[b, :n], scores[b, :n], labels[b, :n] = db, s, dl
    return (boxes, scores, labels, np.asarray(nd, dtype=np.int32), gtb, gtl, np.asarray(ng, dtype=np.int32), crowd, area)


def anchor_cases():
    """The five hand-derived single-image cases (tests/test_coco_eval_cpu.py derives their expectations): name -> (outputs, targets,
    K) in the list form of :func:`pad_lists`.  Every IoU in them (0, .01, .43, 2/3, .77, 1) is off the ten thresholds."""
    f, A = np.float32, [0, 0, 100, 100]

    def out(*dets, label=1):
        return [{"boxes": np.asarray([d[1] for d in dets], dtype=f), "scores": np.asarray([d[0] for d in dets], dtype=f),
                 "labels": np.full(len(dets), label, dtype=np.int64)}]

    def tgt(boxes, labels=None, **kw):
        t = {"boxes": np.asarray(boxes, dtype=f), "labels": np.ones(len(boxes), dtype=np.int64) if labels is None else np.asarray(labels)}
        t.update({k: np.asarray(v) for k, v in kw.items()})
        return [t]

    return {
        "three_dets_two_gt": (out((.9, A), (.8, [500, 500, 600, 600]), (.7, [200, 200, 300, 300])), tgt([A, [200, 200, 300, 300]]), 1),
        "one_det_one_gt": (out((.9, [20, 0, 120, 100])), tgt([A]), 1),
        "empty_cells": (out((.9, [0, 0, 50, 50]), label=2), tgt([[0, 0, 50, 50]], area=[2500.0]), 2),
        "tie": (out((.9, [20, 0, 120, 100]), (.8, A)), tgt([A, [40, 0, 140, 100]]), 1),
        "ignore_crowd_range": (out((.9, A), (.8, A), (.7, [300, 300, 310, 310])),
                               tgt([A, [0, 0, 100, 77], [300, 300, 400, 400]], iscrowd=[1, 0, 0], area=[10000.0, 7700.0, 10000.0]), 1),
    }
