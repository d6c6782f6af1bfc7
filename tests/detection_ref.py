"""NumPy restatement of detector evaluation (include/dif.h, "detector evaluation"; csrc/deteval.hip), written the way the
rule is told: frame by frame, a frame's detections one after another by descending score, with a set of the truths already
detected.  It deliberately does not use the device's claim form (the least rank per truth), so the two can disagree.

`seen` collects what happened on the way; tests/test_detection_ref.py asserts that the cases below make all of it happen."""
import numpy as np

EPS = np.finfo(float).eps
FP, TP, DROPPED = 0, 1, 2
COCO = tuple(np.linspace(0.5, 0.95, 10))
SCAN_TILE = 1024                                 # DIF_DET_SCAN_TILE

EVENTS = ('tp', 'fp_low', 'fp_no_truth', 'fp_taken', 'fp_taken_second_best_free', 'dropped', 'dropped_again', 'iou_tie',
          'iou_at_threshold', 'score_tie_in_frame', 'score_tie_across_frames', 'nan_score', 'neg_inf_score', 'nan_box',
          'frame_without_detections', 'frame_without_truths', 'frame_without_both', 'all_ignored', 'more_than_a_block')


def overlap(a, b):
    """compute_overlap of the reference on the float32 boxes widened to float64, operation by operation; a pair with a
    coordinate that is not finite has overlap 0 (the reference: NaN)."""
    a32, b32 = np.asarray(a, np.float32).reshape(-1, 4), np.asarray(b, np.float32).reshape(-1, 4)
    a, b = a32.astype(np.float64), b32.astype(np.float64)
    ok = np.isfinite(a).all(1)[:, None] & np.isfinite(b).all(1)[None, :]
    a, b = np.where(np.isfinite(a), a, 0.0), np.where(np.isfinite(b), b, 0.0)
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    iw = np.minimum(a[:, 2:3], b[:, 2]) - np.maximum(a[:, 0:1], b[:, 0])
    ih = np.minimum(a[:, 3:4], b[:, 3]) - np.maximum(a[:, 1:2], b[:, 1])
    iw, ih = np.maximum(iw, 0.0), np.maximum(ih, 0.0)
    ua = ((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]))[:, None] + area_b - iw * ih
    ua = np.maximum(ua, EPS)
    return np.where(ok, iw * ih / ua, 0.0)


def average_precision(recall, precision):
    """compute_ap: the curve between the sentinels (0, 0) and (1, 0), the precision replaced by its running maximum from the
    right, and the steps of the recall times that envelope, summed by np.sum."""
    r = np.concatenate([[0.0], np.asarray(recall, np.float64), [1.0]])
    p = np.concatenate([[0.0], np.asarray(precision, np.float64), [0.0]])
    env = np.maximum.accumulate(p[::-1])[::-1]
    step = np.flatnonzero(r[1:] != r[:-1])
    return np.sum((r[step + 1] - r[step]) * env[step + 1])


def rank_order(scores):
    """Rows by descending score, ties to the lower row, NaN last."""
    return np.argsort(-np.asarray(scores, np.float32), kind='stable')


def match(det_boxes, det_scores, det_offsets, gt_boxes, gt_offsets, thresholds, gt_ignore=None, seen=None):
    """One batch -> (assigned [M] int64, iou [M] float64, outcome [J, M] uint8, n_truth)."""
    track, seen = seen is not None, set() if seen is None else seen
    det_boxes, gt_boxes = np.asarray(det_boxes, np.float32).reshape(-1, 4), np.asarray(gt_boxes, np.float32).reshape(-1, 4)
    det_scores = np.asarray(det_scores, np.float32)
    m, t = len(det_boxes), len(gt_boxes)
    ignore = np.zeros(t, bool) if gt_ignore is None else np.asarray(gt_ignore).astype(bool)
    assigned, iou = np.full(m, -1, np.int64), np.zeros(m, np.float64)
    outcome = np.zeros((len(thresholds), m), np.uint8)
    if t and ignore.all():
        seen.add('all_ignored')
    for f in range(len(det_offsets) - 1):
        d0, d1, g0, g1 = det_offsets[f], det_offsets[f + 1], gt_offsets[f], gt_offsets[f + 1]
        if d0 == d1 or g0 == g1:
            seen.add('frame_without_both' if d0 == d1 and g0 == g1 else 'frame_without_detections' if d0 == d1 else 'frame_without_truths')
        if d1 - d0 > 256 and g1 - g0 > 256:
            seen.add('more_than_a_block')
        if d0 == d1:
            continue
        if not np.isfinite(det_boxes[d0:d1]).all():
            seen.add('nan_box')
        s = det_scores[d0:d1]
        if np.isnan(s).any():
            seen.add('nan_score')
        if np.isneginf(s).any():
            seen.add('neg_inf_score')
        if len(np.unique(s[~np.isnan(s)])) < (~np.isnan(s)).sum():
            seen.add('score_tie_in_frame')
        ov = overlap(det_boxes[d0:d1], gt_boxes[g0:g1])
        if g1 > g0:
            best = np.argmax(ov, axis=1)
            assigned[d0:d1] = g0 + best
            iou[d0:d1] = ov[np.arange(d1 - d0), best]
            if ((ov == iou[d0:d1, None]).sum(1)[iou[d0:d1] > 0] > 1).any():
                seen.add('iou_tie')
        walk = d0 + rank_order(s)
        for j, thr in enumerate(thresholds):
            detected, dropped_on = set(), set()
            for d in walk:
                g = assigned[d]
                if g < 0:
                    seen.add('fp_no_truth')
                    continue
                if iou[d] < thr:
                    seen.add('fp_low')
                    continue
                if iou[d] == thr:
                    seen.add('iou_at_threshold')
                if ignore[g]:
                    outcome[j, d] = DROPPED
                    seen.add('dropped_again' if g in dropped_on else 'dropped')
                    dropped_on.add(g)
                elif g not in detected:
                    outcome[j, d] = TP
                    detected.add(g)
                    seen.add('tp')
                else:
                    seen.add('fp_taken')
                    free = track and [k for k in range(g0, g1) if k != g and k not in detected and not ignore[k] and ov[d - d0, k - g0] >= thr]
                    if free:
                        seen.add('fp_taken_second_best_free')
    return assigned, iou, outcome, int((~ignore).sum())


def curve(scores, outcome, n_truth):
    """All detections seen -> dict of order, tp_cum, fp_cum, recall, precision, ap."""
    scores, outcome = np.asarray(scores, np.float32), np.asarray(outcome, np.uint8)
    order = rank_order(scores)
    o = outcome[:, order]
    tp_cum, fp_cum = np.cumsum(o == TP, axis=1, dtype=np.int64), np.cumsum(o == FP, axis=1, dtype=np.int64)
    recall = tp_cum / np.float64(n_truth) if n_truth > 0 else np.zeros(o.shape, np.float64)
    precision = tp_cum / np.maximum((tp_cum + fp_cum).astype(np.float64), EPS)
    ap = np.array([average_precision(recall[j], precision[j]) for j in range(len(o))], np.float64)
    return dict(order=order.astype(np.int64), tp_cum=tp_cum, fp_cum=fp_cum, recall=recall, precision=precision, ap=ap)


def evaluate(case, thresholds, seen=None, chunks=None):
    """A case (see cases()) in one batch, or -- `chunks`: frame counts that sum to N -- batch by batch -> dict of every output.
    Without `seen` nothing is recorded (the look for a free second-best truth costs a walk over the frame's truths)."""
    n = len(case['det_offsets']) - 1
    parts, n_truth, f0 = [], 0, 0
    for c in (chunks or [n]):
        b = batch(case, f0, f0 + c)
        a, v, o, k = match(b['det_boxes'], b['det_scores'], b['det_offsets'], b['gt_boxes'], b['gt_offsets'], thresholds, b['gt_ignore'],
                           seen)
        parts.append((np.where(a >= 0, a + case['gt_offsets'][f0], a), v, o))
        n_truth += k
        f0 += c
    assert f0 == n
    out = dict(assigned=np.concatenate([p[0] for p in parts]), iou=np.concatenate([p[1] for p in parts]),
               outcome=np.concatenate([p[2] for p in parts], axis=1), n_truth=n_truth)
    s = case['det_scores']
    per_frame = [x for f in np.split(s, case['det_offsets'][1:-1]) for x in np.unique(f[~np.isnan(f)])] if seen is not None else []
    if len(set(per_frame)) < len(per_frame):     # a score that two frames carry
        seen.add('score_tie_across_frames')
    out.update(curve(s, out['outcome'], n_truth))
    return out


def batch(case, f0, f1):
    """Frames [f0, f1) of a case as a batch of their own."""
    do, go = case['det_offsets'], case['gt_offsets']
    return dict(det_boxes=case['det_boxes'][do[f0]:do[f1]], det_scores=case['det_scores'][do[f0]:do[f1]], det_offsets=do[f0:f1 + 1] - do[f0],
                gt_boxes=case['gt_boxes'][go[f0]:go[f1]], gt_offsets=go[f0:f1 + 1] - go[f0],
                gt_ignore=None if case['gt_ignore'] is None else case['gt_ignore'][go[f0]:go[f1]])


def _case(name, frames, with_ignore=False):
    """frames: a list of (detections [(x1, y1, x2, y2, score)], truths [(x1, y1, x2, y2) or (x1, y1, x2, y2, ignore)])."""
    db, ds, do, gb, gi, go = [], [], [0], [], [], [0]
    for dets, truths in frames:
        for d in dets:
            db.append(d[:4])
            ds.append(d[4])
        for g in truths:
            gb.append(g[:4])
            gi.append(bool(g[4]) if len(g) > 4 else False)
        do.append(len(db))
        go.append(len(gb))
    return dict(name=name, det_boxes=np.asarray(db, np.float32).reshape(-1, 4), det_scores=np.asarray(ds, np.float32),
                det_offsets=np.asarray(do, np.int64), gt_boxes=np.asarray(gb, np.float32).reshape(-1, 4),
                gt_offsets=np.asarray(go, np.int64), gt_ignore=np.asarray(gi, np.uint8) if with_ignore else None)


def jittered_frames(rng, n_frames, max_dets, max_truths, ignore_share=0.0, round_scores=None):
    """Seeded frames: 0 .. max_truths truths each, 0 .. max_dets detections jittered off them (or off nothing: strays)."""
    frames = []
    for _ in range(n_frames):
        nt, nd = int(rng.integers(0, max_truths + 1)), int(rng.integers(0, max_dets + 1))
        xy = rng.random((nt, 2)) * np.array([560.0, 400.0])
        wh = 12.0 + rng.random((nt, 2)) * 120.0
        truths = np.concatenate([xy, xy + wh, (rng.random((nt, 1)) < ignore_share)], axis=1)
        dets = np.zeros((nd, 5))
        for i in range(nd):
            if nt and rng.random() < 0.8:
                g = truths[int(rng.integers(0, nt))]
                side = (g[2] - g[0] + g[3] - g[1]) / 2
                dets[i, :4] = g[:4] + rng.normal(0.0, 0.12 * rng.random() * side + 1e-3, 4)
            else:
                p = rng.random(2) * np.array([560.0, 400.0])
                dets[i, :4] = np.concatenate([p, p + 12.0 + rng.random(2) * 120.0])
            dets[i, 4] = rng.random()
        if round_scores:
            dets[:, 4] = np.round(dets[:, 4] * round_scores) / round_scores
        frames.append((dets.tolist(), truths.tolist()))
    return frames


def jittered(name, rng, n_frames, max_dets, max_truths, ignore_share=0.0, round_scores=None):
    return _case(name, jittered_frames(rng, n_frames, max_dets, max_truths, ignore_share, round_scores), with_ignore=ignore_share > 0)


def crowd():
    """One frame of 300 truths and 700 detections -- more than a block of either -- between three ordinary frames, so that
    blocks of detections lie inside the frame and across its two ends."""
    rng = np.random.default_rng(31)
    side = jittered_frames(rng, 3, 40, 6, ignore_share=0.1)
    nt, nd = 300, 700
    xy = rng.random((nt, 2)) * np.array([600.0, 440.0])
    truths = np.concatenate([xy, xy + 10.0 + rng.random((nt, 2)) * 30.0, rng.random((nt, 1)) < 0.05], axis=1)
    g = truths[rng.integers(0, nt, nd)]
    dets = np.concatenate([g[:, :4] + rng.normal(0.0, 2.0, (nd, 4)), np.round(rng.random((nd, 1)) * 512) / 512], axis=1)
    return _case('crowd', side[:2] + [(dets.tolist(), truths.tolist())] + side[2:], with_ignore=True)


def sized(m):
    """Exactly m detections in frames of 0 .. 61 (scores rounded to 1/4096: ties inside and across frames)."""
    rng = np.random.default_rng(4000 + m)
    case = jittered('sized_%d' % m, rng, m // 24 + 8, 61, 5, ignore_share=0.1, round_scores=4096)
    assert len(case['det_scores']) >= m
    f = int(np.searchsorted(case['det_offsets'], m, side='left'))
    out = batch(case, 0, f)
    out['det_boxes'], out['det_scores'] = out['det_boxes'][:m], out['det_scores'][:m]
    out['det_offsets'] = np.minimum(out['det_offsets'], m)
    out['name'] = case['name']
    return out


def cases():
    nan, inf = float('nan'), float('inf')
    A, B = (0, 0, 10, 10), (4, 0, 14, 10)
    out = [
        _case('empties', [([], []), ([(0, 0, 5, 5, 0.9), (1, 1, 4, 4, 0.3)], []), ([], [(0, 0, 5, 5)]), ([(0, 0, 5, 5, 0.8)], [(0, 0, 5, 5)]),
                          ([], [])]),
        _case('no_detections', [([], [(0, 0, 5, 5)]), ([], [])]),
        _case('no_truths', [([(0, 0, 5, 5, 0.5)], []), ([(0, 0, 5, 5, 0.6), (0, 0, 5, 5, 0.7)], [])]),
        _case('nothing', [([], []), ([], [])]),
        _case('same_truth', [([(0, 0, 10, 10, 0.6), (1, 0, 11, 10, 0.9)], [A]),
                             ([(0, 0, 10, 9, 0.2), (0, 0, 10, 10, 0.7), (0, 1, 10, 10, 0.5)], [A, (50, 50, 60, 60)])]),
        # the second detection overlaps A most (0.818), A is taken, and B -- free, 0.538 >= 0.5 -- must not be tried
        _case('second_best_free', [([(0, 0, 10, 10, 0.9), (1, 0, 11, 10, 0.8)], [A, B])]),
        _case('duplicate_truths', [([(0, 0, 10, 10, 0.9), (0, 0, 10, 10, 0.8), (0, 0, 9, 10, 0.7)], [(30, 30, 40, 40), A, A])]),
        # (0, 0, 2, 1) against (0, 0, 1, 1): 1 / (2 + 1 - 1) = 0.5 exactly; (0, 0, 4, 3) against (0, 0, 3, 3): 9 / 12 = 0.75
        _case('at_threshold', [([(0, 0, 2, 1, 0.9)], [(0, 0, 1, 1)]), ([(0, 0, 4, 3, 0.4)], [(0, 0, 3, 3)])]),
        _case('scores', [([(0, 0, 10, 10, 0.5), (0, 0, 10, 9, 0.5), (20, 20, 30, 30, 0.5)], [A, (20, 20, 30, 30)]),
                         ([(0, 0, 10, 10, 0.5), (0, 0, 10, 10, nan), (4, 0, 14, 10, -inf), (4, 0, 14, 9, nan)], [A, B]),
                         ([(0, 0, 10, 10, -0.0), (0, 0, 10, 9, 0.0), (4, 0, 14, 10, inf)], [A, B])]),
        _case('bad_boxes', [([(0, 0, nan, 10, 0.9), (0, 0, 10, 10, 0.8), (0, -inf, 10, inf, 0.7)], [A]),
                            ([(0, 0, 10, 10, 0.9)], [(0, 0, inf, 10), A])]),
        # a hit on an ignored truth is dropped and takes nothing: the next one on it is dropped too, and n_truth leaves it out
        _case('ignored', [([(0, 0, 10, 10, 0.9), (0, 0, 10, 9, 0.8), (4, 0, 14, 10, 0.7), (4, 0, 14, 9, 0.6)], [A + (1,), B + (0,)]),
                          ([(0, 0, 10, 5, 0.95)], [A + (1,)])], with_ignore=True),
        _case('all_ignored', [([(0, 0, 10, 10, 0.9), (40, 40, 50, 50, 0.8)], [A + (1,)]), ([(4, 0, 14, 10, 0.7)], [B + (1,)])],
              with_ignore=True),
    ]
    out.append(crowd())
    out.append(jittered('seeded', np.random.default_rng(37), 37, 40, 12, ignore_share=0.08, round_scores=64))
    return out


def walk():
    """(case, thresholds): every case at J = 1 and at J = 10."""
    for case in cases():
        yield case, (0.5,)
        yield case, COCO
