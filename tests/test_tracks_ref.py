"""tests/tracks_ref.py states the tracking rule: checked here against an independent brute-force statement, on its
invariants, on chunked walks, and on the coverage conditions of the generated cases tests/test_tracks_gpu.py walks.  (No
GPU.)  The last test ties the feature's layers to each other: header, library, binding table, method."""
import os
import re

import numpy as np
import pytest

import tracks_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def brute_force(offsets, boxes, emb, metric, tolerance, min_iou, max_gap, kmax):
    """The rule again, sharing nothing with tracks_ref.link but iou32 and np_distance: at every frame the tail set is
    recomputed from `prev` alone, and each link is the exhaustive minimum over all pairs still free."""
    n, m = len(offsets) - 1, int(offsets[-1])
    frame = np.repeat(np.arange(n), np.diff(offsets))
    posn = np.arange(m) - offsets[frame]
    prev = np.full(m, -1, np.int64)
    dist = np.full(m, np.nan, np.float32)
    for f in range(n):
        while True:
            best = None
            for j in np.nonzero((frame == f) & (posn < kmax) & (prev < 0))[0]:
                for i in np.nonzero((frame < f) & (frame >= f - max_gap) & (posn < kmax))[0]:
                    if (prev == i).any():
                        continue
                    if not R.iou32(boxes[i], boxes[j]) >= np.float32(min_iou):
                        continue
                    dd = R.np_distance(emb[j][None], emb[i][None], metric)[0]
                    if not dd <= np.float32(tolerance):
                        continue
                    if best is None or (dd, i, j) < best:
                        best = (dd, i, j)
            if best is None:
                break
            prev[best[2]], dist[best[2]] = best[1], best[0]
    labels, age = np.arange(m), np.ones(m, np.int64)
    for r in range(m):
        if prev[r] >= 0:
            labels[r], age[r] = labels[prev[r]], age[prev[r]] + 1
    return prev, dist, labels, age


def _small(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 7))
    people = int(rng.integers(1, 5))
    off, boxes, emb, _ = R.sequence(seed, n, people, 8, canvas=(120, 90), speed=9.0, box=40.0, noise=0.3, miss=0.25,
                                    false_rate=1.0, blank=tuple(rng.integers(0, 7, 2)) if seed % 3 == 0 else ())
    if seed % 4 == 0 and len(boxes) > 2:                    # exact copies: ties that (i, j) must decide
        k = int(rng.integers(1, len(boxes)))
        emb[k], boxes[k] = emb[k - 1], boxes[k - 1]
        emb[0], boxes[0] = emb[len(boxes) - 1], boxes[len(boxes) - 1]
    return off, boxes, emb, int(rng.integers(1, 4)), int(rng.integers(1, 4)), int(rng.integers(0, 2))


def test_reference_equals_the_brute_force_statement():
    links = starts = ties = 0
    for seed in range(120):
        off, boxes, emb, max_gap, kmax, metric = _small(seed)
        tol = (1.2, 0.35)[metric]
        prev, dist, labels, age, n_new, clipped, _ = R.link(off, boxes, R.dist_of(emb, metric), tol, 0.2, max_gap, kmax)
        bp, bd, bl, ba = brute_force(off, boxes, emb, metric, tol, 0.2, max_gap, kmax)
        assert np.array_equal(prev, bp) and np.array_equal(_bits(dist), _bits(bd)), seed
        assert np.array_equal(labels, bl) and np.array_equal(age, ba), seed
        assert n_new == int((bp < 0).sum())
        assert clipped == int(np.maximum(np.diff(off) - kmax, 0).sum())
        links += int((prev >= 0).sum())
        starts += n_new
        d = dist[prev >= 0]
        ties += len(d) - len(np.unique(d))
    assert links > 100 and starts > 100 and ties > 0, (links, starts, ties)


def _invariants(off, prev, dist, labels, age, max_gap, kmax, row_base=0):
    m = int(off[-1])
    frame = np.repeat(np.arange(len(off) - 1), np.diff(off))
    posn = np.arange(m) - off[frame]
    for r in range(m):
        if prev[r] < 0:
            assert labels[r] == row_base + r and age[r] == 1 and np.isnan(dist[r])
        else:
            i = prev[r] - row_base
            assert 1 <= frame[r] - frame[i] <= max_gap and posn[i] < kmax and posn[r] < kmax
            assert labels[r] == labels[i] and age[r] == age[i] + 1 and not np.isnan(dist[r])
    linked = prev[prev >= 0]
    assert len(np.unique(linked)) == len(linked)            # a face has one successor at most
    for lab in np.unique(labels):                           # a track: one face per frame, starting at the face it is named after
        rows = np.nonzero(labels == lab)[0]
        assert len(np.unique(frame[rows])) == len(rows) and rows[0] == lab - row_base
        assert np.array_equal(age[rows], np.arange(1, len(rows) + 1))


@pytest.mark.parametrize('name', sorted(R.CASES))
@pytest.mark.parametrize('metric', [0, 1])
@pytest.mark.parametrize('max_gap', [1, 2, 8])
def test_invariants_and_coverage_of_the_generated_cases(name, metric, max_gap):
    """The events a tracker's tests must meet happen in every generated case the GPU tests walk: a link across a gap > 1
    (where max_gap admits one), a pair the IoU alone rejects, a pair the tolerance alone rejects, two faces that want one
    tail -- the loser starts a track -- and a track that ends because its gap ran out (an open tail max_gap frames old
    that the frame does not continue)."""
    (off, boxes, emb, who), tols, min_iou, kmax = R.case(name)
    ev = R.new_events()
    prev, dist, labels, age, n_new, clipped, _ = R.link(off, boxes, R.dist_of(emb, metric), tols[metric], min_iou, max_gap, kmax, events=ev)
    _invariants(off, prev, dist, labels, age, max_gap, kmax)
    assert n_new == len(np.unique(labels)) and clipped == 0
    need = {'iou_only', 'tol_only', 'conflict'}
    if max_gap > 1:
        need.add('gap_link')
    assert len(off) - 1 > max_gap
    need.add('gap_out')
    assert all(ev[k] > 0 for k in need), ev
    # the tracker is of use: most faces of a real person carry the label of a track of that person
    real = who >= 0
    assert (who[labels[real]] == who[real]).mean() > 0.9
    if name == 'crowd':                                     # the same faces clipped to 16 positions
        out = R.link(off, boxes, R.dist_of(emb, metric), tols[metric], min_iou, max_gap, 16)
        assert out[5] == int(np.maximum(np.diff(off) - 16, 0).sum()) > 0
        _invariants(off, *out[:4], max_gap, 16)


ALL_EVENTS = ('gap_link', 'iou_only', 'tol_only', 'conflict', 'gap_out')


@pytest.mark.parametrize('metric', [0, 1])
@pytest.mark.parametrize('d', sorted(R.DIM_SEEDS))
def test_coverage_of_the_embedding_size_cases(d, metric):
    """The six-frame case of every embedding size class, at the parameters the GPU test walks it with: all five events."""
    off, boxes, emb = R.dim_case(d)
    tols, min_iou, max_gap, kmax = R.DIM_PARAMS
    ev = R.new_events()
    out = R.link(off, boxes, R.dist_of(emb, metric), tols[metric], min_iou, max_gap, kmax, events=ev)
    _invariants(off, *out[:4], max_gap, kmax)
    assert emb.shape[1] == d and np.diff(off).max() <= kmax and out[5] == 0
    assert all(ev[k] > 0 for k in ALL_EVENTS), ev


@pytest.mark.parametrize('kmax', [4, 64])
@pytest.mark.parametrize('metric', [0, 1])
def test_coverage_of_the_twelve_frames(metric, kmax):
    """The sequence the chunked GPU walks split, at their parameters (kmax None there is 64 here): all five events, with
    faces clipped at kmax 4."""
    off, boxes, emb = R.twelve()
    tols, min_iou, max_gap = R.TWELVE_PARAMS
    ev = R.new_events()
    out = R.link(off, boxes, R.dist_of(emb, metric), tols[metric], min_iou, max_gap, kmax, events=ev)
    _invariants(off, *out[:4], max_gap, kmax)
    assert all(ev[k] > 0 for k in ALL_EVENTS), ev
    assert (out[5] > 0) == (kmax == 4)


@pytest.mark.parametrize('metric', [0, 1])
def test_coverage_of_the_case_at_the_caps(metric):
    """max_gap 32 with 64 positions: all five events, links across 32 and 31 frames, tails and faces at position 63."""
    (off, boxes, emb), tols, min_iou, max_gap, kmax = R.cap_case()
    ev = R.new_events()
    out = R.link(off, boxes, R.dist_of(emb, metric), tols[metric], min_iou, max_gap, kmax, events=ev)
    _invariants(off, *out[:4], max_gap, kmax)
    assert all(ev[k] > 0 for k in ALL_EVENTS), ev
    prev = out[0]
    frame = np.repeat(np.arange(len(off) - 1), np.diff(off))
    posn = np.arange(off[-1]) - off[frame]
    gaps = (frame - frame[np.maximum(prev, 0)])[prev >= 0]
    assert np.nonzero(np.diff(off))[0].tolist() == [0, 1, 32, 33, 34, 35] and np.diff(off).max() == 64 and out[5] == 0
    assert (gaps == 32).sum() > 5 and (gaps == 31).sum() > 5 and (gaps == 1).sum() > 50
    assert posn[prev[prev >= 0]].max() == 63 and posn[prev >= 0].max() == 63


@pytest.mark.parametrize('metric', [0, 1])
def test_long_gaps_case_tells_frames_from_non_empty_frames(metric):
    """'long_gaps' holds faces in frames 0, 4, 14, 22, 23: the gaps are 4, 10, 8 and 1 frames, so at max_gap 8 the first and
    third link and the second must not -- though no NON-EMPTY frame lies between any two of them, and a max_gap of 16 does
    link it: a tracker that counted non-empty frames would get this case wrong."""
    (off, boxes, emb), tols, min_iou, kmax = R.shape_case('long_gaps')
    assert np.nonzero(np.diff(off))[0].tolist() == [0, 4, 14, 22, 23]
    frame = np.repeat(np.arange(24), np.diff(off))
    prev = R.link(off, boxes, R.dist_of(emb, metric), tols[metric], min_iou, 8, kmax)[0]
    assert (prev[frame == 4] >= 0).any() and (prev[frame == 14] == -1).all() and (prev[frame == 22] >= 0).any()
    assert (R.link(off, boxes, R.dist_of(emb, metric), tols[metric], min_iou, 16, kmax)[0][frame == 14] >= 0).any()
    for name in ('sparse_first', 'sparse_last'):
        counts = np.diff(R.shape_case(name)[0][0])
        assert len(counts) == 5 and counts.max() <= 3 and (counts == 0).sum() == 3


def test_chunked_calls_equal_the_whole_at_every_split():
    off, boxes, emb = R.twelve()                             # the sequence the GPU tests split, at their parameters
    fn = R.dist_of(emb, 1)
    whole = R.link(off, boxes, fn, 0.3, 0.2, 3, 4)
    assert (whole[0] >= 0).sum() > 10
    frame = np.repeat(np.arange(12), np.diff(off))
    assert ((frame - frame[np.maximum(whole[0], 0)])[whole[0] >= 0] > 1).any()      # a link across the gap
    cuts = [[0, s, 12] for s in range(0, 13)] + [list(range(13)), [0, 3, 3, 7, 12], [0, 4, 6, 12]]
    for c in cuts:
        got = R.walk_chunks(c, off, boxes, fn, 0.3, 0.2, 3, 4)
        for k in (0, 2, 3):
            assert np.array_equal(got[k], whole[k]), (c, k)
        assert np.array_equal(_bits(got[1]), _bits(whole[1])) and got[4:6] == whole[4:6], c
        assert got[6]['row_base'] == whole[6]['row_base'] == len(boxes)


def test_iou_in_float32():
    assert R.iou32((0, 0, 2, 2), (0, 0, 2, 1)) == np.float32(0.5)
    assert R.iou32((2, 2, 0, 0), (0, 0, 2, 1)) == np.float32(0.5)        # corners in either order
    assert R.iou32((0, 0, 0, 2), (0, 0, 2, 2)) == 0 and R.iou32((0, 0, 1, 1), (2, 2, 3, 3)) == 0
    assert R.iou32((0, 0, np.inf, np.inf), (0, 0, 2, 2)) == 0               # 4 / inf
    assert np.isnan(R.iou32((np.inf, 0, np.inf, 2), (0, 0, 2, 2)))       # an area of (inf - inf) * 2
    assert R.iou32((np.nan, 0, 2, 2), (0, 0, 2, 2)) == 0                 # fmin / fmax drop the NaN: a box without height
    a, b = (0.1, 0.2, 40.3, 41.7), (3.3, 1.9, 44.1, 40.2)
    assert R.iou32(a, b).dtype == np.float32 and abs(float(R.iou32(a, b)) - 37 * 38.3 / (40.2 * 41.5 + 40.8 * 38.3 - 37 * 38.3)) < 1e-6


def test_header_library_binding_table_and_method_carry_the_tracker():
    """Fails on a tree without the feature."""
    from deep_insight_face import _native
    from deep_insight_face.detector.faces import FrameFaces
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'dif.h')).read(), flags=re.S)
    for name, k in {'dif_tracks_link': 27, 'dif_tracks_state_size': 3, 'dif_tracks_workspace_size': 4}.items():
        decl = re.search(r'\b(?:int|int64_t) %s\s*\(([^;]*)\);' % name, header, flags=re.S)
        assert decl and decl.group(1).count(',') + 1 == k, name
        assert hasattr(_native.lib, name), name
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) == k, name
    assert callable(getattr(FrameFaces, 'tracks', None))
    assert _native.lib.dif_version() == 110


def test_arguments_are_checked_before_a_device_is_needed():
    import torch
    from deep_insight_face import _native as N
    from deep_insight_face.detector.faces import FrameFaces
    z = torch.zeros((0,))
    ff = FrameFaces(torch.zeros((3,), dtype=torch.int64), z.long(), torch.zeros((0, 4)), z, None, torch.zeros((0, 8, 8, 3), dtype=torch.uint8))
    with pytest.raises(ValueError):
        ff.tracks(0.3)                                       # no embeddings
    ff = ff._replace(emb=torch.zeros((0, 32)))
    for bad in (dict(max_gap=0), dict(max_gap=33), dict(max_faces_per_frame=65), dict(max_faces_per_frame=0)):
        with pytest.raises(ValueError):
            ff.tracks(0.3, **bad)
    with pytest.raises(RuntimeError):
        ff.tracks(0.3, distance_metric=2)
    t = ff.tracks(0.3, max_gap=3)                            # M = 0: nothing is launched, the state moves on by two frames
    assert t.labels.shape == (0,) and t.state.pad == 2 and t.state.row_base == 0 and int(t.n_new) == 0
    assert ff.tracks(0.3, max_gap=3, state=t.state).state.pad == 3
    assert N.lib.dif_tracks_state_size(0, 4, 32) == -1 and N.lib.dif_tracks_state_size(2, 65, 32) == -1
    assert N.lib.dif_tracks_state_size(2, 3, 5) == 6 * (24 + 16 + 20 + 4) + 8
    assert N.lib.dif_tracks_workspace_size(-1, 1, 1, 0) == -1
    assert N.lib.dif_tracks_link(None, None, None, 0, 0, 32, 0.3, 0.3, 1, 1, 1, 0, None, 0, 0, None, None, None, None, None, None,
                                 None, 0, None, 0, 0, None) != 0
    assert 'null pointer' in N.last_error()
