"""tests/remove_ref.py (the three NumPy lines Gallery.remove is tested against) against a naive loop that fills the holes one
at a time.  No GPU."""
import itertools

import numpy as np
import pytest

from remove_ref import relocate, remove_ref


def naive(rows, R):
    """Pop style: shrink to new_n; walk the holes upwards, each takes the lowest tail row not yet used and not removed."""
    n = len(rows)
    gone = set(int(r) for r in R)
    new_n = n - len(gone)
    out = [rows[i] for i in range(new_n)]
    tail = [t for t in range(new_n, n) if t not in gone]
    pairs = []
    for h in range(new_n):
        if h in gone:
            t = tail.pop(0)
            out[h] = rows[t]
            pairs.append((t, h))
    assert not tail
    return out, pairs


def subsets(n):
    if n <= 7:
        for k in range(n + 1):
            for c in itertools.combinations(range(n), k):
                yield list(c)
        return
    rng = np.random.default_rng(1000 + n)
    yield []                                                   # none
    yield list(range(n))                                       # all
    yield list(range(n - n // 3, n))                           # only tail rows (a contiguous tail block)
    yield [n - 1]
    yield list(range(n // 4))                                  # only head rows: every tail row moves
    yield [0]
    for k in (1, 2, n // 5, n // 2, n - 1):
        for _ in range(6):
            yield rng.permutation(n)[:k].tolist()
    yield rng.permutation(np.arange(n // 2))[:n // 8].tolist()                   # head only, scattered
    yield (n - 1 - rng.permutation(n // 3)[:n // 8]).tolist()                    # tail only, scattered


@pytest.mark.parametrize('n', [1, 2, 7, 64, 65, 300])
def test_remove_ref_equals_naive_loop(n):
    rows = np.arange(n, dtype=np.int64) * 10 + 3               # distinct values: a row is known by its value
    for R in subsets(n):
        k = len(set(R))
        out, frm, to = remove_ref(rows, R)
        want, pairs = naive(rows, R)
        new_n = n - k
        assert out.shape == (new_n,) and np.array_equal(out, np.array(want, dtype=np.int64).reshape(new_n))
        holes = [h for h in sorted(set(R)) if h < new_n]
        assert len(frm) == len(to) == len(holes) <= k
        assert [(int(f), int(t)) for f, t in zip(frm, to)] == pairs
        assert np.array_equal(to, holes) and np.all(np.diff(to) > 0) and np.all(np.diff(frm) > 0)
        assert np.all(frm >= new_n) and not np.isin(frm, R).any()
        assert np.array_equal(np.sort(out), np.sort(np.delete(rows, np.array(R, dtype=np.int64))))     # the survivors, as a multiset
        stay = np.setdiff1d(np.arange(new_n), to)
        assert np.array_equal(out[stay], rows[stay])                             # rows not named in moved_to: still at their index
        where = relocate(np.arange(n), sorted(set(R)), frm, to)
        for i in range(n):
            assert (where[i] == -1) == (i in set(R))
            if where[i] >= 0:
                assert out[where[i]] == rows[i]


def test_remove_ref_duplicates_and_order_collapse():
    rows = np.arange(20) * 7
    a = remove_ref(rows, [5, 18, 5, 2, 18, 19])
    b = remove_ref(rows, [2, 5, 18, 19])
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert a[1].tolist() == [16, 17] and a[2].tolist() == [2, 5]
