"""Gallery.remove / dif_gallery_remove: swap-remove of k enrolled rows in O(k) on the device.  After every
removal the gallery answers `match` (index, distance bits, key bits), `within` and `rank` on both metrics exactly as a fresh
Gallery.set of tests/remove_ref.py's result, in every form the rows are held in (f32 rows and norms, the one-term bf16 copy
row-major and in fragment order, the two-term split copy), with special rows among the removed and the moved, and the
relocation it reports is the reference's."""
import ctypes
import os

import numpy as np
import pytest
import torch

import golden_inputs as gi
from remove_ref import relocate, remove_ref

pytestmark = pytest.mark.gpu


def bits(a):
    return a.view(torch.int32) if torch.is_tensor(a) else np.ascontiguousarray(a).view(np.uint32)


def equal(a, b):
    return torch.equal(a, b) if torch.is_tensor(a) else np.array_equal(a, b)


def answers(g, probes, mates):
    """Everything a gallery answers: per metric match (idx, dist, key), within(0.3, 16) and rank(mates)."""
    out = []
    for metric in (0, 1):
        i, d, k = g.match(probes, metric, return_key=True)
        c, wi, wd = g.within(probes, 0.3, metric, max_hits=16)
        r, md = g.rank(probes, mates, metric)
        out.append((i, bits(d), bits(k), c, wi, bits(wd), r, bits(md)))
    return out


def assert_same(a, b, tag):
    names = ('match idx', 'match dist', 'match key', 'within count', 'within idx', 'within dist', 'rank', 'mate dist')
    for metric in (0, 1):
        for name, x, y in zip(names, a[metric], b[metric]):
            assert equal(x, y), (tag, metric, name)


def fresh_answers(rows, probes, mates, flt, index_base=0):
    from deep_insight_face import oneshot
    fresh = oneshot.Gallery(emd_size=rows.shape[1])
    fresh.set_option('filter', flt)
    fresh.set(rows, index_base)
    out = answers(fresh, probes, mates)
    fresh.close()
    return out


def remove_and_check(g, cur, R, base=0, arg=None):
    """g.remove(R) (global indices) against remove_ref on `cur` -> (the rows that remain, moved_from, moved_to: local)."""
    out, frm, to = remove_ref(cur, np.asarray(R, dtype=np.int64) - base)
    n = len(g)
    mf, mt = g.remove(R if arg is None else arg)
    if torch.is_tensor(mf):
        assert mf.is_cuda and mt.is_cuda and mf.dtype == torch.int64 and mt.dtype == torch.int64
        mf, mt = mf.cpu().numpy(), mt.cpu().numpy()
    assert mf.dtype == np.int64 and np.array_equal(mf, frm + base) and np.array_equal(mt, to + base)
    assert len(g) == out.shape[0] == n - len(np.unique(R))
    return out, frm, to


@pytest.mark.parametrize('flt', [2, 1, 0])
def test_remove_equals_fresh_set(cuda, flt):
    from deep_insight_face import oneshot
    rng = np.random.default_rng(700 + flt)
    base = gi.gallery(6000, seed=93)
    probes, pick = gi.probes_from(base[:5000], 96, seed=94)
    g = oneshot.Gallery(emd_size=512)
    g.set_option('filter', flt)
    g.set(base[:5000])
    state = {'cur': base[:5000].copy(), 'src': pick.copy(), 'moved': 0, 'removed': 0}

    def step(R, tag, arg=None):
        R = np.asarray(R, dtype=np.int64)
        src0, old = state['src'], state['cur']
        cur, frm, to = remove_and_check(g, state['cur'], R, arg=arg)
        src = relocate(src0, np.unique(R), frm, to)
        state.update(cur=cur, src=src)
        assert g.capacity == 5000, tag
        got = answers(g, probes, src)
        assert_same(got, fresh_answers(cur, probes, src, flt), tag)
        idx = got[1][0]
        live = src >= 0
        assert np.array_equal(idx[live], src[live]), tag       # a probe finds its source row where it is now
        went = (src0 >= 0) & ~live
        for j in np.flatnonzero(went):                          # a probe whose source row was removed does not get that row back
            assert idx[j] < len(g) and not np.array_equal(cur[idx[j]], old[src0[j]]), tag
        state['moved'] += int((live & (src != src0)).sum())
        state['removed'] += int(went.sum())
        return frm, to

    frm, to = step([0], 'row 0 alone')
    assert frm.tolist() == [4999] and to.tolist() == [0]
    frm, _ = step([len(g) - 1], 'the last row alone')
    assert len(frm) == 0
    last = int(state['src'].max())                             # the tail block ends behind a probe's source row ...
    assert 4900 < last < len(g) - 1
    frm, _ = step(np.arange(last + 1, len(g)), 'a contiguous tail block')
    assert len(frm) == 0 and len(g) == last + 1
    n = len(g)                                                  # ... so that row is the last one and moves here: 37 head rows
    src = state['src']
    head = np.concatenate([np.sort(src[(src >= 0) & (src < 1000)])[:3], [1, 2]])
    rest = np.setdiff1d(rng.permutation(n - 37)[:60], head)[:37 - len(head)]
    R = np.concatenate([head, rest])
    assert len(np.unique(R)) == 37 and R.max() < n - 37
    frm, to = step(R, '37 head rows, every tail row moves')
    assert np.array_equal(frm, np.arange(n - 37, n))
    assert state['src'][src == last] == R.max()                 # the last survivor fills the last hole
    n = len(g)
    fixed = np.array([n - 1, n - 5, n - 300])
    R = np.concatenate([np.setdiff1d(rng.permutation(n)[:400], fixed, assume_unique=True)[:330], fixed])
    assert len(np.unique(R)) == 333
    frm, _ = step(R, '333 mixed rows', arg=torch.from_numpy(R.astype(np.int32)).to(cuda))
    assert 0 < len(frm) < 333
    n = len(g)
    step([7, 8, 31, 32, 63, 64, 65, n - 3, n - 2, n - 1], 'rows at the 8-, 32- and 64-row boundaries')
    # unsorted, with duplicates == the sorted distinct list (on a twin)
    n = len(g)
    R = np.concatenate([rng.permutation(n)[:50], [n - 2, 15, 16]])
    twin = oneshot.Gallery(emd_size=512)
    twin.set_option('filter', flt)
    twin.set(state['cur'])
    tf, tt = twin.remove(np.unique(R))
    messy = np.concatenate([R[::-1], R[:20], R[-3:]])
    frm, to = step(messy, 'unsorted input with duplicates')
    assert np.array_equal(tf, frm) and np.array_equal(tt, to)
    assert_same(answers(twin, probes, state['src']), answers(g, probes, state['src']), 'twin')
    twin.close()
    # remove, append, remove again: the capacity is retained, nothing reallocates
    n = len(g)
    step(np.concatenate([rng.permutation(n)[:70], np.arange(n - 9, n - 2)]), 'before the append')
    g.update(base[5000:5300])
    state['cur'] = np.concatenate([state['cur'], base[5000:5300]])
    assert g.capacity == 5000 and len(g) == state['cur'].shape[0]
    n = len(g)
    step(np.concatenate([rng.permutation(n)[:70], np.arange(n - 150, n - 120)]), 'after the append')
    assert state['moved'] > 0 and state['removed'] >= 5
    g.close()


def probes_at(rows_now, targets, gen, extra):
    """Noisy copies of the rows `targets` (the ones a removal moved, and their neighbours) and of `extra` random rows."""
    n, D = rows_now.shape
    t = torch.as_tensor(np.clip(np.asarray(targets, dtype=np.int64), 0, n - 1), device=rows_now.device)
    pick = torch.unique(torch.cat([t, torch.randperm(n, device=rows_now.device, generator=gen)[:extra]]))
    p = rows_now[pick] + 0.05 * torch.randn((pick.shape[0], D), device=rows_now.device, generator=gen)
    return torch.nn.functional.normalize(p, dim=1), pick


def tail_patterns(n, rng, step):
    """The removal patterns of test_remove_equals_fresh_set's last three steps."""
    if step == 0:
        return np.array([7, 8, 31, 32, 63, 64, 65, n - 3, n - 2, n - 1])
    if step == 1:
        R = np.concatenate([rng.permutation(n)[:50], [n - 2, 15, 16]])
        return np.concatenate([R[::-1], R[:20], R[-3:]])
    return np.concatenate([rng.permutation(n)[:70], np.arange(n - 150, n - 120)])


@pytest.mark.parametrize('D', [128, 512, 192])
def test_remove_fragment_and_split_layouts(cuda, D):
    """One gallery per form of the filter's copy -- fragment order ('filter' 2, 'frag' 2; D = 192 stays row-major), row-major
    (2, 0), the two-term split copy ('filter' 1) -- and one on the f32 filter take the same removals; the copy that was moved
    (the stats say it is still valid, so the next match runs on it) answers like the f32 filter, and that like a fresh set.
    The probes aim at the rows that moved."""
    from deep_insight_face import oneshot
    gen = torch.Generator(device='cuda').manual_seed(D)
    rng = np.random.default_rng(D)
    G = 5000
    rows = torch.nn.functional.normalize(torch.randn((G + 700, D), device='cuda', generator=gen), dim=1)
    forms = {'g1': (2, 2), 'b1': (2, 0), 'split': (1, 1), 'f32': (0, 1)}
    gal = {}
    for name, (flt, frag) in forms.items():
        gal[name] = oneshot.Gallery(emd_size=D)
        gal[name].set_option('filter', flt)
        gal[name].set_option('frag', frag)
        gal[name].set(rows[:G])
        gal[name].reserve(6000)
        gal[name].update(rows[G:])
    rows_now = rows.clone()

    def valid_copies(tag):
        assert gal['g1'].stat('frag_copy') == (1 if D in (128, 512) else 0), tag
        assert gal['g1'].stat('filter_terms') == 1 and gal['b1'].stat('filter_terms') == 1 and gal['b1'].stat('frag_copy') == 0, tag
        assert gal['split'].stat('filter_terms') == 2 and gal['f32'].stat('filter_terms') == 0, tag

    def remove_all(R, tag):
        nonlocal rows_now
        n = rows_now.shape[0]
        keep, frm, to = remove_ref(np.arange(n), R)
        for name, g in gal.items():
            mf, mt = g.remove(torch.from_numpy(R).to(cuda))
            assert np.array_equal(mf.cpu().numpy(), frm) and np.array_equal(mt.cpu().numpy(), to), (tag, name)
        rows_now = rows_now[torch.from_numpy(keep).to(cuda)]
        valid_copies(tag)                                       # moved, not invalidated: the matches below run on the moved copies
        probes, pick = probes_at(rows_now, np.concatenate([to, to + 1, to - 1, [0, len(keep) - 1]]), gen, 100)
        out = {name: answers(g, probes, pick) for name, g in gal.items()}
        for name in ('g1', 'b1', 'split'):
            assert_same(out[name], out['f32'], (tag, name))
        assert_same(out['f32'], fresh_answers(rows_now, probes, pick, 0), (tag, 'fresh'))
        assert torch.equal(out['g1'][1][0], pick), tag

    valid_copies('enrolled')
    for step in range(2):
        remove_all(tail_patterns(rows_now.shape[0], rng, step), 'pattern %d' % step)
    remove_all(tail_patterns(rows_now.shape[0], rng, 2), 'before the append')
    new = torch.nn.functional.normalize(torch.randn((300, D), device='cuda', generator=gen), dim=1)
    for g in gal.values():
        g.update(new)
        assert g.capacity == 6000
    rows_now = torch.cat([rows_now, new])
    remove_all(tail_patterns(rows_now.shape[0], rng, 2), 'after the append')
    for g in gal.values():
        g.close()


def test_remove_across_the_fragment_threshold(cuda):
    """'frag' = 1 (the default) keeps the copy in fragment order from 2^18 rows up: a removal that takes the row count below
    leaves a copy in the wrong layout, which the next match rewrites."""
    from deep_insight_face import oneshot
    gen = torch.Generator(device='cuda').manual_seed(19)
    rng = np.random.default_rng(19)
    D, G = 128, (1 << 18) + 150
    rows = torch.nn.functional.normalize(torch.randn((G, D), device='cuda', generator=gen), dim=1)
    g = oneshot.Gallery(rows)
    assert g.stat('frag_copy') == 1
    R = np.unique(np.concatenate([rng.permutation(G - 300)[:200], G - 1 - rng.permutation(300)[:100]]))
    assert len(R) == 300
    keep, frm, to = remove_ref(np.arange(G), R)
    mf, mt = g.remove(R)
    assert np.array_equal(mf, frm) and np.array_equal(mt, to) and len(frm) == 200
    assert len(g) == G - 300 < (1 << 18) and g.capacity == G
    rows_now = rows[torch.from_numpy(keep).to(cuda)]
    probes, pick = probes_at(rows_now, np.concatenate([to, to + 1, [0, G - 301]]), gen, 60)
    got = answers(g, probes, pick)
    assert g.stat('frag_copy') == 0 and g.stat('filter_terms') == 1   # rewritten row-major by that match
    assert_same(got, fresh_answers(rows_now, probes, pick, 2), 'across the threshold')
    assert torch.equal(got[1][0], pick)
    g.close()


@pytest.mark.parametrize('flt', [2, 1, 0])
def test_remove_special_rows(cuda, golden_dir, flt):
    """Rows the filter cannot rank (zero, NaN-carrying, huge, tiny) are named by index in the special-row lists: a removal that
    takes one out, or moves one into a hole, rebuilds the lists.  Then the reference's own answers on the degenerate fixtures,
    enrolled with 40 ordinary rows behind them that are removed again."""
    from deep_insight_face import oneshot
    base = gi.gallery(6000, seed=93)
    probes, pick = gi.probes_from(base[:5000], 96, seed=94)
    bad = np.zeros((4, 512), np.float32)
    bad[1, 3] = np.nan
    bad[2] = base[77] * np.float32(1e19)
    bad[3] = base[78] * np.float32(1e-25)
    cur = base[:5000].copy()
    cur[40:44] = bad                                            # head: zero, NaN, huge, tiny
    cur[2000] = bad[1]                                          # a NaN row in the middle
    cur[4990:4994] = bad[::-1]                                  # tail: tiny, huge, NaN, zero ...
    cur[4996:5000] = bad                                        # ... and zero, NaN, huge, tiny in the last four rows
    special = np.array([40, 41, 42, 43, 2000, 4990, 4991, 4992, 4993, 4996, 4997, 4998, 4999])
    g = oneshot.Gallery(emd_size=512)
    g.set_option('filter', flt)
    g.set(cur)
    src = pick.copy()
    assert_same(answers(g, probes, src), fresh_answers(cur, probes, src, flt), 'planted')

    def step(R, tag):
        nonlocal cur, src, special
        cur, frm, to = remove_and_check(g, cur, R)
        src = relocate(src, R, frm, to)
        special = relocate(special, R, frm, to)
        special = special[special >= 0]
        got = answers(g, probes, src)
        assert_same(got, fresh_answers(cur, probes, src, flt), tag)
        return got

    step([40], 'a tail special row (tiny) moves into a special hole (zero)')
    assert 40 in special and 4999 not in special
    for metric in (0, 1):                                       # the first NaN row of each metric wins every search (first-NaN rule)
        first = int(g.match(probes[:4], metric)[0][0])
        assert first in special
        got = step([first], 'the first NaN row of metric %d leaves' % metric)
        assert int(got[metric][0][0]) in special                # a later one (or the special row that filled the hole) is first now
    step(np.sort(special)[::2].copy(), 'half of them')
    got = step(np.sort(special).copy(), 'all of them')
    assert len(special) == 0
    live = src >= 0
    assert np.array_equal(got[1][0][live], src[live])           # ordinary again: every probe finds its source row
    g.close()

    gold = np.load(os.path.join(golden_dir, 'match_degenerate.npz'))
    junk = gi.gallery(40, seed=4321)                            # ordinary rows: never special, and never the arg-min of a fixture
    for name, p, gl in gi.match_degenerate_cases():             # probe (checked against the oracle when this test was written)
        G = gl.shape[0]
        h = oneshot.Gallery(emd_size=gl.shape[1])
        h.set_option('filter', flt)
        h.set(np.concatenate([gl, junk]))
        mf, mt = h.remove(np.arange(G, G + 40))                 # only tail rows: the surviving order is the fixture's
        assert len(mf) == 0 and len(mt) == 0 and len(h) == G
        for metric in (0, 1):
            idx, dist = h.match(p, metric)
            assert np.array_equal(idx, gold['%s_idx%d' % (name, metric)]), (name, metric)
            assert np.array_equal(np.isnan(dist), np.isnan(gold['%s_dmin%d' % (name, metric)])), (name, metric)
        h.close()


def test_remove_index_base_and_arguments(cuda):
    from deep_insight_face import _native as N
    from deep_insight_face import oneshot
    BASE = 10_000
    rng = np.random.default_rng(5)
    rows = gi.gallery(700, seed=95)
    probes, pick = gi.probes_from(rows, 48, seed=96)
    g = oneshot.Gallery(emd_size=512)
    g.set(rows, BASE)
    cur, src = rows.copy(), pick.copy()

    def unchanged(tag):
        assert len(g) == cur.shape[0], tag
        mates = np.where(src >= 0, src + BASE, -1)
        got = answers(g, probes, mates)
        assert_same(got, fresh_answers(cur, probes, mates, 2, BASE), tag)
        return got

    R = np.concatenate([rng.permutation(700)[:40], [699, 3]]) + BASE                # global indices in ...
    cur, frm, to = remove_and_check(g, cur, R, base=BASE)                           # ... and global pairs out
    assert len(to) and to.min() + BASE >= BASE
    src = relocate(src, np.unique(R) - BASE, frm, to)
    got = unchanged('index_base')
    live = src >= 0
    assert np.array_equal(got[1][0][live], src[live] + BASE)
    n = len(g)
    for wrong in ([3], [BASE - 1], [BASE + n], [BASE, BASE + n], [-1], np.array([BASE + 1.0]), np.array([True, False]),
                  np.array([[BASE, BASE + 1]]), np.int64(BASE), torch.tensor([BASE + 0.5]), torch.tensor([True]),
                  torch.tensor([[BASE]]), np.arange(BASE, BASE + n + 1)):
        with pytest.raises(ValueError):
            g.remove(wrong)
        unchanged('after a refused argument')
    # the C entry itself: an unsorted or a duplicated list is refused before anything is touched
    for lst in ([BASE + 5, BASE + 2], [BASE + 2, BASE + 2], [BASE + 2, BASE + n]):
        r = torch.tensor(lst, dtype=torch.int64, device=cuda)
        mf = torch.empty_like(r)
        mt = torch.empty_like(r)
        m = ctypes.c_int64(-7)
        rc = N.lib.dif_gallery_remove(g._h, N.ptr(r), len(lst), N.ptr(mf), N.ptr(mt), ctypes.byref(m), N.stream_ptr())
        assert rc != 0 and 'dif_gallery_remove' in N.last_error()
        unchanged('after a refused list')
    # the pairs are optional
    r = torch.tensor([BASE + 1, BASE + n - 1], dtype=torch.int64, device=cuda)
    m = ctypes.c_int64(-7)
    assert N.lib.dif_gallery_remove(g._h, N.ptr(r), 2, None, None, ctypes.byref(m), N.stream_ptr()) == 0 and m.value == 1
    cur, frm, to = remove_ref(cur, [1, n - 1])
    src = relocate(src, [1, n - 1], frm, to)
    unchanged('without the pair arrays')
    # k = 0
    for empty in ([], np.zeros((0,), np.int32), torch.zeros((0,), dtype=torch.int64, device=cuda)):
        mf, mt = g.remove(empty)
        assert len(mf) == 0 and len(mt) == 0
    assert torch.is_tensor(mf) and mf.is_cuda
    unchanged('k = 0')
    # every row: an empty gallery, which re-enrols by update
    cap = g.capacity
    mf, mt = g.remove(np.arange(BASE, BASE + len(g)))
    assert len(mf) == 0 and len(g) == 0 and g.capacity == cap
    with pytest.raises(ValueError):
        g.match(probes, 1)
    c, wi, wd = g.within(probes, 0.3, 1, max_hits=4)
    assert not c.any() and (wi == -1).all()
    r, md = g.rank(probes, pick + BASE, 1)
    assert (r == -1).all() and np.isnan(md).all()
    g.update(rows[:500])
    cur, src = rows[:500].copy(), np.where(pick < 500, pick, -1)
    assert g.capacity == cap
    unchanged('re-enrolled')
    g.close()
