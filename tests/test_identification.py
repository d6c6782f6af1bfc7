"""evaluation/identification.py: cmc and open_set_rates against plain loops -- NaNs, no mated probes, no unmated probes,
NumPy and CPU-tensor inputs.  No GPU (the functions are array arithmetic; evaluate_identification is in test_rank_gpu.py)."""
import numpy as np
import pytest
import torch

from deep_insight_face.evaluation import identification as ident


def _cmc_loop(rank, max_rank):
    mated = [r for r in rank if r >= 0]
    return np.array([sum(1 for r in mated if r < k) / len(mated) if mated else np.nan
                     for k in range(1, max_rank + 1)], dtype=np.float64)


def _rates_loop(rank, mate_dist, um, thresholds, k):
    mated = [(r, d) for r, d in zip(rank, mate_dist) if r >= 0]
    dirs, far = [], []
    for t in thresholds:
        dirs.append(sum(1 for r, d in mated if r < k and d <= t) / len(mated) if mated else np.nan)   # NaN <= t is False
        far.append(sum(1 for d in um if d <= t) / len(um) if len(um) else np.nan)
    return np.array(dirs, dtype=np.float64), np.array(far, dtype=np.float64)


def _cases():
    rng = np.random.default_rng(5)
    G = 50
    rank = rng.integers(-1, 12, 200).astype(np.int64)
    rank[rng.random(200) < 0.05] = G                             # mates with a NaN distance
    md = rng.random(200).astype(np.float32)
    md[(rank < 0) | (rank == G)] = np.nan
    um = rng.random(37).astype(np.float32)
    um[[3, 20]] = np.nan
    yield 'mixed', rank, md, um
    yield 'no_mated', np.full(9, -1, dtype=np.int64), np.full(9, np.nan, dtype=np.float32), um
    yield 'no_unmated', np.abs(rank), np.where(np.isnan(md), np.float32(0.5), md), np.zeros(0, dtype=np.float32)
    yield 'empty', np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.float32)


THRESHOLDS = np.array([-1.0, 0.0, 0.1, 0.5, 0.9, 1.0, np.nan])


@pytest.mark.parametrize('name', [c[0] for c in _cases()])
@pytest.mark.parametrize('kind', ['numpy', 'tensor'])
def test_cmc_and_open_set_rates(name, kind):
    _, rank, md, um = [c for c in _cases() if c[0] == name][0]
    if kind == 'tensor':
        conv = torch.from_numpy
        back = lambda x: x.numpy()
    else:
        conv = back = lambda x: x
    got = ident.cmc(conv(rank), 10)
    assert (torch.is_tensor(got) if kind == 'tensor' else isinstance(got, np.ndarray))
    got = back(got)
    assert got.dtype == np.float64 and got.shape == (10,)
    np.testing.assert_array_equal(got, _cmc_loop(rank, 10))       # counts divided once: exact, NaN == NaN here
    assert back(ident.cmc(conv(rank), 0)).shape == (0,)
    for k in (1, 5):
        d, f = ident.open_set_rates(conv(rank), conv(md), conv(um), conv(THRESHOLDS) if kind == 'tensor' else list(THRESHOLDS), k=k)
        assert (torch.is_tensor(d) and torch.is_tensor(f)) if kind == 'tensor' else (isinstance(d, np.ndarray) and isinstance(f, np.ndarray))
        d, f = back(d), back(f)
        wd, wf = _rates_loop(rank, md, um, THRESHOLDS, k)
        assert d.dtype == np.float64 and f.dtype == np.float64 and d.shape == wd.shape and f.shape == wf.shape
        np.testing.assert_array_equal(d, wd)
        np.testing.assert_array_equal(f, wf)


def test_rates_meaning():
    rank = np.array([0, 0, 3, -1, 50, 1], dtype=np.int64)          # 5 mated (one of them with a NaN mate), 1 unmated
    md = np.array([0.1, 0.4, 0.2, np.nan, np.nan, 0.3], dtype=np.float32)
    np.testing.assert_array_equal(ident.cmc(rank, 4), [2 / 5, 3 / 5, 3 / 5, 4 / 5])
    d, f = ident.open_set_rates(rank, md, np.array([0.25], dtype=np.float32), [0.2, 0.3, 1.0])
    np.testing.assert_array_equal(d, [1 / 5, 1 / 5, 2 / 5])
    np.testing.assert_array_equal(f, [0.0, 1.0, 1.0])
    d, _ = ident.open_set_rates(rank, md, np.array([0.25], dtype=np.float32), [1.0], k=2)
    np.testing.assert_array_equal(d, [3 / 5])
    with pytest.raises(ValueError):
        ident.cmc(rank, -1)
