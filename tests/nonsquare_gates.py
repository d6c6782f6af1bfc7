"""Shared by the H != W tests (tests/test_nonsquare_gpu.py on the device, tests/test_oracle_nets.py and
tests/test_detector.py on the CPU): the seeded inputs and the comparison functions.  The gates are the ones
tests/test_embed_gpu.py::test_embed_vs_oracle and tests/test_detector.py::test_yolov3_gpu_vs_oracle hold a square
network to: element-wise atol = 2e-4 * max |want|, rtol = 2e-3; embeddings also a cosine gap below 1e-5.  The CPU
tests feed the same functions an oracle run with ONE 3x3 kernel's spatial axes transposed and require them to raise."""
import numpy as np

ATOL_REL, RTOL, COS_TOL = 2e-4, 2e-3, 1e-5


def frames_u8(n, hw, seed=1234):
    """Seeded uint8 images [n, h, w, 3]: no symmetry between the axes."""
    return np.random.default_rng(seed).integers(0, 256, (n, hw[0], hw[1], 3), dtype=np.uint8)


def scaled(u8):
    return u8.astype(np.float32) / np.float32(255.0)


def cosine_gap(a, b):
    a = a.reshape(a.shape[0], -1).astype(np.float64)
    b = b.reshape(b.shape[0], -1).astype(np.float64)
    return 1.0 - (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))


def worst(got, want):
    """max |got - want| / max |want|: the figure the tests print beside the float32-vs-float64 oracle yardstick."""
    return float(np.abs(got.astype(np.float64) - want).max() / np.abs(want).max())


def check_map(got, want):
    """A feature map or a detector map [N, H', W', C] against the oracle's: the full shape, then every element."""
    assert got.shape == want.shape, (got.shape, want.shape)
    assert got.dtype == np.float32 and np.all(np.isfinite(got))
    np.testing.assert_allclose(got, want, atol=ATOL_REL * np.abs(want).max(), rtol=RTOL)
    return worst(got, want)


def check_embedding(got, want):
    """An embedding [N, emd] against the oracle's: cosine gap and every element."""
    assert got.shape == want.shape, (got.shape, want.shape)
    assert got.dtype == np.float32 and np.all(np.isfinite(got))
    gap = cosine_gap(got, want)
    assert gap.max() < COS_TOL, gap
    np.testing.assert_allclose(got, want, atol=ATOL_REL * np.abs(want).max(), rtol=RTOL)
    return worst(got, want)


def transposed(p, name):
    """The parameters with the two spatial axes of one HWIO kernel swapped: what an H/W slip in one layer computes."""
    q = dict(p)
    assert q[name].shape[0] == q[name].shape[1] == 3
    q[name] = np.ascontiguousarray(q[name].transpose(1, 0, 2, 3))
    return q
