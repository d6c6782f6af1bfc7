"""NumPy restatement of csrc/faces.hip's compaction for the tests (test infrastructure only): slots -> the list of faces,
frame-major and in slot order, with CSR offsets."""
import numpy as np


def compact(scores, min_score=0.0, max_faces=None):
    """scores [n, k] -> (count, offsets [n + 1], frame [max_faces], slot [max_faces]), int32.  A slot is a face when
    score >= min_score (inclusive; NaN is none).  count and offsets are exact; the lists hold the first max_faces faces
    (default n * k), then -1."""
    s = np.asarray(scores, dtype=np.float32)
    n, k = s.shape
    max_faces = n * k if max_faces is None else int(max_faces)
    with np.errstate(invalid='ignore'):
        face = s >= np.float32(min_score)
    offsets = np.zeros(n + 1, np.int32)
    offsets[1:] = np.cumsum(face.sum(1))
    f, sl = np.nonzero(face)                               # row-major: frame-major, slot order inside a frame
    frame = np.full(max_faces, -1, np.int32)
    slot = np.full(max_faces, -1, np.int32)
    m = min(len(f), max_faces)
    frame[:m], slot[:m] = f[:m], sl[:m]
    return int(offsets[n]), offsets, frame, slot
