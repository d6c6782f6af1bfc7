"""NumPy restatements of csrc/align.hip for the alignment tests (test infrastructure only): the bilinear warp in float32,
operation by operation as include/dif.h writes it out; the five-point similarity fit in float64; the landmark decode of
the MTCNN cascade in float32."""
import numpy as np

F = np.float32


def warp_affine(frames, matrices, out_hw, k=1):
    """frames uint8 [N,H,W,3]; matrices [N*k, 6] (or anything that reshapes to it), output pixel -> frame position
    -> uint8 [N*k, out_h, out_w, 3].  float32 throughout, every product and sum rounded by itself."""
    frames = np.asarray(frames)
    n, h, w, _ = frames.shape
    m = np.asarray(matrices, dtype=F).reshape(n * k, 6)
    oh, ow = out_hw
    ys, xs = np.meshgrid(np.arange(oh, dtype=F), np.arange(ow, dtype=F), indexing='ij')
    out = np.zeros((n * k, oh, ow, 3), np.uint8)
    with np.errstate(invalid='ignore', over='ignore'):
        for j in range(n * k):
            img = frames[j // k]
            sx = (m[j, 0] * xs + m[j, 1] * ys) + m[j, 2]
            sy = (m[j, 3] * xs + m[j, 4] * ys) + m[j, 5]
            assert sx.dtype == F and sy.dtype == F
            x0, y0 = np.floor(sx), np.floor(sy)
            ok = np.isfinite(sx) & np.isfinite(sy) & (x0 >= F(-1)) & (x0 <= F(w - 1)) & (y0 >= F(-1)) & (y0 <= F(h - 1))
            fx = np.where(ok, sx - x0, F(0)).astype(F)[..., None]
            fy = np.where(ok, sy - y0, F(0)).astype(F)[..., None]
            ix = np.where(ok, x0, F(0)).astype(np.int64)
            iy = np.where(ok, y0, F(0)).astype(np.int64)

            def tap(tx, ty):
                inside = (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
                v = img[np.clip(ty, 0, h - 1), np.clip(tx, 0, w - 1)].astype(F)
                return np.where(inside[..., None], v, F(0)).astype(F)

            p00, p01, p10, p11 = tap(ix, iy), tap(ix + 1, iy), tap(ix, iy + 1), tap(ix + 1, iy + 1)
            top = p00 + (p01 - p00) * fx
            bot = p10 + (p11 - p10) * fx
            v = top + (bot - top) * fy
            assert v.dtype == F
            px = np.minimum(np.maximum(np.floor(v + F(0.5)), F(0)), F(255)).astype(np.uint8)
            out[j] = np.where(ok[..., None], px, 0)
    return out


def fit(landmarks, template):
    """Least-squares similarity (no reflection) landmarks [5, 2] -> template [5, 2], inverted: the float64 2 x 3 matrix
    that takes an output pixel to a frame position; NaNs when the landmarks or the template coincide in one point."""
    p = np.asarray(landmarks, dtype=np.float64)
    q = np.asarray(template, dtype=np.float64)
    if not np.isfinite(p).all():
        return np.full((2, 3), np.nan)
    mp, mq = p.mean(0), q.mean(0)
    pc, qc = p - mp, q - mq
    den = (pc * pc).sum()
    dot = (pc * qc).sum()
    cr = (pc[:, 0] * qc[:, 1] - pc[:, 1] * qc[:, 0]).sum()
    if den == 0 or (dot == 0 and cr == 0):
        return np.full((2, 3), np.nan)
    a, b = dot / den, cr / den
    n2 = a * a + b * b
    ia, ib = a / n2, b / n2
    lin = np.array([[ia, ib], [-ib, ia]])
    return np.concatenate([lin, (mp - lin @ mq)[:, None]], 1)


def apply(matrix, points):
    """2 x 3 matrix on points [..., 2] in float64."""
    m = np.asarray(matrix, dtype=np.float64).reshape(2, 3)
    return np.asarray(points, dtype=np.float64) @ m[:, :2].T + m[:, 2]


def similarity(scale, degrees, tx, ty):
    """Forward 2 x 3 matrix of a similarity: x -> scale * R(degrees) x + (tx, ty), float64."""
    c, s = scale * np.cos(np.radians(degrees)), scale * np.sin(np.radians(degrees))
    return np.array([[c, -s, tx], [s, c, ty]], dtype=np.float64)


def invert(matrix):
    """Inverse of a 2 x 3 affine matrix, float64."""
    m = np.asarray(matrix, dtype=np.float64).reshape(2, 3)
    lin = np.linalg.inv(m[:, :2])
    return np.concatenate([lin, (-lin @ m[:, 2])[:, None]], 1)


def decode_landmarks(onet_out, boxes, h, w):
    """O-Net outputs [S, 16] and the boxes [S, 4] the crops were cut from -> [S, 5, 2]: landmark k = (l + o[6 + k] * cw,
    t + o[11 + k] * ch) on the rectangle clamped to the frame and truncated (dif_crop_resize_multi's), float32."""
    o = np.asarray(onet_out, dtype=F)
    b = np.asarray(boxes, dtype=F)
    l = np.maximum(b[:, 0], F(0)).astype(np.int32)
    t = np.maximum(b[:, 1], F(0)).astype(np.int32)
    r = np.minimum(b[:, 2], F(w)).astype(np.int32)
    bt = np.minimum(b[:, 3], F(h)).astype(np.int32)
    cw, ch = (r - l).astype(F), (bt - t).astype(F)
    x = l.astype(F)[:, None] + o[:, 6:11] * cw[:, None]
    y = t.astype(F)[:, None] + o[:, 11:16] * ch[:, None]
    assert x.dtype == F and y.dtype == F
    return np.stack([x, y], -1)
