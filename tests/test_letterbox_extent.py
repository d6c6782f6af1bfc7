"""dif_letterbox_extent (the host function dif_letterbox takes its resized extent from) against the reference's own
statements, detector/yolov3.py:113-115, in Python's floats:

    scale = min(size / w, size / h);  nw = int(w * scale);  nh = int(h * scale)

The limiting axis comes to `s * (size / s)`, an integer or one ulp below it, and int() makes a whole pixel of that ulp:
an evaluation in float32 -- what the launcher did before -- gives another extent at 8 % of the frame sizes, 1280 x 720
among them.  No device is needed: the entry makes no device call."""
import ctypes

import numpy as np
import pytest

from deep_insight_face import _native as N

VIDEO = [(720, 1280), (360, 640), (288, 352), (576, 720), (720, 720), (540, 720), (1080, 1920), (2160, 3840), (768, 1024),
         (1200, 1600)]


def _python(h, w, size):
    scale = min(size / w, size / h)
    return int(w * scale), int(h * scale)


def _float32(h, w, size):
    """The statements as the launcher evaluated them before: every operand and result a float32.  h, w: int arrays."""
    s, wf, hf = np.float32(size), w.astype(np.float32), h.astype(np.float32)
    scale = np.minimum(s / wf, s / hf)
    assert scale.dtype == np.float32
    return (wf * scale).astype(np.int64), (hf * scale).astype(np.int64)


def _sweep(hmax, wmax, size):
    """Every (h, w) of 1..hmax x 1..wmax: the library's answer equals Python's; where Python gives 0 for an axis -- PIL
    rejects such a resize -- the library fails with `image too thin`.  Returns the library's extents ([hmax, wmax], 0 where it
    failed) and the number of sizes that failed."""
    fn = N.lib.dif_letterbox_extent
    nw, nh = ctypes.c_int(0), ctypes.c_int(0)
    pw, ph = ctypes.byref(nw), ctypes.byref(nh)
    got = np.zeros((2, hmax, wmax), dtype=np.int64)
    bad, thin = [], 0
    for h in range(1, hmax + 1):
        for w in range(1, wmax + 1):
            scale = min(size / w, size / h)
            ew, eh = int(w * scale), int(h * scale)
            rc = fn(h, w, size, pw, ph)
            if ew < 1 or eh < 1:
                thin += 1
                if rc == 0 or 'dif_letterbox_extent: image too thin' not in N.last_error():
                    bad.append((h, w, 'no error', (ew, eh)))
            elif rc != 0 or nw.value != ew or nh.value != eh:
                bad.append((h, w, (rc, nw.value, nh.value), (ew, eh)))
            else:
                got[0, h - 1, w - 1], got[1, h - 1, w - 1] = ew, eh
    assert not bad, (size, len(bad), bad[:8])
    return got, thin


def test_extent_equals_python_at_canvas_416():
    got, thin = _sweep(640, 640, 416)
    assert thin > 0                                   # 1 x 417 and thinner: the sweep reaches the error path
    # the sweep can see the defect: float32 statements disagree with what it just held the library to
    h, w = np.mgrid[1:641, 1:641]
    fw, fh = _float32(h, w, 416)
    ok = (got[0] > 0)
    differ = ok & ((fw != got[0]) | (fh != got[1]))
    assert differ.sum() >= 30000, differ.sum()
    # both directions occur on the square sizes: 11 and 22 are 416 in double and 415 in float32, 23 the reverse
    side = {s: (int(got[0, s - 1, s - 1]), int(fw[s - 1, s - 1])) for s in (11, 22, 23)}
    assert side == {11: (416, 415), 22: (416, 415), 23: (415, 416)}, side


@pytest.mark.parametrize('size', [64, 320, 608])
def test_extent_equals_python_at_other_canvases(size):
    got, _ = _sweep(256, 256, size)
    h, w = np.mgrid[1:257, 1:257]
    fw, fh = _float32(h, w, size)
    # float32 fails inside this sweep as well: one size per canvas that the device tests letterbox
    hh, ww = {64: (20, 41), 320: (20, 77), 608: (42, 56)}[size]
    assert (int(fw[hh - 1, ww - 1]), int(fh[hh - 1, ww - 1])) != (int(got[0, hh - 1, ww - 1]), int(got[1, hh - 1, ww - 1]))


@pytest.mark.parametrize('size', [416, 64, 320, 608])
def test_extent_at_video_sizes(size):
    nw, nh = ctypes.c_int(0), ctypes.c_int(0)
    for a, b in VIDEO:
        for h, w in ((a, b), (b, a)):
            ew, eh = _python(h, w, size)
            assert ew >= 1 and eh >= 1
            assert N.lib.dif_letterbox_extent(h, w, size, ctypes.byref(nw), ctypes.byref(nh)) == 0, N.last_error()
            assert (nw.value, nh.value) == (ew, eh), (h, w, size)


def test_extent_pinned_values():
    """What Python gives, written out: (h, w, canvas) -> (nw, nh).  The float32 statements miss every one of them."""
    from deep_insight_face.detector.yolov3 import letterbox_extent
    pinned = {(360, 640, 416): (416, 234), (720, 1280, 416): (416, 234), (1280, 720, 416): (234, 416),
              (288, 352, 416): (416, 340), (576, 720, 416): (415, 332), (11, 11, 416): (416, 416), (23, 23, 416): (415, 415),
              (20, 41, 64): (64, 31), (20, 49, 64): (63, 26), (42, 56, 608): (608, 456), (20, 77, 320): (319, 83)}
    for (h, w, size), want in pinned.items():
        assert _python(h, w, size) == want, (h, w, size)
        assert letterbox_extent(h, w, size) == want, (h, w, size)
        fw, fh = _float32(np.array([h]), np.array([w]), size)
        assert (int(fw[0]), int(fh[0])) != want, (h, w, size)


def test_extent_errors():
    from deep_insight_face.detector.yolov3 import letterbox_extent
    nw, nh = ctypes.c_int(7), ctypes.c_int(7)
    for h, w, size in [(0, 5, 416), (5, 0, 416), (5, 5, 0), (-1, 5, 416), (5, -3, 416), (5, 5, -416)]:
        assert N.lib.dif_letterbox_extent(h, w, size, ctypes.byref(nw), ctypes.byref(nh)) != 0
        assert 'dif_letterbox_extent: bad sizes' in N.last_error()
    for h, w, size in [(1, 417, 416), (417, 1, 416), (1, 3840, 416), (2, 129, 64), (1, 2 ** 31 - 1, 608)]:
        assert 0 in _python(h, w, size)
        assert N.lib.dif_letterbox_extent(h, w, size, ctypes.byref(nw), ctypes.byref(nh)) != 0
        assert 'dif_letterbox_extent: image too thin' in N.last_error()
        with pytest.raises(ValueError, match='image too thin'):
            letterbox_extent(h, w, size)
    assert N.lib.dif_letterbox_extent(1, 416, 416, ctypes.byref(nw), ctypes.byref(nh)) == 0      # the thinnest that still has a row
    assert (nw.value, nh.value) == (416, 1)
    assert N.lib.dif_letterbox_extent(5, 5, 416, None, ctypes.byref(nh)) != 0 and 'null pointer' in N.last_error()
    assert N.lib.dif_letterbox_extent(5, 5, 416, ctypes.byref(nw), None) != 0 and 'null pointer' in N.last_error()
