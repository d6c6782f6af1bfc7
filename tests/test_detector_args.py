"""The argument checks of dif_nms and the three MTCNN glue entry points (csrc/detector.hip, csrc/mtcnn.hip), which need no
device: every "bad sizes" and "null pointer" branch returns non-zero with its message before anything is launched, and
n == 0 returns 0 with NULL pointers."""
import ctypes


def test_entry_points_check_their_arguments_without_a_device():
    """Every bad size, and every pointer NULL at once; n == 0 returns 0 with NULL pointers."""
    from deep_insight_face import _native as N
    L = N.lib

    def refused(rc, message):
        return rc != 0 and message in N.last_error()

    assert L.dif_mtcnn_propose(None, 0, 3, 3, 8, 0.6, 0.6, None, None, None) == 0
    for n, gh, gw, ld, scale in ((-1, 3, 3, 8, 0.6), (1, 0, 3, 8, 0.6), (1, 3, 0, 8, 0.6), (1, 3, 3, 5, 0.6), (1, 3, 3, 8, 0.0),
                                 (1, 3, 3, 8, -1.0), (1, 3, 3, 8, float('nan'))):
        assert refused(L.dif_mtcnn_propose(None, n, gh, gw, ld, scale, 0.6, None, None, None), 'dif_mtcnn_propose: bad sizes')
    assert refused(L.dif_mtcnn_propose(None, 1, 3, 3, 8, 0.6, 0.6, None, None, None), 'dif_mtcnn_propose: null pointer')

    assert L.dif_mtcnn_gather(None, 0, 4, None, None, None, 4, 9, None, None, None, 4, 0, 0, None) == 0
    for n, k, n_src, n_dst, off in ((-1, 4, 9, 4, 0), (1, 0, 9, 4, 0), (1, 4, 0, 4, 0), (1, 4, 9, 3, 0), (1, 4, 9, 8, -1),
                                    (1, 4, 9, 8, 5)):
        assert refused(L.dif_mtcnn_gather(None, n, k, None, None, None, 4, n_src, None, None, None, n_dst, off, 0, None),
                       'dif_mtcnn_gather: bad sizes')
    assert refused(L.dif_mtcnn_gather(None, 1, 4, None, None, None, 4, 9, None, None, None, 4, 0, 0, None),
                   'dif_mtcnn_gather: null pointer')

    assert L.dif_mtcnn_rescore(None, 0, 8, 0.7, None, None, None, 0, None) == 0
    for slots, ld in ((-1, 8), (4, 5)):
        assert refused(L.dif_mtcnn_rescore(None, slots, ld, 0.7, None, None, None, 0, None), 'dif_mtcnn_rescore: bad sizes')
    assert refused(L.dif_mtcnn_rescore(None, 4, 8, 0.7, None, None, None, 0, None), 'dif_mtcnn_rescore: null pointer')

    assert L.dif_nms(None, None, 0, 10, 1, 5, 0.0, 0.5, None, None, None, None) == 0
    for n, k, c, cap in ((-1, 10, 1, 5), (1, -1, 1, 5), (1, 10, 0, 5), (1, 10, 1, 0)):
        assert refused(L.dif_nms(None, None, n, k, c, cap, 0.0, 0.5, None, None, None, None), 'dif_nms: bad sizes')
    assert refused(L.dif_nms(None, None, 1, 10, 1, 5, 0.0, 0.5, None, None, None, None), 'dif_nms: null pointer')


def test_each_null_pointer_is_refused_without_a_device():
    """Every pointer NULL on its own.  The others point at host memory that is never read: the checks come before the launch."""
    from deep_insight_face import _native as N
    L = N.lib
    host = (ctypes.c_float * 64)()
    p = ctypes.c_void_p(ctypes.addressof(host))

    def refused(rc, message):
        return rc != 0 and message in N.last_error()

    def one_null(count):
        return [tuple(None if i == j else p for i in range(count)) for j in range(count)]

    for head, boxes, scores in one_null(3):
        assert refused(L.dif_mtcnn_propose(head, 1, 2, 2, 8, 0.6, 0.6, boxes, scores, None), 'dif_mtcnn_propose: null pointer')
    for keep, sb, ss, db, ds in one_null(5):
        assert refused(L.dif_mtcnn_gather(keep, 1, 4, sb, ss, p, 4, 9, db, ds, p, 4, 0, 0, None), 'dif_mtcnn_gather: null pointer')
    assert refused(L.dif_mtcnn_gather(p, 1, 4, p, p, None, 4, 9, p, p, p, 4, 0, 1, None),
                   'dif_mtcnn_gather: calibration needs the regression values')
    for out, scores, reg in one_null(3):
        assert refused(L.dif_mtcnn_rescore(out, 4, 8, 0.7, scores, reg, p, 0, None), 'dif_mtcnn_rescore: null pointer')
    assert refused(L.dif_mtcnn_rescore(p, 4, 8, 0.7, p, p, None, 1, None), 'dif_mtcnn_rescore: null pointer')
    for boxes, scores, alive, keep, count in one_null(5):
        assert refused(L.dif_nms(boxes, scores, 1, 10, 1, 5, 0.0, 0.5, alive, keep, count, None), 'dif_nms: null pointer')
