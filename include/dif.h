/* libdif -- C ABI of the MI355X-native embedding + match hot path.
 *
 * The reference (sandyz1000/deep-insight-face) has no FFI: its seam is a duck-typed
 * Python protocol.  Each entry point below names the
 * reference interface it stands behind (paths relative to the reference root).  The
 * Python host side (deep-insight-face_amd/deep_insight_face/) binds these with ctypes
 * and keeps the reference's call signatures; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure; dif_last_error()
 *     returns the message of the calling thread's last failure;
 *   - pointers named *_dev are DEVICE pointers borrowed for the duration of the call
 *     (stream-ordered: the work is enqueued on `stream`, a hipStream_t passed as
 *     void*; NULL = the default stream); host pointers are named *_host;
 *   - handles own their device memory (weights, gallery copy, workspaces) and are not
 *     re-entrant: one handle per process/GPU, calls on one handle from one thread;
 *   - there is NO CPU fallback: without a HIP device every compute entry point fails.
 */
#ifndef DIF_H
#define DIF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DIF_VERSION 110 /* 1.1: + dif_gallery_update / _reserve / _capacity, dif_*_option_name, options "sk2", "mt"; gallery option "frag"; + dif_match_within, dif_match_rank; + dif_gallery_remove; + dif_match_topk, gallery option "topk_seed"; + dif_match_topk_ids; + dif_gallery_cluster, gallery option "cluster_round"; + dif_gallery_dbscan; + dif_match_roc, gallery option "roc_round"; + dif_net_op_describe, dif_net_embed_tap; + dif_letterbox_extent (additions: no entry point changed, the number stays) */

/* distance metrics: evaluation/utility.py:52-66 */
#define DIF_METRIC_SQL2 0   /* sum((a-b)^2, axis=1)                     utility.py:53-56 */
#define DIF_METRIC_COSINE 1 /* arccos(a.b / (|a||b|)) / pi              utility.py:57-62 */
#define DIF_METRIC_SIMILARITY 2 /* dif_pairwise only: the cosine similarity a.b / (|a||b|) itself, i.e.
                                 * utility.py:58-60 before the arccos (common/losses.py:39-40 precedent) */

/* input layouts / dtypes accepted by dif_net_embed */
#define DIF_LAYOUT_NHWC 0 /* the reference's layout (networks/inceptionv3.py:94,98) */
#define DIF_LAYOUT_NCHW 1 /* north_star's torch-side layout */
#define DIF_DTYPE_F32 0
#define DIF_DTYPE_U8 1
/* flags of dif_net_set_input_transform */
#define DIF_INPUT_BGR 1   /* swap R and B (keras vgg16 preprocess_input, predictions.py:95) */
#define DIF_INPUT_HFLIP 2 /* mirror every image left-right (scripts/insight_face.py:117-118 use_flipped_images) */

typedef struct dif_gallery dif_gallery;
typedef struct dif_net dif_net;
typedef struct dif_arcmargin dif_arcmargin;

int dif_version(void);
const char* dif_last_error(void);
/* number of visible HIP devices (0 without a GPU); never fails */
int dif_device_count(void);
/* measurement aid (no reference counterpart): the shader clock in GHz that the current device holds under ~20 ms of
 * back-to-back v_mfma_f32_32x32x2_f32 (pseudo-random operands) on every SIMD, and the TFLOP/s that loop sustained (may be null).  bench.py
 * records it next to its rooflines, which price against the 2.4 GHz peak. */
int dif_probe_mfma_clock(double* ghz_out, double* tflops_out, void* stream);

/* ------------------------------------------------------------------ distances
 * Row-paired distance, out_dev[i] = d(e1[i], e2[i]); n1 or n2 may be 1 (NumPy
 * broadcast of a single row, which is how a probe is compared with a whole gallery
 * in the reference's terms).  Replaces evaluation/utility.py:52-66 `distance`
 * (and its twin :174-188).  metric other than 0/1 fails like the reference's
 * RuntimeError('Undefined distance metric %d').  NaN where the reference gives NaN.
 * d in [1, 8192] (anything else fails with "outside [1, 8192]"): metric 0 and DIF_METRIC_SIMILARITY are NumPy's float32
 * result bit for bit at every such d -- the sums follow NumPy's pairwise-summation tree, which has at most 65 leaves of <= 128
 * elements there (65 at 441 sizes of [7689, 8191], none a multiple of 32) -- and metric 1 within 4 ulp of it.  Tested at
 * every d in 1..300, at sizes up to 8192 and at thirteen of the 65-leaf sizes; the gallery queries below at d = 96, 160, 288
 * (two-term filter), 320, 640, 1024, 2048, 8192 (one-term row-major filter) besides the sizes up to 512; dif_arcmargin_logits
 * at d = 32, 96, 1024, 2048 within s u ((d + 2) A + (d / 64 + 9) |c|) of the float64 value, u = 2^-24, c the cosine,
 * A = sum |e_k w_k| / (|e| |w|) <= 1. */
int dif_pairwise(const float* e1_dev, int64_t n1, const float* e2_dev, int64_t n2, int d, int metric,
                 float* out_dev, void* stream);

/* LFW-protocol threshold sweep (evaluation/utility.py:36-49 calculate_accuracy and :69-77
 * calculate_val_far, as looped by calculate_roc :153-161 and calculate_val :104-107): for every
 * threshold t and test fold f, counts_dev[(f*T + t)*2 + 0/1] = number of pairs of fold f with
 * dist < thresholds[t] that are same / different.  fold_dev[i] = fold whose test split holds
 * pair i (KFold(shuffle=False): contiguous ranges). */
int dif_threshold_counts(const float* dist_dev, const uint8_t* issame_dev, const int32_t* fold_dev, int64_t n,
                         const double* thresholds_dev, int n_thresholds, int n_folds, int32_t* counts_dev,
                         void* stream);

/* ------------------------------------------------------------------ detector post-processing
 * YOLOv3-face box decode and suppression (detector/yolov3.py:36-172).
 * dif_yolo_decode: feats_dev = HOST array of n_layers DEVICE pointers, coarse grid first, each
 * [n_images][gh][gw][3*(5+n_classes)]; grid_hw_host [n_layers][2]; anchors_host [n_layers][3][2]
 * (pixels of the network input, already selected per layer); image_shape_dev [n_images][2] =
 * original (height, width).  Writes boxes_dev [n_images][n_boxes][4] (y_min, x_min, y_max, x_max in
 * image pixels; n_boxes = sum gh*gw*3) and scores_dev [n_images][n_boxes][n_classes] =
 * confidence * class probability (yolo_head :36-66, correct_boxes :69-93, boxes_and_scores :96-106).
 * dif_nms: per (image, class) keep boxes with score >= score_threshold and run the greedy
 * suppression of tf.image.non_max_suppression (get_yolo_output :149-160): keep_idx_dev
 * [n_images][n_classes][max_boxes] (box indices in pick order, -1 padded), keep_count_dev
 * [n_images][n_classes]; alive_ws_dev = n_images*n_classes*n_boxes bytes of scratch.  A box whose score is NaN or
 * -inf never takes part, whatever score_threshold is (-inf included), as tf.image.non_max_suppression admits only
 * score > score_threshold.  boxes_dev must be 16-byte aligned (a box is read as one 4-float vector). */
int dif_yolo_decode(const float* const* feats_dev, const int32_t* grid_hw_host, const float* anchors_host,
                    int n_layers, int n_images, int n_classes, int input_h, int input_w,
                    const float* image_shape_dev, float* boxes_dev, float* scores_dev, void* stream);
int dif_nms(const float* boxes_dev, const float* scores_dev, int n_images, int n_boxes, int n_classes, int max_boxes,
            float score_threshold, float iou_threshold, uint8_t* alive_ws_dev, int32_t* keep_idx_dev,
            int32_t* keep_count_dev, void* stream);

/* Image resampling around the detector, uint8 NHWC in and out.
 * dif_letterbox: aspect-preserving BICUBIC resize (PIL semantics incl. antialiasing) onto a
 *   size x size canvas of (128,128,128)                       detector/yolov3.py:108-119
 *   PIL's 8-bit arithmetic operation by operation: weights in double, normalised, rounded to 22-bit fixed point, int32
 *   sums, an 8-bit image between the horizontal and the vertical pass -- PIL's bytes (tested against Pillow 12)
 * dif_crop_resize: per frame, box (left, top, right, bottom) + margin/2 per side, clamped
 *   (detector/run.py:63-87), resampled to size x size by area coverage (cv2 INTER_AREA, which is what
 *   predictions.py:93,154 selects); an empty / NaN box gives a black crop.
 * dif_letterbox_extent: where the picture lies on dif_letterbox's canvas.  nw_out / nh_out (HOST pointers) = the resized
 *   extent, exactly the reference's  scale = min(size / w, size / h); nw = int(w * scale); nh = int(h * scale)  in Python's
 *   floats (IEEE double, one rounding per operation; float32 gives another pixel count at 8 % of the frame sizes up to
 *   640 x 640 -- 1280 x 720 is 416 x 234 in the reference and 416 x 233 in float32).  The picture occupies columns
 *   [(size - nw) / 2, (size - nw) / 2 + nw) and rows [(size - nh) / 2, (size - nh) / 2 + nh) (integer division), the rest is
 *   grey; dif_letterbox resamples with the factors w / nw and h / nh.  No device call; fails as dif_letterbox does: "bad
 *   sizes" for h, w or size < 1, "image too thin" where an axis comes to 0 pixels (PIL rejects that resize too). */
int dif_letterbox(const uint8_t* frames_dev, int n, int h, int w, uint8_t* out_dev, int size, void* stream);
int dif_letterbox_extent(int h, int w, int size, int* nw_out, int* nh_out);
int dif_crop_resize(const uint8_t* frames_dev, int n, int h, int w, const float* boxes_ltrb_dev, float margin,
                    uint8_t* out_dev, int size, void* stream);
/* dif_area_resize: whole images [n][h][w][3] -> [n][out_h][out_w][3] by the same area coverage: the
 *   `cv2.resize(image, size, interpolation=Image.BICUBIC)` of predictions.py:93,154 (PIL's BICUBIC
 *   constant 3 is cv2.INTER_AREA) for crops that are not at the embedder's input size yet. */
int dif_area_resize(const uint8_t* images_dev, int n, int h, int w, uint8_t* out_dev, int out_h, int out_w,
                    void* stream);

/* ------------------------------------------------------------------ MTCNN cascade (BASELINE configs[4] as worded)
 * NOT IN THE REFERENCE (config.py:37, detector/run.py:124 name it in comments only; the detector it ships is YOLOv3-face,
 * above).  The three networks are dif_net archs "mtcnn_pnet" (any input >= 12 x 12; output map [H', W', 8] = logits 2 |
 * box regression 4 | 0 0), "mtcnn_rnet" (24 x 24 -> [8]) and "mtcnn_onet" (48 x 48 -> [16] = logits 2 | box 4 | landmarks
 * 10); inputs are (x - 127.5) / 128 (dif_net_set_input_transform).  The entry points below are the arithmetic between
 * them, on static shapes -- a fixed number of slots per frame and stage, an empty slot has score -1 -- so that a batch of
 * frames runs the whole cascade without a host round trip; dif_nms (above) does every suppression (scores >= 0 take part).
 * The calling convention kept from the reference is detector/run.py:120-173 (deep_insight_face.detector.mtcnn).
 * dif_mtcnn_propose: head map [n][gh][gw][ld] of P-Net at pyramid scale `scale` -> one proposal per cell:
 *   boxes_dev [n][gh*gw][4] = trunc((2 g + 1) / scale), trunc((2 g + 12) / scale) as (x1, y1, x2, y2) in frame pixels,
 *   scores_dev [n][gh*gw] = P(face) = softmax(logits)[1], or -1 below `threshold`.
 * dif_mtcnn_gather: slot (f, dst_offset + j) of the destination arrays ([n][n_dst] slots) <- source slot (f, keep[f][j])
 *   ([n][n_src] slots; src_reg rows are src_reg_ld floats apart -- the P-Net map itself serves, offset to its box
 *   channels), keep < 0 -> an empty slot; calibrate != 0: the box is regressed (x += reg * (side + 1)), squared around its
 *   centre and truncated first.  dst_reg_dev may be NULL.
 * dif_mtcnn_rescore: network outputs out_dev [slots][ld] -> scores (P(face) where the slot was alive and passes
 *   `threshold`, else -1) and reg_dev [slots][4]; plain_regression != 0 also regresses boxes_dev in place without
 *   squaring (the cascade's last step).
 * dif_crop_resize_multi: k boxes per frame, boxes [n][k][4] (left, top, right, bottom), valid_dev [n][k] (may be NULL;
 *   negative = empty slot -> black crop) -> out_dev [n*k][size][size][3]; arithmetic of dif_crop_resize. */
int dif_mtcnn_propose(const float* head_dev, int n, int gh, int gw, int ld, float scale, float threshold, float* boxes_dev,
                      float* scores_dev, void* stream);
int dif_mtcnn_gather(const int32_t* keep_dev, int n, int k, const float* src_boxes_dev, const float* src_scores_dev,
                     const float* src_reg_dev, int src_reg_ld, int n_src, float* dst_boxes_dev, float* dst_scores_dev,
                     float* dst_reg_dev, int n_dst, int dst_offset, int calibrate, void* stream);
int dif_mtcnn_rescore(const float* out_dev, int slots, int ld, float threshold, float* scores_dev, float* reg_dev,
                      float* boxes_dev, int plain_regression, void* stream);
int dif_crop_resize_multi(const uint8_t* frames_dev, int n, int h, int w, const float* boxes_ltrb_dev, const float* valid_dev,
                          int k, float margin, uint8_t* out_dev, int size, void* stream);

/* ------------------------------------------------------------------ five-point landmark alignment (csrc/align.hip)
 * O-Net's landmarks -> similarity transform onto the ArcFace five-point template -> aligned crop, on the device.  The
 * reference aligns on the host (api.py:132-145: cv2.getAffineTransform + cv2.warpAffine).  PARITY WITH cv2.warpAffine IS
 * UNPINNED: cv2 quantises coordinates to 1/32 pixel and weighs in 15-bit fixed point; what is pinned (and tested bit for
 * bit against a NumPy restatement) is this float32 arithmetic, without fused multiply-add:
 *   sx = (m00 x + m01 y) + m02, sy = (m10 x + m11 y) + m12;  x0 = floor(sx), fx = sx - x0 (y likewise);
 *   taps p00 = pix(x0, y0), p01 = pix(x0 + 1, y0), p10 = pix(x0, y0 + 1), p11 = pix(x0 + 1, y0 + 1) as float;
 *   top = p00 + (p01 - p00) fx, bot = p10 + (p11 - p10) fx, v = top + (bot - top) fy, out = min(max(floor(v + 0.5), 0), 255).
 * Matrix direction: DESTINATION -> SOURCE, a row-major 2 x 3 matrix [m00 m01 m02 m10 m11 m12] takes an output pixel index
 *   (x, y) to a frame position (cv2.warpAffine with WARP_INVERSE_MAP, or the inverse of the matrix cv2 is usually given).
 * Pixel convention: integer pixel indices are the sample positions (cv2's), no half-pixel offset.
 * Border: constant zero -- a tap outside the frame contributes 0.0; a pixel whose 2 x 2 footprint lies wholly outside the
 *   frame, or whose sx / sy is not finite, is 0.
 * NaN rule: a crop whose matrix holds a NaN (or an infinity) is black.
 *
 * dif_warp_affine: frames_dev uint8 [n_frames][h][w][3]; matrices_dev float [n_frames * k][6]; k crops per frame -- crop j
 *   reads frame j / k; out_dev uint8 [n_frames * k][out_h][out_w][3].
 * dif_align_crop: the matrix of each crop is fitted in the same launch from its five landmarks (landmarks_dev float
 *   [n_frames * k][5][2], (x, y) in frame pixels) and five template points in output pixels (template_host: 10 floats ON
 *   THE HOST, x0 y0 ... x4 y4; NULL = the standard ArcFace 112 x 112 template (38.2946, 51.6963), (73.5318, 51.5014),
 *   (56.0252, 71.7366), (41.5493, 92.3655), (70.7299, 92.2041) times size / 112): the least-squares similarity (rotation,
 *   uniform scale, translation, no reflection -- Umeyama in 2-D, closed form) landmarks -> template, inverted.  valid_dev
 *   float [n_frames * k] or NULL: a negative value marks an empty slot.  The crop is black and its matrix six NaNs when the
 *   slot is empty, a landmark is not finite, or the landmarks / the template coincide in one point.  out_dev uint8
 *   [n_frames * k][size][size][3]; matrices_out_dev float [n_frames * k][6] or NULL: the matrices used (direction as above).
 * dif_mtcnn_landmarks: the landmarks of the cascade's output slots.  out_dev: O-Net's outputs [n * n_src][ld], ld >= 16
 *   (logits 2 | box 4 | landmark x 5 | landmark y 5: left eye, right eye, nose, left and right mouth corner, relative to
 *   the crop the network saw); boxes_dev [n][n_src][4]: the slots' boxes as dif_crop_resize_multi was given them, i.e.
 *   BEFORE dif_mtcnn_rescore(plain_regression = 1) regresses them in place; keep_dev [n][k]: the last dif_nms's kept slots
 *   (< 0 = empty -> ten zeros); h, w: the frame's size.  landmarks_dev [n][k][5][2] = (l + ox cw, t + oy ch) where
 *   (l, t, cw, ch) is the rectangle clamped to the frame and truncated that the crop was cut from -- the library's
 *   deviation from the published code, which refers to the unclamped box and zero-pads. */
int dif_warp_affine(const uint8_t* frames_dev, int n_frames, int h, int w, const float* matrices_dev, int k, uint8_t* out_dev,
                    int out_h, int out_w, void* stream);
int dif_align_crop(const uint8_t* frames_dev, int n_frames, int h, int w, const float* landmarks_dev, const float* valid_dev, int k,
                   const float* template_host, uint8_t* out_dev, int size, float* matrices_out_dev, void* stream);
int dif_mtcnn_landmarks(const float* out_dev, int ld, const float* boxes_dev, const int32_t* keep_dev, int n, int n_src, int k, int h,
                        int w, float* landmarks_dev, void* stream);

/* ------------------------------------------------------------------ every face in a frame (csrc/faces.hip)
 * The detectors fill a fixed number of slots per frame (k; score -1 = an empty slot).  These entry points turn the slots
 * of a batch into one dense list of faces, so that the crop, the embedder and the match run on the M faces that are
 * there and not on n * k slots (deep_insight_face.detector.faces: gather_faces, FramePipeline.faces,
 * MtcnnFramePipeline.faces).  The reference's counterpart is detect_multiple_faces (detector/run.py:63-87), per image
 * on the host.
 * dif_faces_compact: scores_dev float [n][k] -> the slots with score >= min_score (inclusive; a NaN score is no face).
 *   ORDER: frame-major, and inside a frame in slot order -- the detector's pick order, best score first -- so the list
 *   is deterministic (one block scans the slots; no atomics).  offsets_dev int32 [n + 1]: exclusive prefix sum of the
 *   faces per frame (CSR: the faces of frame f are entries offsets[f] .. offsets[f + 1] - 1), never truncated;
 *   count_dev int32 [1] = offsets[n], the exact total; frame_dev / slot_dev int32 [max_faces]: frame and slot of the
 *   first max_faces faces, the entries after them -1 (both may be NULL when max_faces = 0).  n = 0 writes count = 0 and
 *   offsets[0] = 0 (scores_dev may be NULL).  Nothing comes back to the host: a caller that sizes its buffers by the
 *   total reads count_dev once (4 bytes, ONE synchronisation per batch -- the only one of the path); a caller that
 *   cannot wait passes max_faces = n * k buffers and runs the list forms below over all of them (-1 entries are inert).
 *   k < 1, max_faces < 0, n * k >= 2^31 - 1024 or a NULL pointer fail.
 * In the list forms below, frame_dev / slot_dev int32 [m] name one slot per output row; an entry outside [0, n) x
 *   [0, k) (-1 by convention) reads nothing.  m = 0 is a no-op.
 * dif_crop_resize_list: out_dev uint8 [m][size][size][3]; crop j is bit-identical to crop frame[j] * k + slot[j] of
 *   dif_crop_resize_multi(frames, n, h, w, boxes [n][k][4], NULL, k, margin, ...); a -1 entry gives a black crop.
 * dif_align_crop_list: crop j and matrix j (matrices_out_dev float [m][6] or NULL) are bit-identical to those of slot
 *   frame[j] * k + slot[j] of dif_align_crop(frames, n, h, w, landmarks [n][k][5][2], NULL, k, template_host, ...); a
 *   -1 entry gives a black crop and six NaNs.
 * dif_faces_gather: dst_dev float [m][row_floats] <- row frame[j] * k + slot[j] of src_dev float [n][k][row_floats]
 *   (boxes: 4, scores: 1, landmarks: 10); a -1 entry gives zeros. */
int dif_faces_compact(const float* scores_dev, int n, int k, float min_score, int max_faces, int32_t* count_dev, int32_t* offsets_dev,
                      int32_t* frame_dev, int32_t* slot_dev, void* stream);
int dif_crop_resize_list(const uint8_t* frames_dev, int n, int h, int w, const float* boxes_ltrb_dev, int k, const int32_t* frame_dev,
                         const int32_t* slot_dev, int m, float margin, uint8_t* out_dev, int size, void* stream);
int dif_align_crop_list(const uint8_t* frames_dev, int n, int h, int w, const float* landmarks_dev, int k, const int32_t* frame_dev,
                        const int32_t* slot_dev, int m, const float* template_host, uint8_t* out_dev, int size, float* matrices_out_dev,
                        void* stream);
int dif_faces_gather(const float* src_dev, int row_floats, int n, int k, const int32_t* frame_dev, const int32_t* slot_dev, int m,
                     float* dst_dev, void* stream);

/* ------------------------------------------------------------------ gallery + 1:N match
 * The reference has no 1:N entry point; the semantics are utility.distance broadcast
 * over gallery rows + np.argmin (first minimum).  Housed Python-side under
 * deep_insight_face.oneshot (north_star). */
int dif_gallery_create(dif_gallery** out, int d);
int dif_gallery_destroy(dif_gallery* g);
/* copy `n` rows of `d` floats from device memory into the handle and precompute the
 * per-row norms; index_base = global index of row 0 (gallery row-sharded over ranks) */
int dif_gallery_set(dif_gallery* g, const float* rows_dev, int64_t n, int64_t index_base, void* stream);
int64_t dif_gallery_size(const dif_gallery* g);
/* incremental enrolment (no reference counterpart: the reference keeps its "database" as a Python dict of encodings,
 * predictions.py:98-126 `verify(image, identity, database, ...)`, and re-reads it per call).
 * dif_gallery_update: overwrite rows [first_row, first_row + n) with `n` rows from device memory, or append them
 *   (first_row == dif_gallery_size; first_row beyond it would leave a gap and fails); the rows must fit the
 *   capacity.  Costs O(n): only those rows' norms and filter copy are recomputed (dif_gallery_set is one pass over
 *   the whole gallery).  The match results are exactly those of a dif_gallery_set with the resulting rows.
 * dif_gallery_reserve: grow the capacity (rows are kept; never shrinks); dif_gallery_set sizes it to its `n`.
 * dif_gallery_capacity: rows the handle can hold without reallocating. */
int dif_gallery_update(dif_gallery* g, const float* rows_dev, int64_t n, int64_t first_row, void* stream);
/* dif_gallery_remove: un-enrol the `k` rows listed in rows_dev (device memory: GLOBAL indices, index_base included, strictly
 *   ascending, every one inside [index_base, index_base + dif_gallery_size)).  Swap-remove: the size drops to new_n = size - k;
 *   rows below new_n that are not listed keep their indices, the listed ones below new_n are holes, and the i-th surviving row of
 *   the tail [new_n, size) moves into the i-th hole (both ascending).  The moves are reported so the caller can fix its name
 *   table: moved_from_dev[i] -> moved_to_dev[i] (global indices, device memory, `k` slots each or NULL), i < *n_moved_out <= k
 *   (host; may be NULL); slots beyond hold -1, as dif_match_within's unused list slots do.  Afterwards every answer of dif_match /
 *   dif_match_within / dif_match_rank is exactly that of a dif_gallery_set with the resulting rows; the capacity stays.
 *   Costs O(k), no pass over the gallery (unless a listed or moved row was one the filter cannot rank: then the special-row lists
 *   are rebuilt as after dif_gallery_update, 8 bytes per row read).  The filter's copy is moved with the rows, not recomputed.
 *   The vacated slots [new_n, size) are overwritten with zeros in every device form of the rows: a removed template does not stay in
 *   device memory.  The call SYNCHRONISES the stream (it reads the number of moves, and the input's validity, before it touches
 *   the gallery): an unsorted, duplicated or out-of-range list fails and leaves the gallery as it was. */
int dif_gallery_remove(dif_gallery* g, const int64_t* rows_dev, int64_t k, int64_t* moved_from_dev, int64_t* moved_to_dev,
                       int64_t* n_moved_out, void* stream);
int dif_gallery_reserve(dif_gallery* g, int64_t capacity, void* stream);
int64_t dif_gallery_capacity(const dif_gallery* g);
/* options.  "filter": what the MFMA stage of dif_match -- a candidate filter with a proven error bound; the winner
 * is chosen on the reference's own float32 arithmetic whatever it is -- runs on.  2 (default): the gallery rows and the
 * probes rounded to bf16 once (one bf16 MFMA per 16 k; bound ~0.008 |q|: a few rows per probe re-ranked; the copy
 * costs d * 2 bytes per row); 1: two-term split-bf16 copies (three MFMAs per 16 k; bound 1.6e-4 |q|; d * 4 bytes per
 * row); 0: the f32 MFMA on the rows themselves (no copy).  Results are identical.  Embedding sizes that are not
 * multiples of 64, or below 128, take the two-term form under 2 as well.  The copy is built by dif_gallery_set, or by
 * the first dif_match after the option changed; changing it frees the copy the new filter does not read (in either
 * order with dif_gallery_set); when a copy cannot be allocated the f32 filter serves and nothing fails
 * (dif_gallery_get_stat "split_copy" / "filter_terms" tell).
 * "frag": 1 (default) the one-term copy ("filter" = 2) is kept in MFMA-fragment order and the filter runs on
 * match_g1_kernel (the probes resident in LDS, the gallery streamed once from HBM straight into the MFMA operand
 * registers) where the embedding size is a multiple of 128 up to 512 and the gallery holds at least 2^18 rows (below,
 * that kernel's waves would not get a tile each); 2: whatever the row count; 0: row-major, match_b1_kernel.  Same
 * answers, same bytes per row; the copy is rewritten in the other layout by the next dif_match / dif_gallery_set
 * (also when dif_gallery_update takes the row count across the threshold).
 * "clamp_nan": 0 (default) dif_match reports NaN where the reference's distance is NaN; 1 reports the
 * distance of the similarity clamped to [-1, 1] instead (0 for a similarity rounded above 1, 1 below -1).  The
 * arg-min is the reference's either way.
 * "bd": 1 (default) the two-term filter ("filter" = 1) runs on match_bd_kernel from 65 probes up; 0 keeps it on
 * match_tile_kernel for every batch (tests, A/B).  Same answers.
 * "bd_fill": 1 (default) .. 16: blocks of match_bd_kernel per resident slot (development; no effect measured).
 * "topk_seed": 0 (default) the seed stage of dif_match_topk evaluates the k gallery tiles with the smallest search keys
 * per probe; n > 0 makes it n tiles (1: a loose first tolerance, the sweep stage does the work).  Same answers for every
 * value (tests, A/B).  dif_match_topk_ids starts its growing seed at the same number.
 * "cluster_round": 0 (default) dif_gallery_cluster (and each sweep of dif_gallery_dbscan) takes a sixteenth of the rows as the probes of one round, in whole blocks
 * of 128 and at least 2048 (a round's MFMA pass stops at its last probe's row: sixteen rounds do 17 / 32 of the square, one
 * round all of it); n > 0, a multiple of 128, makes it n probes.  Either way at most what the census workspace allows (2^27
 * words / the number of 128-row tiles).  Same answers for every value (tests: several rounds on a small gallery).
 * "roc_round": 0 (default) dif_match_roc takes as many probes per round as its mask workspace allows (2^24 masks of 16 bytes /
 * the number of 128-row tiles, in whole blocks of 128, at least 128); n > 0, a multiple of 128, makes it n probes when that is
 * fewer.  Same answers for every value (tests: several rounds at a small shape).
 * "within_round": 0 (default) dif_match_within, dif_match_rank, dif_match_rank_at and their tagged forms take as many probes per round as the census
 * workspace allows (2^27 words / the number of 128-row tiles, in whole blocks of 128, at least 128); n > 0, a multiple of 128,
 * makes it n probes when that is fewer.  Same answers for every value (tests: several rounds at a small shape).
 * "topk_round": 0 (default) dif_match_topk, dif_match_topk_ids and their tagged forms take as many probes per round as the
 * tile-word workspace allows (2^26 floats / the number of 128-row tiles, in whole blocks of 128, at least 128); n > 0, a multiple
 * of 128, makes it n probes when that is fewer.  Same answers for every value (tests: several rounds at a small shape).
 * "roc_blocks": 0 (default) the resolve stage of dif_match_roc launches at most 2048 blocks, each taking 512 masks per trip;
 * n in 1 .. 65536 makes it at most n.  Same answers for every value (tests: one block that takes many trips at a small shape).
 * Every key the library accepts is listed here (dif_gallery_option_name; tests/test_cabi_symbols.py). */
int dif_gallery_set_option(dif_gallery* g, const char* key, int value);
/* read-outs (no reference counterpart; for capacity planning and tests).  "split_copy": 1 when the filter's bf16 copy
 * of the current rows exists; "filter_terms": bf16 terms per operand the next dif_match's filter runs on (1 or 2; 0 = the f32 rows);
 * "frag_copy": 1 when that copy is held in MFMA-fragment order (gallery option "frag");
 * "row_bytes": device bytes held per gallery row; "exact_probes": how many probes the
 * last dif_match on `stream` sent to the exact whole-gallery search (synchronises the stream); "roc_resolved": how many pairs the
 * last dif_match_roc on `stream` evaluated one by one, being too close to a threshold to call (synchronises the stream);
 * "topk_ids_tiles": how many (probe, 128-row tile) pairs the last dif_match_topk_ids on `stream` evaluated row by row, over
 * all its probes (synchronises the stream); "topk_tagged_tiles": the same count for the last dif_match_topk_tagged or
 * dif_match_topk_ids_tagged on `stream` -- a tile without a row eligible for the probe is never among them, so with few rows
 * eligible it is about the number of tiles that hold one (synchronises the stream; 0 before the first tagged call);
 * "within_tagged_tiles": the same count for the last dif_match_within_tagged, dif_match_rank_tagged or
 * dif_match_rank_at_tagged on `stream`: the (probe, 128-row tile) pairs evaluated row by row -- a tile without an eligible row
 * that could be a hit (resp. closer or tied) is never among them, whatever the probe (synchronises the stream; 0 before the
 * first such call). */
int dif_gallery_get_stat(dif_gallery* g, const char* key, int64_t* out, void* stream);
/* top-1 search of n probes [n][d]: idx_out_dev[n] = np.argmin over the reference's float32 distances
 * (int64 global index; first minimum; a row whose reference distance is NaN ranks first, as in
 * np.argmin: a similarity rounded beyond +-1, a zero-norm or non-finite gallery row or probe --
 * utility.py:58-62 guards none of them), dist_out_dev[n] = that row's distance (NaN where the
 * reference's is NaN unless "clamp_nan" is set), key_out_dev[n] (optional, may be NULL) = the ranking
 * key: the reference distance itself, -inf for NaN; comparable across gallery shards. */
int dif_match(dif_gallery* g, const float* probes_dev, int n, int metric, int64_t* idx_out_dev,
              float* dist_out_dev, float* key_out_dev, void* stream);
/* range search of n probes [n][d]: every enrolled row within `tolerance` of each probe, exact.  Per probe q
 *     dist  = utility.distance(q[None, :], gallery, metric)        the reference's float32 values
 *     hits  = np.flatnonzero(dist <= tolerance)                    inclusive; NaN <= t is False: a NaN distance is never a hit
 *     count_out_dev[p] = len(hits)                                 exact, however large
 *     idx_out_dev[p][0 .. K)  = hits[:K] + index_base              the K = max_hits LOWEST rows, ascending (dif_gallery_set's
 *     dist_out_dev[p][0 .. K) = dist[hits[:K]]                     index_base: global indices, so shard lists concatenate in rank order)
 *   unused slots hold idx -1 and dist NaN.  max_hits in [0, DIF_WITHIN_MAX_HITS]; with 0 only the counts are produced and the
 *   two list pointers may be NULL.  An empty gallery gives counts of 0 (not an error); n = 0 is a no-op; a NaN tolerance, a
 *   max_hits outside the range or a metric other than 0 / 1 fails.
 * Units: the tolerance is in the units of utility.distance -- metric 0 is the SQUARED L2 distance (a face_distance tolerance
 *   of 0.6 is 0.36 here), metric 1 is arccos(similarity) / pi in [0, 1].
 * The distance compared and reported is exactly the one dif_match / dif_pairwise report for that pair: metric 0 bit-identical
 *   to the reference; metric 1 up to the arccos (evaluated in double and rounded once; NumPy's float32 arccos is within 2 ulp),
 *   so against NumPy a pair whose distance lies within ~2e-6 of the tolerance may fall on the other side.
 * NaN rule: with "clamp_nan" 0 (default) a similarity that rounding pushes beyond +-1 is NaN in the reference and NOT a hit --
 *   that includes a probe identical to an enrolled row whose similarity rounds above 1; with "clamp_nan" 1 the clamped distance
 *   (0 or 1) is compared and reported.  Zero-norm and non-finite rows or probes follow the same rule: whatever IEEE arithmetic
 *   gives the reference, and NaN is never a hit.
 * Costs one pass of the f32 MFMA over the gallery (the stage of dif_match with "filter" = 0) plus the reference arithmetic on
 *   the 128-row tiles that hold a hit among the first max_hits or a row too close to the tolerance to call; no host
 *   synchronisation in steady state; its workspace (2 bytes per probe and 128 rows) is apart from dif_match's. */
#define DIF_WITHIN_MAX_HITS 8192
int dif_match_within(dif_gallery* g, const float* probes_dev, int n, int metric, float tolerance, int max_hits,
                     int64_t* count_out_dev /* [n] */, int64_t* idx_out_dev /* [n][max_hits], or NULL when max_hits == 0 */,
                     float* dist_out_dev /* same shape */, void* stream);
/* rank of the mate: where does one given enrolled row rank among ALL enrolled rows by distance to the probe?  The quantity
 * behind rank-k identification rates, the CMC curve and open-set DIR / FAR (deep_insight_face/evaluation/identification.py).
 * Per probe q with mate row m = mate_idx_dev[p] (int64 GLOBAL index: dif_gallery_set's index_base is subtracted):
 *     d  = utility.distance(q[None, :], gallery, metric)           the reference's float32 values
 *     dm = d[m - index_base]
 *     rank_out_dev[p]      = count(d < dm) + count(d[:m - index_base] == dm)     0-based; exact ties go to the lower index
 *     mate_dist_out_dev[p] = dm                                    (optional, may be NULL)
 *   For a row of distances without NaN this is the mate's position in np.argsort(d, kind='stable').  Rows of the mate's own
 *   identity count like any other row: with several rows per identity the caller passes the row they mean.
 *   Unmated probe -- m == -1 or anywhere outside [index_base, index_base + size): rank -1, mate_dist NaN, no gallery row is
 *   read for it.  An empty gallery makes every probe unmated.  n = 0 is a no-op; a metric other than 0 / 1 or a NULL
 *   handle, probes, mate_idx or rank_out fails.
 * Units: mate_dist is in the units of utility.distance -- metric 0 the SQUARED L2 distance, metric 1 arccos(similarity) / pi.
 * The distances compared are exactly the ones dif_match / dif_match_within / dif_pairwise report for the pair, under the
 *   handle's "clamp_nan": metric 0 bit-identical to the reference; metric 1 up to the arccos (evaluated in double and rounded
 *   once; NumPy's float32 arccos is within 2 ulp), so against NumPy a row whose distance lies within ~2e-6 of dm may fall on
 *   the other side of it.  mate_dist is bit-identical to dif_pairwise's value for (q, gallery[m]).
 * NaN rule: NaN compares False -- a row whose distance is NaN is never "closer" (dif_match_within's "NaN is never a hit").  A
 *   mate whose own distance is NaN (a similarity rounded beyond +-1 with "clamp_nan" 0, a zero-norm or non-finite row or probe)
 *   gives rank = dif_gallery_size ("behind every row": a miss at every k, distinct from unmated) and mate_dist NaN.
 * Relation to dif_match: where no distance of the probe's row is NaN, rank == 0 exactly when dif_match returns m.  They differ
 *   where there are NaNs: np.argmin ranks a NaN first, the rank never counts one.
 * Costs one pass of the f32 MFMA over the gallery (dif_match_within's census) plus the reference arithmetic on the 128-row
 *   tiles that hold a row too close to dm to call -- the mate's own tile is always one; no host synchronisation in steady state;
 *   shares dif_match_within's workspace (calls on one stream are ordered) plus 8 bytes per probe. */
int dif_match_rank(dif_gallery* g, const float* probes_dev, int n, int metric, const int64_t* mate_idx_dev /* [n] */,
                   int64_t* rank_out_dev /* [n] */, float* mate_dist_out_dev /* [n], may be NULL */, void* stream);
/* top-k search of n probes [n][d]: the k nearest enrolled rows of each probe, in order, exact.  Per probe q
 *     d     = utility.distance(q[None, :], gallery, metric)        the reference's float32 values
 *     order = np.argsort(d, kind='stable')                         ascending distance; exact ties go to the lower row
 *     keep  = order[~np.isnan(d[order])][:k]                       a NaN distance is never listed
 *     idx_out_dev[p][0 .. len(keep))  = keep + index_base          (dif_gallery_set's index_base: global indices)
 *     dist_out_dev[p][0 .. len(keep)) = d[keep]
 *   unused slots -- k above the row count, or fewer than k rows with a distance that is not NaN -- hold idx -1 and dist NaN;
 *   an empty gallery gives all padding (not an error).  k in [1, DIF_TOPK_MAX]; n = 0 is a no-op; a k outside the range, a
 *   metric other than 0 / 1 or a NULL handle, probes or output fails.
 * Units and arithmetic: as dif_match_within / dif_match_rank -- the distances ordered and reported are exactly the ones those
 *   (and dif_match, dif_pairwise) report for the pair under the handle's "clamp_nan": metric 0 bit-identical to the reference;
 *   metric 1 up to the arccos (evaluated in double and rounded once; NumPy's float32 arccos is within 2 ulp), so against NumPy
 *   two rows whose distances lie within ~2e-6 of each other may swap.  On the library's own distances the list is exact on
 *   both metrics: dif_match_rank of idx_out[p][j] returns (j, dist_out[p][j]).
 * NaN rule: a row whose distance is NaN is never listed (with "clamp_nan" 1 the clamped 0 / 1 is ordered and reported
 *   instead).  Where no distance of the probe is NaN, idx_out[p][0] is dif_match's row; they differ where there are NaNs.
 * Costs one pass of the f32 MFMA over the gallery (dif_match_within's, keeping one minimum key per 128-row tile and probe)
 *   plus the reference arithmetic on the tiles that can hold one of the k rows -- about k tiles per probe (option
 *   "topk_seed"); no host synchronisation in steady state; its workspace (4 bytes per probe and 128 rows) is its own. */
#define DIF_TOPK_MAX 128
int dif_match_topk(dif_gallery* g, const float* probes_dev, int n, int metric, int k, int64_t* idx_out_dev /* [n][k] */,
                   float* dist_out_dev /* [n][k] */, void* stream);
/* identity-level top-k search of n probes [n][d]: the k nearest distinct IDENTITIES of each probe, each with its best row, in
 * order, exact.  The gallery stores no labels: row_labels_dev [size] int64 holds them in local row order, as dif_match_roc
 * takes them; exclude_dev [n] int64 (optional, may be NULL) names one identity per probe to leave out.  Per probe q
 *     d     = utility.distance(q[None, :], gallery, metric)        the reference's float32 values
 *     ok    = ~np.isnan(d) & (row_labels >= 0) & (row_labels != exclude[p])
 *     order = np.argsort(d, kind='stable');  order = order[ok[order]]
 *     first = order[np.sort(np.unique(row_labels[order], return_index=True)[1])]    each identity's first, i.e. best, row;
 *     keep  = first[:k]                                                             exact ties go to the lower row
 *     idx_out_dev[p][0 .. len(keep))   = keep + index_base          (dif_gallery_set's index_base: global indices)
 *     dist_out_dev[p][0 .. len(keep))  = d[keep]
 *     label_out_dev[p][0 .. len(keep)) = row_labels[keep]           (optional, may be NULL)
 *   unused slots -- fewer than k identities with a usable row -- hold idx -1, dist NaN and label -1; an empty gallery gives all
 *   padding (not an error).  A negative row label takes the row out, as in dif_match_roc.  exclude_dev NULL, or a negative
 *   entry, excludes nothing; with the probe's own identity excluded the list holds the k nearest OTHER identities (k = 1: the
 *   hardest negative).  Labels are compared as full int64.  k in [1, DIF_TOPK_MAX]; n = 0 is a no-op; a k outside the range, a
 *   metric other than 0 / 1 or a NULL handle, probes, idx or dist output (or row labels with rows enrolled) fails.
 * Units, arithmetic, "clamp_nan" and the NaN rule: dif_match_topk's -- metric 0 bit-identical to the reference; metric 1 up to
 *   the arccos, so against NumPy two identities whose best distances lie within ~2e-6 of each other may swap, or an identity
 *   may be reported with another of its rows that close to its best.  On the library's own distances the list is exact on both
 *   metrics: dif_match_rank of idx_out[p][j] returns dist_out[p][j] as the mate's distance.
 * Relations: with all-distinct labels the result is dif_match_topk's, bit for bit; with one label the list has one entry,
 *   dif_match's row where no distance is NaN.
 * Costs dif_match_topk's MFMA pass, unchanged (a tile's minimum key is taken over all its rows, a lower bound of the minimum
 *   over the usable ones), plus the reference arithmetic on the tiles that can hold one of the k rows.  The seed stage grows:
 *   it starts with "topk_seed" tiles (0: k) and doubles while more tiles than that remain below the tolerance of the list so
 *   far, so a gallery with many rows per identity costs a few dozen tiles per probe, not hundreds.  Same answers for every
 *   "topk_seed".  dif_gallery_get_stat "topk_ids_tiles" counts the tiles evaluated.  No host synchronisation in steady state;
 *   shares dif_match_topk's workspace (calls on one stream are ordered) plus one 8-byte counter. */
int dif_match_topk_ids(dif_gallery* g, const float* probes_dev, int n, int metric, int k,
                       const int64_t* row_labels_dev /* [size] */, const int64_t* exclude_dev /* [n], or NULL */,
                       int64_t* idx_out_dev /* [n][k] */, float* dist_out_dev /* [n][k] */,
                       int64_t* label_out_dev /* [n][k], or NULL */, void* stream);
/* watch-lists: dif_match_topk and dif_match_topk_ids over the rows each probe is allowed to see.  The gallery stores no tags:
 * row_tags_dev [size] int64 holds one 64-bit set per enrolled row in local row order (as row_labels_dev is kept by the caller:
 * permute it by dif_gallery_remove's moves), probe_masks_dev [n] int64 one set per probe.
 *     eligible[p][r] = (row_tags[r] & probe_masks[p]) != 0         on the raw 64 bits: a negative value has bit 63 set
 *   A tag of 0 is never eligible; a mask of 0 gives all padding.  Per probe q
 *     d = utility.distance(q[None, :], gallery, metric);  d[~eligible[p]] = NaN
 *   and the result is dif_match_topk's for that d (dif_match_topk_tagged), or dif_match_topk_ids' with
 *   ok &= eligible[p] (dif_match_topk_ids_tagged): the same order (ties to the lower row), NaN rule, "clamp_nan", padding
 *   (-1 / NaN / label -1), index_base, k in [1, DIF_TOPK_MAX], units and arithmetic -- metric 0 bit-identical to the reference,
 *   metric 1 up to the arccos.  An ineligible row is never listed, however many of them are nearer than the first eligible one.
 *   n = 0 is a no-op; an empty gallery gives all padding (not an error) and reads neither array; with rows enrolled a NULL
 *   row_tags_dev or probe_masks_dev fails, as do dif_match_topk's / dif_match_topk_ids' own argument errors.
 * Relations: with every (row, probe) pair eligible -- all tags and masks -1, say -- the results are the untagged calls', bit for
 *   bit; the tagged list of a probe equals the untagged list over a gallery of its eligible rows alone, indices mapped back.
 * Costs the untagged call's MFMA pass with 8 more bytes read per row: the tile word is the minimum key over the tile's
 *   ELIGIBLE rows, and a tile with no eligible row for the probe is marked and never evaluated row by row, whatever the
 *   tolerance -- so a selective mask makes the call cheaper, not dearer.  Within an evaluated tile an ineligible row is skipped
 *   before any arithmetic.  dif_gallery_get_stat "topk_tagged_tiles" counts the tiles evaluated.  No host synchronisation in
 *   steady state; shares dif_match_topk's workspace (calls on one stream are ordered) plus one 8-byte counter.  The untagged
 *   entries run the kernels they ran before. */
int dif_match_topk_tagged(dif_gallery* g, const float* probes_dev, int n, int metric, int k,
                          const int64_t* row_tags_dev /* [size] */, const int64_t* probe_masks_dev /* [n] */,
                          int64_t* idx_out_dev /* [n][k] */, float* dist_out_dev /* [n][k] */, void* stream);
int dif_match_topk_ids_tagged(dif_gallery* g, const float* probes_dev, int n, int metric, int k,
                              const int64_t* row_labels_dev /* [size] */, const int64_t* exclude_dev /* [n], or NULL */,
                              const int64_t* row_tags_dev /* [size] */, const int64_t* probe_masks_dev /* [n] */,
                              int64_t* idx_out_dev /* [n][k] */, float* dist_out_dev /* [n][k] */,
                              int64_t* label_out_dev /* [n][k], or NULL */, void* stream);
/* which enrolled rows are the same person: exact single-linkage clustering of the gallery's own rows at a tolerance, i.e. the
 * connected components of the graph whose edges are the pairs of rows within `tolerance`.  With n = dif_gallery_size:
 *     for i in range(n):                                            every enrolled row is a probe
 *         d = utility.distance(rows[i][None, :], rows[:i + 1], metric)      the reference's float32 values, rows 0..i only
 *         for j in np.flatnonzero(d <= tolerance): unite(i, j)      inclusive; NaN <= t is False
 *     labels_out_dev[i] = index_base + the smallest row number of i's component;  n_clusters_dev[0] = number of components
 *   Only the lower triangle is evaluated (row i as the probe, row j <= i as the enrolled row): the reference's arithmetic is
 *   symmetric in its two arguments, and stated this way the result does not depend on it.  A label is the smallest row of its
 *   component, so the result is canonical: it depends neither on thread order nor on the order in which edges are found, and
 *   two calls give identical arrays.  A row whose distance to every other row is NaN or above the tolerance is a component of
 *   its own (label = its own row): a zero-norm or non-finite row under metric 1, for instance.
 * Units, arithmetic and NaN rule: dif_match_within's, under the handle's "clamp_nan".  tolerance < 0 gives n singletons; under
 *   metric 1 a tolerance >= 1 joins every pair whose distance is not NaN.  With "clamp_nan" 0 two IDENTICAL rows whose
 *   similarity rounds above 1 are NOT joined under metric 1 (their distance is NaN): de-duplicating exact copies under
 *   metric 1 wants "clamp_nan" 1.  Metric 1 pairs within ~2e-6 of the tolerance may differ from NumPy's (the arccos).
 * Incremental form (enrolment): first_row = r > 0 and labels_in_dev = the labels_out of a call over rows [0, r) with the same
 *   tolerance, metric and index_base.  The union-find starts from those labels, only rows [r, n) are probes (each against
 *   rows[:i + 1]) and the result equals the full call's at O((n - r) n) cost.  first_row = n copies the labels.  After
 *   dif_gallery_remove row numbers have moved and earlier labels are void: run the full call.  labels_in_dev may alias
 *   labels_out_dev.  A labels_in entry outside [index_base, index_base + its own row] cannot come from such a call; it is
 *   detected on the device, without a host read: n_clusters_dev[0] = -1 then, and labels_out holds no meaning.
 * An empty gallery writes n_clusters = 0.  A metric other than 0 / 1, a NaN tolerance, an embedding size that is not a
 *   multiple of 32, first_row outside [0, n], labels_in_dev NULL with first_row > 0, or a NULL handle or output fails.
 * Costs the lower triangle of dif_match_within's f32 MFMA pass (half the work of running every row as its probe) plus the
 *   reference arithmetic on the 128-row tiles that hold a row within, or too close to, the tolerance; nothing of size n x n
 *   is kept; no host synchronisation in steady state.  Workspace: dif_match_within's (shared; calls on one stream are
 *   ordered) plus 4 bytes per row.  Probes go in rounds (gallery option "cluster_round"). */
int dif_gallery_cluster(dif_gallery* g, int metric, float tolerance, int64_t first_row,
                        const int64_t* labels_in_dev /* [first_row], or NULL when first_row == 0 */,
                        int64_t* labels_out_dev /* [n] */, int64_t* n_clusters_dev /* [1] */, void* stream);
/* density clustering with noise (DBSCAN) of the gallery's own rows, exact, on the edges of dif_gallery_cluster: a row is the
 * core of a person only if at least min_samples rows, itself included, lie within `tolerance`; clusters grow through cores
 * only; a row that is no core but has one within the tolerance (a border row) joins that core's cluster and spreads it no
 * further, so it cannot bridge two people; every other row is noise.  With n = dif_gallery_size:
 *     E = {(i, j) : j < i and utility.distance(rows[i][None, :], rows[j][None, :], metric) <= tolerance}
 *                                                    row i is the probe; the reference's float32 values; inclusive;
 *                                                    NaN <= t is False; self pairs are not edges
 *     degree[i] = 1 + number of edges of E that contain i           the row itself always counts, whatever distance(i, i) is
 *     core[i]   = degree[i] >= min_samples
 *     clusters  = connected components of the graph (core rows, edges of E with both ends core)
 *     label[c]  = index_base + smallest row of c's component         for a core row c
 *     label[b]  = label[a(b)]                                        for a row b that is no core and has a core neighbour:
 *                                                    a(b) = the core neighbour with the smallest float32 distance, the value
 *                                                    of the edge as E evaluated it; exact ties go to the lower row number
 *     label[x]  = -1                                                 for every other row (noise), whatever index_base is
 *     counts_dev[0] = number of clusters;  counts_dev[1] = number of noise rows
 *   labels_out_dev[i] = label[i];  degree_out_dev[i] = degree[i] when the pointer is not NULL.
 *   The result is a function of the edge set and its distance values alone: degrees are integer sums, a cluster's label is
 *   its smallest core row, and a border row's cluster is a minimum over (distance, row) -- none depends on thread order or on
 *   the order in which edges are found; two calls, or other round sizes, give identical arrays.  min_samples = 1 gives
 *   dif_gallery_cluster's labels bit for bit and no noise; min_samples > n gives n noise rows and no cluster; tolerance < 0
 *   gives degree 1 everywhere.
 * Units, arithmetic and NaN rule: dif_gallery_cluster's (dif_match_within's), under the handle's "clamp_nan".
 * There is no incremental form: a new row changes the degrees of the rows already enrolled, and with them which rows are core.
 * An empty gallery writes counts = {0, 0}.  Fails where dif_gallery_cluster fails -- a metric other than 0 / 1, a NaN
 *   tolerance, an embedding size that is not a multiple of 32, a NULL handle, labels or counts -- and for min_samples < 1.
 * Costs two sweeps of dif_gallery_cluster's lower triangle -- degrees first, links second; the second keeps the first one's
 *   census when one round covers the gallery -- i.e. about twice dif_gallery_cluster; nothing of size n x n is kept; no host
 *   synchronisation in steady state.  Workspace: dif_gallery_cluster's (shared; calls on one stream are ordered) plus 12 bytes
 *   per row.  Probes go in rounds (gallery option "cluster_round"). */
int dif_gallery_dbscan(dif_gallery* g, int metric, float tolerance, int min_samples, int64_t* labels_out_dev /* [n] */,
                       int32_t* degree_out_dev /* [n], or NULL */, int64_t* counts_dev /* [2]: clusters, noise */,
                       void* stream);
/* all-pairs verification counts at every threshold, exact: how many genuine (equal labels) and impostor (different labels) pairs
 * of (probe, enrolled row) have a distance below each of T thresholds -- the numerators and denominators of TAR / VAL and FAR
 * over EVERY pair (deep_insight_face/evaluation/verification.py), where utility.calculate_val_far sees a list of pairs.
 * Per call, with B = n probes and G = dif_gallery_size rows:
 *     dist  = utility.distance(q[:, None], gallery[None, :], metric)    the reference's float32 values, B x G, never materialised
 *     use   = (probe_labels[:, None] >= 0) & (row_labels[None, :] >= 0) & (arange(G)[None, :] + index_base >= first_row[:, None])
 *     same  = probe_labels[:, None] == row_labels[None, :]
 *     accept_out_dev[j][0] = sum(use &  same & (dist < thresholds[j]))  np.less, as calculate_val_far: STRICT; NaN < t is False
 *     accept_out_dev[j][1] = sum(use & ~same & (dist < thresholds[j]))
 *     totals_out_dev = [sum(use & same), sum(use & ~same), sum(use & same & isnan(dist)), sum(use & ~same & isnan(dist))]
 * Inputs: probe_labels_dev int64 [n]; row_labels_dev int64 [G] in LOCAL row order -- the caller owns the labels as it owns the
 *   name table dif_gallery_remove reports moves for; the handle stores none.  A negative label takes that probe or row out of
 *   every pair.  first_row_dev int64 [n], or NULL for all zeros, is compared with the GLOBAL row index (index_base included): a
 *   labelled set evaluated against itself passes own row + 1 and gets every unordered pair once and no row with itself.
 * Outputs are int64, on the device, and are not read back by the call: accept [n_thresholds][2], totals [4].
 * Thresholds: float32 [n_thresholds] on the device, NON-DECREASING, 1 <= n_thresholds <= DIF_ROC_MAX_THRESHOLDS.  Duplicates,
 *   values <= 0 (accept nothing; so does -inf), values > 1 and +inf (accepts every distance that is neither NaN nor +inf itself) are allowed.  A NaN
 *   threshold, a decreasing pair or an n_thresholds outside the range fails with an error string: the thresholds are the one
 *   thing the call copies to the host (at most 4 KB), so it synchronises the stream once, before anything is
 *   launched.  For that reason the call CANNOT be recorded under stream capture (hipGraph, torch.cuda.graph), unlike the other
 *   searches of the gallery.
 *   A float64 threshold t of the reference (np.arange) compares with a float32 distance as the smallest float32 >= t does:
 *   convert with that rule, not by rounding to nearest (oneshot.Gallery.roc does).
 * Strictness: dist < t is dist <= nextafterf(t, -inf), the device dif_match_rank uses.
 * Units, arithmetic and NaN rule: dif_match_within's, under the handle's "clamp_nan" -- metric 0 bit-identical to the
 *   reference; metric 1 up to the arccos (evaluated in double and rounded once), so against NumPy a pair within ~2e-6 of a
 *   threshold may fall on its other side.  The counts are exact on the distances dif_pairwise / dif_match_within report.
 * An empty gallery gives zeros; n = 0 launches no search and still zeroes the outputs.
 * Costs ONE pass of the f32 MFMA over the gallery per round of probes whatever n_thresholds is (dif_match_within's main loop,
 *   tiles and key; each key is binned by a binary search of an LDS table) plus the reference arithmetic on exactly the pairs
 *   too close to a threshold to call, one by one.  Counts are integers throughout: two calls give identical arrays.  Workspace,
 *   its own: 16 bytes per probe and 128 rows (gallery option "roc_round").  The counts of row shards add. */
#define DIF_ROC_MAX_THRESHOLDS 1024
int dif_match_roc(dif_gallery* g, const float* probes_dev, int n, int metric, const int64_t* probe_labels_dev /* [n] */,
                  const int64_t* row_labels_dev /* [size] */, const int64_t* first_row_dev /* [n], or NULL */,
                  const float* thresholds_dev /* [n_thresholds] */, int n_thresholds,
                  int64_t* accept_out_dev /* [n_thresholds][2] */, int64_t* totals_out_dev /* [4] */, void* stream);
/* merge R per-shard results laid out [R][n] (after an all-gather): lowest key, then
 * lowest global index -- equals np.argmin over the concatenated gallery */
int dif_match_merge(const float* keys_dev, const int64_t* idx_dev, const float* dist_dev, int R, int n,
                    int64_t* idx_out_dev, float* dist_out_dev, void* stream);
/* the same merge over ONE all-gathered buffer of R per-rank records, each n*16 bytes:
 * { float key[n]; float dist[n]; int64 idx[n]; } -- dif_match can write its three outputs straight
 * into a rank's record (key_out = rec, dist_out = rec + n floats, idx_out = rec + 2n floats), so the
 * N>1 step needs one collective for the partial results */
int dif_match_merge_packed(const void* packed_dev, int R, int n, int64_t* idx_out_dev, float* dist_out_dev,
                           void* stream);
/* ------------------------------------------------------------------ sharded gallery: the other queries (csrc/match_shard.hip)
 * A gallery row-sharded over R handles (dif_gallery_set's index_base; disjoint sets of global indices, in any order, not
 * necessarily contiguous) answers dif_match_topk, dif_match_topk_ids, dif_match_within, dif_match_rank and dif_match_roc
 * exactly as ONE handle holding all the rows would, bit for bit: every shard runs the local query on all n probes, the
 * per-shard results are laid out [R][n][...] (each rank's record contiguous: one all-gather per exchange) and merged by the
 * entries below.  All of them: 1 <= R <= DIF_SHARD_MAX; on the device, nothing read on the host, no atomics, deterministic;
 * n = 0 is a no-op; an R outside the range, a negative n or a NULL pointer fails.  dif_match_roc needs no entry: its int64
 * accept [T][2] and totals [4] of row shards add.  dif_gallery_cluster / dif_gallery_dbscan do not merge (their edges cross
 * shards).
 * dif_shard_merge_topk: R lists in dif_match_topk's order -- ascending (dist, idx), then -1 / NaN padding -- per probe
 *     live  = [(dist[r][p][j], idx[r][p][j]) for r, j if idx[r][p][j] >= 0]        a slot with idx < 0 is padding whatever
 *     keep  = sorted(live)[:k]                                                      its dist says
 *     idx_out_dev[p][0 .. len(keep)), dist_out_dev[p][0 .. len(keep)) = keep; the other slots idx -1, dist NaN
 *   Distances of live slots are >= +0 or +inf, never NaN (dif_match_topk lists none); their bit patterns are copied.  Equal to
 *   dif_match_topk over the whole gallery: a row among the k nearest of all rows is among the k nearest of its shard.
 *   k in [1, DIF_TOPK_MAX].  Costs R k binary searches of log k steps per list and probe: microseconds.
 * dif_shard_merge_topk_ids: the same with one entry per label: of sorted(live), an entry stays only if no earlier entry carries
 *   its label; the first k of those, then idx -1, dist NaN, label -1.  label_out_dev may be NULL.  Equal to dif_match_topk_ids
 *   over the whole gallery (every shard queried with the same exclude): an identity of the whole-gallery list has its best row in
 *   some shard, where fewer than k identities are ahead of it, so that shard lists it at its true distance; any other entry
 *   stands at a distance no better than its identity's true one and displaces nothing.  The lists are folded one at a time
 *   into a k-entry accumulator in LDS, which gives the same list (csrc/match_shard.hip has the argument).
 * dif_shard_merge_within: count_out_dev[p] = sum over r of count_dev[r][p]; the list is the max_hits LOWEST global indices of
 *   the union of the R lists (each ascending by index, padding behind), ascending, with their distances, then -1 / NaN -- for
 *   contiguous shards in rank order the concatenation.  max_hits in [0, DIF_WITHIN_MAX_HITS]; with 0 only the counts are
 *   produced and the four list pointers may be NULL.
 * dif_shard_merge_rank: consumes the per-shard outputs of dif_match_mate_dist and dif_match_rank_at (below).  Per probe:
 *     owner = the LOWEST r with owned_dev[r][p] != 0     (disjoint shards: at most one; overlapping shards are not allowed,
 *                                                          the rule only makes the kernel total)
 *     rank_out_dev[p]      = sum over r of count_dev[r][p], or -1 without an owner      (unmated, as dif_match_rank)
 *     mate_dist_out_dev[p] = mate_dist_dev[owner][p], or NaN without an owner           (optional, may be NULL)
 *   With count_dev all zeros it only selects the owner's distance: the step between the two local calls. */
#define DIF_SHARD_MAX 64
int dif_shard_merge_topk(const int64_t* idx_dev /* [R][n][k] */, const float* dist_dev /* [R][n][k] */, int R, int n, int k,
                         int64_t* idx_out_dev /* [n][k] */, float* dist_out_dev /* [n][k] */, void* stream);
int dif_shard_merge_topk_ids(const int64_t* idx_dev /* [R][n][k] */, const float* dist_dev /* [R][n][k] */,
                             const int64_t* label_dev /* [R][n][k] */, int R, int n, int k, int64_t* idx_out_dev /* [n][k] */,
                             float* dist_out_dev /* [n][k] */, int64_t* label_out_dev /* [n][k], or NULL */, void* stream);
int dif_shard_merge_within(const int64_t* count_dev /* [R][n] */, const int64_t* idx_dev /* [R][n][max_hits] */,
                           const float* dist_dev /* [R][n][max_hits] */, int R, int n, int max_hits,
                           int64_t* count_out_dev /* [n] */, int64_t* idx_out_dev /* [n][max_hits] */,
                           float* dist_out_dev /* [n][max_hits] */, void* stream);
int dif_shard_merge_rank(const int64_t* count_dev /* [R][n] */, const int64_t* owned_dev /* [R][n] */,
                         const float* mate_dist_dev /* [R][n] */, int R, int n, int64_t* rank_out_dev /* [n] */,
                         float* mate_dist_out_dev /* [n], or NULL */, void* stream);
/* rank against a mate the shard need not hold: dif_match_rank forms dm from its own row m; a shard without m is handed dm.
 * dif_match_mate_dist: only the mate's distance.  Per probe q with m = mate_idx_dev[p] (int64 GLOBAL index):
 *     owned_out_dev[p]     = 1 if index_base <= m < index_base + size else 0          (int64)
 *     mate_dist_out_dev[p] = utility.distance(q, gallery[m - index_base], metric) where owned, NaN where not
 *   bit-identical to dif_match_rank's mate_dist, under the handle's "clamp_nan"; it may be NaN where owned as well
 *   (dif_match_rank's NaN-mate case).  Costs O(n d): no census, no pass over the gallery.
 * dif_match_rank_at: the shard's share of the rank.  With d the shard's reference distances, dm = mate_dist_in_dev[p] and
 *   row the LOCAL row number:
 *     count_out_dev[p] = count(d < dm) + count((d == dm) & (index_base + row < m))    NaN compares False: never closer
 *   m is compared as a full int64 and may lie below, inside or above the shard (a mate of -1 or beyond every shard is
 *   legal here: "unmated" is decided by dif_shard_merge_rank, from owned).  dm NaN gives count = dif_gallery_size.  Summed over
 *   disjoint shards that is dif_match_rank's count(d < dm) + count(d[:m] == dm) over the whole gallery, and with dm NaN its size.
 *   The kernels, thresholds, arithmetic and cost are dif_match_rank's (the mate's distance is read, not computed; the tie
 *   test is on the global row); it shares that call's workspace (calls on one stream are ordered).  An empty shard gives 0.
 * n = 0 is a no-op; a metric other than 0 / 1 or a NULL handle or pointer fails. */
int dif_match_mate_dist(dif_gallery* g, const float* probes_dev, int n, int metric, const int64_t* mate_idx_dev /* [n] */,
                        float* mate_dist_out_dev /* [n] */, int64_t* owned_out_dev /* [n]: 0 / 1 */, void* stream);
int dif_match_rank_at(dif_gallery* g, const float* probes_dev, int n, int metric, const int64_t* mate_idx_dev /* [n] */,
                      const float* mate_dist_in_dev /* [n] */, int64_t* count_out_dev /* [n] */, void* stream);
/* watch-lists on the range search and the rank: dif_match_within, dif_match_rank and the two shard-local halves over the rows
 * each probe is allowed to see.  row_tags_dev [size] int64 and probe_masks_dev [n] int64 are dif_match_topk_tagged's: the
 * gallery stores no tags (keep them as row labels are kept, permuted by dif_gallery_remove's moves), and
 *     eligible[p][r] = (row_tags[r] & probe_masks[p]) != 0         on the raw 64 bits
 *   A tag of 0 is never eligible, a mask of 0 sees no row.  Per probe q
 *     d = utility.distance(q[None, :], gallery, metric);  d[~eligible[p]] = NaN
 *   and the result is the untagged call's for that d:
 * dif_match_within_tagged: hits = flatnonzero(d <= tolerance): an ineligible row is never counted and never listed -- the
 *   count and the max_hits lowest hits are those of the eligible rows, however many foreign rows precede them; a mask of 0
 *   gives count 0 and all padding.
 * dif_match_rank_tagged: the rank among the rows the probe may see, rank = count(d < dm) + count(d[:m] == dm): ineligible rows
 *   are never closer and never tie.  An INELIGIBLE mate is a mate whose distance is NaN: rank = dif_gallery_size ("behind every
 *   row", a miss at every k) and mate_dist NaN -- distinct from an unmated probe (rank -1).
 * dif_match_mate_dist_tagged: owned as before (the shard holds the row); the distance is NaN where the mate is not eligible.
 * dif_match_rank_at_tagged: the count over the shard's ELIGIBLE rows; dm NaN gives dif_gallery_size, as before.  The sums of
 *   dif_shard_merge_within / dif_shard_merge_rank are unchanged: counts over eligible rows add.
 * Everything else is the untagged calls': the inclusive <=, NaN never a hit, "clamp_nan", index_base, max_hits in
 *   [0, DIF_WITHIN_MAX_HITS], "within_round", metric 0 bit-identical to the reference, metric 1 up to the arccos.
 * n = 0 is a no-op; an empty gallery gives counts 0 / every probe unmated (rank_at: 0) and reads neither array; with rows
 *   enrolled a NULL row_tags_dev or probe_masks_dev fails, as do the untagged calls' own argument errors.
 * Relations: with every pair eligible (all tags and masks -1) the results are the untagged calls', bit for bit; the tagged
 *   answer of a probe equals the untagged answer over a gallery of its eligible rows alone, indices (and the mate's row) mapped.
 * Costs the untagged call's MFMA pass with 8 more bytes read per row: the census counts eligible rows only, so its 16-bit
 *   word is 0 exactly when the tile holds no eligible row that is SURE or not OUT, and such a tile is never evaluated row by
 *   row -- also for a probe outside the bound's validity, whose census counts every eligible row as borderline.  Within an
 *   evaluated tile an ineligible row is skipped before any arithmetic.  dif_gallery_get_stat "within_tagged_tiles" counts the
 *   tiles evaluated (dif_match_mate_dist_tagged evaluates none and leaves it alone).  No host synchronisation in steady state;
 *   shares the untagged calls' workspace plus one 8-byte counter.  The untagged entries run the kernels they ran before. */
int dif_match_within_tagged(dif_gallery* g, const float* probes_dev, int n, int metric, float tolerance, int max_hits,
                            const int64_t* row_tags_dev /* [size] */, const int64_t* probe_masks_dev /* [n] */,
                            int64_t* count_out_dev /* [n] */, int64_t* idx_out_dev /* [n][max_hits] */,
                            float* dist_out_dev /* [n][max_hits] */, void* stream);
int dif_match_rank_tagged(dif_gallery* g, const float* probes_dev, int n, int metric, const int64_t* mate_idx_dev /* [n] */,
                          const int64_t* row_tags_dev /* [size] */, const int64_t* probe_masks_dev /* [n] */,
                          int64_t* rank_out_dev /* [n] */, float* mate_dist_out_dev /* [n], or NULL */, void* stream);
int dif_match_mate_dist_tagged(dif_gallery* g, const float* probes_dev, int n, int metric,
                               const int64_t* mate_idx_dev /* [n] */, const int64_t* row_tags_dev /* [size] */,
                               const int64_t* probe_masks_dev /* [n] */, float* mate_dist_out_dev /* [n] */,
                               int64_t* owned_out_dev /* [n]: 0 / 1 */, void* stream);
int dif_match_rank_at_tagged(dif_gallery* g, const float* probes_dev, int n, int metric, const int64_t* mate_idx_dev /* [n] */,
                             const float* mate_dist_in_dev /* [n] */, const int64_t* row_tags_dev /* [size] */,
                             const int64_t* probe_masks_dev /* [n] */, int64_t* count_out_dev /* [n] */, void* stream);

/* ------------------------------------------------------------------ embedding network
 * Stands behind the Keras model object of the reference:
 *   bottleneck_network(net, emd_size, input_shape)(default_model_ver)   networks/triplet.py:73-85
 *   emd_model.predict_on_batch(x[N,H,W,3]) -> [N,emd]                    predictions.py:96,156; evaluation/evals.py:56
 * arch: "resnet" (keras ResNet50V2, triplet.py:90-91), "iresnet50", "iresnet100" (also "vgg16", "mobilenet", "nn4",
 *       "yolov3", "mtcnn_pnet" / "mtcnn_rnet" / "mtcnn_onet")
 * head: "v1" (triplet.py:102-117), "v2" (GDC + L2-norm, triplet.py:119-141),
 *       "v3" (bare backbone, triplet.py:143-146); ignored for iresnet*. */
int dif_net_create(dif_net** out, const char* arch, const char* head, int emd_size, int in_h, int in_w);
int dif_net_destroy(dif_net* net);
/* parameter table, in model order.  Shapes are Keras conventions: conv kernels
 * [kh,kw,cin,cout], depthwise [kh,kw,c,1], dense [in,out], vectors [c]. */
int dif_net_param_count(const dif_net* net);
int dif_net_param_info(const dif_net* net, int i, const char** name, int* ndim, int64_t shape[4]);
/* copy one parameter from HOST memory (model.load_weights, api.py:87) */
int dif_net_set_param(dif_net* net, const char* name, const float* data_host, int64_t count);
/* read one parameter back to HOST memory (model.save_weights, networks/inceptionv3.py:86-88) */
int dif_net_get_param(const dif_net* net, const char* name, float* data_host, int64_t count);
/* input transform applied while converting to the internal NHWC4 f32 layout:
 * y[c] = x[bgr ? 2-c : c] * scale + bias[c]   (predictions.py:94,154 `* rescale`;
 * predictions.py:95 keras vgg16 preprocess_input = BGR swap + mean subtraction);
 * flags = DIF_INPUT_BGR | DIF_INPUT_HFLIP (1 keeps meaning "bgr") */
int dif_net_set_input_transform(dif_net* net, float scale, const float bias[3], int flags);
/* pack weights for the kernels, upload, and size the activation workspace */
int dif_net_finalize(dif_net* net, int max_batch);
/* execution options (no reference counterpart: Keras picks its kernels by itself).  EVERY key the library accepts is
 * listed here with its default (tests/test_cabi_symbols.py compares this list with dif_net_option_name); an unknown key
 * fails.  Unless a key says "before dif_net_finalize" it may be changed between forwards.  Most keys choose between
 * kernel families that compute the same products (the parity tests run both sides); "wino" and "bf16x3" change the
 * products (f32 throughout with "wino"; see each).
 *   "pipe"       1 (default): short-K convolutions may take the software-pipelined kernel (conv_pipe_kernel);
 *                0: every convolution stays on the plain implicit-GEMM kernel
 *   "bdp"        1 (default): 3x3 / stride 1 layers with several tiles per resident block may take the kernel that retires
 *                a tile's epilogue inside the next tile's K-steps (conv_bdp_kernel); 0: never; 2: wherever its
 *                restrictions allow (tests)
 *   "stem"       1 (default): 3-channel first layers run on their own kernels (stem.hip, elementwise.hip); 0: on the
 *                general implicit-GEMM kernel
 *   "patch"      1 (default): 3x3 / stride 1 / pad 1 layers keep the tile's input pixels + halo in LDS per 32-channel
 *                slice (a tap is an address offset); 0: the per-K-step gather
 *   "patch2d"    1 (default): the 8x8-tile form of that path on maps whose sides are multiples of 8; 0: off
 *   "bd"         1 (default): the patch kernels fetch the weights in MFMA-fragment order straight from L2 into registers
 *                (B-direct mainloop); 0: weights staged through LDS
 *   "t2"         1 (default): short-K 3x3 layers on 8-aligned maps run on conv_t2_kernel (128 pixels x 64 channels per
 *                block, two 8x8 sub-tiles); 0: the 64 x 64 kernels
 *   "tn"         1 (default): linear-patch 3x3 layers with whole 128-channel column blocks run on conv_tn_kernel
 *                (64 pixels x 128 channels per block, one whole tile per block); 0: conv_bdp_kernel / conv_igemm_kernel
 *   "sk2"        1 (default): layers with few tiles and a long K loop -- the reference's own call shapes, ONE image
 *                (predictions.py:152-156) or a batch of 12 (scripts/insight_face.py:112) -- run as split-K partials +
 *                a reduce / epilogue launch (conv_splitk.hpp); 0: round 4's persistent stream-K grid
 *   "mt"         1 (default): at ONE image per call (predictions.py:152-156) a layer runs in one launch on 16 x 16 tiles,
 *                operands straight from L2 into the MFMA registers, K split over the block's waves (conv_minitile.hpp);
 *                0: the split-K pair / the large-batch kernels
 *   "wino"       a level.  1: 3x3 / stride 1 layers on even maps of at most 16 x 16 (IResNet's 14 x 14 stage) run as
 *                Winograd F(2x2,3x3) from 64 images per launch up (conv_wino_kernel): 2.25x fewer MFMA multiply-adds, f32
 *                operands, transforms and accumulation, different products -- about twice the direct path's rounding
 *                error per layer; 2 (default): level 1 plus the same layers on the wider even maps up to 112 x 112
 *                (IResNet's 28 x 28, 56 x 56 and 112 x 112 stages) from 128 images per launch up, all of them by the same
 *                kernel in half-size blocks, two per CU (the same bits), and, also from 128 images per launch up, the layers
 *                the even-map rule leaves out (reported as conv_winox_kernel): maps of at most 16 x 16 with an odd side and
 *                at least 2048 Winograd tiles per launch (IResNet's 7 x 7 stage: tiled as the map zero-padded to even
 *                sides) and even maps whose first output is written at even pixels only ("ysub"); 0: the direct f32 fma
 *                chain everywhere.  Any time;
 *                raised after a dif_net_finalize that ran below it, the new level takes effect at the next
 *                dif_net_finalize, which builds the transformed weights; lowered and raised back, at the next forward
 *   "bf16x3"     0 (default): float32 MFMA -- with "wino" = 0 a bit-exact f32 fma chain, the reference's arithmetic;
 *                1 (before dif_net_finalize): throughput mode -- every f32 operand split into bf16 terms, bf16 MFMA
 *                products accumulated in f32 (f32-level accuracy, same 1e-5 cosine gate, not bit-identical)
 *   "bf_terms"   3 (default) or 2: bf16 terms per operand in that mode (six / three MFMA products per multiply-add)
 *   "ysub"       1 (default; before dif_net_finalize): a first output read only by a 1x1 / stride 2 layer is written at
 *                even pixels only; 0: written whole
 *   "lane_split" -1 (default; before dif_net_finalize): the executor's lanes run half-chip persistent grids where the
 *                work per launch is small; 0: whole-chip grids; 1: half-chip grids always
 *   "lane_prio"  0 (default; before dif_net_finalize): all lanes of a multi-lane forward run on least-priority streams
 *                (own hardware queues, whatever else the process created); 1: lane 0 on the caller's stream
 *   "dbg"        0 (default): development aid, bit mask (256: block traces from dif_net_embed_clock; 1024: every layer on
 *                the general epilogue; 33554432: at "wino" = 2 the odd maps and the sub-sampled outputs -- the
 *                conv_winox_kernel layers -- stay on the direct kernels, the A/B switch of that class; other bits: ablations
 *                of the kernel under work)
 * env DIF_OPTIONS="key=value,..." applies keys to every net of the process at dif_net_finalize (A/B runs of the tools). */
int dif_net_set_option(dif_net* net, const char* key, int value);
/* the i-th key dif_net_set_option / dif_gallery_set_option accepts, NULL past the last one (so that the list above can be
 * checked against the library) */
const char* dif_net_option_name(int i);
const char* dif_gallery_option_name(int i);
int dif_net_output_dim(const dif_net* net, int64_t shape[3]); /* {emd,1,1} or {C,H,W} for v3 */
/* networks with several outputs (arch "yolov3": the three detection maps, coarse first; emd_size
 * carries the class count): out_dev then holds output 0 for all n images, then output 1, ... */
int dif_net_output_count(const dif_net* net);
int dif_net_output_info(const dif_net* net, int i, int64_t shape[3]); /* {C,H,W} of output i */
/* forward n <= max_batch images; x_dev is [n,H,W,3] (NHWC) or [n,3,H,W] (NCHW), f32 or u8;
 * out_dev is [n][emd] float32 (v3: [n,H,W,C] NHWC). */
int dif_net_embed(dif_net* net, const void* x_dev, int n, int layout, int dtype, float* out_dev, void* stream);
/* measurement aid: one forward of n images on a single lane whose convolution kernels record every block's life in
 * shader cycles and in 100 MHz ticks; ghz_out = the life-weighted mean shader clock held inside those kernels
 * (bench.py reports it beside rooflines priced at the 2.4 GHz peak) */
int dif_net_embed_clock(dif_net* net, const void* x_dev, int n, int layout, int dtype, float* out_dev, double* ghz_out,
                        void* stream);
/* algorithmic FLOPs of one forward per image (2 * MACs of every conv/dense), for rooflines */
double dif_net_flops_per_image(const dif_net* net);
/* profiling aids: number of layer ops (= kernel launches) per forward, their names and
 * algorithmic MACs per image, and a forward that brackets every launch with HIP events on
 * `stream` and returns the per-op milliseconds (ms_host[dif_net_launch_count]).  The
 * profiled forward synchronises the stream; it is a diagnostic, never the timed path. */
int dif_net_launch_count(const dif_net* net);
int dif_net_op_info(const dif_net* net, int i, const char** name, const char** kernel, double* macs_per_image);
/* compulsory HBM traffic of op i for the mixed roofline (bench.py: t_roof = max(flops / MFMA peak, bytes / HBM rate) per
 * launch): bytes of activations per image that the op must read (the input elements it uses, the shortcut) and write
 * (its one or two outputs), and the bytes of its parameters (read once per launch whatever the batch).  `kernel` of
 * dif_net_op_info is the instantiation the op's LAST launch ran (`family<tile, operand form>`), the family before. */
int dif_net_op_traffic(const dif_net* net, int i, double* act_bytes_per_image, double* param_bytes);
int dif_net_embed_profile(dif_net* net, const void* x_dev, int n, int layout, int dtype, float* out_dev,
                          void* stream, float* ms_host);
/* test aids: one layer at a time against a reference of that layer.
 * dif_net_op_describe: what launch i (the index of dif_net_op_info) hands its kernel, as one line of key=value pairs; the
 * pointer is valid until the next call on that net; works before dif_net_finalize (which may still turn a first output
 * into its even pixels -- y_sub -- and its reader's stride into 1: the line says what holds when it is asked).  Keys:
 *   kind (input conv maxpool dwfull l2norm lrn zero upsample copy dwconv gdctail), name;
 *   x, res, y, y2: "-" or nine integers -- the ROOT tensor's H,W,C, then the view window coff,oy,ox and the view's H,W,C;
 *   k=KH,KW stride pad=top,left cin cin_true cout; act act2 pre_act (none relu prelu relu6) const_alpha res_stride y_sub
 *   chw_flatten k_order; pool (max l2 avg) zero_pad ceil; w bias alpha alpha2: parameter NAMES (dif_net_param_info) or "-";
 *   bn bn2 pre_bn: "-" or "<prefix>,<eps>" with parameters <prefix>/gamma, /beta, /moving_mean, /moving_variance;
 *   w_pw w_dense: kind=gdctail's 1x1 convolution [1,1,512,emd] and dense layer [emd,emd] behind the depthwise `w`, parameter
 *   names; "-" elsewhere;  lrn=radius,bias,alpha,beta: the constants kind=lrn hands lrn_kernel (%.9g); "-" elsewhere.
 * `kernel` of dif_net_op_info names the form a gdctail launch ran: gdc_tail_kernel<KSPLIT=8>, gdc_tail_kernel<KSPLIT=2> or
 * gdc_tail_a_kernel+gdc_tail_b_kernel.
 * dif_net_embed_tap: one forward of n in [1, max_batch] images on a single lane (as dif_net_embed_profile) which, right after
 * launch i is enqueued, copies the first n images of the root buffers of that launch's x, res, y and y2 -- the memory the
 * kernel was handed, [n,H,W,C] of the root -- device to device on `stream` into x_tap .. y2_tap (null, or an operand the
 * launch does not have: skipped).  No sync, no extra kernel; the launches are those of dif_net_embed on one lane. */
const char* dif_net_op_describe(const dif_net* net, int i);
int dif_net_embed_tap(dif_net* net, const void* x_dev, int n, int layout, int dtype, float* out_dev, int i, float* x_tap,
                      float* res_tap, float* y_tap, float* y2_tap, void* stream);

/* ------------------------------------------------------------------ template pooling (csrc/templates.hip)
 * One mean embedding per identity, exact: the rows that carry one label (the images of a person, the frames of a track;
 * the labels of dif_gallery_cluster / dif_gallery_dbscan) are pooled into one template row, which is what a 1:N system
 * enrols (deep_insight_face.templates: TemplatePool, pool_templates; detector.faces.FrameFaces.templates).  The
 * arithmetic is NumPy's float32, bit for bit (tests/templates_ref.py restates it):
 *   sums[t] = ((x_r0 + x_r1) + x_r2) + ... over the label's rows in ascending row number, every add rounded to float32
 *             (np.add.reduce(x[labels == l], axis=0)); with weights (... + fl(w_r * x_r)), the product rounded before
 *             the add (no FMA), and wsum[t] = ((w_r0 + w_r1) + ...);
 *   mean    = sums / float32(count), or sums / wsum; weights are used as given, NaN and Inf propagate;
 *   normalised: mean / sqrt(add.reduce(mean * mean)) in NumPy's pairwise order (np.linalg.norm(mean, axis=1,
 *             keepdims=True)); a zero-norm template is a NaN row.
 * A row with a NEGATIVE label is left out (the convention of dif_match_roc and dif_match_topk_ids; dbscan's noise);
 * the templates are the distinct non-negative labels in ascending order; T may be 0.  Labels are full int64.
 * The sums are sequential, so pooling is INCREMENTAL: a caller keeps labels [T] ascending, sums [T][d], wsum [T]
 * (weighted pools) and counts [T] int64, hands them back as the state of the next call, and the result is bit-identical
 * to one call over all rows ever added, in order.  The handle owns only workspace (the sort's buffers and the order
 * they leave behind), grown on demand; all state is the caller's.  One add = dif_pool_group, ONE host read of
 * t_out_dev (8 bytes, the only synchronisation, as dif_faces_compact has one) to size the outputs, dif_pool_reduce;
 * dif_pool_finish turns sums into templates whenever they are wanted.  No call reads anything back or waits.
 * dif_pool_group: a stable LSD radix sort (8-bit digits; a digit that is constant over all keys costs nothing) of
 *   (label, position), the t0 state labels -- ascending, distinct, >= 0; NULL when t0 = 0 -- in front of the n new
 *   ones, so that a stored template is first in its segment.  Writes index_out_dev int64 [n]: the position of each
 *   row's template among the templates AFTER this add (-1 for a negative label), and t_out_dev int64 [1]: T, their
 *   number (t0 <= T <= t0 + n).  t0 + n < 2^31.  The output does not depend on thread or block order.
 * dif_pool_reduce: uses the order the preceding dif_pool_group on the same handle left behind (its t0 and n), and
 *   fails if there was none, or if t is outside [t0, t0 + n], or -- once the group has run, which it has for a caller
 *   that read t_out_dev -- if t is not the T it wrote; kernels enqueued behind a group that is still running check t on
 *   the device and write nothing into buffers of a wrong size.  state_sums_dev [t0][d], state_wsum_dev [t0],
 *   state_counts_dev [t0]: the state (NULL when t0 = 0); rows_dev float [n][d]; weights_dev float [n], or NULL for an
 *   unweighted pool (state_wsum_dev and wsum_out_dev are then not used and may be NULL).  Writes labels_out_dev [t],
 *   sums_out_dev [t][d], wsum_out_dev [t], counts_out_dev [t], none of which may overlap the state.  A segment's rows
 *   are never split across accumulators: one thread owns four columns of one template and adds its rows in order, with
 *   the loads of sixteen rows in flight; parallelism comes from the columns and the templates.  Rows and sums must be
 *   aligned to 16 bytes.
 * dif_pool_finish: out_dev float [t][d] = the means (normalize = 0) or the normalised templates; wsum_dev NULL divides
 *   by float32(counts_dev).  t = 0 is a no-op.
 * d not a positive multiple of 32, a NULL pointer where one is needed and sizes out of range fail. */
typedef struct dif_pool dif_pool;
int dif_pool_create(dif_pool** out, int d);
int dif_pool_destroy(dif_pool* p);
int dif_pool_group(dif_pool* p, const int64_t* state_labels_dev, int64_t t0, const int64_t* labels_dev, int64_t n,
                   int64_t* index_out_dev, int64_t* t_out_dev, void* stream);
int dif_pool_reduce(dif_pool* p, const float* state_sums_dev, const float* state_wsum_dev, const int64_t* state_counts_dev,
                    const float* rows_dev, const float* weights_dev, int64_t t, int64_t* labels_out_dev, float* sums_out_dev,
                    float* wsum_out_dev, int64_t* counts_out_dev, void* stream);
int dif_pool_finish(const float* sums_dev, const float* wsum_dev, const int64_t* counts_dev, int64_t t, int d, int normalize,
                    float* out_dev, void* stream);
/* dif_pool_best: the best shot of every label -- the ONE row with the greatest key (a face quality, say) -- on the order a
 *   dif_pool_group on the same handle left behind, with dif_pool_reduce's checks: it fails without a group, for a t outside
 *   [t0, t0 + n] and, once the group has run, for a t that is not the T it wrote; behind a group that is still running the
 *   kernel checks t on the device and writes nothing.  State (NULL when t0 = 0): state_key_dev float [t0],
 *   state_row_dev int64 [t0], state_counts_dev int64 [t0], as an earlier call wrote them for the labels the group was
 *   given as its state.  key_dev float [n]: the key of new row i, whose GLOBAL row is row_base + i; a caller advances
 *   row_base by n per call, so that stored rows lie below new ones.  Per distinct non-negative label, ascending:
 *     labels_out_dev [t]   the label
 *     key_out_dev [t], row_out_dev [t]   the entry with the greatest key among the stored entry and the label's new
 *                          rows, and its global row.  Exact ties go to the lower global row; -0.0 ties with +0.0; a NaN
 *                          key is never chosen; -inf is an ordinary key and beats "nothing".  A label whose keys are
 *                          all NaN: row -1, key NaN (and such a stored entry is "nothing" to the next call)
 *     counts_out_dev [t]   the rows seen for the label, NaN keys included (stored count + new rows)
 *   One thread per label walks its segment in order -- the stored entry, then the new rows in ascending row -- and takes
 *   a row when its key is strictly greater: no atomics, no dependence on thread order, and calls over chunks equal one
 *   call over all rows, bit for bit.  Outputs may not overlap the state.  t = 0 is a no-op. */
int dif_pool_best(dif_pool* p, const float* state_key_dev, const int64_t* state_row_dev, const int64_t* state_counts_dev,
                  const float* key_dev, int64_t row_base, int64_t t, int64_t* labels_out_dev, float* key_out_dev,
                  int64_t* row_out_dev, int64_t* counts_out_dev, void* stream);

/* ------------------------------------------------------------------ face quality (csrc/quality.hip)
 * Per-face image and pose measures from what the video path already holds on the device: the crops the embedder is
 * given, the five landmarks and the boxes (deep_insight_face.detector.quality: face_quality; FrameFaces.quality / .best).
 * Not in the reference.  tests/quality_ref.py restates every column in NumPy, bit for bit.
 * crops_dev uint8 [m][S][S][3], 3 <= S <= 256; landmarks_dev float [m][5][2] or NULL -- left eye (le), right eye (re),
 * nose, left mouth corner (ml), right mouth corner (mr), as (x, y) in frame pixels; boxes_dev float [m][4] left, top,
 * right, bottom or NULL, with the frame size frame_h, frame_w; lo, hi in [0, 255].
 * stats_out_dev int64 [m][6], exact.  With c the three stored channels of a pixel as integers,
 *     g      = (c0 + 2*c1 + c2 + 2) >> 2          symmetric in channels 0 and 2: RGB and BGR crops measure the same
 *     L(y,x) = g(y-1,x) + g(y+1,x) + g(y,x-1) + g(y,x+1) - 4*g(y,x)   for the interior 1 <= y, x <= S-2 only: nothing
 *              outside the crop is read and nothing wraps from one row into the next
 *   the columns are  sum g, sum g*g, sum L, sum L*L, #{g <= lo}, #{g >= hi}; the first, second, fifth and sixth over all
 *   n = S*S pixels, the third and fourth over the k = (S-2)^2 interior pixels.
 * out_dev float [m][DIF_QUALITY_COLS]; each value is formed in float64 exactly as written (no contraction) and rounded once:
 *   0 brightness  sum_g / (n*255)
 *   1 contrast    sqrt((n*sum_g2 - sum_g^2) / (n*n)) / 255
 *   2 sharpness   (k*sum_L2 - sum_L^2) / (k*k)                       the variance of the Laplacian
 *   3 clipped     (n_dark + n_bright) / n
 *   4 eye_dist    sqrt(e2),  ex = re.x-le.x, ey = re.y-le.y, e2 = ex*ex + ey*ey
 *   5 roll        ey / eye_dist                                     the sine of the in-plane angle
 *   6 yaw         2*t - 1,  t = ((nose.x-le.x)*ex + (nose.y-le.y)*ey) / e2      0: the nose projects onto the middle
 *   7 nose_drop   ((nose.x-cx)*vx + (nose.y-cy)*vy) / (vx*vx + vy*vy),  c = (le+re)*0.5, v = (ml+mr)*0.5 - c
 *   8 inside      (iw*ih) / ((r-l)*(b-t)),  iw = max(min(r, W) - max(l, 0), 0), ih = max(min(b, H) - max(t, 0), 0)
 *   9 score       sharpness * (1 - clipped) * max(0, 1 - abs(yaw)) * inside
 *   The numerators of columns 0 to 3 are formed in int64 and converted to double exactly (below 2^53 for S <= 256).  The
 *   factors of column 9 are the float32 values of columns 2, 3, 6 and 8 converted back to double, multiplied left to
 *   right; the yaw factor is left out without landmarks, the inside factor without boxes.  Columns 4 to 7 are NaN for
 *   every row without landmarks, column 8 without boxes.  min and max propagate NaN (np.minimum, np.maximum): a NaN
 *   landmark or box coordinate gives NaN in the columns that use it and in the score.  Coincident eyes give 0/0 = NaN
 *   for roll and yaw, a box without area NaN.  The score is a convention without parameters; nobody has measured it
 *   against recognition accuracy.
 * One block per crop: the crop is read once, gray is staged in LDS as bytes, partial sums are kept per thread and reduced
 * by wave and block in 64-bit; no atomics, no dependence on thread order.  m = 0 launches nothing.  A size outside
 * [3, 256], lo or hi outside [0, 255], m outside [0, 2^31) and a NULL pointer where one is needed fail. */
#define DIF_QUALITY_COLS 10
int dif_face_quality(const uint8_t* crops_dev, int64_t m, int size, const float* landmarks_dev, const float* boxes_dev,
                     float frame_h, float frame_w, int lo, int hi, int64_t* stats_out_dev, float* out_dev, void* stream);

/* ------------------------------------------------------------------ tracks
 * The faces of a sequence of frames linked into tracks (csrc/tracks.hip; not in the reference, whose
 * detect_multiple_faces sees one image at a time).  A face continues the track whose last face, at most max_gap frames
 * ago, overlaps it in the image and lies within the embedding tolerance; a track holds at most one face per frame.
 * One sequence per call: n_frames frames with m faces in frame-major order, offsets_dev int64 [n_frames + 1] (read on
 * the device only), boxes_dev float [m][4] left / top / right / bottom, emb_dev float [m][d].  offsets must ascend from
 * offsets[0] = 0 to offsets[n_frames] = m; the host cannot check that without a read.  Whatever they hold, no row outside
 * [0, m) is touched (values are clamped to [0, m] and a descending one closes an empty frame), but a row that no frame
 * covers receives NO output and is not counted in n_new_out_dev.
 *   position   of a face = its index inside its frame; a face at a position >= kmax is CLIPPED: never linked in either
 *              direction, a track of its own, counted in clipped_out_dev.  kmax in [1, DIF_TRACKS_MAX_FACES].
 *   open tail  at frame f: an unclipped face i that nothing has been linked after yet, 1 <= f - frame[i] <= max_gap
 *              (frames without faces count as frames); max_gap in [1, DIF_TRACKS_MAX_GAP].
 *   Frames in ascending order.  The candidates of frame f are the pairs (open tail i, unclipped face j of f) with
 *     iou(box_i, box_j) >= min_iou    box_iou of the detectors' suppression in float32, every product and sum rounded on
 *                                     its own; a NaN IoU is no candidate; a box without area has IoU 0
 *     dist <= tolerance               dist = dif_pairwise's value for (emb_j, emb_i) bit for bit: metric 0 squared L2,
 *                                     metric 1 arccos(cos) / pi, NaN where the reference has NaN; a NaN is no candidate
 *   taken in ascending (dist, i, j) -- dist as a float32 number, ties to the lower i, then the lower j -- and accepted
 *   when neither i nor j was accepted earlier in the frame: prev[j] = i, link_dist[j] = dist, i is no tail any more.
 *   A face of the frame left without a predecessor starts a track: prev -1, link_dist NaN.
 * Outputs, per face: prev_out_dev int64 [m] (a GLOBAL row: row_base + the row of the call, or the row a stored face
 *   had in its own call), link_dist_out_dev float [m], labels_out_dev int64 [m] (the global row of the first face of the
 *   track), age_out_dev int64 [m] (1 at a start, age[prev] + 1); n_new_out_dev int64 [1] the tracks started,
 *   clipped_out_dev int64 [1].  Every output is a function of the inputs alone, whatever the order of threads and blocks.
 * Continuing: state_out_dev (or NULL) receives the last max_gap frames -- stored faces, skipped frames and frames of this
 *   call alike -- in max_gap x state_k_out fixed slots (dif_tracks_state_size bytes: per slot label, age, global row,
 *   box, embedding and whether it is still a tail; per frame its number of unclipped faces; clipped faces are not kept,
 *   they are never tails).  state_k_out >= kmax and >= state_k_in.  The next call takes it as state_in_dev with
 *   state_k_in = that state_k_out, the same max_gap and d, row_base = the faces seen so far, and state_pad = the frames
 *   of batches without a face that the caller skipped since (no call is needed for those).  The stored frames precede
 *   the call's: their links stand and they only serve as tails.  A sequence walked in chunks of any sizes gives the
 *   labels, ages, link distances and (global) prevs of one call over the whole, bit for bit.  state_in_dev NULL: a new
 *   sequence.  The state is not modified; state_out_dev may not overlap it.
 * workspace_dev: dif_tracks_workspace_size(m, max_gap, kmax, state_k_in) bytes of the caller's (0 for state_k_in when
 *   there is no state), aligned to 8 bytes like the states; contents need not be kept between calls, and calls that
 *   share a workspace must be ordered on one stream.  It holds the candidate table float [m][max_gap][max(kmax,
 *   state_k_in)] and one flag per face.
 * passes: 0 = all three, which is what every caller but a measurement passes; or a set of DIF_TRACKS_PASS_* to time a
 *   pass alone (tools/tracks_bench.py).  A pass run alone reads what the pass before it left in the workspace -- the walk
 *   the candidate table, the state pass the walk's flags -- so its outputs mean something only directly after a call with
 *   passes = 0 and the same arguments on the same workspace; on any other workspace contents they are unspecified (no
 *   row outside the buffers is touched: table values are only compared).
 * Costs: the candidate pass is one block per (face, gap): the IoU of every pair, the distance -- one wave per pair, as
 *   dif_pairwise -- only of the pairs the IoU admits.  The walk is one block and sequential in the frames.  The three
 *   launches are stream-ordered; nothing is read back and nothing waits.  m = 0 is allowed (the state still advances).
 * Fails before any launch on: a NULL pointer where one is needed, kmax, state_k_in or state_k_out outside
 *   [1, DIF_TRACKS_MAX_FACES], max_gap outside [1, DIF_TRACKS_MAX_GAP], a metric other than 0 or 1, d outside [1, 8192]
 *   (dif_pairwise's range), negative sizes, n_frames above 2^30 or m above 2^31 - 1, faces without a frame, a workspace
 *   that is too small or misaligned.
 * The two size functions return -1 on such arguments. */
#define DIF_TRACKS_MAX_FACES 64
#define DIF_TRACKS_MAX_GAP 32
#define DIF_TRACKS_PASS_CAND 1
#define DIF_TRACKS_PASS_WALK 2
#define DIF_TRACKS_PASS_STATE 4
int64_t dif_tracks_state_size(int max_gap, int k, int d);
int64_t dif_tracks_workspace_size(int64_t m, int max_gap, int kmax, int state_k_in);
int dif_tracks_link(const int64_t* offsets_dev /* [n_frames + 1] */, const float* boxes_dev /* [m][4] */,
                    const float* emb_dev /* [m][d] */, int64_t n_frames, int64_t m, int d, float tolerance, float min_iou,
                    int max_gap, int metric, int kmax, int64_t row_base, const void* state_in_dev /* or NULL */,
                    int state_k_in, int64_t state_pad, int64_t* prev_out_dev /* [m] */, float* link_dist_out_dev /* [m] */,
                    int64_t* labels_out_dev /* [m] */, int64_t* age_out_dev /* [m] */, int64_t* n_new_out_dev /* [1] */,
                    int64_t* clipped_out_dev /* [1] */, void* state_out_dev /* or NULL */, int state_k_out,
                    void* workspace_dev, int64_t workspace_bytes, int passes, void* stream);

/* ------------------------------------------------------------------ redaction (csrc/redact.hip)
 * The faces of a batch of frames hidden in the frames themselves, on the device: filled, pixelated or smoothed
 * (deep_insight_face.detector.redact: redact_frames; FrameFaces.redact).  Not in the reference, whose detector/run.py only
 * crops.  tests/redact_ref.py restates the rule in NumPy, bit for bit.  All arithmetic on pixels is integer and exact; the
 * box arithmetic is float32, every product and every sum rounded on its own (no contraction).
 * Inputs: frames_dev uint8 [n][h][w][3], 1 <= h, w <= DIF_REDACT_MAX_SIDE; offsets_dev int64 [n + 1], the CSR offsets of the
 *   faces per frame, ascending from 0 to m (read on the device only; whatever they hold, no row outside [0, m) and no frame
 *   outside [0, n) is touched, and a row that no frame covers is left out); boxes_dev float [m][4] left, top, right, bottom
 *   in frame pixels; select_dev uint8 [m] or NULL = every face, non-zero = redact; mode 0 (fill), 1 (pixelate), 2 (smooth);
 *   shape 0 (box), 1 (ellipse); cells in [1, DIF_REDACT_MAX_CELLS]; min_cell in [1, DIF_REDACT_MAX_SIDE]; margin float32,
 *   finite; fill three bytes ON THE HOST, one per channel.
 * Region of face i, from its box (l, t, r, b):
 *    1. bw = r - l; bh = b - t.
 *    2. any of l, t, r, b not finite, or !(bw > 0), or !(bh > 0): the face has no region.
 *    3. le = l - margin*bw; re = r + margin*bw; te = t - margin*bh; be = b + margin*bh.
 *    4. any of the four not finite, or !(re > le), or !(be > te): no region.
 *    5. each of the four is clamped to [-4096, 12288].
 *    6. X0 = floor(le), X1 = ceil(re), Y0 = floor(te), Y1 = ceil(be).
 *    7. X1 <= X0 or Y1 <= Y0: no region.
 *    8. the unclipped region is [X0, X1) x [Y0, Y1), Rw x Rh pixels; both sides are at most 16384.
 *    9. the clipped region is its intersection with the frame [0, w) x [0, h);
 *   10. empty: no region.
 * Cells: c = max(ceil(max(Rw, Rh) / cells), min_cell) in integers; pixel (x, y) of the unclipped region lies in cell
 *   ((x - X0) / c, (y - Y0) / c): the grid is anchored at the UNCLIPPED corner, and both indices are below `cells`.  Without
 *   min_cell a face narrower than `cells` pixels would get c = 1 and leave untouched; min_cell = 1 keeps the plain rule.
 * Cell mean, per channel and per cell that meets the frame: S and k = the sum and the count of the SOURCE pixels of
 *   the cell inside the frame -- pixels outside the shape and pixels under other faces count like any other --, v = (2 S + k) / (2 k)
 *   in integers: the mean rounded half up.  S reaches 255 * 2^26: the sums are 64-bit.
 * Shape: box covers every pixel of the clipped region; ellipse covers the pixel at dx = x - X0, dy = y - Y0 iff
 *   Rh^2 (2 dx + 1 - Rw)^2 + Rw^2 (2 dy + 1 - Rh)^2 <= Rw^2 Rh^2 in int64 (every term below 2^57).  A 4 x 4 region covers all
 *   but its four corners; a side of one pixel is covered.
 * Value of a covered pixel:
 *   fill      the three bytes of `fill`.
 *   pixelate  its cell's mean.
 *   smooth    the bilinear interpolation of the rounded cell means between cell centres, in integers:
 *               a = 2 dx + 1 - c;  i0 = floor(a / 2c);  fa = a - 2c i0 in [0, 2c);  b, j0, fb likewise from dy
 *               i0, i1 = i0 + 1, j0, j1 = j0 + 1 are clamped to the cells that meet the frame: from the cell of the clipped
 *               region's first pixel to the cell of its last pixel, per axis
 *               V = (2c - fa)(2c - fb) v[j0][i0] + fa (2c - fb) v[j0][i1] + (2c - fa) fb v[j1][i0] + fa fb v[j1][i1]
 *               value = (V + 2 c^2) / (4 c^2);  V reaches 255 * 2^30: 64-bit.
 *             It hides exactly what pixelate hides -- cells^2 means -- without the block edges, and needs nothing but the
 *             means; a windowed blur would read neighbours that another block is writing.
 * Overlap: a pixel that several selected faces of its frame cover takes the value of the LOWEST row among them (rows are
 *   best first inside a frame).  Every value comes from the source frames, so the result depends on neither launch nor
 *   thread order, and every output byte has one writer.  An unselected face is never a reason to write a pixel; its pixels
 *   under a selected face's region are redacted all the same.
 * out_dev uint8 [n][h][w][3] receives the values of the covered pixels; every other byte of it is left as it was.  out_dev ==
 *   frames_dev (in place) is allowed in every mode and gives the bytes of the out-of-place call on a copy; an out that
 *   overlaps the frames in part fails.
 * Two stream-ordered launches, both sized from m and cells alone: pass 1 writes the means of every (face, cell) that has
 *   pixels into the workspace (skipped in mode 0), pass 2 paints from the workspace and the boxes and reads no frame.  A cell's
 *   sum is split over up to 16 waves whose partial sums are added in wave order.  Nothing is read back, no atomics.
 * workspace_dev: dif_frames_redact_workspace_size(m, cells) = m * cells * cells * 4 bytes of the caller's, aligned to 4
 *   bytes; contents need not be kept between calls, and calls that share a workspace must be ordered on one stream.
 * n = 0 or m = 0 launches nothing.  Fails before any launch on: h or w outside [1, DIF_REDACT_MAX_SIDE], cells, min_cell,
 *   mode or shape outside their ranges, a margin that is not finite, negative sizes, n above 2^31 - 1 or m * cells above
 *   2^31 - 1, a NULL pointer where one is needed (select_dev may be NULL), a workspace that is too small or misaligned, an
 *   out that overlaps the frames in part.  dif_frames_redact_workspace_size returns -1 on such arguments. */
#define DIF_REDACT_MAX_CELLS 64
#define DIF_REDACT_MAX_SIDE 8192
int64_t dif_frames_redact_workspace_size(int64_t m, int cells);
int dif_frames_redact(const uint8_t* frames_dev /* [n][h][w][3] */, int64_t n, int h, int w,
                      const int64_t* offsets_dev /* [n + 1] */, const float* boxes_dev /* [m][4] */, int64_t m,
                      const uint8_t* select_dev /* [m], or NULL */, int mode, int shape, int cells, int min_cell, float margin,
                      const uint8_t* fill /* [3], host */, uint8_t* out_dev /* [n][h][w][3] */, void* workspace_dev,
                      int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ annotation (csrc/annotate.hip)
 * The opposite picture to redaction: a ring round every face of a batch of frames, a filled plate with its label next to
 * it and a square on every landmark, painted into the frames on the device (deep_insight_face.detector.annotate:
 * compose_text, NameTable, annotate_frames, palette; FrameFaces.annotate).  The reference draws with OpenCV on the host
 * (detector/utility.py draw_boxes, detector/yolov3.py draw, api.py show_plot); nothing of OpenCV's rasterisation or of its
 * Hershey font is restated here -- parity with cv2.rectangle / cv2.putText is unpinned.  tests/annotate_ref.py restates both
 * rules below in NumPy, bit for bit.  The paint is opaque: no pixel is read, nothing is blended.
 *
 * dif_annotate_compose: the label of every face, written on the device.
 * Inputs: names_dev uint8 [g][ln], one NUL-padded name per gallery row, or NULL; idx_dev int64 [m], the gallery row of each
 *   face, or NULL; known_dev uint8 [m], non-zero = the face is known, or NULL = every face is; values_dev float32 [m], the
 *   value to print after the name, or NULL; decimals in [0, 4]; unknown, a string ON THE HOST of at most
 *   DIF_ANNOTATE_MAX_TEXT bytes, which may be empty; text_dev uint8 [m][l], the output, 1 <= l <= DIF_ANNOTATE_MAX_TEXT.
 * Row i:
 *   base   names and idx given, the face known and 0 <= idx[i] < g: the bytes of names[idx[i]] up to its first NUL or ln.
 *          Otherwise: the bytes of unknown.
 *   value  values given: one space if the base is not empty, then the number.  A NaN prints as "nan".  Otherwise
 *          a = min(|v|, 99999) in float32; c = (int64) floor((double) a * 10^decimals + 0.5), one float64 product and one
 *          sum; '-' if v < 0 and c > 0; c / 10^decimals in decimal; with decimals > 0 a '.' and c % 10^decimals padded with
 *          zeros to `decimals` digits.  (At two decimals 0.125 prints 0.13, -0.004 prints 0.00 and infinity 99999.00; the float32
 *          nearest to 0.005 is 0.00499999989 and prints 0.00, the least float32 not below 0.005 prints 0.01.)
 *   cut    the result is cut at l bytes and padded with NUL; a text of l bytes has no NUL.
 * One thread per row.  m = 0 launches nothing.  Fails before any launch on: decimals or l outside their ranges, unknown NULL
 *   or too long, m negative or above 2^31 - 1, names_dev given with g < 0 or ln < 1, text_dev NULL.
 *
 * dif_frames_annotate: the drawing.
 * Inputs: out_dev uint8 [n][h][w][3], 1 <= h, w <= DIF_REDACT_MAX_SIDE, the frames, painted in place (there is no source:
 *   out of place is a copy first); offsets_dev, boxes_dev, select_dev and margin as dif_frames_redact takes them -- whatever
 *   offsets hold, no row outside [0, m) and no frame outside [0, n) is touched, and a row that no frame covers is left out;
 *   landmarks_dev float [m][5][2] (x, y) or NULL; text_dev uint8 [m][l] or NULL, 1 <= l <= DIF_ANNOTATE_MAX_TEXT (l is not
 *   looked at without text); colors_dev uint8 [m][3] or NULL = the three bytes `color` ON THE HOST for every face;
 *   thickness t in [0, DIF_ANNOTATE_MAX_THICKNESS]; scale s in [1, DIF_ANNOTATE_MAX_SCALE]; mark r in
 *   [-1, DIF_ANNOTATE_MAX_MARK], -1 = no marks.
 * What face i paints, in its colour C:
 *   box     [X0, X1) x [Y0, Y1) from steps 1 to 8 of the redaction rule with the same margin.  A face without a region there
 *           paints nothing at all; a region wholly outside the frame may still paint, its ring or plate can reach in.
 *   ring    the pixels of [X0 - t, X1 + t) x [Y0 - t, Y1 + t) outside the box: round the face, never over it.
 *   plate   only with len > 0, len = the bytes of text[i] before the first NUL, at most l.  Tw = (6 len - 1) s, Th = 7 s,
 *           Pw = Tw + 2 s, Ph = 9 s.  PX0 = X0 - t; if PX0 + Pw > w then PX0 = w - Pw; if PX0 < 0 then PX0 = 0.
 *           PY0 = Y0 - t - Ph; if PY0 < 0 then PY0 = Y1 + t: no room above puts the plate below the box.
 *           The plate is [PX0, PX0 + Pw) x [PY0, PY0 + Ph).
 *   glyphs  (u, v) = (x - PX0 - s, y - PY0 - s) inside [0, Tw) x [0, Th): character k = u / (6 s), column (u % (6 s)) / s,
 *           row v / s.  Column 5 is the gap between characters; otherwise the pixel is a text pixel iff bit 4 - column of
 *           that row of the glyph of byte text[i][k] is set.  Text pixels are black if 299 R + 587 G + 114 B >= 128000 for
 *           C = (R, G, B), else white.
 *   font    5 x 7, drawn for this project (csrc/font5x7.hpp): printable ASCII 0x20 .. 0x7E, any other byte shows a glyph
 *           with every pixel set.  dif_annotate_glyph(code, rows) writes the seven rows of the glyph of byte `code`, top
 *           first, bit 4 = the left column (a host call; code outside 0x20 .. 0x7E gives the all-set glyph).
 *   marks   with r >= 0, for each of the five landmarks whose two coordinates are finite: both are clamped to
 *           [-4096, 12288]; mx = floor(px + 0.5f) in float32, my likewise; the mark is [mx - r, mx + r] x [my - r, my + r].
 *   Inside one face the plate with its glyphs comes first, then the marks, then the ring.
 * Between faces: a pixel that several selected faces of its frame paint takes the paint of the LOWEST row among them (best
 *   first), as in redaction.  What a lower face takes is its whole footprint: its ring, its whole plate -- opaque whether or
 *   not a pixel is a text pixel -- and its marks; never the inside of its box.  An unselected face paints nothing and shields
 *   nothing.  Every output byte has at most one writer, so the result depends on neither launch nor thread order.
 * One launch of a fixed number of blocks per face.  Nothing is read back, no atomics; every loop is bounded by h, w, l or two
 *   values of offsets.  n = 0 or m = 0 launches nothing.  Fails before any launch on: h or w outside
 *   [1, DIF_REDACT_MAX_SIDE], thickness, scale or mark outside their ranges, a margin that is not finite, text_dev given
 *   with l outside its range, negative sizes, n above 2^31 - 1 or 4 m above 2^31 - 1, out_dev, offsets_dev or boxes_dev NULL,
 *   colors_dev and color both NULL. */
#define DIF_ANNOTATE_MAX_TEXT 64
#define DIF_ANNOTATE_MAX_THICKNESS 64
#define DIF_ANNOTATE_MAX_SCALE 8
#define DIF_ANNOTATE_MAX_MARK 16
int dif_annotate_glyph(int code, uint8_t* rows /* [7], host */);
int dif_annotate_compose(const uint8_t* names_dev /* [g][ln], or NULL */, int64_t g, int ln, const int64_t* idx_dev /* [m], or NULL */,
                         const uint8_t* known_dev /* [m], or NULL */, const float* values_dev /* [m], or NULL */, int decimals,
                         const char* unknown /* host */, int64_t m, uint8_t* text_dev /* [m][l] */, int l, void* stream);
int dif_frames_annotate(uint8_t* out_dev /* [n][h][w][3] */, int64_t n, int h, int w, const int64_t* offsets_dev /* [n + 1] */,
                        const float* boxes_dev /* [m][4] */, int64_t m, const float* landmarks_dev /* [m][5][2], or NULL */,
                        const uint8_t* text_dev /* [m][l], or NULL */, int l, const uint8_t* colors_dev /* [m][3], or NULL */,
                        const uint8_t* color /* [3], host */, const uint8_t* select_dev /* [m], or NULL */, float margin,
                        int thickness, int scale, int mark, void* stream);

/* ------------------------------------------------------------------ detector evaluation (csrc/deteval.hip)
 * The detections of a detector matched to labelled boxes, and the precision / recall curve and average precision of all
 * of them, on the device (deep_insight_face.detector.utility: compute_overlap, compute_ap; deep_insight_face.evaluation.
 * detection: evaluate_detections, DetectionEvaluator; FrameFaces.evaluate).  The reference ships the two primitives,
 * detector/utility.py:281-306 compute_overlap and :309-334 compute_ap (py-faster-rcnn); the rule around them is that of their
 * consumers (keras-retinanet / keras-yolo3 `evaluate`) with Pascal VOC's "difficult" flags.  tests/detection_ref.py restates
 * it in NumPy as the sequential loop.  Parity with the WIDER FACE devkit's own protocol is unpinned.
 *
 * dif_box_overlap: out[i][c] = compute_overlap(a, b)[i][c] in float64 on the float32 coordinates (left, top, right, bottom)
 *   widened to float64, the reference's operations in its order -- area_b = (b2 - b0) * (b3 - b1); iw = min(a2, b2) -
 *   max(a0, b0); ih = min(a3, b3) - max(a1, b1); both clamped below at 0; ua = (a2 - a0) * (a3 - a1) + area_b - iw * ih,
 *   clamped below at DBL_EPSILON; iw * ih / ua; no +1, no fused multiply-add -- so the reference's value bit for bit.
 *   Deviation: a pair with a coordinate that is not finite has overlap 0 (the reference: NaN).
 *
 * dif_det_match: one batch of whole frames.
 * Inputs: det_offsets_dev int64 [n_frames + 1] and gt_offsets_dev int64 [n_frames + 1], the exclusive prefix sums of the
 *   detections and of the truths per frame; det_boxes_dev float [m][4], det_scores_dev float [m], in any order inside a
 *   frame; gt_boxes_dev float [t][4]; gt_ignore_dev uint8 [t], non-zero = an ignored truth, or NULL = none is; thr_host,
 *   j IoU thresholds as doubles ON THE HOST, 1 <= j <= DIF_DET_MAX_THRESHOLDS, each in (0, 1].  Whatever the offsets hold,
 *   no row outside [0, m) or [0, t) is touched; a detection that no frame covers has no truth.
 * Outputs: assigned_out_dev int32 [m]: the first maximum (np.argmax: the lowest row) of the detection's overlaps with the
 *   truths of its frame, as a row of gt_boxes, -1 in a frame without truths; iou_out_dev double [m]: that maximum, 0
 *   without one; outcome_out_dev uint8 [j][m]; n_truth_out_dev int64 [1]: the truths that are not ignored.
 * Outcome at threshold thr[j], a frame's detections walked by descending score -- ties to the lower row, NaN last, that is
 *   np.argsort(-scores, kind='stable'):
 *     assigned < 0 or iou < thr[j]      DIF_DET_FP       (iou == thr[j] is a hit)
 *     else the truth is ignored         DIF_DET_DROPPED  neither true nor false positive; it takes nothing
 *     else the truth is not yet taken   DIF_DET_TP       and the truth is taken
 *     else                              DIF_DET_FP       a detection never falls through to its second-best truth
 *
 * dif_det_curve: all detections seen, whatever batches they came in.
 * Inputs: scores_dev float [m]; outcome_dev uint8 [j][m] as dif_det_match wrote it (batches concatenated along m);
 *   n_truth_dev int64 [1] ON THE DEVICE, the sum over the batches.
 * Outputs: order_out_dev int64 [m]: the rows by descending score (the order above, over all m); tp_cum_out_dev and
 *   fp_cum_out_dev int64 [j][m]: the inclusive counts of outcomes DIF_DET_TP / DIF_DET_FP in that order; recall_out_dev
 *   double [j][m] = tp_cum / n_truth, 0 with n_truth = 0; precision_out_dev double [j][m] = tp_cum / max(tp_cum + fp_cum,
 *   DBL_EPSILON), one float64 division each; ap_out_dev double [j] = compute_ap of the two curves (dif_det_ap).  m = 0
 *   writes ap = 0 and nothing else.  The order of a batch restricted to a frame is the order of all rows restricted to it,
 *   so batches of any sizes give the bits of one call.
 *
 * dif_det_ap: out_dev double [1] = compute_ap(recall, precision) of m points, double each: with the sentinels (0, 0) in front
 *   and (1, 0) behind, the envelope -- the running maximum of the precision from the right, a NaN taken over as np.maximum
 *   does -- and the sum of (recall[i] - recall[i - 1]) * envelope[i] over the i where the recall changes.  The terms are summed
 *   in a fixed order -- per tile of DIF_DET_SCAN_TILE points a fixed tree, the tiles last to first -- so equal curves give
 *   equal bits; NumPy sums pairwise, and the two orders differ by at most (number of terms) * 2^-52 on a curve whose recall
 *   ends at or below 1.  dif_det_curve's ap has the bits of dif_det_ap on its own curves.
 *
 * workspace_dev: dif_det_workspace_size(m, t, j) bytes of the caller's, aligned to 8 (dif_det_curve: t = 0).  Nothing is read
 *   back to the host and no block waits for another; the only atomics are an integer minimum and an integer sum.  Every
 *   output is a function of the inputs alone.  Fails before any launch on: sizes negative or above DIF_DET_MAX_ROWS, j or a
 *   threshold outside its range, rows without a frame, a NULL pointer that is needed, a workspace too small. */
#define DIF_DET_MAX_THRESHOLDS 16
#define DIF_DET_MAX_ROWS 0x7fff0000
#define DIF_DET_SCAN_TILE 1024
#define DIF_DET_FP 0
#define DIF_DET_TP 1
#define DIF_DET_DROPPED 2
int dif_box_overlap(const float* a_dev /* [n][4] */, int64_t n, const float* b_dev /* [k][4] */, int64_t k, double* out_dev /* [n][k] */,
                    void* stream);
int64_t dif_det_workspace_size(int64_t m, int64_t t, int j);
int dif_det_match(const int64_t* det_offsets_dev /* [n_frames + 1] */, const float* det_boxes_dev /* [m][4] */,
                  const float* det_scores_dev /* [m] */, int64_t m, const int64_t* gt_offsets_dev /* [n_frames + 1] */,
                  const float* gt_boxes_dev /* [t][4] */, const uint8_t* gt_ignore_dev /* [t], or NULL */, int64_t t, int64_t n_frames,
                  const double* thr_host /* [j] */, int j, int32_t* assigned_out_dev /* [m] */, double* iou_out_dev /* [m] */,
                  uint8_t* outcome_out_dev /* [j][m] */, int64_t* n_truth_out_dev /* [1] */, void* workspace_dev, int64_t workspace_bytes,
                  void* stream);
int dif_det_curve(const float* scores_dev /* [m] */, const uint8_t* outcome_dev /* [j][m] */, const int64_t* n_truth_dev /* [1] */, int64_t m,
                  int j, int64_t* order_out_dev /* [m] */, int64_t* tp_cum_out_dev /* [j][m] */, int64_t* fp_cum_out_dev /* [j][m] */,
                  double* recall_out_dev /* [j][m] */, double* precision_out_dev /* [j][m] */, double* ap_out_dev /* [j] */,
                  void* workspace_dev, int64_t workspace_bytes, void* stream);
int dif_det_ap(const double* recall_dev /* [m] */, const double* precision_dev /* [m] */, int64_t m, double* out_dev /* [1] */, void* stream);

/* ------------------------------------------------------------------ ArcMargin logits
 * Not in the reference (north_star only; ArcFace, Deng et al. 2019):
 * logits = s * cos(theta + m * onehot(label)); labels_dev NULL -> s * cos(theta). */
int dif_arcmargin_create(dif_arcmargin** out, int d, int64_t n_classes, float s, float m);
int dif_arcmargin_destroy(dif_arcmargin* a);
int dif_arcmargin_set_weight(dif_arcmargin* a, const float* w_dev, void* stream); /* [C][d], rows normalised internally */
int dif_arcmargin_logits(dif_arcmargin* a, const float* emb_dev, const int64_t* labels_dev, int n,
                         float* logits_dev, void* stream); /* [n][C] */

#ifdef __cplusplus
}
#endif
#endif /* DIF_H */
