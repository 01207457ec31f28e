/*
 * leafhip.h — C ABI of libleafhip.so: the MI355X (gfx950) hot path of leaffliction.
 *
 * The reference (Kiripiro/leaffliction) is pure Python and has no FFI; the
 * boundary each entry point replaces is the third-party library call the
 * reference makes on its hot path.  Each declaration cites
 * the reference call site (path:line under the reference tree) it stands in for.
 *
 * Conventions (last row):
 *  - every buffer is a caller-owned DEVICE pointer (torch tensors on the host
 *    side); the library never allocates, frees or synchronises;
 *  - all work is enqueued on the hipStream_t passed as `stream` (void* here so
 *    that the header needs no HIP include; 0 = the null stream);
 *  - return value: 0 = LF_OK, negative = error (see lf_last_error());
 *    nothing throws or exits across the ABI; the library is re-entrant and
 *    keeps no mutable global state beyond the thread-local error string;
 *  - integer / byte results are bit-exact with the reference's CPU path;
 *    float tolerances are stated per function.
 *
 * Image layouts: "HWC u8" = [N][H][W][3] uint8 interleaved RGB (what
 * np.array(PIL.Image) yields); "NCHW f32" = [N][C][H][W] float.
 */
#ifndef LEAFHIP_H
#define LEAFHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LF_OK 0
#define LF_ERR_INVALID (-1)   /* bad argument (null pointer, non-positive dim, unsupported size) */
#define LF_ERR_LAUNCH (-2)    /* HIP reported a launch error */
#define LF_ERR_WORKSPACE (-3) /* workspace too small */

#define LF_VERSION 100

typedef void* lf_stream_t;

int lf_version(void);
/* Thread-local description of the last error returned on this thread ("" if none). */
const char* lf_last_error(void);

/* The first `width` bytes of `rows` rows between a page-locked host slab and its device mirror (asynchronous on
 * `stream`; to_host: 1 = device -> host, 0 = host -> device): the balancer moves the used front of each fixed-size
 * slot, not the slot (dataset_balancer.py's pixels never left host memory; here they cross PCIe twice). */
int lf_copy_rows(void* dst, size_t dst_pitch, const void* src, size_t src_pitch, size_t width, size_t rows, int to_host,
                 lf_stream_t stream);

/* ------------------------------------------------------------------------- */
/* A1 — augmentation / input side (uint8, bit-exact)                          */
/* ------------------------------------------------------------------------- */

/* u8 HWC -> f32 NCHW with exact x/255.0f, optional per-channel (x-mean)/denom.
 * Replaces np.array(img) + ImageTransforms.normalize_array
 * (srcs/utils/image_utils.py:117-130) and, when mean/denom are non-null, the
 * keras Normalization layer (srcs/model/cnn.py:84-86): denom[c] =
 * max(sqrt(var[c]), eps) is computed by the caller; mean3/denom3 are HOST pointers to
 * 3 floats (model constants passed by value into the launch).  Bit-exact vs numpy f32. */
int lf_pack_hwc_u8_to_nchw_f32(const uint8_t* in, float* out, int n, int h, int w,
                               const float* mean3, const float* denom3, lf_stream_t stream);

/* Per-image, per-channel 256-bin histogram: hist[n][c][v] (int32).
 * Replaces PIL Image.histogram() inside ImageOps.autocontrast
 * (srcs/preprocessing/image_augmenter.py:127).  `hist` is overwritten. */
int lf_hist_u8(const uint8_t* in, int32_t* hist, int n, int h, int w, lf_stream_t stream);

/* autocontrast LUT from histograms: lut[n][c][256] u8, cutoff[n] in percent.
 * Restates PIL ImageOps.autocontrast's cut / lo / hi / scale / offset
 * arithmetic in IEEE double (image_augmenter.py:127).  Bit-exact. */
int lf_autocontrast_lut(const int32_t* hist, const double* cutoff, uint8_t* lut, int n,
                        lf_stream_t stream);

/* out[n][y][x][c] = lut[n][c][in[n][y][x][c]]  (PIL Image.point(lut)). */
int lf_lut_apply_u8(const uint8_t* in, const uint8_t* lut, uint8_t* out, int n, int h, int w,
                    lf_stream_t stream);

/* Batch assembly from a device-resident dataset (the loader's cache=True, sequence.py:47-58,
 * kept in HBM instead of host RAM): dst[i][:] = src[index[i]][:] for rows of row_bytes bytes
 * (one resized uint8 image each).  index: int32 device array, values the caller has checked. */
int lf_gather_rows_u8(const uint8_t* src, const int32_t* index, uint8_t* dst, int n_out,
                      size_t row_bytes, lf_stream_t stream);

/* ImageAugmenter.flip (image_augmenter.py:20-31): mode[n] = 0 -> FLIP_LEFT_RIGHT,
 * 1 -> FLIP_TOP_BOTTOM. */
int lf_flip_u8(const uint8_t* in, uint8_t* out, const int32_t* mode, int n, int h, int w,
               lf_stream_t stream);

/* ImageAugmenter.distortion's noise add (image_augmenter.py:121-124):
 * out = (u8)(in + (u8)(int)noise) with uint8 wrap-around, noise in float64
 * exactly as np.random.normal returned it (same shape as the image). */
int lf_noise_wrap_add_u8(const uint8_t* in, const double* noise, uint8_t* out, size_t nbytes,
                         lf_stream_t stream);

/* The same wrap-around add when the noise was already cast to uint8 on the host (numpy's own
 * astype, image_augmenter.py:121-123; the codec worker processes of DatasetBalancer do that next
 * to the JPEG decode): out = in + add mod 256, bytewise.  nbytes % 4 == 0, 4-byte aligned. */
int lf_add_wrap_u8(const uint8_t* in, const uint8_t* add, uint8_t* out, size_t nbytes,
                   lf_stream_t stream);

/* Same op with the noise drawn on the device: counter-based Philox4x32-10 +
 * Box-Muller N(0, sigma) keyed by (seed, byte index).  Statistically, not
 * bit-wise, equal to the numpy stream; used for the synthetic C3 pass. */
int lf_noise_philox_add_u8(const uint8_t* in, uint8_t* out, size_t nbytes, uint64_t seed,
                           float sigma, lf_stream_t stream);

/* ImageAugmenter.distortion (image_augmenter.py:121-131), first half in one pass: out = in + noise
 * (mod 256) TOGETHER WITH the per-image, per-channel histogram of `out` that ImageOps.autocontrast
 * takes next (hist [N][3][256] int32, as lf_hist_u8 gives it) — the noisy image is not read back
 * just to be counted.  add != NULL: the uint8 noise plane of lf_add_wrap_u8; add == NULL: the
 * Philox noise of lf_noise_philox_add_u8 (same seed -> same bytes).  h*w*3 % 16 == 0, 16-byte
 * aligned buffers. */
int lf_noise_hist_u8(const uint8_t* in, const uint8_t* add, uint8_t* out, int32_t* hist, int n, int h,
                     int w, uint64_t seed, float sigma, lf_stream_t stream);

/* apply_mask (srcs/utils/mask_utils.py:67-79) and blur.py:74-75:
 * out = mask > 127 ? img : color (color 0 or 255), mask is [N][H][W] u8. */
int lf_mask_composite_u8(const uint8_t* img, const uint8_t* mask, uint8_t* out, int n, int h,
                         int w, int color, lf_stream_t stream);

/* cv2.cvtColor(rgb, COLOR_RGB2HSV) on uint8 (hist.py:184, blur.py:44):
 * OpenCV's 8-bit fixed-point path, H in [0,180).  Parity unpinned (no cv2). */
int lf_rgb2hsv_u8(const uint8_t* rgb, uint8_t* hsv, size_t npixels, lf_stream_t stream);

/* cv2.cvtColor(rgb, COLOR_RGB2GRAY) on uint8 (blur.py:27):
 * (4899 R + 9617 G + 1868 B + 8192) >> 14. */
int lf_rgb2gray_u8(const uint8_t* rgb, uint8_t* gray, size_t npixels, lf_stream_t stream);

/* cv2.GaussianBlur(img, (k,k), sigma) on uint8 with BORDER_REFLECT_101
 * (blur.py:61,72): separable, both passes fused through LDS, OpenCV's 8.8
 * fixed-point kernel (kq: HOST array of ksize uint16 taps, sum 256).  channels = 1 or 3,
 * ksize odd <= 31; odd ksize 3..15 with every tap <= 255 takes the dot-product fast path. */
int lf_gauss_blur_u8(const uint8_t* in, uint8_t* out, int n, int h, int w, int channels,
                     const uint16_t* kq, int ksize, lf_stream_t stream);

/* HSV colour-region statistics of apply_histogram_filter (hist.py:22-67,
 * 181-189, 248-256): per image, with leaf = (s>10)&(v>15)&(v<245):
 * counts[n][0] = leaf pixels, [1..8] = the 8 predicate counts,
 * [9..13] = the 5 hue-range counts; hsv_hist[n][3][256] = histograms of H,S,V
 * over leaf pixels.  Input is RGB HWC u8 (the HSV conversion is fused). int64-free:
 * all counters int32. */
#define LF_HSV_NCOUNTS 14
int lf_hsv_region_stats(const uint8_t* rgb, int32_t* counts, int32_t* hsv_hist, int n, int h,
                        int w, lf_stream_t stream);

/* apply_blur_filter (srcs/transform/filters/blur.py:18-79) given the leaf mask its
 * make_mask_func returned (leaf = mask > 0): gray -> Canny(50,150,L2) dilated by the 3x3
 * MORPH_ELLIPSE element (x0.4) + uint8(min-max normalised Sobel magnitude) (x0.3) + brown
 * regions (hue_lo <= H <= hue_hi, S >= s_min, V <= v_max, inside the leaf; closed, then dilated
 * twice) (x0.6, skipped when use_brown = 0) + min-max normalised mean |rgb - GaussianBlur15|
 * (x0.2) -> min-max normalised to uint8 -> GaussianBlur 5x5 -> kept under the leaf mask,
 * replicated to RGB.  rgb/out [n][h][w][3], leaf_mask [n][h][w]; kq15 / kq5: HOST arrays of
 * the 8.8 fixed-point Gaussian taps (15 taps for sigma 0 -> 2.6, 5 taps for cfg.gaussian_sigma).
 * Parity unpinned (no cv2); every step follows oracle/cv_ops.py:blur_saliency bit for bit. */
size_t lf_blur_saliency_workspace(int n, int h, int w);
int lf_blur_saliency_u8(const uint8_t* rgb, const uint8_t* leaf_mask, uint8_t* out, int n, int h,
                        int w, int use_brown, int hue_lo, int hue_hi, int s_min, int v_max,
                        const uint16_t* kq15, const uint16_t* kq5, void* workspace,
                        size_t ws_bytes, lf_stream_t stream);

/* _create_inclusive_mask (srcs/transform/filters/mask.py:727-831), the default strategy of make_mask
 * (mask.py:548-582, config.yaml:6 "inclusive"), on the working image: colour predicates in 8-bit HSV and
 * L*a*b* (mask.py:735-770), gray / purple / untextured background removal (:772-789), Canny(30, 100)
 * edges dilated 3x3 (:791-794), open 3x3 / close 9x9 / close 7x7 with cv2's MORPH_ELLIPSE elements
 * (:806-815), largest 8-connected component (:817-824), close 5x5 (:826-829).
 * rgb [N,H,W,3] -> mask [N,H,W] 0 / 255.  green_lo / green_hi: cfg.green_hue_range (config.yaml:10);
 * kq15: HOST pointer to the 15 Q8.8 taps of GaussianBlur(gray, (15, 15), 0).
 * The upscale before it (_prepare_working_image, mask.py:29-50) and GrabCut / brown extension after it
 * (:307-392) are not part of this call.  Parity unpinned (no cv2); follows oracle/cv_ops.py:inclusive_mask. */
size_t lf_inclusive_mask_workspace(int n, int h, int w);
int lf_inclusive_mask_u8(const uint8_t* rgb, uint8_t* mask, int n, int h, int w, int green_lo,
                         int green_hi, const uint16_t* kq15, void* workspace, size_t ws_bytes,
                         lf_stream_t stream);

/* make_mask (srcs/transform/filters/mask.py:548-582) for the default strategy ("inclusive"): working-image
 * upscale (cv2.resize INTER_CUBIC, :29-50), the inclusive candidate (lf_inclusive_mask_u8), _postprocess_mask
 * (pcv.fill, close, open, largest external contour, filled polygon, :53-69), the Otsu fallback of the HSV
 * channel when no contour of area > 1 exists (:395-411), the brown-region extension (:335-392) and the nearest
 * resize of the mask back to the input size (:526-545).  GrabCut / shadow refinements are not part of it.
 * rgb [N,H,W,3] -> mask [N,H,W] 0 / 255; contour [N,cap,2] int32 (x, y) of the largest external contour of the
 * final mask, in input coordinates (float32(p) / float32(scale), truncated, when rescale); counts [N] = its TRUE
 * number of points (0: no contour) — when counts[i] > cap only the first cap points were stored and the caller
 * must run image i again with a larger cap; flags [N]: bit 0 the fallback mask was taken, bit 2 a step bound was
 * hit (a bug: treat as an error).  wh x ww: the working size (H x W when rescale == 0).  The working image must
 * fit one workgroup's LDS (four bit planes, 140 KiB; square working images up to 519 x 519): larger sizes are
 * rejected before any launch.  kq15: HOST pointer to
 * the 15 Q8.8 taps of GaussianBlur(gray, (15, 15), 0).  Parity unpinned (no cv2 / PlantCV / skimage). */
typedef struct {
    int green_lo, green_hi;            /* green_hue_range (config.yaml:10) */
    int fill_size, morph_kernel;       /* config.yaml:14-15 */
    int hsv_channel;                   /* hsv_channel_for_mask: 0 h, 1 s, 2 v */
    int use_lab_brown;                 /* brown predicate: 0 HSV, 1 L*a*b* */
    int brown_hue_lo, brown_hue_hi, brown_s_min, brown_v_max;
    int lab_a_min, lab_b_min;
    int brown_min_area_px, brown_morph_kernel;
} lf_make_mask_params;
size_t lf_make_mask_workspace(int n, int h, int w, int wh, int ww);
int lf_make_mask_u8(const uint8_t* rgb, uint8_t* mask, int32_t* contour, int32_t* counts, int32_t* flags,
                    int n, int h, int w, int wh, int ww, int rescale, double scale,
                    const lf_make_mask_params* params, int cap, const uint16_t* kq15, void* workspace,
                    size_t ws_bytes, lf_stream_t stream);

/* apply_brown_filter (srcs/transform/filters/brown.py) for a same-size batch: leaf = mask > 0; the brown predicate
 * on the pixel as handed in (8-bit HSV lo <= h <= hi, s >= s_min, v <= v_max, or L*a*b* a >= a_min, b >= b_min
 * when use_lab_brown) inside the leaf; MORPH_OPEN then MORPH_CLOSE with the (k, k) MORPH_ELLIPSE element
 * (k = morph_kernel in [1, 31]); 8-connected components of area >= min_area_px kept.
 * rgb [N,H,W,3], mask [N,H,W] -> out [N,H,W,3] (kept pixels set to (255, 100, 0)), stats [N][3] int32
 * {count, brown area, leaf area}; flags [N]: bit 2 a step bound was hit (a bug: treat as an error).  An image must
 * fit one workgroup's LDS (two bit planes, 140 KiB): larger sizes are rejected before any launch.  Parity
 * unpinned (no cv2). */
typedef struct {
    int use_lab_brown;                 /* 0 HSV, 1 L*a*b* */
    int hue_lo, hue_hi, s_min, v_max;  /* brown_hue_range, brown_s_min, brown_v_max */
    int lab_a_min, lab_b_min;
    int min_area_px, morph_kernel;     /* brown_min_area_px, brown_morph_kernel */
} lf_brown_params;
size_t lf_brown_spots_workspace(int n, int h, int w);
int lf_brown_spots_u8(const uint8_t* rgb, const uint8_t* mask, uint8_t* out, int32_t* stats, int32_t* flags,
                      int n, int h, int w, const lf_brown_params* params, void* workspace, size_t ws_bytes,
                      lf_stream_t stream);

/* Lesions: the components lf_brown_spots_u8 keeps for the same (rgb, mask, params), as a table of integers.  The
 * pipeline is that function's, stated once in the library: leaf = mask > 0; the brown predicate on the pixel as
 * handed in, inside the leaf; MORPH_OPEN then MORPH_CLOSE with the (k, k) MORPH_ELLIPSE element; the 8-connected
 * components of area >= min_area_px are the lesions.
 * rgb [N,H,W,3], mask [N,H,W] -> table [N][cap][LF_LESION_FIELDS] int64, counts [N] int32, flags [N] int32.
 * counts[n] is the true number of lesions of image n, also when it exceeds cap.  One row per lesion, in raster order
 * of the lesion's first pixel (topmost row first, then leftmost column); rows at and after min(counts[n], cap) are
 * zero.  The fields:
 *    0 area: pixels;  1..4 x0, y0, bw, bh: the tight bounding box;
 *    5, 6 sum_x, sum_y: sums of the pixel coordinates (the centroid is sum / area, formed by the caller);
 *    7..9 sum_r, sum_g, sum_b: sums of the input image's channels over the lesion's pixels;
 *    10 border_px: lesion pixels with at least one 4-neighbour that is not in the lesion (outside the image counts as
 *       not in it);
 *    11 margin_px: lesion pixels with at least one 4-neighbour that is not leaf (mask == 0, or outside the image).
 * flags [N]: bit 0 the image has at least one lesion; bit 1 counts[n] > cap, the table holds the first cap; bit 2 a
 * union-find step bound was hit (a bug: treat as an error).
 * Integer arithmetic throughout; the only atomics are integer adds, minima and maxima, whose result does not depend
 * on their order, so two launches on the same inputs give the same bits.  One workgroup per image, the planes in LDS:
 * an image must fit as for lf_brown_spots_u8 (two bit planes, 140 KiB).  Checked before any launch, with nothing
 * written: that limit, n <= 65535, 1 <= morph_kernel <= 31, cap >= 1, the workspace's size
 * (lf_lesion_table_workspace) and its 256-byte alignment.  Parity unpinned (no cv2). */
#define LF_LESION_FIELDS 12
size_t lf_lesion_table_workspace(int n, int h, int w);
int lf_lesion_table(const uint8_t* rgb, const uint8_t* mask, int64_t* table, int32_t* counts, int32_t* flags,
                    int n, int h, int w, int cap, const lf_brown_params* params, void* workspace, size_t ws_bytes,
                    lf_stream_t stream);

/* apply_roi_filter (srcs/transform/filters/roi.py) for a batch, reading the contour buffer lf_make_mask_u8 made
 * (contour [N,cap,2] int32 (x, y), counts [N]; counts[i] <= cap, points inside the image): bbox [N][4] int32
 * (x, y, w, h) = cv2.boundingRect; canvas [N,roi_h,roi_w,3] = the box letterboxed into the canvas (INTER_AREA,
 * zero border); vis [N,H,W,3] = the input with the box drawn (cv2.rectangle, (255, 0, 0), thickness 2).
 * flags [N]: bit 0 the image has a contour (else vis is the input, canvas and bbox are zero), bit 2 a count above
 * cap or a point outside the image (an error).  The cv2 readings: the comment above roi_kernel in
 * lf_filters.hip.  No workspace.  Parity unpinned (no cv2). */
int lf_roi_u8(const uint8_t* rgb, const int32_t* contour, const int32_t* counts, int cap, uint8_t* canvas,
              uint8_t* vis, int32_t* bbox, int32_t* flags, int n, int h, int w, int roi_h, int roi_w,
              lf_stream_t stream);

/* Leaf measurements from the contour buffer lf_make_mask_u8 made (contour [N,cap,2] int32 (x, y), counts [N]): the
 * geometry srcs/transform/filters/analyze.py draws (centroid, extreme points, convex hull, PCA axes) and the shape
 * numbers pcv.analyze_object computes there, as data.  One workgroup per image; no image is read; two launches give
 * the same bits.  Limits, checked before the launch: h, w <= 4096 and cap <= 65536, which keep every integer sum
 * below 2^57, inside int64.  The points may repeat and the contour may touch itself.
 * flags [N] as lf_roi_u8: bit 0 the image has a contour (else its records and hull are zero), bit 2 a count below 0
 * or above cap or a point outside the image (an error; nothing outside [0, min(count, cap)) is read), or a hull
 * past its capacity, which no point set can cause (a bug: treat as an error).
 * With P_0 .. P_{m-1} the points, P_m = P_0 and c_i = x_i * y_{i+1} - x_{i+1} * y_i:
 * ints [N][32] int64, exact:
 *    0 npts = m;  1 area2s = sum c_i (signed);  2 s10 = sum (x_i + x_{i+1}) c_i;  3 s01 = sum (y_i + y_{i+1}) c_i;
 *    4..7 bbox x, y, w, h (cv2.boundingRect, lf_roi_u8's);
 *    8..15 left, right, top, bottom as (x, y): the first point in contour order with the least x, the greatest x,
 *      the least y, the greatest y (numpy argmin / argmax);
 *    16 in_frame: 1 when the bbox touches no image border (x > 0, y > 0, x + w < W, y + h < H);
 *    17..21 sx, sy, sxx, sxy, syy: sums of x, y, x^2, x y, y^2 over the points;
 *    22 hull_n, 23 hull_area2 = |sum c| over the hull, 24 feret2 = the greatest squared distance between two hull
 *      vertices;
 *    25..28 i0min, i0max, i1min, i1max: indices of the points with the least and the greatest projection on the
 *      major axis (vx, vy) and on its normal (-vy, vx);  29..31 zero.
 * hull [N][2 * min(h, w)][2] int32: the strict convex hull of the points (no three vertices collinear), starting at
 *   the lexicographically smallest (x, y), every consecutive triple with a positive cross product; rows from hull_n
 *   on are zero.  One point gives 1 vertex; two or more points on one line give its 2 end points.  A strict hull of
 *   lattice points has at most two vertices per row and per column, so the capacity always suffices.
 * vals [N][16] float64:
 *    0 area = |area2s| / 2;  1 perimeter = sum |P_{i+1} - P_i|;
 *    2, 3 cx, cy = s10 / (3 area2s), s01 / (3 area2s) (cv2.moments' m10 / m00, m01 / m00), the mean of the points
 *      when area2s == 0;
 *    4 hull_area = hull_area2 / 2;  5 solidity = area / hull_area, 0 when hull_area is 0;
 *    6 circularity = 4 pi area / perimeter^2, 0 when the perimeter is 0;  7 feret = sqrt(feret2);
 *    8, 9 l1 >= l2: eigenvalues of the population covariance (1 / m) of the points;
 *    10, 11 vx, vy: the unit eigenvector of l1 with vx > 0, or vx == 0 and vy > 0; (1, 0) when l1 == l2;
 *    12, 13 axis_major, axis_minor: greatest minus least projection on (vx, vy) and on (-vy, vx);
 *    14 axis_angle_deg = atan2(vy, vx) in degrees;  15 zero. */
int lf_shape_stats(const int32_t* contour, const int32_t* counts, int cap, int64_t* ints, double* vals,
                   int32_t* hull, int32_t* flags, int n, int h, int w, lf_stream_t stream);

/* apply_analyze_filter's picture (srcs/transform/filters/analyze.py) for a same-size batch, drawn from the contour
 * buffer lf_make_mask_u8 made, lf_shape_stats' records for the same contours and Canny edges:
 * rgb [N,H,W,3], mask [N,H,W], edges [N,H,W], contour [N,cap,2], counts [N], ints [N][32], vals [N][16],
 * hull [N][2 * min(h, w)][2] -> out [N,H,W,3] (must not overlap rgb), flags [N] with lf_roi_u8's bits: bit 0 the
 * image has a contour (else out is the input; the reference's "Analyze: no object" caption needs cv2's font and is
 * not drawn), bit 2 a count outside [0, cap] or a point outside the image (an error; out is the input).  Limits as
 * lf_shape_stats (h, w <= 4096, cap <= 65536), checked before any launch.  No workspace; two launches give the same
 * bits.  The records are not trusted: the hull count is cut to its capacity, indices into [0, m), coordinates as
 * below, and no pixel outside the image is touched.
 *
 * Drawing rules.  cv2 is not available to pin LineAA or FillConvexPoly, so these are the project's own rules, in
 * integers throughout, restated in numpy by tests/draw_ref.py; they reproduce the cv2 readings the ROI box relies
 * on (an axis-aligned thickness-2 line is the rows y - 1 .. y + 1 with a plus-sign cap; the radius-3 disc has rows
 * 3, 5, 7, 7, 7, 5, 3 wide).  Parity unpinned (no cv2).
 *   Points are integer (x, y).  For a segment A -> B and a pixel p: d = B - A, L2 = |d|^2, u = (p - A) . d,
 *   c = (p - A) x d, all in int64.
 *   Thick segment (thickness 2, colour k): p = k when its distance to the segment is <= 1: |p - A|^2 <= 1 if u <= 0,
 *     |p - B|^2 <= 1 if u >= L2, c^2 <= L2 otherwise.  A = B gives the plus sign at A.  An overwrite: no order.
 *   Disc (radius 3, centre q, colour k): p = k when |p - q|^2 <= 12.
 *   Anti-aliased segment (thickness 1, colour k): the pixels with 0 <= u <= L2 and c^2 < L2 (A = B: the pixel A
 *     alone) are blended once each, per channel out = (a k + (256 - a) out + 128) >> 8 with
 *     a = 256 - floor(sqrt(floor(65536 c^2 / L2))) (A = B: a = 256).  Segments are drawn one after another in the
 *     stated order; a pixel two segments touch is blended twice, in that order.
 *   Clipping: a pixel outside the image is skipped; nothing else clips.
 *   Record coordinates (the centroid, the extreme points, the hull's vertices) are clamped to [-16384, 16383] before
 *     drawing.  Only the centroid of a self-touching contour with a small signed area can be that far out; the clamp
 *     keeps c^2 below 2^62.
 * Paint order for an image with a contour P_0 .. P_{m-1}, on a copy of the input (analyze.py's order):
 *   1 the contour: thick segments P_i -> P_{(i+1) mod m} in (255, 0, 0);
 *   2 the centroid marker: (cx, cy) = vals[2], vals[3] truncated toward zero; thick segments
 *     (cx - 7, cy) -> (cx + 7, cy) and (cx, cy - 7) -> (cx, cy + 7) in (255, 255, 0);
 *   3 for left, right, top, bottom (ints[8..15]) in that order: the disc at the point, then the anti-aliased
 *     segment centroid -> point, both in (255, 255, 0);
 *   4 the hull: anti-aliased segments H_i -> H_{(i+1) mod hull_n}, i = 0 .. hull_n - 1, in (0, 255, 0) (one vertex:
 *     one degenerate segment; two: the segment there and back);
 *   5 the axes: thick segments P[i0min] -> P[i0max] in (255, 255, 0), then P[i1min] -> P[i1max] in (255, 0, 255)
 *     (ints[25..28]);
 *   6 every pixel with edges > 0 and mask > 0 becomes (0, 255, 255). */
int lf_analyze_overlay_u8(const uint8_t* rgb, const uint8_t* mask, const uint8_t* edges, const int32_t* contour,
                          const int32_t* counts, int cap, const int64_t* ints, const double* vals,
                          const int32_t* hull, uint8_t* out, int32_t* flags, int n, int h, int w,
                          lf_stream_t stream);

/* cv2.Canny(gray, low, high, L2gradient=l2gradient), aperture 3, for gray [N,H,W] uint8 of any size -> edges
 * [N,H,W] uint8 (0 / 255): Sobel with replicated borders, the magnitude |dx| + |dy| against floor(threshold) or,
 * with l2gradient, dx^2 + dy^2 against floor(min(32767, threshold)^2); low > high are swapped; 22.5 / 67.5 degree
 * sectors in 15-bit fixed point, the asymmetric > / >= neighbour tests, 8-connected hysteresis (in LDS when the
 * plane fits 156 KiB, in memory otherwise).  Parity unpinned (no cv2): oracle/cv_ops.canny is the same reading. */
size_t lf_canny_workspace(int n, int h, int w);
int lf_canny_u8(const uint8_t* gray, uint8_t* edges, int n, int h, int w, double low, double high, int l2gradient,
                void* workspace, size_t ws_bytes, lf_stream_t stream);

/* The pixel stages of the pseudo-landmarks filter (srcs/transform/filters/landmarks.py: CLAHE, bilateralFilter,
 * goodFeaturesToTrack) for a same-size batch of planes [N,H,W], h, w >= 8 (smaller images are rejected before the
 * launch).  Parity unpinned (no cv2): these are the project's own rules, in integers throughout, restated in numpy by
 * tests/landmarks_ref.py; `//` is the floor division of non-negative integers.
 *
 * lf_clahe_u8: createCLAHE(clipLimit 2.0, tileGridSize (8, 8)).apply(gray) -> out (uint8).
 *   Wp, Hp = W, H rounded up to multiples of 8; the added columns / rows are the image reflected (reflect-101).
 *   A tile is tw x th = Wp/8 x Hp/8 with area a; clip = max(1, (2 a) // 256).  Per tile, from its 256-bin histogram:
 *   excess = sum max(h_i - clip, 0) and the bins are cut to clip; every bin gets excess // 256; with
 *   r = excess % 256 > 0 and step = max(256 // r, 1) the bins 0, step, 2 step, ... get 1 more each while the index
 *   is < 256 and units of r remain; lut[i] = min(255, (2 * 255 * cum_i + a) // (2 a)), cum the inclusive prefix sum.
 *   Per pixel (x, y): fx = 2x + 1 - tw, tx = floor(fx / (2 tw)), ax = fx - 2 tw tx; the tiles tx and tx + 1, each
 *   clamped to [0, 7], weigh 2 tw - ax and ax; the same in y;
 *   out = (sum lut * wx * wy + 2 tw th) // (4 tw th) over the four tiles.  Hp * Wp <= 2^27.
 *   Two launches: one workgroup per (image, tile), then a pixel pass.  workspace: the 64 LUTs of every image.
 *
 * lf_bilateral_u8: bilateralFilter(gray, d = 5, sigmaColor, sigmaSpace) with the weights as Q16 tables on the
 *   DEVICE: wc [256] int32 by |v - centre|, ws [5] int32 by dx^2 + dy^2, each in [0, 65536].  The taps are the 21
 *   offsets with dx^2 + dy^2 <= 4, reflect-101 borders; a tap weighs w = (ws[dx^2 + dy^2] * wc[|v - centre|] + 2^15)
 *   >> 16; out = (2 sum w v + sum w) // (2 sum w), the centre value when sum w is 0.  The caller makes the tables
 *   (ops.bilateral_tables: rint(65536 exp(-k^2 / (2 sigma^2))) in float64), so no device exp enters the result.
 *   gray and out must differ.
 *
 * lf_corner_score_u8: cornerMinEigenVal(blockSize 3, ksize 3) in integers -> score int32.  dx, dy = the 3 x 3 Sobel
 *   with reflect-101 borders; A = sum dx^2, B = sum dx dy, C = sum dy^2 over the 3 x 3 block, the dx / dy planes
 *   continued by reflect-101 again; S = A + C - isqrt((A - C)^2 + 4 B^2), isqrt the exact floor of the root (the
 *   radicand is below 2^49).  0 <= S < 2^25.
 *
 * lf_good_features: goodFeaturesToTrack's selection on a score plane (int32, values in [0, 2^31)) under a mask
 *   (uint8, > 0 = inside) -> points [N,max_points,2] int32 (x, y), rows past the count zero, counts [N].
 *   Smax = the largest score where mask > 0; Smax = 0 gives no points.  A pixel is live when q_den S > q_num Smax.
 *   A candidate is a live pixel with mask > 0, not on the outermost rows or columns, whose S is >= every live
 *   8-neighbour's S.  Candidates are ordered by S descending, then (y, x) ascending; going down that order one is
 *   taken unless a taken one lies within dx^2 + dy^2 < min_dist^2; selection stops at max_points.  One workgroup per
 *   image: the candidates are compacted to a key list, then at most max_points rounds of arg-max with suppression.
 *   q_num >= 0, q_den > 0, 0 <= min_dist <= 16384, 1 <= max_points <= 2^20.  Two launches give the same bits. */
size_t lf_clahe_workspace(int n, int h, int w);
int lf_clahe_u8(const uint8_t* gray, uint8_t* out, int n, int h, int w, void* workspace, size_t ws_bytes,
                lf_stream_t stream);
int lf_bilateral_u8(const uint8_t* gray, const int32_t* wc, const int32_t* ws, uint8_t* out, int n, int h, int w,
                    lf_stream_t stream);
int lf_corner_score_u8(const uint8_t* gray, int32_t* score, int n, int h, int w, lf_stream_t stream);
size_t lf_good_features_workspace(int n, int h, int w);
int lf_good_features(const int32_t* score, const uint8_t* mask, int32_t* points, int32_t* counts, int n, int h, int w,
                     int q_num, int q_den, int min_dist, int max_points, void* workspace, size_t ws_bytes,
                     lf_stream_t stream);

/* apply_landmarks_filter (srcs/transform/filters/landmarks.py) for a same-size batch: rgb [N,H,W,3], the mask
 * [N,H,W], contour [N,cap,2] and counts [N] that lf_make_mask_u8 gave for these images, the brown numbers of the
 * config (lf_brown_params: predicate, brown_morph_kernel, brown_min_area_px), landmarks_count and the two Q16 tables
 * of lf_bilateral_u8 (device) -> out [N,H,W,3] (must not overlap rgb); points [N,pcap,3] int32 (kind, x, y), kind
 * 0 border, 1 vein, 2 disease, in placement order, rows past the counts zero; pcounts [N,3] per kind; flags [N] as
 * lf_roi_u8: bit 0 the image has a contour (else out is the input and there are no points; the reference's
 * "Landmarks: no object" caption needs cv2's font and is not drawn), bit 2 a count outside [0, cap], a point outside
 * the image, a step bound that was hit or an enhanced contour of more than 8 (H + W) points (an error: out is the
 * input, the counts are zero).
 * Quotas: total = max(1, landmarks_count), bq = vq = max(1, total // 3), dq = max(1, total - bq - vq),
 * pcap = bq + vq + 5 dq = lf_landmarks_points_cap(landmarks_count).
 * A sequence of launches on one stream: gray, lf_clahe_u8, the saliency filter's Sobel pass, two lf_canny_u8, lf_bilateral_u8,
 * two lf_corner_score_u8 on workspace planes, then one workgroup per image with four bit planes in LDS (make_mask's
 * limit, 140 KiB: larger images are rejected before any launch).  h, w >= 8.  Two launches give the same bits.
 *
 * Landmark rules, for an image with a contour C and leaf M = mask > 0.  Parity unpinned (no cv2): the project's own
 * rules, restated in numpy by tests/landmarks_ref.py.
 *   1 Enhanced mask: E = close5((M) | close5(brown_px & M)), the 5 x 5 MORPH_ELLIPSE element, pixels outside the
 *     image never win.  C' = the largest external contour of E (make_mask's reading: Suzuki-Abe, CHAIN_APPROX_SIMPLE,
 *     equal areas: the last discovered); E empty: C' = C.
 *   2 Border: bq points resample the closed polygon C' as the reference's resample_contour reads, in float64:
 *     segment lengths sqrt((double)(dx^2 + dy^2)), the closing segment included; cumulative lengths summed in index
 *     order; targets t_i = i * (total / bq); the segment pointer j advances while cum[j + 1] < t;
 *     a = (t - cum[j]) / (cum[j + 1] - cum[j]), 0 for a zero-length segment; the point is
 *     (1 - a) P_j + a P_{j+1}, truncated.  total = 0 gives the single point P_0.
 *   3 Vein: q = CLAHE(gray(rgb)); e1 = Canny(q, 30, 90, L2); e2 = Canny(bilateral(q), 50, 130, L2); e3 = the Sobel
 *     magnitude of q (float32, reflect-101) min-max normalised to 0 .. 255, truncated to uint8, > 40 (the saliency
 *     filter's reading); edges = (e1 | e2 | e3) & erode3(E); D = dilate3(edges) (the 3 x 3 ellipse is the cross).
 *     Points: lf_good_features(lf_corner_score(q), D, 2 / 1000, min_dist 2, max_points vq).  Fewer than vq: with cnt
 *     the set pixels of D in raster order and need = vq - placed, the pixels of rank (i (cnt - 1)) // (need - 1),
 *     i = 0 .. need - 1 (rank 0 when need = 1) follow; none when cnt = 0.
 *   4 Disease: brown_px & E, opened then closed with the brown_morph_kernel ellipse; its 8-connected components of
 *     area >= brown_min_area_px, by area descending, ties in raster order of their first pixel;
 *     quota = min(max(ncomp, total_area // 50), 5 dq).  Walking the components while placed < quota:
 *     k = max(1, min(area // 40, quota - placed)); its points are lf_good_features(lf_corner_score(gray(rgb)), the
 *     component, 5 / 1000, min_dist 3, max_points k), taken one by one, each counting, until placed >= dq; a
 *     component that yields none gets its centroid (sum x // area, sum y // area).
 *   5 Picture, on a copy of rgb, in this order: the border points as discs of radius 2 in (255, 0, 0); C' closed as
 *     anti-aliased segments in (0, 255, 0), in contour order; the vein points as discs of radius 2 in (0, 0, 255);
 *     the disease points as discs of radius 4 in (139, 69, 19).  A disc of radius r is |p - q|^2 <= r^2 + r, an
 *     overwrite (the radius-3 disc of the drawing rules above is the same rule); the anti-aliased segment is that of
 *     the drawing rules above.  Only the image border clips. */
int lf_landmarks_points_cap(int landmarks_count);
size_t lf_landmarks_workspace(int n, int h, int w, int landmarks_count);
int lf_landmarks_u8(const uint8_t* rgb, const uint8_t* mask, const int32_t* contour, const int32_t* counts, int cap,
                    const lf_brown_params* params, int landmarks_count, const int32_t* wc, const int32_t* ws,
                    uint8_t* out, int32_t* points, int32_t* pcounts, int32_t* flags, int n, int h, int w,
                    void* workspace, size_t ws_bytes, lf_stream_t stream);

/* ------------------------------------------------------------------------- */
/* JPEG encode (the file Pillow's Image.save(path, quality=q) writes)          */
/* ------------------------------------------------------------------------- */
/* Replaces ImageLoader.save_pil_image / save_array (srcs/utils/image_utils.py:49-56; the balancer's output
 * step, dataset_balancer.py:201-207) for images of any size: baseline, 4:2:0, Annex K Huffman
 * tables, JFIF 1.01 — libjpeg-turbo's integer pipeline restated (jccolor, jcsample h2v2, jfdctint,
 * jcdctmgr, jchuff, jcmarker), so the bytes equal Pillow's.
 * lf_jpeg_fdct_quant_u8 (GPU): rgb [N,H,W,3] -> coef int16 [N][ceil(H/16) * ceil(W/16) MCUs][Y00 Y01 Y10 Y11 Cb Cr][64],
 *   quantised, in zigzag order (768 bytes per MCU, 16-byte aligned).  Sizes that are not whole MCUs are padded as
 *   libjpeg pads them (replicated edges, dummy blocks: jcprepct.c, jcsample.c, jccoefct.c).
 * lf_jpeg_write_file (HOST, no GPU call in it; also exported by libleafcodec.so for the codec worker
 *   processes): one image's coefficients -> the complete file in `out`; returns its length, -1 on bad
 *   arguments or if `cap` (take lf_jpeg_file_bound) is too small.
 * lf_jpeg_quant_tables (HOST): jpeg_set_quality(quality, force_baseline) tables, row-major. */
int lf_jpeg_fdct_quant_u8(const uint8_t* rgb, int16_t* coef, int n, int h, int w, int quality,
                          lf_stream_t stream);
void lf_jpeg_quant_tables(int quality, uint8_t* lum64, uint8_t* chroma64);
size_t lf_jpeg_file_bound(int h, int w);
long lf_jpeg_write_file(const int16_t* coef, int h, int w, int quality, uint8_t* out, size_t cap);
/* The entropy coding on the GPU as well: lf_jpeg_entropy_u8 turns the coefficients of N images (image i at
 * coef + i*coef_stride bytes, the layout above) into their Huffman-coded, byte-stuffed scans: row i of `out`
 * (out_stride bytes) = int32 length, then the bytes; length -1 when a scan does not fit its row.
 * lf_jpeg_wrap_scan (HOST, also in libleafcodec.so) puts the markers around such a scan: the complete file. */
size_t lf_jpeg_entropy_workspace(int n, size_t out_stride);
int lf_jpeg_entropy_u8(const void* coef, size_t coef_stride, uint8_t* out, size_t out_stride, int n, int h,
                       int w, void* workspace, size_t ws_bytes, lf_stream_t stream);
long lf_jpeg_wrap_scan(const uint8_t* scan, size_t scan_len, int h, int w, int quality, uint8_t* out, size_t cap);
/* The same two GPU steps for images of DIFFERENT sizes in one launch each (the balancer's rotated canvases: a rotation
 * with expand=True gives every output its own size; dataset_balancer.py:201-207 saves each with Image.save):
 * items[i] (device memory) = where image i's pixels start in rgb_base (bytes; any alignment), where its coefficients
 * go in coef_base (int16 elements, a multiple of 8), where its scan goes in out_base (bytes, a multiple of 4; the same
 * place as its pixels is fine: the coefficients are complete before the scan is written), the number of the first of
 * its lf_jpeg_fdct_groups(h, w) passes (running sum over the images before it), its size, and 6 x its MCUs.
 * out_room: the bytes each scan may take (int32 length first, -1 when it did not fit), as out_stride above. */
typedef struct {
    int64_t rgb_off, coef_off, out_off, group_start;
    int32_t h, w, nblocks, reserved;
} lf_jpeg_item;
long lf_jpeg_fdct_groups(int h, int w);
int lf_jpeg_fdct_quant_items_u8(const uint8_t* rgb_base, int16_t* coef_base, const lf_jpeg_item* items, int n,
                                long total_groups, int quality, lf_stream_t stream);
int lf_jpeg_entropy_items_u8(const void* coef_base, const lf_jpeg_item* items, uint8_t* out_base, size_t out_room, int n,
                             void* workspace, size_t ws_bytes, lf_stream_t stream);
/* Decoding, the same split the other way round (Image.open(path).convert("RGB"), image_utils.py:19-33 — the
 * balancer's input step and the loader's):
 * lf_jpeg_read_file (HOST, also in libleafcodec.so): markers + Huffman decoding of a baseline 4:2:0 file of
 *   whole MCUs -> coef (the layout above, still quantised; coef_cap in int16 elements) and qtab128 (the file's
 *   luminance and chrominance tables, 64 uint16 each, row-major).  Returns 0; 1 when the file is of a kind it
 *   does not cover (progressive, other samplings, grey, ragged size: decode with libjpeg); -1 when it is corrupt.
 *   Only YCbCr files are taken (lf_jpeg_idct_rgb_u8 always converts): a file libjpeg reads as RGB — no JFIF APP0
 *   and an Adobe APP14 with transform 0, or neither marker and the component ids 'R', 'G', 'B' — returns 1, from
 *   this entry and from lf_jpeg_scan_prepare and the _ragged twins alike.  A Huffman table with an all-ones code
 *   is corrupt (-1), as it is to libjpeg.
 * lf_jpeg_idct_rgb_u8 (GPU): dequantisation + jidctint islow IDCT + h2v2 fancy upsampling + YCbCr->RGB for N
 *   images of one size; image i's coefficients at coef + i*coef_stride bytes, its tables at qtab + i*qtab_stride. */
int lf_jpeg_read_file(const uint8_t* data, size_t len, int16_t* coef, size_t coef_cap, uint16_t* qtab128,
                      int* h, int* w);
/* The same decoding with the Huffman step on the GPU as well (jdhuff.c's decode_mcu; the balancer's input step):
 * lf_jpeg_scan_prepare (HOST, also in libleafcodec.so): markers only.  The slot receives the quantisation tables
 *   at [0, 256), and at lf_jpeg_scan_aux_offset(h, w) = align16(256 + 3hw) a 32-byte header, the four Huffman
 *   tables as they stood in the file, the offsets of the restart intervals and the entropy-coded bytes with the
 *   0xFF00 stuffing undone and the RSTn markers taken out (layout: lf_jpeg_host.cpp).  *hash = FNV-1a of the
 *   Huffman tables: images decoded in one launch must share it.  Returns 0; 1 = decode this file on the host
 *   (lf_jpeg_read_file / libjpeg); -1 = corrupt markers.
 * lf_jpeg_huffman_u8 (GPU): N prepared slots of one size -> each slot's coefficient area [256, 256 + 3hw) in
 *   lf_jpeg_read_file's layout (then lf_jpeg_idct_rgb_u8 as before).  mode 0: one workgroup per image decodes 256
 *   subsequences of the scan at once (self-synchronising; lf_jpeg_huff.hip), and the images that kernel does not
 *   take (scans of a megabyte and more) go through the one-lane-per-image kernel; mode 1: that kernel for all.  (A scan
 *   up to 96 KB is staged in LDS, a longer one is read where it lies; restart intervals are decoded one per thread.)
 *   status[i] (int32, device): 0 decoded; 1 the scan is malformed or ends early (what lf_jpeg_read_file answers
 *   with -1: give the file to libjpeg for the reference's verdict); 2 (one-lane-per-image kernel only: it shares
 *   one set of tables among 64 images) the image's hash differs from that of the first image of its group; 3 no
 *   prepared scan in the slot. */
size_t lf_jpeg_scan_aux_offset(int h, int w);
int lf_jpeg_scan_prepare(const uint8_t* data, size_t len, uint8_t* slot, size_t cap, int* h, int* w, uint64_t* hash);
int lf_jpeg_huffman_u8(void* slots, size_t stride, int n, int h, int w, int* status, int mode, lf_stream_t stream);
size_t lf_jpeg_decode_workspace(int n, int h, int w);
int lf_jpeg_idct_rgb_u8(const void* coef, size_t coef_stride, const void* qtab, size_t qtab_stride,
                        uint8_t* rgb, int n, int h, int w, void* workspace, size_t ws_bytes,
                        lf_stream_t stream);
/* The same decoding for files of ANY height and any width from 5 up, images of DIFFERENT sizes in one launch per
 * step (the rotated canvases Augmentation writes: Image.rotate(angle, expand=True) gives every output a size of its
 * own, dataset_balancer.py:201-207; the loader and the balancer's input step read them back).  The scan of a ragged
 * size holds ceil(h/16) * ceil(w/16) whole MCUs; libjpeg cuts the planes to h x w (chroma: ceil(h/2) x ceil(w/2))
 * BEFORE the fancy upsampling, so the image's own last chroma row / column stands in for the missing neighbour.
 * Narrower files (chroma width 1 or 2: libjpeg-turbo's upsampler does something else there) return 1.
 * lf_jpeg_read_file_ragged, lf_jpeg_scan_prepare_ragged (HOST, also in libleafcodec.so): the twins of the two
 *   functions above, same verdicts, same slot layout with the coefficient area sized by the MCUs:
 *   [256, 256 + 768 * ceil(h/16) * ceil(w/16)), the aux block at lf_jpeg_scan_aux_offset_ragged(h, w) behind it
 *   (for whole MCUs the very layout of the functions above).
 * lf_jpeg_dec_item, one per image (the same array on the device for the kernels and on the host for the checks
 *   before the launch): slot_off = where its slot starts in `slots` (bytes, a multiple of 16), slot_bytes = the
 *   slot's size, rgb_off = where its pixels go in `rgb` (tightly packed [h][w][3], any byte: neighbours may be packed
 *   against it, nothing outside its 3hw bytes is written), plane_off = 384 x the MCUs of the images before it (its
 *   padded Y / Cb / Cr planes in the workspace), group_start = the running sum of lf_jpeg_fdct_groups(h, w).
 * lf_jpeg_huffman_items_u8 (GPU): lf_jpeg_huffman_u8 with the geometry taken per image; modes and status codes as
 *   there (the one-lane-per-image kernel shares the tables of the first image among 64 consecutive items).
 * lf_jpeg_idct_rgb_items_u8 (GPU): dequantisation + IDCT into padded planes (one launch), cut + fancy upsampling +
 *   YCbCr->RGB (one launch).  lf_jpeg_decode_items_workspace: bytes of workspace for n host descriptors. */
typedef struct {
    int64_t slot_off, rgb_off, plane_off, group_start;
    int32_t h, w;
    int64_t slot_bytes;
} lf_jpeg_dec_item;
int lf_jpeg_read_file_ragged(const uint8_t* data, size_t len, int16_t* coef, size_t coef_cap, uint16_t* qtab128,
                             int* h, int* w);
size_t lf_jpeg_scan_aux_offset_ragged(int h, int w);
int lf_jpeg_scan_prepare_ragged(const uint8_t* data, size_t len, uint8_t* slot, size_t cap, int* h, int* w,
                                uint64_t* hash);
int lf_jpeg_huffman_items_u8(void* slots, size_t slots_bytes, const lf_jpeg_dec_item* items,
                             const lf_jpeg_dec_item* host_items, int n, int* status, int mode, lf_stream_t stream);
size_t lf_jpeg_decode_items_workspace(const lf_jpeg_dec_item* host_items, int n);
int lf_jpeg_idct_rgb_items_u8(const void* slots, size_t slots_bytes, const lf_jpeg_dec_item* items,
                              const lf_jpeg_dec_item* host_items, int n, uint8_t* rgb, size_t rgb_bytes,
                              void* workspace, size_t ws_bytes, lf_stream_t stream);

/* HOST (also in libleafcodec.so): np.random.RandomState(seed).normal(loc, scale, n) — the distortion op's noise
 * plane (srcs/preprocessing/image_augmenter.py:121-123) — from MT19937 and numpy's legacy polar Gaussian with
 * libm's log / sqrt: out64 (optional) the float64 values, bit for bit; out8 (optional) their numpy astype(uint8). */
int lf_legacy_normal_u8(uint32_t seed, double loc, double scale, size_t n, uint8_t* out8, double* out64);
/* The same planes for N seeds at once on the GPU (lf_noise.hip; one workgroup per plane): out + i*out_stride receives
 * RandomState(seeds[i]).normal(loc, scale, count).astype(uint8).  flags[i] (int32, device): 0 = the plane is numpy's
 * byte for byte; 1 = some value lay within 1e-9 of an integer, where the last bit of log() decides the cast — make
 * that plane with lf_legacy_normal_u8; 2 = ran out of attempts (cannot happen for count >= 16; same remedy). */
int lf_legacy_normal_batch_u8(const uint32_t* seeds, double loc, double scale, size_t count, uint8_t* out,
                              size_t out_stride, int n, int* flags, lf_stream_t stream);

/* ------------------------------------------------------------------------- */
/* Geometric ops (Pillow semantics, bit-exact; coordinates in IEEE double)    */
/* ------------------------------------------------------------------------- */

/* Image.transform(size, AFFINE|PERSPECTIVE, coeffs, BICUBIC) (image_augmenter.py:44-94).
 * coeffs[n][8] double (affine uses the first 6, a6 = a7 = 0), output same size,
 * outside pixels black.  `perspective` bit 0: PERSPECTIVE (vs AFFINE) map; bit 1: hint that
 * the maps are axis-aligned scales (a1 = a3 = 0, e.g. ImageAugmenter.skew) — selects a kernel
 * that reuses horizontally interpolated rows down a column; the hint is verified per image
 * and never changes results. */
int lf_warp_bicubic_u8(const uint8_t* in, uint8_t* out, const double* coeffs, int perspective,
                       int n, int h, int w, lf_stream_t stream);

/* Image.rotate(angle, expand=True, fillcolor="white") NEAREST path
 * (image_augmenter.py:37): Pillow's 16.16 fixed-point affine.  fix6[n][6] are the
 * int32 fixed-point coefficients a0,a1,a2',a3,a4,a5' computed on the host exactly as
 * Pillow's affine_fixed does.  in: [n][h][w][3].  The output is a ragged batch (the
 * expanded canvas depends on the angle): image i writes ohw[i] = (oh, ow) pixels,
 * packed RGB, at byte offset out_off[i] of `out`; pixels whose source falls outside
 * get `fill`.  max_out_pixels = max_i oh*ow sizes the grid. */
int lf_affine_nearest_fixed_u8(const uint8_t* in, uint8_t* out, const int32_t* fix6,
                               const int32_t* ohw, const int64_t* out_off, int n, int h, int w,
                               int max_out_pixels, int fill, lf_stream_t stream);

/* Pillow two-pass separable resample with 8-bit intermediates and 22-bit
 * fixed-point coefficients (Image.resize(..., LANCZOS), image_utils.py:109-114,
 * image_augmenter.py:110).  bounds/coefficients are computed on the host exactly as
 * Resample.c's precompute_coeffs + normalize_coeffs_8bpc do; a crop box is folded into
 * them (xmin/ymin index the uncropped image).
 * Horizontal pass: in [n][h][w][3] -> tmp [n][h][ow][3]; vertical: -> out [n][oh][ow][3].
 * xbounds [ow][2] = (xmin, count), xk [ow][kx]; ybounds [oh][2], yk [oh][ky] (int32);
 * with per_image_coeffs != 0 each table has a leading [n] dimension.  Coefficients must
 * satisfy |k| < 2^23 (normalised 22-bit weights always do): the kernels multiply with
 * full-rate 24-bit operands. */
int lf_resample_u8(const uint8_t* in, uint8_t* tmp, uint8_t* out, int n, int h, int w, int oh,
                   int ow, const int32_t* xbounds, const int32_t* xk, int kx,
                   const int32_t* ybounds, const int32_t* yk, int ky, int per_image_coeffs,
                   lf_stream_t stream);

/* The same resample with both passes fused in one kernel (32x32 output tiles, the tile's input
 * window and the 8-bit intermediate kept in LDS; no tmp buffer).  Preconditions: kx, ky <= 10,
 * ow % 4 == 0, and the windows of any 32 consecutive outputs span at most 48 inputs on either
 * axis (crop -> resize back, scales up to ~1.25); the host checks the last one on its tables
 * before choosing this entry (ops.crop_resize_plan).  Bit-identical to lf_resample_u8. */
int lf_resample_tile_u8(const uint8_t* in, uint8_t* out, int n, int h, int w, int oh, int ow,
                        const int32_t* xbounds, const int32_t* xk, int kx, const int32_t* ybounds,
                        const int32_t* yk, int ky, int per_image_coeffs, lf_stream_t stream);

/* Image.resize((S, S), LANCZOS) for images of DIFFERENT sizes in one launch: what the reference's loader does one
 * file after the other (`resize_image`, srcs/utils/image_utils.py:109-114, called from srcs/dataio/sequence.py:74-125
 * and the predictor), for a chunk of an augmented tree whose rotate(expand=True) canvases each have a size of their
 * own.  The fused kernel of lf_resample_tile_u8 with the geometry taken per image; bit-identical to lf_resample_u8.
 * lf_resample_item, one per image (the same array on the device for the kernel and on the host for the checks before
 *   the launch): in_off = where its tightly packed [h][w][3] pixels start in `in` (any byte: what
 *   lf_jpeg_idct_rgb_items_u8 writes), out_index = the row of `out` [n_out][oh][ow][3] it is written to, tile_start =
 *   the running sum of ceil(oh/32) * ceil(ow/32) over the items before it, xtab / ytab = where its axis tables start
 *   in `tables` (int32 elements), kx / ky = their taps per output.
 * An axis table is [o][2] bounds (start, count) followed by [o][k] coefficients, o = ow (xtab) or oh (ytab), as
 *   lf_resample_u8 takes them; images of one length share one table.  An identity table (count 1, weight 1 << 22)
 *   stands for an axis Pillow skips; both axes identity is an exact copy.
 * Limits: kx, ky <= 16, ow % 4 == 0, out 4-byte aligned, and the windows of any 32 consecutive outputs span at most
 *   96 inputs with starts that do not decrease; the host checks the last on its tables (ops.ResampleTables).
 *   Windows are clamped against the image on the device.  No allocation, no synchronisation.
 * lf_resample_items_fits (HOST): 1 if a h x w image is taken for an oh x ow output — both sides at most 2.5 x the
 *   output's (conservative: a few longer axes would fit the window rule too), ow % 4 == 0. */
typedef struct {
    int64_t in_off;        /* bytes: where the image's [h][w][3] pixels start in `in` (any byte) */
    int64_t tile_start;    /* running sum of ceil(oh/32)*ceil(ow/32) over the items before it */
    int32_t h, w;
    int32_t out_index;     /* row of `out` this image is written to */
    int32_t xtab, ytab;    /* int32 offsets of the axis tables in `tables` */
    int32_t kx, ky;        /* taps per output of each table */
    int32_t reserved;
} lf_resample_item;
int lf_resample_items_fits(int h, int w, int oh, int ow);
int lf_resample_items_u8(const uint8_t* in, size_t in_bytes, uint8_t* out, int n_out, int oh, int ow,
                         const lf_resample_item* items, const lf_resample_item* host_items, int n,
                         const int32_t* tables, size_t table_elems, lf_stream_t stream);

/* cv2.resize(img, (ow, oh), interpolation=cv2.INTER_LANCZOS4) for a same-size batch in [n][h][w][3] ->
 * out [n][oh][ow][3] (the resize of the reference's training transform, srcs/cli/Transformation.py:799-801 and
 * :941-946), with its _apply_light_augmentation (:984-1005) fused into the store.  Eight fixed taps per axis,
 * coefficients short(cvRound(c * 2048)), source index clamp(s - 3 + i, 0, len - 1), a 32-bit horizontal
 * intermediate, (v + (1 << 21)) >> 22 saturated to 8 bits; the 32-bit sums wrap.  The full reading: the comment
 * at the top of lf_resize_cv.hip.  cv2 is not available to check against: parity with it is unpinned.
 * tables (int32, on the device; host_tables = the same values in host memory, read before the launch to size the
 *   tiles): xofs[ow], xcoef[ow][8], yofs[oh], ycoef[oh][8], ofs = floor of the source coordinate (not clamped;
 *   it must not decrease along an axis), as ops.lanczos4_axis_table builds them.  Equal sizes give a copy.
 * aug: null, or [n][4] float64 on the device {use_b, b, use_c, c}: if use_b != 0, p = (uint8)clip(p * b, 0, 255);
 *   then if use_c != 0, p = (uint8)clip((p - 127.5) * c + 127.5, 0, 255), float64 without FMA contraction.
 * Any sizes: output tiles of up to 32 x 32 whose source window is at most 56 x 56 (the tile shrinks with the scale,
 * down to one output).  No allocation, no synchronisation. */
int lf_resize_lanczos4_u8(const uint8_t* in, uint8_t* out, int n, int h, int w, int oh, int ow,
                          const int32_t* tables, const int32_t* host_tables, const double* aug,
                          lf_stream_t stream);

/* ------------------------------------------------------------------------- */
/* A2 — leaf_cnn conv stack (fp32, NCHW activations)                           */
/* ------------------------------------------------------------------------- */
/* Conv weights are kept in "IKO" layout [Cin][k*k][Cout] (tap = ky*k + kx); the keras
 * HWIO kernel [k][k][Cin][Cout] maps to it by a transpose at the artifact boundary. */

/* keras Conv2D(cout, ksize, padding="same", use_bias=False) forward
 * (srcs/model/cnn.py:27-29,44): y[n][co] = sum_{ci,tap} w[ci][tap][co] * x[n][ci] (cross-
 * correlation, zero padding).  Optional fused input prologue (both pointers non-null):
 * x' = x*in_scale[ci] + in_shift[ci], then relu if in_relu — the producer's
 * BatchNorm(+ReLU) applied while staging (cnn.py:30-31); padding stays exactly zero.
 * Implicit GEMM on v_mfma_f32_32x32x2_f32: result equals an fp32 fmaf chain over
 * k = (ci, tap) in ascending order.  Tolerance vs fp32 torch conv2d: 1e-4 relative.
 * dgrad is the same call on dy with lf_conv2d_dgrad_weights_f32's output; accumulate != 0
 * adds into y (residual gradient joins) instead of overwriting it.
 * Every 3x3 convolution but the Cin <= 4 stem (lf_conv2d_takes_wino_filters != 0) computes Winograd
 * F(2x2,3x3) and reads its filters already transformed: wino_u from lf_conv2d_wino_filters_f32 (below) is
 * required, w is not read and may be null.  Without wino_u such a call returns LF_ERR_INVALID and launches
 * nothing.  All other calls read w and ignore wino_u.  The same holds for lf_conv2d_stats_f32 and
 * lf_conv2d_bnbwd_f32. */
int lf_conv2d_f32(const float* x, const float* w, float* y, int n, int cin, int h, int wd, int cout,
                  int ksize, const float* in_scale, const float* in_shift, int in_relu,
                  int accumulate, lf_stream_t stream, const float* wino_u);

/* The same forward convolution with both operands rounded to bf16 (round to nearest even) while
 * staging and fp32 accumulation on v_mfma_f32_32x32x16_bf16 — the reduced-precision inference mode
 * (the reference predicts under Keras' mixed_float16 policy by default, train.py:53-117;
 * BASELINE configs[4]).  x and y stay fp32 NCHW, so every other kernel of the forward pass is
 * shared with the fp32 path.  Weights are packed once per model with
 * lf_conv2d_bf16_prep_weights: fp32 IKO [cin][k*k][cout] -> bf16 [ceil(cin/16)][k*k][cout][16]
 * (lf_conv2d_bf16_weight_elems uint16 elements, channels past cin zero).  Requires w % 4 == 0,
 * cout % 32 == 0 (lf_conv2d_bf16_act with bf16 output also takes cout == 16 with w % 8 == 0 and cin <= 3 in fp32
 * or cin 16 / 32 in bf16; 1x1: cin 32), ksize 1 or 3.  Tolerance vs lf_conv2d_f32: bf16 operand rounding, 2^-8
 * relative per product (tests bound the error by 2e-2 of the output's scale). */
size_t lf_conv2d_bf16_weight_elems(int cin, int cout, int ksize);
int lf_conv2d_bf16_prep_weights(const float* w_iko, uint16_t* wprep, int cin, int cout, int ksize,
                                lf_stream_t stream);
int lf_conv2d_bf16_f32(const float* x, const uint16_t* wprep, float* y, int n, int cin, int h, int wd,
                       int cout, int ksize, const float* in_scale, const float* in_shift, int in_relu,
                       lf_stream_t stream);

/* The reduced-precision forward pass with bf16 ACTIVATION STORAGE as well (what mixed_float16
 * keeps between layers): the same convolution reading and / or writing bf16 NCHW tensors
 * (x_bf16 / y_bf16 flags; the fused prologue and the accumulation stay fp32).  The block's plane
 * kernels on bf16 tensors are those of the training step below: lf_gap_stats_bf16 without mask
 * sums, and lf_block_tail_fwd_train_bf16 without dropout or route bytes.
 * out_scale / out_shift / out_relu: optional epilogue v*out_scale[co]+out_shift[co] (+ReLU) on the
 * fp32 accumulators — at inference the layer's folded BatchNorm(+ReLU), so that what is stored is
 * the activation itself and the consumer needs no prologue (a bf16 input without prologue is staged
 * by interleaving the stored bits, no arithmetic).  The tail's a_scale / a_shift may then be null
 * (y holds relu(BN(.)) already). */
int lf_conv2d_bf16_act(const void* x, int x_bf16, const uint16_t* wprep, void* y, int y_bf16, int n,
                       int cin, int h, int wd, int cout, int ksize, const float* in_scale,
                       const float* in_shift, int in_relu, const float* out_scale,
                       const float* out_shift, int out_relu, lf_stream_t stream);
/* The block's second convolution at inference TOGETHER WITH the squeeze of its SE gate (cnn.py:33-41:
 * GlobalAveragePooling2D over relu(BN(conv2))): stores the bf16 activation like lf_conv2d_bf16_act and
 * leaves means[n][co] = mean over the plane of the STORED (rounded) values — summed in the
 * convolution's epilogue, per image, so the activation is not read back from memory for the pool
 * (lf_gap_stats_bf16 remains for everything else).  Workspace: lf_conv2d_bf16_act_mean_workspace bytes. */
size_t lf_conv2d_bf16_act_mean_workspace(int n, int cin, int h, int wd, int cout, int ksize, int x_bf16);
int lf_conv2d_bf16_act_mean(const void* x, int x_bf16, const uint16_t* wprep, uint16_t* y, int n, int cin,
                            int h, int wd, int cout, int ksize, const float* in_scale,
                            const float* in_shift, int in_relu, const float* out_scale,
                            const float* out_shift, int out_relu, float* means, void* workspace,
                            size_t ws_bytes, lf_stream_t stream);

/* ------------------------------------------------------------------------- */
/* A2 — class activation maps: where on the leaf a prediction comes from      */
/* ------------------------------------------------------------------------- */
/* The reference explains nothing: its ImageProcessor pastes a display-only Mask picture beside the prediction
 * (srcs/predict/predictor.py:46,99).  leaf_cnn ends in MaxPool -> GlobalAveragePooling2D -> Dense
 * (srcs/model/cnn.py:96-101), so the class activation map of Zhou et al. (CVPR 2016) is an identity here:
 *     logit_c = b_c + mean_{y,x} cam_c(y,x),    cam_c(y,x) = sum_k W[k][c] * F[k][y][x]
 * with F the last stage's pooled output and W the dense kernel.
 *
 * lf_cam_maps: up to 8 class slots per image in one pass over the features.
 *   feat     [N][K][h][w] NCHW, fp32 or bf16 (feat_bf16 != 0), read once whatever m is;
 *   w        [K][C] fp32 (the layout of dense.w);
 *   classes  [N][m] int32 on the device, 1 <= m <= 8, values in [0, C), repeats allowed;
 *   classes_host  optional HOST copy of classes: when non-null every value is checked against [0, C) and a value
 *            outside returns LF_ERR_INVALID before anything is launched.  The kernel itself clamps a class into
 *            [0, C), so w is never read outside whatever the device buffer holds;
 *   cam      [N][m][h][w] fp32 = sum_k w[k][classes[n][j]] * feat[n][k]  (no bias);
 *   peak     [N][m] fp32 = max(0, max_{y,x} cam[n][j]).
 * The sum over k is four ascending fmaf chains over consecutive quarters of the channels, added left to right:
 * |cam - exact| <= (K + 2) 2^-24 sum_k |w f|; no atomics, two launches give the same bits.  K <= 512.
 *
 * lf_cam_overlay_u8: slot `slot` of such maps blended into img [N][H][W][3] uint8 -> out (same shape), per pixel
 * in fp32:  sx = (x + 0.5)(w/W) - 0.5 clamped to [0, w-1], x0 = floor(sx), x1 = min(x0+1, w-1), fx = sx - x0, the
 * same in y, v = the bilinear value of cam;  t = peak > 0 ? max(v, 0)/peak : 0  (as max(v, 0) * (1/peak));
 *   r = clamp(1.5 - |4t - 3|, 0, 1),  g = clamp(1.5 - |4t - 2|, 0, 1),  b = clamp(1.5 - |4t - 1|, 0, 1);
 *   a = alpha t;  out = floor(a 255 colour + (1 - a) img + 0.5).
 * A pixel without positive evidence keeps its byte exactly; a map that is nowhere positive returns img.
 * Any H, W, h, w >= 1; 0 <= alpha <= 1; img and out must not overlap.  Against the formulas in float64 a byte may
 * differ by one where the value before the floor lies within 1e-3 of an integer. */
int lf_cam_maps(const void* feat, int feat_bf16, const float* w, const int32_t* classes,
                const int32_t* classes_host, float* cam, float* peak, int n, int k, int h, int wd, int c, int m,
                lf_stream_t stream);
int lf_cam_overlay_u8(const uint8_t* img, const float* cam, const float* peak, uint8_t* out, int n, int hh, int ww,
                      int h, int wd, int m, int slot, float alpha, lf_stream_t stream);

/* ---- Text and canvas: the pictures that carry titles (Transformation's mosaic, create_mosaic in
 * srcs/cli/Transformation.py; predict's montage, PredictionVisualizer.create_montage).  The reference writes its text
 * with cv2.putText (Hershey) and PIL's ImageDraw; neither is available, so the rules below are this project's own
 * integer rules and claim no pixel parity with either.  tests/text_ref.py and tests/canvas_ref.py restate them in
 * numpy; the kernels match them bit for bit.
 *
 * Text.  The font is the project's 5x7 bitmap font (csrc/lf_font5x7.h): 95 glyphs, ASCII 0x20..0x7E, 7 bytes per
 * glyph, one per row, top row first, bit 4 the leftmost of 5 columns; a character is drawn into a cell 6 columns wide
 * (one blank column of advance) and 7 rows high; a byte outside 0x20..0x7E draws as '?'.
 * lf_font5x7 (HOST): copies the 95*7 bytes of the table to `out`.
 *
 * lf_draw_text_u8: n_items strings drawn in place into img [N][H][W][3] uint8, one launch for all of them.
 *   items   [n_items][8] int32 on the device: {image, x, y, first, length, colour, scale, first_group};
 *           the string is chars[first .. first + length), colour = r | g << 8 | b << 16, 1 <= scale <= 8,
 *           0 <= length <= 4096; the table is ordered by image (ascending); first_group is the running sum of
 *           ceil(6*scale*length * 7*scale / 256) over the strings before it (the workgroup the string's box starts at);
 *   items_host  HOST copy of items: every field is checked against the above, the image index against [0, N) and
 *           the characters against chars_bytes, before anything is launched (LF_ERR_INVALID otherwise);
 *   chars   the bytes of all strings on the device.
 * Pixel rule for a string s of length L at origin (x, y) with scale k: with u = px - x and v = py - y, pixel
 * (px, py) is painted iff 0 <= v < 7k, 0 <= u < 6kL, (u mod 6k)/k < 5 and the bit of row v/k, column (u mod 6k)/k of
 * glyph s[u/(6k)] is set.  A painted pixel takes the colour (opaque); nothing else is written.  Pixels outside the
 * image are dropped; negative origins are legal.  Where strings of one image overlap, the string later in the table
 * wins whatever order the hardware runs them in: a lane writes only if no later string of its image paints the pixel.
 * A table of empty strings launches nothing.
 *
 * Canvas.  lf_canvas_tiles_u8: out [N][OH][OW][3] uint8 composed from T source batches in one launch.
 *   plan    int32 block on the device, plan_ints long: T tile descriptors of 12 ints, then the shade rectangles of
 *           6 ints, then the axis tables;  plan_host is its HOST copy, checked in full before the launch.
 *   tile    {dst_x, dst_y, dst_w, dst_h, src_h, src_w, channels, xtab, ytab, ptr_lo, ptr_hi, flags}: source t is
 *           [N][src_h][src_w][channels] uint8 at the device address ptr_hi:ptr_lo, channels 3 or 1 (gray, replicated);
 *           tiles lie inside the canvas and do not overlap; at most 64.  xtab / ytab are the positions in the plan of
 *           the tile's axis tables, dst_w and dst_h entries of {i, k}.  flags bit 0: the tile has its source's size,
 *           three channels and rows of whole dwords, and may be copied with aligned dword loads.
 *   table   for destination index d of D over a source length S: pos = (d + 0.5) * S / D - 0.5 in float64,
 *           i = floor(pos), f = pos - i; i < 0 -> i = 0, f = 0; i >= S - 1 -> i = S - 1, f = 0; k = rint(f * 2048).
 *           The second tap is min(i + 1, S - 1).
 *   pixel   (ky0 * (kx0 * a + kx1 * b) + ky1 * (kx0 * c + kx1 * d) + 2^21) >> 22 with k0 = 2048 - k1, a b the two
 *           taps of row i_y, c d those of the second row, in 32-bit integers.  A tile of its source's own size is an
 *           exact copy.  A pixel in no tile gets fill = r | g << 8 | b << 16.
 *   shade   {x, y, w, h, num, den}, 0 <= num <= den <= 65536, at most 64, applied in table order after the tiles to
 *           every channel of the pixels inside: v' = (v * num + den / 2) / den  (den / 2 and the division truncate).
 * The kernel finishes runs of four pixels (12 bytes, aligned dword stores) when OW, every dst_x and every dst_w are
 * multiples of four and out is 4-byte aligned, single pixels otherwise; the bytes are the same.  Integer arithmetic
 * only, no atomics; two launches give the same bits.  out must not overlap a source. */
int lf_font5x7(uint8_t* out);
int lf_draw_text_u8(uint8_t* img, int n, int h, int w, const int32_t* items, const int32_t* items_host, int n_items,
                    const uint8_t* chars, size_t chars_bytes, lf_stream_t stream);
int lf_canvas_tiles_u8(uint8_t* out, int n, int oh, int ow, const int32_t* plan, const int32_t* plan_host,
                       size_t plan_ints, int n_tiles, int n_shades, int fill, lf_stream_t stream);

/* ---- Charts: Transformation's Hist figure (apply_histogram_filter, srcs/transform/filters/hist.py:181-297) drawn
 * from lf_hsv_region_stats' numbers.  The reference draws it with matplotlib; the rules below are this project's own
 * integer rules and claim no pixel parity with it.  tests/chart_ref.py restates them in numpy; the kernel matches it
 * bit for bit.
 *
 * lf_hist_figure_u8: counts [N][14] int32 and hsv_hist [N][3][256] int32 (lf_hsv_region_stats' outputs, on the
 * device) -> out [N][LF_HIST_FIG_H][LF_HIST_FIG_W][3] uint8, the geometry of the figure: every pixel of out is
 * written, none outside it.  The lettering is a second launch (lf_draw_text_u8) the host formats from the 14 counts
 * (transform.hist_figure_texts).  Null pointers and n <= 0 are refused before any launch.
 *
 * The figure is 960 x 640 on white (255, 255, 255), four panels of 480 x 320: (column 0, row 0) the colour regions,
 * (1, 0) the HSV histograms, (0, 1) the summary (text only: the kernel leaves it white), (1, 1) the hue ranges.  Each
 * chart panel has a plot rectangle {x0, y0, PW, PH} in figure coordinates (the LF_CHART_*_RECT constants); below,
 * (lx, ly) = (x - x0, y - y0), and every division truncates.
 *   Frame   the pixels with lx = -1, lx = PW, ly = -1 or ly = PH and -1 <= lx <= PW, -1 <= ly <= PH are black: the
 *           frame lies around the plot rectangle, so nothing drawn inside touches it.
 *   Grid    inside the rectangle, the columns lx = k PW / 4 and the rows ly = k PH / 4, k = 1, 2, 3, are LF_CHART_GRID.
 *   Regions eight horizontal bars, bar i (counts[1 + i], REGION_KEYS order) in the rows LF_CHART_REGION_SLOT * i +
 *           [LF_CHART_REGION_BAR_LO, LF_CHART_REGION_BAR_HI) and the columns lx < len, in LF_CHART_REGION_COLOURS[i]:
 *           with total = counts[0], len = (min(max(c, 0), total) * PW + total / 2) / total in int64, 0 when total <= 0.
 *           No minimum length.
 *   Hues    five vertical bars, bar i (counts[9 + i], HUE_KEYS order) in the columns LF_CHART_HUE_SLOT * i +
 *           [LF_CHART_HUE_BAR_LO, LF_CHART_HUE_BAR_HI) and the rows ly >= PH - hgt, in LF_CHART_HUE_COLOURS[i]: with
 *           m = max(1, the largest of the five max(c, 0)), hgt = (max(c, 0) * PH + m / 2) / m in int64.
 *   HSV     each of the H, S, V histograms (entries below zero count as zero) is summed into 64 bins of four values,
 *           in int64; ymax = max(1, the largest of the 192 bins).  Bin j has its point at lx = LF_CHART_HSV_PITCH * j +
 *           LF_CHART_HSV_PITCH / 2, ly = PH - 2 - hp with hp = (min(b, ymax) * (PH - 3) + ymax / 2) / ymax: the span
 *           PH - 3 keeps a thick segment (one pixel around its points) inside the rectangle.  A curve is the 63 thick
 *           segments ("Drawing rules" above: distance <= 1, int64 terms) between neighbouring points, in tab:orange
 *           (255, 127, 14) for H, tab:green (44, 160, 44) for S, tab:blue (31, 119, 180) for V; a channel whose 64
 *           bins are all zero has no curve.  Markers: the columns lx = (LF_CHART_HSV_PITCH * v + 3) / 4 for hue
 *           v = 15, 35, 85 are LF_CHART_MARKER in the rows with ly mod 8 < 4 (dashed).
 *   Order   background, grid, markers, frames, region and hue bars, curves H, S, V: the later wins.  A pixel's colour
 *           is a function of the image's 14 + 768 numbers and its own coordinates alone: the kernel evaluates the
 *           elements in this order for each pixel (for a curve, the segments whose columns reach it), with no order
 *           between threads and no atomics; two launches give the same bits.
 * The numbers are not trusted: negative counts are zero, a count over its total is the total, and by the formulas a
 * bar or a curve stays inside its plot rectangle whatever they are.  Colours are r | g << 8 | b << 16. */
#define LF_HIST_FIG_H 640
#define LF_HIST_FIG_W 960
#define LF_CHART_PANEL_W 480
#define LF_CHART_PANEL_H 320
#define LF_CHART_REGIONS_RECT {110, 40, 300, 240}
#define LF_CHART_HSV_RECT {528, 40, 384, 240}
#define LF_CHART_HUES_RECT {520, 370, 400, 220}
#define LF_CHART_REGION_SLOT 30
#define LF_CHART_REGION_BAR_LO 5
#define LF_CHART_REGION_BAR_HI 25
#define LF_CHART_HUE_SLOT 80
#define LF_CHART_HUE_BAR_LO 16
#define LF_CHART_HUE_BAR_HI 64
#define LF_CHART_HSV_PITCH 6
#define LF_CHART_GRID 0xe0e0e0
#define LF_CHART_MARKER 0x808080
#define LF_CHART_CURVE_COLOURS {0x0e7fff, 0x2ca02c, 0xb4771f}
#define LF_CHART_REGION_COLOURS {0x327d2e, 0x32cd9a, 0x00d7ff, 0x3f85cd, 0x3c14dc, 0x4f4f2f, 0xdec4b0, 0xd30094}
#define LF_CHART_HUE_COLOURS {0x3ca03c, 0x00a5ff, 0x2827d6, 0xbd6794, 0x7f7f7f}
int lf_hist_figure_u8(const int32_t* counts, const int32_t* hsv_hist, uint8_t* out, int n, lf_stream_t stream);

/* ------------------------------------------------------------------------- */
/* A2 — the mixed-precision TRAINING step (bf16 storage, fp32 arithmetic)      */
/* ------------------------------------------------------------------------- */
/* The reference trains under keras.mixed_precision.set_global_policy("mixed_float16") unless
 * --no-mixed-precision is given (srcs/cli/train.py:179-190): layer outputs and gradients are
 * 16-bit, variables, BatchNorm statistics, softmax / loss and the optimizer are fp32.  BASELINE
 * configs[3] asks for that step in bf16.  Here: every activation / gradient tensor in HBM is bf16
 * NCHW, every MFMA operand is bf16 (v_mfma_f32_32x32x16_bf16, fp32 accumulators), all other
 * arithmetic is fp32, master weights / Adam state / BatchNorm state are fp32.  A value is rounded
 * (nearest even) exactly where it is stored or staged as an operand, and every statistic a later
 * kernel relies on is taken over the ROUNDED values.  Tolerance vs the fp32 step: bf16 operand
 * rounding (2^-9 relative per element); vs oracle/cnn_ref.py evaluated with the same rounding
 * points the tests bound each gradient tensor's error norm (tests/test_train_bf16_gpu.py).
 *
 * lf_conv2d_bf16_train: forward convolution (Conv2D, cnn.py:27-29) or input-gradient convolution
 * (the same call on dY with lf_conv2d_dgrad_weights_f32 -> lf_conv2d_bf16_prep_weights) writing
 * bf16; x is fp32 (x_bf16 = 0: the normalised network input) or bf16; optional prologue
 * relu?(x*in_scale+in_shift) = the producer's BatchNorm(+ReLU) (cnn.py:30-31); accumulate != 0:
 * y = bf16(conv + y) (residual gradient joins).  tile_part (may be null) receives per-(channel,
 * part) sums, part < lf_conv2d_bf16_stats_tiles(...) — one per tile, or one per workgroup on the
 * streaming path that serves Cin, Cout <= 64 —, layout [cout][parts][2]:
 *   mask_y == null: BatchNormalization forward statistics {sum (y-pivot), sum (y-pivot)^2}
 *     (feed lf_bn_train_stats_tiles_f32; pivot = the moving mean, may be null);
 *   mask_y != null: the backward sums of the BatchNorm this gradient feeds, {sum d, sum d*mask_y}
 *     with d = y*[mask_y*mask_scale+mask_shift > 0 or !mask_relu] (feed lf_bn_bwd_sums_tiles_f32).
 * Requires w % 4 == 0, ksize 1 or 3, 16-byte aligned x / wprep, and cout % 32 == 0 or else cout == 16 with
 * w % 8 == 0 and an input of cin <= 3 in fp32 (3x3) or cin 16 (3x3) / 32 (3x3, 1x1) in bf16 — the layers of a
 * 16-wide stage and the input gradients that flow into it, which only the streaming path serves. */
long long lf_conv2d_bf16_stats_tiles(int n, int cin, int h, int w, int cout, int ksize, int x_bf16);
int lf_conv2d_bf16_train(const void* x, int x_bf16, const uint16_t* wprep, uint16_t* y, int n, int cin,
                         int h, int w, int cout, int ksize, const float* in_scale,
                         const float* in_shift, int in_relu, int accumulate, float* tile_part,
                         size_t tile_part_bytes, const float* pivot, const uint16_t* mask_y,
                         const float* mask_scale, const float* mask_shift, int mask_relu,
                         lf_stream_t stream);

/* Conv2D weight gradient dw[cin][k*k][cout] (fp32, overwritten) from bf16 tensors, K = pixels on
 * the bf16 MFMA with fp32 partial slabs summed in a fixed order (deterministic).  x: the conv's
 * input as stored (bf16; fp32 when cin*9 <= 32, the stem) with the optional prologue
 * relu?(x*in_scale+in_shift); g: dY itself, or — with bn_y — the gradient w.r.t. the output of the
 * BatchNormalization(+ReLU) that follows the conv, in which case the BatchNorm backward is formed
 * while staging exactly as lf_conv2d_wgrad_bn_f32 does (alpha_nc / add_nc [n][cout] optional,
 * coef [5][cout] from lf_bn_bwd_sums*_f32) and dY is also written to dy_out (bf16, may be null)
 * for the input-gradient convolution.  Requires w % 4 == 0, cout == 16 or cout % 32 == 0, cin % 4 == 0
 * (or the stem), 16-byte aligned tensors.  workspace >= lf_conv2d_wgrad_bf16_workspace(...) bytes. */
size_t lf_conv2d_wgrad_bf16_workspace(int n, int cin, int h, int w, int cout, int ksize);
int lf_conv2d_wgrad_bf16(const void* x, const uint16_t* g, const uint16_t* bn_y, const float* alpha_nc,
                         const float* add_nc, const float* coef, int bn_relu, uint16_t* dy_out,
                         float* dw, int n, int cin, int h, int w, int cout, int ksize,
                         const float* in_scale, const float* in_shift, int in_relu, void* workspace,
                         size_t ws_bytes, lf_stream_t stream);

/* The plane kernels of the training step on bf16 tensors — the arithmetic of lf_gap_f32 (with
 * mask_sums), lf_block_tail_fwd_f32 (route bytes, SpatialDropout2D keep-scales),
 * lf_block_tail_bwd_f32 and lf_bcast_planes_f32 (cnn.py:35-49,94-101), fp32 after widening;
 * pooled / dr / out are rounded to bf16 where stored and the per-plane sums are over the rounded
 * gradient.  hw % 4 == 0, w % 4 == 0, h even.  lf_block_tail_fwd_train_bf16 takes route = NULL when
 * no backward pass follows (inference). */
int lf_gap_stats_bf16(const uint16_t* x, float* out, float* mask_sums, int n, int c, int hw,
                      const float* scale, const float* shift, int relu, lf_stream_t stream);
int lf_block_tail_fwd_train_bf16(const uint16_t* y, const float* a_scale, const float* a_shift,
                                 const float* s, const uint16_t* sc, const float* sc_scale,
                                 const float* sc_shift, int sc_relu, const float* drop, uint8_t* route,
                                 uint16_t* pooled, int n, int c, int h, int w, lf_stream_t stream);
int lf_block_tail_bwd_bf16(const uint16_t* dp, const uint8_t* route, const uint16_t* y,
                           const float* a_scale, const float* a_shift, const float* drop, uint16_t* dr,
                           float* ds, float* plane_sums, const uint16_t* sc_y, float* sc_sums, int n,
                           int c, int h, int w, lf_stream_t stream);
int lf_bcast_planes_bf16(const float* v, uint16_t* out, int planes, int hw, float scale,
                         lf_stream_t stream);
/* fp32 <-> bf16 (round to nearest even) of a flat buffer: the data-parallel gradient bucket
 * crosses xGMI as bf16 (2.5 MB instead of 5 MB). */
int lf_cast_f32_bf16(const float* in, uint16_t* out, size_t count, lf_stream_t stream);
int lf_cast_bf16_f32(const uint16_t* in, float* out, size_t count, lf_stream_t stream);

/* Which tile variant (template instantiation) the dispatcher picks for a shape — used by
 * bench.py to attribute measured launch durations to kernel names.  (For H = 28 the 28x8
 * variant walks two images as one strip; lf_conv2d_stats_tiles accounts for that.) */
int lf_conv2d_variant(int h, int wd, int cout, int ksize);
int lf_conv2d_wgrad_variant(int n, int cin, int h, int wd, int cout, int ksize);

/* Plan queries: which kernel and which code path the dispatchers take for a launch, computed by the
 * same host functions the launchers use.  Host only: they launch nothing and need no device (the
 * coverage test tests/test_conv_plans.py compares the benchmark's layers with the tested shapes).
 * lf_conv2d_plan (lf_conv2d_f32 / _stats_f32 / _bnbwd_f32), out[4]:
 *   {variant, Cin <= 4 stem instantiation, images per strip (stack), vector path by shape}
 *   Arithmetic: every 3x3 plan but the stem's (out[1] = 1) computes Winograd F(2x2,3x3) on the
 *   variant's spatial tile (32 output channels per workgroup, 16 for variant 6); the stem and all
 *   1x1 plans compute the direct implicit GEMM.  The choice depends on ksize and out[0..1] only.
 * lf_conv2d_wgrad_plan (lf_conv2d_wgrad_f32 / _bn_f32), out[4]:
 *   {variant (5 = small-Cin), items per split (1, 2 or 3 = three or more), reduce stages (1 or 2),
 *    fused BN allowed}
 * lf_conv2d_bf16_plan (entry 0 = lf_conv2d_bf16_act, 1 = _act_mean, 2 = _train; accumulate and mask
 * as passed to _train), out[14]:
 *   {streaming, TAPS, CI, NCO (0: one 16-channel block), NB, TW, TH, XBF, YBF, TR, RMW (streaming) or WIDE (K-chunked),
 *    segments > 1, interleave, units per workgroup > 1}   (fields a kernel has not are 0)
 * lf_conv2d_wgrad_bf16_plan (lf_conv2d_wgrad_bf16), out[13]:
 *   {TAPS, TW, TH, CIB, COB, STEM, G, WPRQ, segments > 1, interleave, units per workgroup > 1,
 *    reduce stages, tiles per unit (1, 2 or 3 = three or more)} */
int lf_conv2d_plan(int n, int cin, int h, int wd, int cout, int ksize, int* out);
int lf_conv2d_wgrad_plan(int n, int cin, int h, int wd, int cout, int ksize, int* out);
int lf_conv2d_bf16_plan(int n, int cin, int h, int w, int cout, int ksize, int x_bf16, int y_bf16, int entry,
                        int accumulate, int mask, int* out);
int lf_conv2d_wgrad_bf16_plan(int n, int cin, int h, int w, int cout, int ksize, int* out);

/* Conv2D followed by BatchNormalization in training mode (cnn.py:28-33,40-45): the same
 * convolution, and in its epilogue the per-tile sums of (y - pivot[co]) and (y - pivot[co])^2 for
 * every output channel -> tile_part[co][tile][2] (tile < lf_conv2d_stats_tiles(...)).  pivot
 * (device, [cout], may be null) only conditions the sum of squares; pass the layer's moving
 * mean.  lf_bn_train_stats_tiles_f32 (below) turns the tile sums into the batch statistics, so
 * the activation is not read again. */
long long lf_conv2d_stats_tiles(int n, int cin, int h, int w, int cout, int ksize);
int lf_conv2d_stats_f32(const float* x, const float* w, float* y, int n, int cin, int h, int wd,
                        int cout, int ksize, const float* in_scale, const float* in_shift,
                        int in_relu, const float* pivot, float* tile_part, size_t tile_part_bytes,
                        lf_stream_t stream, const float* wino_u);

/* Input-gradient convolution whose output g feeds a BatchNormalization backward (mask_y = that
 * BN's input, same shape as y): besides y (= conv, or y += conv with accumulate) the epilogue
 * leaves per-tile {sum d, sum d*mask_y}, d = y*[mask_y*mask_scale[co]+mask_shift[co] > 0 or
 * !mask_relu], in tile_part[co][tile][2] for lf_bn_bwd_sums_tiles_f32 — the BN backward's
 * reduction pass over g and its input disappears. */
int lf_conv2d_bnbwd_f32(const float* x, const float* w, float* y, int n, int cin, int h, int wd,
                        int cout, int ksize, int accumulate, const float* mask_y,
                        const float* mask_scale, const float* mask_shift, int mask_relu,
                        float* tile_part, size_t tile_part_bytes, lf_stream_t stream, const float* wino_u);

/* w [Cin][k*k][Cout] -> wt [Cout][k*k (flipped)][Cin]: the weights with which
 * lf_conv2d_f32(dy, wt, dx, n, cout, h, w, cin, k, ...) is the input gradient. */
int lf_conv2d_dgrad_weights_f32(const float* w, float* wt, int cin, int ksize, int cout,
                                lf_stream_t stream);

/* The 3x3 filters w [cin][9][cout] in the Winograd F(2x2,3x3) domain, U = G g G^T (16 floats per filter,
 * index row*4+col; additions and halvings only, so the bits do not depend on where it is computed):
 *   dgrad == 0: u [cin][cout][16], the wino_u of the forward convolution with w;
 *   dgrad != 0: u [cout][cin][16] from the flipped taps, the wino_u of the input-gradient convolution
 *               lf_conv2d_f32(dy, ., dx, n, cout, h, w, cin, 3, ...) — equal to dgrad == 0 applied to
 *               lf_conv2d_dgrad_weights_f32's output.
 * u: cin*cout*64 bytes, 16-byte aligned, supplied by the caller.  The weights change once per optimizer
 * step, so one launch per layer and role serves every convolution launch of the step.
 * lf_conv2d_takes_wino_filters: 1 if lf_conv2d_f32 / _stats_f32 / _bnbwd_f32 need wino_u for this shape
 * (cin, cout: the convolution's own). */
int lf_conv2d_takes_wino_filters(int cin, int h, int wd, int cout, int ksize);
int lf_conv2d_wino_filters_f32(const float* w, float* u, int cin, int cout, int dgrad, lf_stream_t stream);

/* Weight gradient dw[ci][tap][co] = sum_{n,y,x} x'[n][ci][y+ky-1][x+kx-1] * dy[n][co][y][x]
 * (x' = optional prologue as above) in two steps: lf_conv2d_wgrad_f32 writes one partial
 * slab per workgroup into a workspace of lf_conv2d_wgrad_workspace(...) bytes;
 * lf_conv2d_wgrad_reduce_f32 sums them in a fixed order (two-stage when there are many):
 * dw = beta*dw + sum (deterministic, no float atomics; the workspace tail is scratch). */
size_t lf_conv2d_wgrad_workspace(int n, int cin, int h, int wd, int cout, int ksize);
int lf_conv2d_wgrad_f32(const float* x, const float* dy, int n, int cin, int h, int wd, int cout,
                        int ksize, const float* in_scale, const float* in_shift, int in_relu,
                        void* workspace, size_t ws_bytes, lf_stream_t stream);
int lf_conv2d_wgrad_reduce_f32(void* workspace, float* dw, int n, int cin, int h, int wd,
                               int cout, int ksize, float beta, lf_stream_t stream);
/* Weight gradient whose dY operand is a BatchNormalization backward, formed on the fly:
 * dY = coef2*dz + coef3*bn_y + coef4, dz = (g*alpha_nc+add_nc)*[bn_y*coef0+coef1 > 0 or !bn_relu]
 * (coef from lf_bn_bwd_sums_f32), also written to dy_out [n][cout][h][w] (may be null: the stem
 * has no input gradient) for the input-gradient convolution that follows.  3x3 (the small-Cin
 * stem kernel included) and 1x1, shapes for which lf_conv2d_wgrad_bn_supported() != 0; same
 * workspace and reduce step as lf_conv2d_wgrad_f32. */
int lf_conv2d_wgrad_bn_supported(int n, int cin, int h, int w, int cout, int ksize);
int lf_conv2d_wgrad_bn_f32(const float* x, const float* g, const float* bn_y,
                           const float* alpha_nc, const float* add_nc, const float* coef,
                           int bn_relu, float* dy_out, int n, int cin, int h, int w, int cout,
                           int ksize, const float* in_scale, const float* in_shift, int in_relu,
                           void* workspace, size_t ws_bytes, lf_stream_t stream);

/* Backward of a projection shortcut (1x1 conv + BatchNormalization) in one pass over x, g and bn_y:
 *   dyp = coef2*dz + coef3*bn_y + coef4, dz = g*[bn_y*coef0+coef1 > 0 or !bn_relu]   (the dy_out of
 *         lf_conv2d_wgrad_bn_f32 without alpha_nc / add_nc, bit for bit; kept on chip, never written)
 *   dw[ci][co] = sum_{n,px} x[n][ci][px] * dyp[n][co][px]       (overwritten)
 *   dx[n][ci][px] = sum_co w[ci][co] * dyp[n][co][px]           (overwritten; accumulate onto it afterwards)
 * x [n][cin][h*w] is the conv's input as it stands (no prologue), g / bn_y [n][cout][h*w], coef [5][cout] from
 * lf_bn_bwd_sums*_f32, w [cin][1][cout].  Both products run on the fp32 MFMA; the weight gradient is summed
 * from one slab per workgroup in a fixed order (no float atomics: the same inputs give the same bits).
 * It replaces lf_conv2d_wgrad_bn_f32 (ksize 1, dy_out) + lf_conv2d_wgrad_reduce_f32 + lf_conv2d_dgrad_weights_f32
 * + lf_conv2d_f32, which stay the route for every shape it does not take.
 * lf_conv2d_proj_bwd_supported != 0 requires: cin 32 or 64 and cout == 2*cin (the filter bank is held in
 * registers; so cin, cout % 32 == 0 and cin*cout <= 8192), h*w % P == 0 with P = 64 pixels per work item,
 * cout*h*w < 2^30, and x, g, bn_y, w, dx non-null and 16-byte aligned (only their addresses are looked at).
 * The caller keeps the four-call route for everything else; lf_conv2d_proj_bwd_f32 rejects it.
 * lf_conv2d_proj_bwd_plan (host only, supported shapes): out[3] = {P, items per workgroup (1, 2, 3 = three
 * or more), slab reduce stages (1 or 2)}.  workspace >= lf_conv2d_proj_bwd_workspace(...) bytes (0: unsupported). */
int lf_conv2d_proj_bwd_supported(const float* x, const float* g, const float* bn_y, const float* w,
                                 const float* dx, int n, int cin, int h, int wd, int cout);
int lf_conv2d_proj_bwd_plan(int n, int cin, int h, int wd, int cout, int* out);
size_t lf_conv2d_proj_bwd_workspace(int n, int cin, int h, int wd, int cout);
int lf_conv2d_proj_bwd_f32(const float* x, const float* g, const float* bn_y, const float* coef, int bn_relu,
                           const float* w, float* dx, float* dw, int n, int cin, int h, int wd, int cout,
                           void* workspace, size_t ws_bytes, lf_stream_t stream);

/* Depthwise 3x3 convolution, padding "same", depth multiplier 1, no bias: the first half of the separable
 * conv block (srcs/model/cnn.py:22-25, SeparableConv2D); the pointwise half is lf_conv2d_* with ksize == 1.
 *   y[n][c][i][j] = sum_t w[c][t] * a[n][c][i+ky-1][j+kx-1],  t = ky*3+kx,  w [C][9],
 * a = relu?(x*in_scale[c]+in_shift[c]) being the producer's BatchNorm(+ReLU) applied while loading (in_scale /
 * in_shift both null or both set); a tap outside the image adds 0, not relu(in_shift).  x, y [n][c][h][w]; any
 * h, w >= 1 (16-byte rows where w % 4 == 0 and x, y are 16-byte aligned, single columns otherwise).
 * Constraints: n <= 65535, h*w < 2^30, n*c*w < 2^31.  y must not overlap x.
 * The reference hands the block's kernel_regularizer to this layer, for which Keras has no such argument: this
 * project reads it as L2 on BOTH kernels of a separable conv block, depthwise and pointwise, and on nothing else. */
int lf_dwconv3x3_f32(const float* x, const float* w, float* y, int n, int c, int h, int wd,
                     const float* in_scale, const float* in_shift, int in_relu, lf_stream_t stream);
/* Both gradients of lf_dwconv3x3_f32 (cnn.py:22-25) in one pass over dy and x:
 *   dw[c][t]       = sum_{n,i,j} dy[n][c][i][j] * a[n][c][i+ky-1][j+kx-1]        (overwritten)
 *   dx[n][c][i][j] (+)= sum_t w[c][t] * dy[n][c][i-ky+1][j-kx+1]
 * dx is the gradient with respect to a, not x (the producer's BatchNorm backward applies the ReLU mask), as with
 * the dense input-gradient convolution; accumulate != 0 adds into dx; dx may be null (the stem), and then nothing
 * but dw and the workspace is written.  dw is deterministic: every lane leaves its nine partial sums in the
 * workspace (lf_dwconv3x3_bwd_workspace(...) bytes, 4-byte aligned) and a second kernel adds them in a fixed
 * order; no float atomics.  Constraints as for the forward; dx must not overlap x or dy. */
size_t lf_dwconv3x3_bwd_workspace(int n, int c, int h, int wd);
int lf_dwconv3x3_bwd_f32(const float* x, const float* w, const float* dy, float* dx, int accumulate, float* dw,
                         int n, int c, int h, int wd, const float* in_scale, const float* in_shift, int in_relu,
                         void* workspace, size_t ws_bytes, lf_stream_t stream);

/* Knowledge distillation: the head (lf_head_fwd_f32 / lf_head_bwd_f32 below) with a soft-target term from a
 * teacher's probabilities tprobs [n][c].  Per sample, with z = feat w + b, y = ytrue, T = temperature > 0 (finite),
 * 0 <= alpha <= 1:
 *   p    = softmax(z)                      p_T = softmax(z / T)
 *   lt_j = log(max(tprobs_j, FLT_MIN))     q_T = softmax(lt / T)        FLT_MIN = 1.17549435e-38
 *   hard = -sum_j y_j log(clip(p_j, 1e-7, 1 - 1e-7))                    (lf_head_fwd_f32's loss)
 *   kd   = T^2 sum_j q_T,j (log q_T,j - log p_T,j)                      (both logs as log-softmax)
 *   loss = (1 - alpha) hard + alpha kd
 * Outputs: probs = p, soft [n][c] = p_T - q_T (what the backward entry needs), loss [n], kd [n] (the kd term alone;
 * may be null).  The teacher's probabilities suffice, its logits are not needed: softmax(lt / T) does not depend on
 * the constant that log tprobs drops.  The clamp bounds a class whose teacher probability underflowed to 0: it
 * enters with lt = log FLT_MIN = -87.3, i.e. relative weight exp(-87.3 / T) (3e-10 at T = 4), not with weight zero.
 * The maxima, sums and loss terms are reduced across the 64 lanes of a wave, so probs agrees with lf_head_fwd_f32
 * within rounding, not bit for bit.  c <= 4096. */
int lf_head_distill_fwd_f32(const float* feat, const float* w, const float* b, const float* ytrue,
                            const float* tprobs, float temperature, float alpha, float* probs, float* soft,
                            float* loss, float* kd, int n, int f, int c, lf_stream_t stream);
/* dlogits = [(1 - alpha)(probs - ytrue) + alpha T soft] * inv_n: the gradient of the mean of `loss` over 1 / inv_n
 * samples, with the unclipped rule of lf_head_bwd_f32 for the hard term.  dfeat = dlogits w^T, dw = feat^T dlogits,
 * db = sum_n dlogits, computed as lf_head_bwd_f32 computes them.  T = 1 makes it lf_head_bwd_f32 on the mixed target
 * (1 - alpha) ytrue + alpha tprobs; alpha = 0 makes it lf_head_bwd_f32. */
int lf_head_distill_bwd_f32(const float* feat, const float* w, const float* probs, const float* ytrue,
                            const float* soft, float temperature, float alpha, float* dlogits, float* dfeat,
                            float* dw, float* db, int n, int f, int c, float inv_n, lf_stream_t stream);

/* Class weights and the focal loss: the head (lf_head_fwd_f32 / lf_head_bwd_f32 below) with a weight per class,
 * cw [c] (device memory; null = no weights), and the modulating factor (1 - p)^gamma.  Per sample, with
 * z = feat w + b, p = softmax(z) and y = ytrue, which is soft (label smoothing and mixed targets arrive that way):
 *   s    = sum_j cw_j y_j                                   cw == null: s = 1 exactly
 *   m_j  = (1 - p_j)^gamma                                  gamma == 0: m_j = 1 exactly, also at p_j = 1
 *                                                           (powf(0, 0) is taken as 1)
 *   loss = s sum_j -y_j m_j log(clip(p_j, 1e-7, 1 - 1e-7))  (lf_head_fwd_f32's clip; m_j takes the unclipped p_j)
 * Outputs: probs = p, loss [n], sw [n] = s (the sample's weight, for reporting; may be null).
 * gamma is accepted only if it is 0 or lies in [1, 8]; a NaN, a negative gamma, one in (0, 1) and one above 8 are
 * refused before any launch.  (x -> x^gamma is not Lipschitz at 0 for gamma < 1, and 1 - p loses all its relative
 * accuracy as p -> 1: there is no honest rounding bound in (0, 1).)  The values of cw are the caller's to validate
 * (finite, >= 0, not all zero).  gamma == 0 with cw == null is lf_head_fwd_f32's loss; maxima and sums are reduced
 * across the 64 lanes of a wave, so it agrees within rounding, not bit for bit.  c <= 4096, n > 0, f > 0.
 * Unlike Keras' class_weight, which weighs a sample by cw_label alone, the sample weight here is taken over the
 * target as it arrives: with label smoothing ls it is (1 - ls) cw_label + ls mean(cw), and a mixed target weighs by
 * its mixture.  The loss is divided by the batch size (inv_n below), not by the sum of the weights, as in Keras. */
int lf_head_focal_fwd_f32(const float* feat, const float* w, const float* b, const float* ytrue, const float* cw,
                          float gamma, float* probs, float* loss, float* sw, int n, int f, int c,
                          lf_stream_t stream);
/* The gradient of the mean of `loss` over 1 / inv_n samples, by the unclipped rule, as lf_head_bwd_f32's:
 *   l_j = log(max(p_j, FLT_MIN))                            FLT_MIN = 1.17549435e-38
 *   u_j = y_j (gamma (1 - p_j)^(gamma-1) p_j l_j - m_j)     gamma == 0: u_j = -y_j
 *   dlogits_k = s (u_k - p_k sum_j u_j) inv_n
 * (u_j is p_j d(loss / s)/dp_j, and the softmax Jacobian dp_j/dz_k = p_j ([j == k] - p_k) does the rest.)
 * dfeat = dlogits w^T, dw = feat^T dlogits, db = sum_n dlogits, computed as lf_head_bwd_f32 computes them.  A sample
 * with s == 0 (its classes all have weight 0) gets a dlogits row of exact zeros.  gamma as for the forward entry. */
int lf_head_focal_bwd_f32(const float* feat, const float* w, const float* probs, const float* ytrue,
                          const float* cw, float gamma, float* dlogits, float* dfeat, float* dw, float* db, int n,
                          int f, int c, float inv_n, lf_stream_t stream);

/* Mixup and CutMix: lf_input_stage_f32 (below) writing a blend of two model views per image, and the same blend of
 * the targets.  For a batch of n images of h x w, mix8[i] = {partner, w_out, w_in, y0, y1, x0, x1, t} (device, f32):
 *   A_i  = image i after its own aug4[i] (flip, rotation, contrast about its own mean, clamp) on the [0,1] image:
 *          what lf_input_stage_f32 normalises; A_p the same for image p = partner with aug4[p] and p's means.
 *   out[i](y, x) = (v - mean) / denom,  v = w A_i(y, x) + (1 - w) A_p(y, x),
 *          w = w_in where y0 <= y < y1 and x0 <= x < x1 (output coordinates), w = w_out elsewhere.
 *   w == 1: A_p is not sampled and v = A_i(y, x); w == 0: A_i is not sampled and v = A_p(y, x).  Such a pixel equals
 *          lf_input_stage_f32's of that view bit for bit.
 *   targets (lf_mix_targets_f32): out[i] = y[p] + t (y[i] - y[p]); t == 1 stores y[i] and t == 0 stores y[p] exactly.
 * Mixup with factor l is w_out = w_in = t = l and an empty box; CutMix is w_out = 1, w_in = 0,
 * t = 1 - (y1 - y0)(x1 - x0) / (h w); an unmixed row is w_out = w_in = t = 1.  partner may equal i.
 * The rows are device data, so the entries cannot refuse a bad one without a sync: both clamp partner into
 * [0, n - 1] and w_out, w_in, t into [0, 1], and read a NaN as 0 there; a NaN box edge puts every pixel outside.
 * Other arguments, scratch and constraints as for lf_input_stage_f32 (means_ws: n*24 floats, all n images' means
 * are taken).  lf_mix_targets_f32: y, out [n][c], n <= 65535, c <= 4096, out must not overlap y. */
int lf_input_stage_mix_f32(const uint8_t* in, float* out, int n, int h, int w, const float* aug4,
                           const float* mix8, const float* mean3, const float* denom3, float* means_ws,
                           lf_stream_t stream);
int lf_mix_targets_f32(const float* y, const float* mix8, float* out, int n, int c, lf_stream_t stream);

/* The online augmentation policy: one projective warp, one colour transform and one erase box per image, in place
 * of lf_input_stage_f32's flip / rotation / contrast.  in u8 HWC [n,h,w,3] -> out f32 NCHW [n,3,h,w]; pol24 (device,
 * f32 [n][24]) holds per image
 *   {a,b,c,d,e,f,g,k}     floats 0..7: the inverse map, output -> source, a homography whose last entry is 1;
 *   M (3x3, row-major), t floats 8..16 and 17..19: the colour transform;
 *   {y0,y1,x0,x1}         floats 20..23: the erase box.
 * mean3 / denom3 are host pointers, both set or both null, as for lf_pack_hwc_u8_to_nchw_f32.  No scratch: there is
 * no mean pass, contrast pivots on a constant that t carries.  Output pixel (oy, ox):
 *   erase   y0 <= oy < y1 and x0 <= ox < x1 (output coordinates): the value stored is exactly 0.0f, with
 *           normalisation the dataset mean, and nothing is sampled.  A NaN edge, or y1 <= y0, or x1 <= x0, puts every
 *           pixel outside.
 *   warp    cx = (w-1)/2, cy = (h-1)/2, u = ox - cx, v = oy - cy, in fp32 in this order and without contraction:
 *             den = max(g*u + k*v + 1, 1/16)
 *             fx  = (a*u + b*v + c)/den + cx          fy = (d*u + e*v + f)/den + cy
 *           (the division correctly rounded), fx and fy then clamped into [-2^20, 2^20] (a NaN is read as -2^20);
 *           x0 = floor(fx), ax = fx - x0, y0 = floor(fy), ay = fy - y0, the taps x0, x0 + 1, y0, y0 + 1 reflected as
 *           lf_tta_views_f32 reflects them, and b = top + (bot - top)*ay, top = v00 + (v01 - v00)*ax,
 *           bot = v10 + (v11 - v10)*ax on the bytes as floats; p = b/255 per channel.  A mirror is a = -1: there is
 *           no flip field.
 *   colour  q_c = min(max(((M_c0*p_r + M_c1*p_g) + M_c2*p_b) + t_c, 0), 1), a NaN read as 0.
 *   value   q_c, or (q_c - mean_c)/denom_c with mean3 set: the subtraction and the division each rounded on its own,
 *           the arithmetic of lf_pack_hwc_u8_to_nchw_f32.
 * Exact cases: the identity row ({1,0,0,0,1,0,0,0}, M = I, t = 0, an empty box) equals lf_pack_hwc_u8_to_nchw_f32 bit
 * for bit; a pure mirror (a = -1), or an integer translation (c, f), with the identity M equals the pack of the
 * mirrored or moved (reflected) image bit for bit.
 * The rows are device data, so a bad one cannot be refused without a sync.  Whatever a row holds (NaN, infinities, a
 * huge perspective term) nothing outside `in` is read and every value stored is finite and lies between the images of
 * 0 and 1 under the normalisation; which value such a row gives is not specified.
 * Refused before any launch: null buffers, n <= 0, n > 65535, h < 2, w < 2, h*w > 2^28, mean3 / denom3 not both set
 * or both null, a mean that is not finite, a denom that is zero or not finite. */
int lf_input_stage_policy_f32(const uint8_t* in, float* out, int n, int h, int w, const float* pol24,
                              const float* mean3, const float* denom3, lf_stream_t stream);

/* Test-time augmentation: v views of every image of a batch in one launch, and the v probability rows of every
 * image folded back into one.
 * lf_tta_views_f32: in u8 HWC [n,h,w,3] -> out f32 NCHW [n*v,3,h,w], image-major: row i*v + k is view k of image i.
 * view6 is a HOST pointer to v rows {flip, cos, sin, zoom, dy, dx}, 1 <= v <= 16 (copied into the kernel's
 * arguments: no upload, no scratch); mean3 / denom3 as for lf_pack_hwc_u8_to_nchw_f32.  Output pixel (oy, ox) of a
 * view, with cx = (w-1)/2, cy = (h-1)/2, u = ox - cx, t = oy - cy, in fp32 in this order and without contraction:
 *   fx = zoom*(cos*u - sin*t) + cx + dx        fy = zoom*(sin*u + cos*t) + cy + dy
 *   x0 = floor(fx), ax = fx - x0; y0 = floor(fy), ay = fy - y0; the taps x0, x0 + 1, y0, y0 + 1 are reflected
 *   (d c b a | a b c d | d c b a, any number of periods, negative indices too), and flip != 0 then mirrors the two x
 *   taps (x -> w-1-x): the flip precedes the rotation, as in lf_input_stage_f32.  zoom < 1 magnifies the centre.
 *   b = top + (bot - top)*ay, top = v00 + (v01 - v00)*ax, bot = v10 + (v11 - v10)*ax on the bytes as floats;
 *   out = b/255, then (. - mean)/denom with mean3 set: each division and the subtraction rounded on its own, the
 *   arithmetic of lf_pack_hwc_u8_to_nchw_f32.  There is no contrast term.
 * A row with cos = 1, sin = 0, zoom = 1 and integer dy, dx therefore equals lf_pack_hwc_u8_to_nchw_f32 of the moved
 * (and mirrored) image bit for bit; row {0,1,0,1,0,0} is the plain model input.
 * Refused before any launch: null buffers, n <= 0, h < 2, w < 2, v outside 1..16, n*v > 65535, a value of view6 that
 * is not finite, zoom == 0, mean3 / denom3 not both set or both null.
 * lf_tta_combine_f32: probs [n*v, c] image-major; weight a HOST pointer to v floats, each >= 0 and finite with a
 * positive sum S (added in ascending order in fp32), or null for all ones.
 *   out[i][j] = (sum_k weight[k] * probs[i*v + k][j]) / S, the sum in ascending k in fp32;
 *   top[i]    = argmax_j out[i][j], the lowest index on ties (np.argmax);
 *   agree[i]  = the number of views k with weight[k] > 0 whose own argmax (same tie rule) equals top[i].
 * One wave per image; c <= 4096, 1 <= v <= 16, n > 0. */
int lf_tta_views_f32(const uint8_t* in, float* out, int n, int h, int w, const float* view6, int v,
                     const float* mean3, const float* denom3, lf_stream_t stream);
int lf_tta_combine_f32(const float* probs, const float* weight, int v, float* out, int32_t* top, int32_t* agree,
                       int n, int c, lf_stream_t stream);

/* ---- Calibration: temperature scaling of probability rows ------------------- */
/* A model here hands out probabilities p [n][c] (f32), not logits, and that is enough.  With
 *   z_j = ln(max(p_j, FLT_MIN))          FLT_MIN = 1.17549435e-38, in float64
 *   q   = softmax(beta z)                beta = 1 / T > 0 the inverse temperature
 * q is the temperature-scaled softmax of the logits: ln p differs from them by a constant per row, which the softmax
 * drops.  A probability that underflowed to 0 is read as FLT_MIN (z = -87.3), not as weight zero; so is a NaN.
 * All per-row arithmetic is float64, every operation rounded on its own (no contraction).
 *
 * lf_calib_stats: labels int32 [n]; betas a HOST pointer to k doubles, 1 <= k <= 8, each finite and > 0; 1 <= bins
 * <= 64.  A row whose label lies outside [0, c) is skipped (counted, and left out of everything but pred).  Per beta,
 * summed over the other rows, with y the label, m = beta ln(max_j p_j), s = sum_j exp(beta z_j - m), q_j =
 * exp(beta z_j - m) / s, mu = sum_j q_j z_j:
 *   nll   = m + ln s - beta z_y
 *   g     = mu - z_y                          d nll / d beta
 *   h     = sum_j q_j (z_j - mu)^2            d2 nll / d beta2: a second pass about mu, never negative
 *   brier = sum_j (q_j - [j == y])^2
 *   conf  = max_j q_j = 1 / s
 *   bin b = min(bins - 1, (int)(conf * bins)): the rows in it, the sum of their conf, and those with pred == y
 * Independent of beta: pred[i] = the lowest index attaining the maximum of the INPUT row (np.argmax; so no
 * prediction moves with beta; written for skipped rows too), the number of rows with pred == y, the number skipped,
 * and cm[y][pred] += 1.
 * Outputs (device): sums f64 [k][5 + bins] = {nll, g, h, brier, conf, the bins' conf sums}; counts i32
 * [k][2][bins] = {rows per bin, correct rows per bin}, followed by {correct, skipped}; pred i32 [n] or null; cm i32
 * [c][c] or null, cleared by the call.  ws: lf_calib_stats_workspace(n, k, bins) bytes, 8-byte aligned (0: bad
 * arguments).
 * Order of summation: a wave adds its rows i, i + waves, ... in ascending order (one lane per beta, in registers;
 * the bins in a table of the wave's own), a workgroup its waves in order, a second one-workgroup kernel the
 * workgroups in order; the number of workgroups depends on n alone.  No float goes through an atomic: the same
 * input gives the same bits.  (cm is counted with integer atomics.)
 *
 * lf_calib_apply_f32: out[i][j] = (float) q_ij for one beta, conf[i] = (float)(1 / s_i) = max_j out[i][j], top[i] =
 * pred as above.  out == probs (in place) is allowed; any other overlap of out and probs is refused.
 * Both: n > 0, 1 <= c <= 4096. */
size_t lf_calib_stats_workspace(int n, int k, int bins);
int lf_calib_stats(const float* probs, const int32_t* labels, int n, int c, const double* betas, int k, int bins,
                   double* sums, int32_t* counts, int32_t* pred, int32_t* cm, void* ws, size_t ws_bytes,
                   lf_stream_t stream);
int lf_calib_apply_f32(const float* probs, double beta, float* out, float* conf, int32_t* top, int n, int c,
                       lf_stream_t stream);

/* ---- Conformal: prediction sets with guaranteed coverage (split conformal prediction) ---- */
/* Inputs: probability rows p f32 [n][c], n > 0, 1 <= c <= 256; u f32 [n] in [0, 1], one value per row, or null: 1.0
 * for every row.  Anything else (a null buffer, an unknown kind, lambda not finite or < 0, kreg < 0, stats without
 * labels) returns -1 with a message before any launch.
 *
 * Order.  Within a row class k stands before class j iff p_k > p_j, or p_k == p_j and k < j: a total order on the
 * f32 values; a NaN reads as 0.  r(j) is the number of classes before j (the rank; 0: the prediction, np.argmax).
 * Cumulative mass.  m(j) is the float64 sum of the probabilities of the classes before j, added in rank order from
 * 0.0: m at rank r + 1 = m at rank r + (double)p at rank r.  Every float64 operation is rounded on its own (no
 * contraction), in exactly this order.
 * Score of class j, in float64:
 *   LF_CONFORMAL_LAC   1.0 - (double)p_j                              (u is not read)
 *   LF_CONFORMAL_APS   m(j) + (double)u * (double)p_j                 (the product of two f32 is exact in f64)
 *   LF_CONFORMAL_RAPS  the APS score + lambda * (double)max(0, r(j) + 1 - kreg), the penalty added last;
 *                      lambda >= 0 finite, kreg >= 0.  lambda and kreg are not read by the other kinds.
 * Set.  Class j is a member iff score(j) <= qhat[j] (false when either is a NaN; true for every j at +inf).  With
 * force_top the class of rank 0 is always a member.  A marginal threshold is the same value c times.
 * Threshold (on the host: predict/conformal.py).  From n calibration scores k = ceil((n + 1)(1 - alpha)), computed
 * exactly (alpha is the fraction its decimal string names, 0 < alpha < 1); qhat is the k-th smallest score, +inf
 * when k > n.  Marginal: one qhat from the scores of the rows' labels.  Class-conditional: qhat[j] from the rows whose
 * label is j; a class with k_j > n_j gets +inf.
 * Because the arithmetic and its order are fixed, the kernel equals a numpy float64 transcription of these lines in
 * every bit (tests/conformal_ref.py), and `<=` stays exact when qhat is itself one of the scores.
 *
 * lf_conformal_scores: labels i32 [n] -> score f64 [n] = the score of the row's label, rank i32 [n] = r(label).  A
 * row whose label lies outside [0, c) gets (NaN, -1).
 * lf_conformal_sets: qhat f64 [c] on the device (8-byte aligned) -> member u8 [n][c] (1 or 0), size i32 [n] = the
 * members of the row.  labels i32 [n] or null; with labels, stats i64 [4 + (c + 1) + 3 c] or null (8-byte aligned,
 * cleared by the call), over the rows whose label lies in [0, c) -- the others count in `skipped` alone, their
 * member and size are written all the same:
 *   {rows, skipped, covered, size_sum}      covered: the label is a member; size_sum: the sum of size
 *   size_hist[s], s = 0 .. c                rows with size s
 *   per class k: {rows, covered, size_sum}  the same over the rows whose label is k
 * One wave per row, the ranks and sums across the wave; a launch runs at most 8,192 waves, a wave then takes the
 * rows w, w + waves, ...  No float goes through an atomic; the counters are added with integer ones. */
#define LF_CONFORMAL_LAC 0
#define LF_CONFORMAL_APS 1
#define LF_CONFORMAL_RAPS 2
int lf_conformal_scores(const float* probs, const int32_t* labels, const float* u, int n, int c, int kind,
                        double lambda, int kreg, double* score, int32_t* rank, lf_stream_t stream);
int lf_conformal_sets(const float* probs, const float* u, const double* qhat, int n, int c, int kind, double lambda,
                      int kreg, int force_top, const int32_t* labels, uint8_t* member, int32_t* size,
                      long long* stats, lf_stream_t stream);

/* ---- Novelty score: Mahalanobis distance of the pooled features to the nearest class ---- */
/* feat f32 [n][d] are rows of the network's pooled feature vector (GlobalAveragePooling's output).  Both calls: n > 0,
 * d a multiple of 16 with 16 <= d <= 256, 1 <= c <= 4096; anything else returns -1 with a message before any launch.
 *
 * lf_feat_moments: the sums a per-class Gaussian fit with one shared covariance needs, in float64.  labels i32 [n].
 * The call ADDS INTO four device accumulators (8-byte aligned; a fit is many calls, one per forward pass):
 *   count   i64 [c]     rows of class k
 *   skipped i64 [1]     rows whose label lies outside [0, c): they are counted here and nowhere else
 *   sum     f64 [c][d]  sum of the rows of class k
 *   gram    f64 [d][d]  sum_r f_r f_r^T over the counted rows, the full symmetric matrix
 * A product of two f32 values is exact in f64, so only the additions round.  Every output element has one owner,
 * which adds the rows in ascending order from 0 and then adds that partial to the accumulator: the same calls give
 * the same bits.  No float goes through an atomic (skipped is counted with an integer one).  The Gram matrix is
 * computed on the f64 matrix cores (v_mfma_f64_16x16x4_f64) in upper 16 x 16 tiles, four rows to an instruction;
 * the tiles below the diagonal receive the transposed partial of their mirror tile.
 *
 * lf_maha_score_f32: mu0 f32 [d] (the pooled mean), w f32 [d][d] row-major (the whitening matrix; 16-byte aligned),
 * m f32 [c][d] (the whitened, centred class means).  In f32:
 *   t_j     = feat[i][j] - mu0[j]
 *   z_k     = sum_j w[k][j] t_j       an fmaf chain from 0 (v_mfma_f32_32x32x2_f32) in the order j = 0, d/2, 1,
 *                                     d/2 + 1, ..., d/2 - 1, d - 1
 *   d2[i][k] = sum_j (z_j - m[k][j])^2   an fmaf chain from 0 in the order j = 0 .. d - 1; a non-finite value
 *                                     (NaN or inf) is stored and read as +inf
 *   score[i] = min_k d2[i][k], nearest[i] = the lowest k attaining it; a row with no finite d2 gets (+inf, 0).
 * d2 f32 [n][c] may be null; score f32 [n]; nearest i32 [n]. */
int lf_feat_moments(const float* feat, const int32_t* labels, int n, int d, int c, long long* count,
                    long long* skipped, double* sum, double* gram, lf_stream_t stream);
int lf_maha_score_f32(const float* feat, const float* mu0, const float* w, const float* m, int n, int d, int c,
                      float* d2, float* score, int32_t* nearest, lf_stream_t stream);

/* ---- Nearest neighbours: the k gallery rows closest to each query row, exactly ---- */
/* lf_knn_topk_f32: q f32 [nq][d] (queries), g f32 [ng][d] (the gallery; 16-byte aligned), exclude i32 [nq] or null:
 * the gallery row query i must not return, -1 for none (a leave-one-out search passes 0 .. nq - 1).
 * Out: d2 f32 [nq][k] and idx i32 [nq][k].  The rule, in f32:
 *   qn_i   = sum_c q[i][c]^2          an fmaf chain from 0 in the order c = 0 .. d - 1; gn_j likewise over g[j]
 *   dot_ij = sum_c q[i][c] g[j][c]    an fmaf chain from 0 (v_mfma_f32_32x32x2_f32) in the order c = 0, 4, 1, 5, 2,
 *                                     6, 3, 7, then 8, 12, 9, 13, ...: each run of 8 features in that order, the
 *                                     runs ascending
 *   d2_ij  = max(0, fmaf(-2, dot_ij, qn_i + gn_j)); a non-finite value (NaN or an infinity) is +inf; a zero is +0
 *   Row i of the output holds the k smallest pairs (d2_ij, j) over all j != exclude[i], ascending in the TOTAL order
 *   "smaller d2 first, the lower j on equal d2".  With fewer than k eligible rows the remaining slots hold (+inf, -1),
 *   after every eligible row, those at distance +inf included.
 * The order is total, so the output does not depend on tiling, on `segments` or on the order in which candidates are
 * met; no atomic is used; the same call gives the same bits.  The distance matrix is never written: a workgroup
 * holds lf_knn_query_tile() queries in LDS, walks one of `segments` equal runs of ceil(ng / segments) gallery rows and
 * keeps k pairs per query; with segments > 1 the runs' lists go to the workspace and a second kernel merges them.
 * lf_knn_segments(nq, ng) is the number of runs that fills the device at that size (1 when the query tiles alone do;
 * 0: bad arguments).  ws: 16-byte aligned, lf_knn_topk_workspace(nq, ng, k, segments) bytes (0: bad arguments): gn,
 * then the runs' lists.
 * Refused before any launch (-1 with a message): a null buffer, nq < 1, ng < 1, d not a multiple of 16 in 16..256,
 * k outside 1..lf_knn_max_k() = 32, segments outside 1..64, a misaligned g or ws, a workspace that is too small. */
int lf_knn_query_tile(void);
int lf_knn_max_k(void);
int lf_knn_segments(int nq, int ng);
size_t lf_knn_topk_workspace(int nq, int ng, int k, int segments);
int lf_knn_topk_f32(const float* q, const float* g, int nq, int ng, int d, int k, const int32_t* exclude,
                    int segments, float* d2, int32_t* idx, void* ws, size_t ws_bytes, lf_stream_t stream);

/* ---- Embedding map: exact (dense) t-SNE of feature rows, and the marks of its chart ---- */
/* van der Maaten & Hinton's t-SNE without approximation and without random numbers: one feature matrix gives one map.
 *
 * Affinities (lf_tsne_perplexity_f32).  Row i of d2 f32 [n][n] (squared distances), the entry j = i left out BY INDEX
 * (its value is never read into the rule), d_ij = (double)d2[i][j] - (double)min_{k != i} d2[i][k]:
 *   p_{j|i} = exp(-beta_i d_ij) / S,  S = sum_{k != i} exp(-beta_i d_ik),  p_{i|i} = 0, stored as f32.
 *   beta_i: bisection on the row's entropy H = ln S + beta sum(d e) / S against ln(perplexity).  beta = 1, lo = 0,
 *   hi = inf.  One evaluation computes H at beta; it stops when |H - ln perplexity| <= 1e-5 or when it was the 100th.
 *   Otherwise, H too large: lo = beta, and beta doubles while hi is inf, else moves to (lo + hi) / 2; H too small:
 *   hi = beta and beta moves to (lo + hi) / 2.  The beta of the last evaluation is used and reported (beta f64 [n]),
 *   with the number of evaluations (evals i32 [n]).  All of it in float64, exp included.
 *   A row's sums: thread t of 256 adds its entries j = t, t + 256, ... in order, the 64 lanes of a wave fold by
 *   __shfl_down 32, 16, ..., 1, the four waves add as ((w0 + w1) + w2) + w3.  One workgroup per row; the row is read
 *   once into LDS, so p may be d2 itself (in place).
 * Symmetric P (lf_tsne_symmetrize_f32).  P_ij = (p_{j|i} + p_{i|j}) / (float)(2n): one f32 addition, one correctly
 *   rounded f32 division; in place, by 32 x 32 tiles, the workgroup of tile (a, b), a <= b, writing (b, a) as well
 *   from LDS.  The result is exactly symmetric.
 * Forces at a map y f32 [n][2] (lf_tsne_forces_f32), w_ij = 1 / (1 + |y_i - y_j|^2) for j != i (by index):
 *   attr_i = sum_j P_ij w_ij (y_i - y_j)      f32 [n][2]
 *   rep_i  = sum_j w_ij^2 (y_i - y_j)         f32 [n][2]
 *   z_i    = sum_j w_ij                       f64 [n]
 *   kl (f64 [n][2], or null: no logarithm is taken): a_i = sum_{j: P_ij > 0} P_ij ln P_ij, b_i = sum_{..} P_ij ln w_ij.
 *   Per pair, all in f64 from the f32 operands: the differences (exact), d2 = fma(dy, dy, dx * dx),
 *   w = 1 / (1 + d2); the terms fma(P * w, dx, .), fma(w * w, dx, .), w, fma(P, ln P, .) and fma(P, -log1p(d2), .)
 *   (ln w, taken so that it keeps its digits where w is close to 1) add in f64.  attr and
 *   rep are rounded to f32 once, when a row's sums are stored.
 *   Order, a function of n alone: a wave owns row i; lane l adds its entries j = 256 t + 4 l + e (e = 0 .. 3 inside
 *   t = 0, 1, ...) in ascending order, the lanes fold by __shfl_down 32, 16, ..., 1.  No atomics; the same call gives
 *   the same bits.  P is streamed once, the y_j come from LDS in chunks of 4096 points, nothing of size n^2 is
 *   written.
 *   With Z = sum_i z_i: KL = sum_i a_i - sum_i b_i + ln Z * sum P.
 * Step (lf_tsne_step_f32), one workgroup of 1024 threads.  Z = sum z_i (f64: thread t adds i = t, t + 1024, ... in
 *   order, __shfl_down fold, the 16 waves from the left).  Per coordinate, in f64 from the f32 state:
 *   grad = 4 (e attr - rep / Z);  gain <- (grad > 0) != (vel > 0) ? gain + 0.2f : gain * 0.8f, then max(gain, 0.01f),
 *   both in f32;  vel <- (float)(mu vel - eta gain grad);  t = y + vel (f64);  y <- (float)(t - mean_c), mean_c the
 *   f64 sum of the column's t (same order as Z) divided by n.  With kl (the forces' pieces) and kl_out f64 [1]:
 *   kl_out[0] = sum a - sum b + ln Z * sum_p, sum_p the caller's f64 sum of P.
 * Refused before any launch: null buffers, n outside 2..lf_tsne_max_points() = 16384 (symmetrize: 1..), a perplexity
 * that is not finite or below 1, p / y not 16-byte aligned, kl without kl_out.
 *
 * lf_scatter_points_u8: m round marks into img u8 [h][w][3] in place, all integer.  xy i32 [m][2] = (x, y) pixel
 * centres, colour i32 [m] an index into palette u8 [colours][3], radius 0..64, owner i32 [h][w] workspace (zeroed by
 * the call).  Every pixel inside the picture with dx^2 + dy^2 <= radius^2 of mark k takes atomicMax(owner, k + 1)
 * (an integer atomic: the outcome does not depend on the order, the mark with the highest index wins); then owned
 * pixels get their mark's palette colour and all others stay.  A mark whose colour lies outside the palette takes no
 * pixel.  Centres may lie anywhere (the sums are 64-bit); nothing is written outside the picture.  Refused before any
 * launch: null buffers, m outside 1..2^20, radius outside 0..64, colours, h or w below 1, h * w above 2^28. */
int lf_tsne_max_points(void);
int lf_tsne_perplexity_f32(const float* d2, int n, double perplexity, float* p, double* beta, int32_t* evals,
                           lf_stream_t stream);
int lf_tsne_symmetrize_f32(float* p, int n, lf_stream_t stream);
int lf_tsne_forces_f32(const float* p, const float* y, int n, float* attr, float* rep, double* z, double* kl,
                       lf_stream_t stream);
int lf_tsne_step_f32(float* y, float* vel, float* gain, const float* attr, const float* rep, const double* z, int n,
                     double exaggeration, double eta, double momentum, const double* kl, double sum_p,
                     double* kl_out, lf_stream_t stream);
int lf_scatter_points_u8(const int32_t* xy, const int32_t* colour, int m, int radius, const uint8_t* palette,
                         int colours, uint8_t* img, int h, int w, int32_t* owner, lf_stream_t stream);

/* ---- Near-duplicate search: 128-bit difference hashes and their all-pairs Hamming search ---- */
/* Integer and exact throughout; no float appears.
 *
 * lf_dhash128_u8: in u8 HWC [n,h,w,3], 9 <= h, w <= 4096 -> sig i32 [n][V][4], V = variants in {1, 2, 4, 8}.
 *   Pixel value: y = 77 R + 150 G + 29 B (no shift).
 *   Cells: a 9 x 9 grid.  Cell row r covers image rows [(r*h + 4) / 9, ((r+1)*h + 4) / 9) in C integer division,
 *   cell column c the columns [(c*w + 4) / 9, ((c+1)*w + 4) / 9).  The bounds are mirror-symmetric, b(9-c) = w - b(c),
 *   and every cell holds at least floor(w/9) >= 1 columns: the grid of a mirrored image is exactly the mirrored grid.
 *   Per cell: sum (64 bits) of y over its pixels and cnt, the number of its pixels.
 *   darker(a, b) = sum_a * cnt_b < sum_b * cnt_a in 64-bit arithmetic: strict, a tie gives 0.  At 4096 x 4096 a cell
 *   has at most 456 * 456 pixels of at most 65,280 each: a product stays below 2.83e15 < 2^63.
 *   Variant s, with h = s & 1, v = (s >> 1) & 1, t = (s >> 2) & 1 (applied to sums and counts alike):
 *     G_s[r][c] = G[r1][c1],  (r0, c0) = t ? (c, r) : (r, c),  r1 = v ? 8 - r0 : r0,  c1 = h ? 8 - c0 : c0.
 *   Variants 0 .. V-1 are written.  Variant 1 is exactly the signature of the left-right mirrored image; with h == w
 *   the eight variants are the signatures of the eight flips and quarter turns.
 *   Signature: 128 bits; bit 8r + c (r, c in 0..7) = darker(G_s[r][c], G_s[r][c+1]), bit 64 + 8r + c =
 *   darker(G_s[r][c], G_s[r+1][c]); bit k lives in word k / 32 at position k % 32.
 *   One workgroup per image, which is read once; no global atomics.
 *   Refused before any launch: null buffers, n <= 0, h or w outside 9..4096, V not in {1, 2, 4, 8}.
 *
 * lf_hamming_pairs_count / lf_hamming_pairs_fill: a = na signatures of 4 int32, row i at a + i * a_stride (a_stride
 * >= 4, in int32: variant 0 of an [na][Va][4] array has a_stride = 4 * Va); b i32 [nb][V][4] on a 16-byte boundary.
 *   distance(i, j) = min over s < V of popcount(a_i xor b_{j,s}); s = the lowest variant reaching the minimum.
 *   A pair is reported when distance <= threshold (0..128); with self != 0 (a is variant 0 of b, na == nb) only
 *   pairs with i < j.
 *   The columns j are cut into chunks = lf_hamming_pairs_chunks(na, nb) runs (0: bad arguments), which depends on
 *   (na, nb) alone.  count writes counts i32 [na][chunks], the matches of row i in chunk k.  fill takes offsets i64
 *   [na][chunks], the EXCLUSIVE running sum of counts in that order (i major, chunk minor), and writes out i32
 *   [total][4] on a 16-byte boundary: rows {i, j, distance, s} in ascending (i, j) order.  Nothing is appended
 *   through an atomic: the same input gives the same rows in the same places.
 *   Refused before any launch: null buffers, na or nb <= 0, V not in {1, 2, 4, 8}, threshold outside 0..128,
 *   a_stride < 4, a misaligned buffer, self with na != nb, a chunks argument other than lf_hamming_pairs_chunks.
 *   The launch geometry, for callers and tests that want to reason about it: a workgroup holds lf_hamming_pairs_rows()
 *   rows of a and stages lf_hamming_pairs_tile() columns of b at a time; a chunk is ceil(ceil(nb / tile) / chunks)
 *   whole tiles of columns. */
int lf_dhash128_u8(const uint8_t* in, int32_t* sig, int n, int h, int w, int variants, lf_stream_t stream);
int lf_hamming_pairs_tile(void);
int lf_hamming_pairs_rows(void);
int lf_hamming_pairs_chunks(int na, int nb);
int lf_hamming_pairs_count(const int32_t* a, long long a_stride, int na, const int32_t* b, int nb, int variants,
                           int threshold, int self, int32_t* counts, int chunks, lf_stream_t stream);
int lf_hamming_pairs_fill(const int32_t* a, long long a_stride, int na, const int32_t* b, int nb, int variants,
                          int threshold, int self, const long long* offsets, int chunks, int32_t* out,
                          lf_stream_t stream);

/* ---- residual tail, fp32 training step: the values at the recorded positions kept at pooled size ---- */
/* lf_block_tail_fwd_f32 (below) that also writes, at pooled size [n][c][h/2][w/2], the raw y and the raw sc at the
 * window position the route byte records (the first maximum in scan order): y_at and sc_at, either may be null (not
 * written).  p and route are those of lf_block_tail_fwd_f32, bit for bit.
 * lf_block_tail_bwd_kept_f32 is lf_block_tail_bwd_f32 (below) reading them: where y_at (sc_at) is given, the sums
 * take y_at[pooled index] (sc_at[...]) in place of y[recorded position] (sc_y[...]) and y (sc_y) may be null, so the
 * backward pass reads pooled-size tensors instead of touching every cache line of the full-size planes to use one
 * pixel in four.  The same values enter the same sums in the same order: dr, ds, plane_sums and sc_sums are those
 * of lf_block_tail_bwd_f32 on the same inputs, bit for bit. */
int lf_block_tail_fwd_keep_f32(const float* y, const float* a_scale, const float* a_shift, const float* s,
                               const float* sc, const float* sc_scale, const float* sc_shift, int sc_relu,
                               const float* drop, uint8_t* route, float* p, float* y_at, float* sc_at, int n, int c,
                               int h, int w, lf_stream_t stream);
int lf_block_tail_bwd_kept_f32(const float* dp, const uint8_t* route, const float* y, const float* y_at,
                               const float* a_scale, const float* a_shift, const float* drop, float* dr, float* ds,
                               float* plane_sums, const float* sc_y, const float* sc_at, float* sc_sums, int n, int c,
                               int h, int w, lf_stream_t stream);

/* ---- input stage ----------------------------------------------------------- */
/* u8 HWC -> f32 NCHW with the model's train-time augmentation fused (cnn.py:74-86):
 * keras RandomFlip("horizontal") -> RandomRotation (bilinear, fill_mode="reflect") ->
 * RandomContrast on the [0,1] image, then Normalization (x-mean)/denom.  aug4[n] =
 * {flip 0/1, cos, sin, contrast factor} (device, drawn by the host RNG); mean3/denom3 are
 * HOST pointers (or both null); means_ws is a device scratch of n*24 floats
 * (8 partial channel sums per image).
 * Stochastic layers: statistical parity with keras, exact parity with oracle/cnn_ref.py. */
int lf_input_stage_f32(const uint8_t* in, float* out, int n, int h, int w, const float* aug4,
                       const float* mean3, const float* denom3, float* means_ws,
                       lf_stream_t stream);

/* ---- BatchNorm (keras BatchNormalization: momentum 0.99, eps 1e-3; cnn.py:30,45) ---- */
/* out = act(x*scale[c] + shift[c]) over [n][c][hw] (BN apply, optional ReLU). */
int lf_scale_shift_act_f32(const float* x, float* out, int n, int c, int hw, const float* scale,
                           const float* shift, int relu, lf_stream_t stream);
size_t lf_bn_workspace(int c);
/* Training statistics of y [n][c][hw]: batch mean / biased variance per channel; writes
 * mean, invstd = 1/sqrt(var+eps), scale = gamma*invstd, shift = beta - mean*scale, and
 * updates moving_mean/var <- moving*momentum + batch*(1-momentum). */
int lf_bn_train_stats_f32(const float* y, int n, int c, int hw, const float* gamma,
                          const float* beta, float* moving_mean, float* moving_var, float momentum,
                          float eps, float* mean, float* invstd, float* scale, float* shift,
                          void* workspace, size_t ws_bytes, lf_stream_t stream);
/* Same outputs as lf_bn_train_stats_f32 from the tile sums of lf_conv2d_stats_f32 (taken about
 * moving_mean, which must not have changed in between); tiles = lf_conv2d_stats_tiles(...). */
int lf_bn_train_stats_tiles_f32(const float* tile_part, long long tiles, int n, int c, int hw,
                                const float* gamma, const float* beta, float* moving_mean,
                                float* moving_var, float momentum, float eps, float* mean,
                                float* invstd, float* scale, float* shift, void* workspace,
                                size_t ws_bytes, lf_stream_t stream);
/* Inference scale/shift from the moving statistics. */
int lf_bn_infer_scale_shift_f32(int c, const float* gamma, const float* beta,
                                const float* moving_mean, const float* moving_var, float eps,
                                float* scale, float* shift, lf_stream_t stream);
/* BatchNorm backward with the upstream chain folded in: dz = g*alpha_nc[n][c] + add_nc[n][c]
 * (both optional), zeroed where the forward's ReLU was inactive when relu != 0 — the mask is
 * recomputed as y*scale[c]+shift[c] > 0 from the pre-BN tensor, so the activation is never
 * stored; dy = gamma*invstd*(dz - mean(dz) - xhat*mean(dz*xhat)); dgamma = sum dz*xhat,
 * dbeta = sum dz.  plane_g / plane_m (optional, [n][c][2], relu case only): when the producer
 * of g already left per-plane sums {sum g*mask, sum g*mask*y} (lf_block_tail_bwd_f32) and the
 * forward left {sum mask, sum mask*y} (lf_gap_f32; needed with add_nc), the two channel sums
 * (with relu == 0 the plane sums are unmasked and alpha_nc / add_nc must be null)
 * come from those and g / y are read once (for dy) instead of twice.  have_sums != 0: dgamma /
 * dbeta already hold the sums (lf_bn_bwd_sums_tiles_f32) and only the apply pass runs. */
int lf_bn_bwd_f32(const float* g, const float* alpha_nc, const float* add_nc, const float* y,
                  const float* mean, const float* invstd, const float* scale, const float* shift,
                  int relu, const float* gamma, float* dy, float* dgamma, float* dbeta,
                  const float* plane_g, const float* plane_m, int have_sums, int n, int c, int hw,
                  void* workspace, size_t ws_bytes, lf_stream_t stream);

/* The two channel sums of lf_bn_bwd_f32 without the apply pass: dgamma, dbeta and coef [5][c] =
 * {scale, shift, P, Q, R} such that dy = P*dz + Q*y + R with dz = (g*alpha+add)*[y*scale+shift>0
 * or !relu].  lf_conv2d_wgrad_bn_f32 forms dy from g and y with these while it computes the
 * weight gradient, so the standalone apply pass (2 reads + 1 write) disappears. */
int lf_bn_bwd_sums_f32(const float* g, const float* alpha_nc, const float* add_nc, const float* y,
                       const float* mean, const float* invstd, const float* scale,
                       const float* shift, int relu, const float* gamma, float* dgamma, float* dbeta,
                       float* coef, const float* plane_g, const float* plane_m, int n, int c, int hw,
                       void* workspace, size_t ws_bytes, lf_stream_t stream);

/* lf_bn_bwd_sums_f32 from the tile sums of lf_conv2d_bnbwd_f32 (no alpha/add). */
int lf_bn_bwd_sums_tiles_f32(const float* tile_part, long long tiles, const float* mean,
                             const float* invstd, const float* scale, const float* shift,
                             const float* gamma, float* dgamma, float* dbeta, float* coef, int n,
                             int c, int hw, void* workspace, size_t ws_bytes, lf_stream_t stream);

/* ---- pooling / broadcast ---- */
/* out[p] = mean over hw of act(x[p][:]*scale[c]+shift[c]), c = p % C (GlobalAveragePooling2D,
 * cnn.py:13,98; scale/shift null = plain mean; relu applies with the prologue).  mask_sums
 * (optional, [planes][2]) receives {count of x*scale+shift > 0, sum of x over those}. */
int lf_gap_f32(const float* x, float* out, int planes, int hw, int c, const float* scale,
               const float* shift, int relu, float* mask_sums, lf_stream_t stream);
/* out[p][:] = v[p]*scale (GAP backward). */
int lf_bcast_planes_f32(const float* v, float* out, int planes, int hw, float scale,
                        lf_stream_t stream);

/* ---- Squeeze-Excite (cnn.py:9-17): s = sigmoid(relu(m w1 + b1) w2 + b2) ---- */
/* m [n][c], w1 [c][cr], w2 [cr][c]; z1 = hidden activations (saved for backward).
 * Backward writes dm = dL/dm * dm_scale (dm_scale = 1/(H*W) folds the GlobalAveragePooling2D
 * the squeeze came through). */
int lf_se_fwd_f32(const float* m, const float* w1, const float* b1, const float* w2,
                  const float* b2, float* z1, float* s, int n, int c, int cr, lf_stream_t stream);
size_t lf_se_bwd_workspace(int n, int c, int cr);
int lf_se_bwd_f32(const float* ds, const float* m, const float* z1, const float* s,
                  const float* w1, const float* w2, float* dm, float* dw1, float* db1, float* dw2,
                  float* db2, int n, int c, int cr, float dm_scale, void* workspace,
                  size_t ws_bytes, lf_stream_t stream);

/* ---- residual tail (cnn.py:47-48,94-96): Add -> ReLU -> SpatialDropout2D -> MaxPool2D(2) ---- */
/* r = relu(sc' + a*s[n][c]) with a = relu(y*a_scale[c]+a_shift[c]) (BN2+ReLU fused; a = y when
 * a_scale is null) and sc' = act(sc*sc_scale[c]+sc_shift[c]) (projection BN, or BN+ReLU of the
 * producer when sc_relu) or sc;  p = drop[n][c] * maxpool2x2(r) (drop = 0 or 1/(1-rate)).
 * r itself is not stored: route [n][c][h/2][w/2] (one byte per pooled value) records where the
 * value came from (bits 0-1: first maximum in scan order) and whether it was > 0 (bit 2). */
int lf_block_tail_fwd_f32(const float* y, const float* a_scale, const float* a_shift,
                          const float* s, const float* sc, const float* sc_scale,
                          const float* sc_shift, int sc_relu, const float* drop, uint8_t* route,
                          float* p, int n, int c, int h, int w, lf_stream_t stream);
/* dr = gradient wrt (sc' + a*s): dp*drop routed to the recorded position of each window whose
 * maximum was > 0; ds[n][c] = sum_hw dr*a (SE gate gradient); plane_sums [n][c][2] =
 * {sum dr*[a>0], sum dr*[a>0]*y} for lf_bn_bwd_f32 (y goes with ds / plane_sums; plane_sums
 * needs a_scale); sc_y (the projection shortcut's pre-BN tensor, optional) with sc_sums
 * [n][c][2] = {sum dr, sum dr*sc_y}: the same for the shortcut's BatchNormalization (no mask). */
int lf_block_tail_bwd_f32(const float* dp, const uint8_t* route, const float* y,
                          const float* a_scale, const float* a_shift, const float* drop, float* dr,
                          float* ds, float* plane_sums, const float* sc_y, float* sc_sums, int n,
                          int c, int h, int w, lf_stream_t stream);

/* ---- head (cnn.py:98-101; train/utils.py:30-35) ---- */
/* probs = softmax(feat w + b), w [f][c]; loss[n] = -sum_j ytrue[n][j] log(clip(probs)). */
int lf_head_fwd_f32(const float* feat, const float* w, const float* b, const float* ytrue,
                    float* probs, float* loss, int n, int f, int c, lf_stream_t stream);
/* dlogits = (probs - ytrue) * inv_n (softmax + cross-entropy without the clip); dfeat = dlogits w^T;
 * dw = feat^T dlogits; db = sum_n dlogits.  Differentiating through the loss's clip to [1e-7, 1 - 1e-7]
 * instead gives a different dlogits only where a probability is saturated (a clipped class passes no
 * gradient, and the renormalisation term changes with it); this entry does not follow that rule. */
int lf_head_bwd_f32(const float* feat, const float* w, const float* probs, const float* ytrue,
                    float* dlogits, float* dfeat, float* dw, float* db, int n, int f, int c,
                    float inv_n, lf_stream_t stream);
int lf_mul_f32(const float* a, const float* b, float* out, size_t count, lf_stream_t stream);

/* ---- optimizer (train/utils.py:17-27 AdamW + clipnorm; :44-57 EMA) ---- */
/* Flat buffers; tensor t occupies [offsets[t], offsets[t+1]).  Per tensor: g' = g + 2*l2[t]*w
 * (kernel_regularizer gradient), clip_by_norm(g', clipnorm) per tensor (0 = off), decoupled
 * decay w -= lr*wd*w, Adam with bias correction at `step` (1-based), then
 * ema = copy ? w : decay*ema + (1-decay)*w (ema may be null).  norms_out: ntensors floats (the
 * pre-clip gradient norms, for logging); workspace: lf_adamw_workspace(ntensors) bytes. */
size_t lf_adamw_workspace(int ntensors);
int lf_adamw_step_f32(float* param, const float* grad, float* m, float* v, float* ema,
                      const long long* offsets, const float* l2, int ntensors, long long max_count,
                      float lr, float beta1, float beta2, float eps, float weight_decay,
                      float clipnorm, long long step, float ema_decay, int ema_copy,
                      float* norms_out, void* workspace, size_t ws_bytes, lf_stream_t stream);
int lf_ema_update_f32(float* ema, const float* w, size_t count, float decay, int copy,
                      lf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LEAFHIP_H */
