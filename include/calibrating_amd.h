/*
 * calibrating_amd.h -- C ABI of libcalibrating_amd.so: the MI355X (gfx950) stereo-depth hot path of
 * DIYer22/calibrating, `Stereo.get_depth(img1, img2)`.
 *
 * Every entry point replaces one native (cv2 / NumPy) call the reference makes on that path; the
 * file:line after "replaces" points into /root/reference/calibrating/.  All image / volume pointers
 * are DEVICE pointers unless the name ends in `_host`; `stream` is a hipStream_t passed as void*
 * (NULL = the default stream).  Launches are asynchronous on `stream`; the compute entry points never synchronise the
 * device or a stream (camd_sgbm_status and the data-dependent count of camd_depth_to_point_cloud's caller excepted).
 * The init-time calls camd_sgbm_create / camd_sgbm_destroy / camd_sgbm_set_option(CAMD_OPT_PATH, CAMD_PATH_CONCURRENT)
 * allocate and free device memory (hipMalloc / hipFree synchronise implicitly) and are not for stream capture;
 * camd_sgbm_create fills the padding of its cost volume on a private stream and waits for that stream only.
 * Return value: 0 on success, a negative camd_status otherwise;
 * camd_last_error() then holds a message (thread-local).
 *
 * Handles are not thread-safe: use one handle per host thread / stream.
 */
#ifndef CALIBRATING_AMD_H
#define CALIBRATING_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum camd_status {
    CAMD_OK = 0,
    CAMD_ERR_BAD_ARG = -1,     /* size/type mismatch (cv2 raises cv2.error there) */
    CAMD_ERR_UNSUPPORTED = -2, /* parameter outside what the kernels implement */
    CAMD_ERR_NO_DEVICE = -3,   /* no HIP device / not gfx950 */
    CAMD_ERR_HIP = -4,         /* a HIP runtime call failed */
    CAMD_ERR_NOMEM = -5
} camd_status;

const char* camd_last_error(void);
int camd_version(void);
/* 0 when a gfx950 device is usable by this process, CAMD_ERR_NO_DEVICE otherwise */
int camd_device_ok(void);

/* ---- SGBM ------------------------------------------------------------------------------------
 * replaces cv2.StereoSGBM_create(...) and .compute(left, right):
 *   stereo_matching.py:48-58 (create; field order = keyword order there, plus preFilterCap, mode)
 *   stereo_matching.py:63    (compute), stereo_matching.py:64 (getMinDisparity)                */
typedef struct camd_sgbm_params {
    int minDisparity;
    int numDisparities;
    int blockSize;
    int P1;
    int P2;
    int disp12MaxDiff;
    int preFilterCap;
    int uniquenessRatio;
    int speckleWindowSize;
    int speckleRange;
    int mode; /* CAMD_MODE_SGBM = 0 (5 paths; the reference's call), CAMD_MODE_HH = 1 (8 paths),
                 CAMD_MODE_SGBM_3WAY = 2 (four row stripes x three paths), CAMD_MODE_HH4 = 3 (4 paths) */
} camd_sgbm_params;
enum { CAMD_MODE_SGBM = 0, CAMD_MODE_HH = 1, CAMD_MODE_SGBM_3WAY = 2, CAMD_MODE_HH4 = 3 };

typedef struct camd_sgbm camd_sgbm;

/* Workspace (device) bytes a handle for these sizes allocates. 0 on bad arguments. */
size_t camd_sgbm_workspace_bytes(const camd_sgbm_params* p, int width, int height, int channels,
                                 int max_batch);
/* Allocates the per-pair workspace for `max_batch` pairs of width x height x channels (1 or 3) u8.
 * Parameters are normalised as cv2's computeDisparitySGBM does and no further: numDisparities is used AS GIVEN (218 stays
 * 218; only the internal volume is padded, to a multiple of 32 above 64), blockSize <= 0 -> 5 and otherwise only its
 * half blockSize / 2 is used (an even size acts as the next odd one, as in cv2), P1 <= 0 -> 2, P2 <= 0 -> 5, then
 * P2 = max(P2, P1 + 1), uniquenessRatio < 0 -> 10, disp12MaxDiff <= 0 -> 1, preFilterCap -> max(cap, 15) | 1.
 * Refused with CAMD_ERR_UNSUPPORTED and a message, never computed differently (cv2.StereoSGBM_create accepts all of
 * these; INTEGRATION.md section D says what each limit comes from): numDisparities > 512, blockSize > 15 (> 11 for
 * MODE_SGBM_3WAY), P2 > 24000, preFilterCap > 127, 0 < width - numDisparities <= blockSize / 2 (cv2's own result is
 * undefined there), MODE_SGBM_3WAY on images too low for its four stripes. */
int camd_sgbm_create(const camd_sgbm_params* p, int width, int height, int channels, int max_batch,
                     camd_sgbm** out);
int camd_sgbm_destroy(camd_sgbm* h);
/* left/right: u8 [batch][height][width*channels] with row pitch `pitch` bytes and `image_stride`
 * bytes between consecutive pairs; disp: int16 [batch][height][width] (disparity * 16, cv2's
 * fixed point) with `disp_pitch` / `disp_stride` bytes.  batch <= max_batch.                    */
int camd_sgbm_compute(camd_sgbm* h, const uint8_t* left, const uint8_t* right, size_t pitch,
                      size_t image_stride, int16_t* disp, size_t disp_pitch, size_t disp_stride,
                      int batch, void* stream);
/* geometry of the internal cost volume: x in cost coordinates [0,width1), d in [0,D), padded to Dp */
int camd_sgbm_query(const camd_sgbm* h, int* width1, int* D, int* Dp, int* minX1);
/* stage-wise parity hooks: copy the volume of pair `index` of the last compute, [height][width1][Dp]
 * int16, to dst (device).  which: 0 = matching cost C (incl. +P2), 1 = aggregated S,
 * 2 = raw disparity before median/speckle as int16 [height][width] */
int camd_sgbm_debug_copy(camd_sgbm* h, int which, int index, void* dst, void* stream);
/* options: CAMD_OPT_PATH selects the aggregation implementation (all bit-identical):
 *   CAMD_PATH_AUTO (default)  concurrent scans for calls of <= 4 pairs of 1080p/D=128-sized work (<= 8 for
 *                             MODE_HH), band passes above
 *   CAMD_PATH_SCAN            one line-scan launch per direction, sequential (generic fallback)
 *   CAMD_PATH_BAND            fused band-wavefront passes (throughput; D in (32, 256])
 *   CAMD_PATH_CONCURRENT      all directions at once into per-direction volumes (latency; <= 8 pairs per call)
 * MODE_SGBM_3WAY has no per-direction volumes: AUTO takes the line scans for little work per call (under ~2.5 pairs of
 * 1080p/D=128-sized work) and the band passes above; CAMD_PATH_BAND / CAMD_PATH_CONCURRENT force the band passes
 * (where D allows; the winners are decided inside the last pass for D % 8 == 0, by a separate kernel otherwise).
 * CAMD_OPT_KEEP_S 1 = the band path also stores the final S volume (for camd_sgbm_debug_copy(which = 1)). */
enum { CAMD_OPT_PATH = 0, CAMD_OPT_KEEP_S = 1, CAMD_OPT_COST = 2, CAMD_OPT_SATURATE = 3, CAMD_OPT_3WAY_SIMD_LANES = 4,
       CAMD_OPT_EXACT = 5 };  /* (6 = CAMD_OPT_PHASES: calibrating_amd_experimental.h) */
enum { CAMD_PATH_AUTO = 0, CAMD_PATH_SCAN = 1, CAMD_PATH_BAND = 2, CAMD_PATH_CONCURRENT = 3 };
/* CAMD_OPT_COST selects how the matching-cost volume C is built (bit-identical results):
 *   CAMD_COST_AUTO (default)  the fused kernel where it is instantiated (blockSize <= 11), else the split pair
 *   CAMD_COST_FUSED           k_cost: BT pixel cost + blockSize x blockSize box sum + P2 -> C, written once
 *   CAMD_COST_SPLIT           k_hsum (BT + horizontal sum) -> intermediate volume -> k_vsum (vertical sum) -> C */
enum { CAMD_COST_AUTO = 0, CAMD_COST_FUSED = 1, CAMD_COST_SPLIT = 2 };
/* CAMD_OPT_SATURATE: int16 overflow behaviour of the box-sum recurrences that build C:
 *   1 (default)  saturate like OpenCV's CV_SIMD build (v_int16 + / -), which is what cv2 wheels run
 *   0            wrap modulo 2^16 like OpenCV's scalar build
 * The two differ only if blockSize^2 * channels * (2*ftzero + 63) + P2 > 32767 AND the image content drives a
 * window sum past 32767 (e.g. blockSize >= 11 on RGB with a large preFilterCap).
 * CAMD_OPT_3WAY_SIMD_LANES (MODE_SGBM_3WAY only): 8 (default) = the winner-take-all tie rule of cv2's 8-lane SIMD builds
 * (per lane slot the last disparity attaining the slot minimum, then the smallest of those), 1 = the scalar build's
 * smallest disparity.  Only exact ties are affected.
 * CAMD_OPT_EXACT: what happens to a pair whose cost volume left the int16 regime of the aggregation kernels (a value
 * below P2, possible only after an int16 overflow of the box sums, i.e. only when blockSize^2 * channels *
 * (2*ftzero + 63) + P2 > 32767 and the images are adversarial):
 *   1 (default)  it is aggregated again in plain int arithmetic, exactly as OpenCV's scalar code does (slow, one set
 *                of per-direction volumes of workspace)
 *   0            it is refused: its disparities are written as invalid and camd_sgbm_status / the next
 *                camd_sgbm_compute return CAMD_ERR_HIP (also what happens when that workspace could not be allocated)
 * Either way a result that differs from OpenCV's is never handed back silently. */
int camd_sgbm_set_option(camd_sgbm* h, int option, int value);
/* synchronises `stream` and reports whether a device-side bounded wait of the last computes timed out, or a pair
 * was refused (CAMD_OPT_EXACT).  Without this call neither can pass unnoticed: the affected disparities are written as
 * invalid ((minDisparity - 1) * 16), and the next camd_sgbm_compute on the handle returns CAMD_ERR_HIP. */
int camd_sgbm_status(camd_sgbm* h, void* stream);
/* per-stage GPU time of the last compute, measured with hipEvents on `stream` (enable first).
 * stage names: camd_sgbm_stage_name(i), i in [0, camd_sgbm_num_stages()): "cost", "hsum", "vsum" (the split cost pair),
 * "scan" (aggregation; on the band path its first pass), "scan_last", "wta" (winner-take-all / LR check), "median",
 * "speckle" */
int camd_sgbm_set_profiling(camd_sgbm* h, int enable);
int camd_sgbm_num_stages(void);
const char* camd_sgbm_stage_name(int i);
int camd_sgbm_get_profile(camd_sgbm* h, float* ms_per_stage, int n);

/* replaces cv2.medianBlur(disp, disp, 3) and cv2.filterSpeckles inside StereoSGBM.compute; exported
 * for stage-wise parity.  src/dst int16 [batch][h][w] contiguous; dst != src.                      */
int camd_median3_s16(const int16_t* src, int16_t* dst, int w, int h, int batch, void* stream);
/* in place; labels_ws: device scratch of camd_speckle_workspace_bytes(w,h,batch) */
size_t camd_speckle_workspace_bytes(int w, int h, int batch);
int camd_filter_speckles_s16(int16_t* img, int w, int h, int new_val, int max_speckle_size,
                             int max_diff, void* labels_ws, int batch, void* stream);

/* ---- remaps ----------------------------------------------------------------------------------
 * replaces cv2.remap(img, mapx, mapy, interp) on u8 HWC with CV_32FC1 maps, BORDER_CONSTANT 0:
 *   stereo_camera.py:217-228 (INTER_LANCZOS4, both cameras)
 * x_shift implements stereo_camera.py:230-240 (translation_rectify_img): dst[:, x] takes the remap
 * result of column x - x_shift, vacated columns are 0.                                          */
enum { CAMD_INTER_NEAREST = 0, CAMD_INTER_LINEAR = 1, CAMD_INTER_LANCZOS4 = 4 };
int camd_remap_u8(const uint8_t* src, int sw, int sh, int cn, size_t src_pitch, size_t src_stride,
                  const float* mapx, const float* mapy, uint8_t* dst, int dw, int dh,
                  size_t dst_pitch, size_t dst_stride, int interp, int x_shift, int batch,
                  void* stream);
/* replaces cv2.undistort(img1, K, D) (stereo_camera.py:430-431): bilinear fixed-point remap through
 * the CV_16SC2 + CV_16UC1 maps cv2.undistort builds internally (camd_undistort_maps_host).       */
int camd_remap_fixed_bilinear_u8(const uint8_t* src, int sw, int sh, int cn, size_t src_pitch,
                                 size_t src_stride, const int16_t* mapxy, const uint16_t* mapa,
                                 uint8_t* dst, int dw, int dh, size_t dst_pitch, size_t dst_stride,
                                 int batch, void* stream);
/* host, init time: the stripe-wise fixed-point maps of cv2.undistort (2*w*h int16 + w*h uint16); csrc/tables.hip,
 * beside its device twin camd_undistort_maps                                                      */
int camd_undistort_maps_host(const double K[9], const double* dist, int ndist, int w, int h,
                             int16_t* mapxy_host, uint16_t* mapa_host);
/* ---- rig tables on the GPU (init time, or per batch when the rig / target size changes) -------------
 * replaces cv2.initUndistortRectifyMap(A, dist, R, Anew, (w, h), CV_32FC1):
 *   stereo_camera.py:159-165 (rectify maps of both cameras)   utils.py:184-191 (unrectify maps)
 * and, when valid_mask != NULL, valid_mask_from_remap (stereo_camera.py:167-176) against a src_w x src_h
 * source image, fused.  A, Anew: 3x3 row-major host doubles; R: 3x3 or NULL (identity); dist: up to 12
 * coefficients (k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4), host.  mapx / mapy: device float [h][w];
 * valid_mask: device u8 [h][w] or NULL.  Bit-identical to the host construction (float64 internally,
 * X/Y/W accumulated along each row like OpenCV's scalar loop).                                         */
int camd_init_undistort_rectify_map(const double A[9], const double* dist, int ndist, const double* R,
                                    const double Anew[9], int w, int h, float* mapx, float* mapy,
                                    uint8_t* valid_mask, int src_w, int src_h, void* stream);
/* device version of camd_undistort_maps_host: mapxy int16 [h][w][2], mapa uint16 [h][w] (device) */
int camd_undistort_maps(const double K[9], const double* dist, int ndist, int w, int h, int16_t* mapxy,
                        uint16_t* mapa, void* stream);
/* process-wide options.  CAMD_GOPT_LANCZOS_FIX_GROUP_LO: first index (3 or 4; default 4 = ksize/2) of the 2x2 tap
 * group of a Lanczos-4 table entry that takes the weight-sum correction -- SURVEY.md A.10 uncertainty U15, the same
 * switch the CPU oracle exposes (oracle_switches.lanczos_fix_group_lo), so that one flip moves both. */
enum { CAMD_GOPT_LANCZOS_FIX_GROUP_LO = 0 };
int camd_set_global_option(int option, int value);
/* host, init time: the 32x32-phase int16 weight tables cv2.remap uses (1024*64 / 1024*4 entries) */
int camd_lanczos4_table_host(int16_t* tab_host);
int camd_bilinear_table_host(int16_t* tab_host);

/* replaces boxx.resize -> cv2.resize(..., INTER_LINEAR) around the matcher when max(h, w) > cfg["max_size"]:
 *   stereo_matching.py:62 (u8 RGB pair, downsize)   stereo_matching.py:66 (float32 disparity, upsize)
 * src [batch][sh][sw][cn], dst [batch][dh][dw][cn], contiguous. */
int camd_resize_linear_u8(const uint8_t* src, int sw, int sh, int cn, uint8_t* dst, int dw, int dh, int batch,
                          void* stream);
int camd_resize_linear_f32(const float* src, int sw, int sh, float* dst, int dw, int dh, int batch,
                           void* stream);

/* ---- depth -----------------------------------------------------------------------------------
 * replaces stereo_matching.py:63-69 (int16 -> f32, clip, < minD*16 -> 0, /16, identity resize),
 * stereo_camera.py:510-512 (+= min_disparity, * rectify_valid_mask1) and
 * stereo_camera.py:408-413 (Stereo.disparity_to_depth) in one pass.
 * valid_mask: u8 [h][w] shared by the batch; disparity: f32, depth: f64 (NumPy >= 2 dtype).      */
int camd_disp_to_depth(const int16_t* disp16, const uint8_t* valid_mask, int w, int h,
                       int sgbm_min_disparity, int add_min_disparity, int translate,
                       double baseline_fx, double max_depth, float* disparity, double* depth,
                       int batch, void* stream);
/* The same for the matcher's downsizing branch (cfg["max_size"] < max(h, w), the reference's default 1000):
 * disp16 is the int16 disparity of the sw x sh DOWNSIZED pair; stereo_matching.py:63-69 in full -- float32, clip,
 * < minD*16 -> 0, /16, boxx.resize (cv2.resize INTER_LINEAR) back to w x h, * w / sw -- then stereo_camera.py:510-513
 * and :408-413 as above, one pass.                                                                                  */
int camd_disp16_resized_to_depth(const int16_t* disp16, int sw, int sh, const uint8_t* valid_mask, int w, int h,
                                 int sgbm_min_disparity, int add_min_disparity, int translate,
                                 double baseline_fx, double max_depth, float* disparity, double* depth,
                                 int batch, void* stream);
/* replaces utils.rotate_depth_by_remap (utils.py:192-199) as called by Stereo.unrectify_depth
 * (stereo_camera.py:415-428): z' = M20*(u*z) + M21*(v*z) + M22*z, then INTER_NEAREST remap.      */
int camd_unrectify_depth(const double* depth, int w, int h, const double M_row2_host[3],
                         const float* mapx, const float* mapy, double* out, int ow, int oh,
                         int batch, void* stream);
/* replaces the per-rig part of Stereo.distort_depth (stereo_camera.py:440-462): every pixel of the undistorted w x h
 * image of camera K through cv2.undistortPoints(., K, None) -> cv2.projectPoints(., 0, 0, K, dist) -> .astype(int32)
 * (truncation) -> np.unique(axis=0, return_index=True).  src_index: device int32 [h][w]; entry [y][x] is the LOWEST
 * row-major source index v*w + u whose target is (x, y), or -1 where no pixel lands (a hole).  dist: ndist <= 14
 * host doubles (k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4 tauX tauY); non-zero tauX / tauY (tilted sensor) are refused with
 * CAMD_ERR_UNSUPPORTED.  stats: device int32[6] = {n_out, minU, maxU, minV, maxV, n_nonfinite}: how many source pixels
 * have a target outside [0, w) x [0, h) (non-finite targets included; they are counted and never written) and the
 * range of the finite targets.  The reference raises IndexError for a target >= w / >= h and wraps a negative one to
 * the far edge; a caller that wants neither reads stats once per table and refuses the rig when n_out != 0.        */
int camd_distort_index_map(const double K[9], const double* dist, int ndist, int w, int h, int32_t* src_index,
                           int32_t* stats, void* stream);
/* replaces stereo_camera.py:438,463 (res = zeros; res[y, x] = depths[index]) as a gather through src_index:
 * out[b][p] = src_index[p] < 0 ? 0 : depth[b][src_index[p]].  depth / out: [batch][h][w] of elem_bytes = 8 (float64)
 * or 4 (float32), contiguous, out != depth, batch <= 2^19; an index outside [0, w*h) reads nothing and yields 0.    */
int camd_distort_depth(const void* depth, int elem_bytes, int w, int h, const int32_t* src_index, void* out, int batch,
                       void* stream);

/* ---- depth post-ops (the step after get_depth in the reference's demos) ---------------------------
 * replaces utils.depth_to_point_cloud (utils.py:213-246): non-zero depths in row-major order of the sampling
 * grid (the depth image itself, or its cv2.resize(INTER_NEAREST) to round(size * rate) when rate != 1) ->
 * points [N][3] = Kinv * (u z, v z, z); uv (optional) [N][2] = the (u, v) of each point (return_xyzuv).
 * depth: f64 [h][w]; capacity = rows available in points/uv (grid_w * grid_h always suffices, see
 * camd_point_cloud_grid); *count (device u64) receives N; workspace: camd_point_cloud_workspace_bytes.   */
int camd_point_cloud_grid(int w, int h, double rate, int* grid_w, int* grid_h);
size_t camd_point_cloud_workspace_bytes(int w, int h, double rate);
int camd_depth_to_point_cloud(const double* depth, int w, int h, const double Kinv_host[9], double rate,
                              double* points, double* uv, size_t capacity, unsigned long long* count,
                              void* workspace, void* stream);
/* replaces utils.apply_T_to_point_cloud (utils.py:152-161): out = (T * [p, 1])[:3], T 4x4 row-major host */
int camd_apply_T_to_point_cloud(const double* points, size_t n, const double T_host[16], double* out,
                                void* stream);
/* replaces utils.point_cloud_to_depth / point_cloud_to_arr2d without values (utils.py:249-318): project with
 * K, round half-to-even to a pixel, nearest z wins (the reference sorts far-to-near and overwrites).
 * points: f64 rows of point_stride >= 3 doubles; keys_ws: device scratch of w*h*8 bytes; depth: f64 [h][w] */
int camd_point_cloud_to_depth(const double* points, size_t n, int point_stride, const double K_host[9], int w,
                              int h, double bg_value, double* depth, unsigned long long* keys_ws, void* stream);
/* replaces Cam.project_cam2_depth (camera.py:298-309) = the three calls above composed, as ONE scatter
 * pass without materialising the point cloud: depth2 f64 [h2][w2] of camera 2 -> depth1 f64 [h1][w1].      */
int camd_project_depth(const double* depth2, int w2, int h2, const double K2inv_host[9],
                       const double T_2in1_host[16], const double K1_host[9], double rate, int w1, int h1,
                       double* depth1, unsigned long long* keys_ws, void* stream);
/* ---- the z-buffer with a payload: what the nearest point CARRIES arrives in the pixel ---------------------------
 * Both entry points below run three passes over scratch the caller provides: keys_ws (8 bytes per target pixel and
 * image: atomicMin of an order-preserving key of the projected z), owner_ws (4 bytes per target pixel and image:
 * atomicMax of 1 + the index of the sources that hold that key), then one gather per target pixel.  Points that
 * share a pixel AND have bit-equal z: the larger index wins (index = row-major cell of the sampling grid / row of the
 * point array) -- a stable far-to-near sort followed by the reference's last-write-wins; np.argsort's default sort
 * leaves that case to its internals.  Identical calls give identical bits.
 *
 * replaces utils.get_reproject_remap (utils.py:332-344): depth_to_point_cloud(return_xyzuv) -> apply_T_to_point_cloud
 * -> point_cloud_to_arr2d(values = np.float32(uv), bg_value = -1), without materialising the cloud.  depth2: f64
 * [batch][h2][w2], image b at depth2 + b * depth_stride (doubles); K2inv, T_2in1 (4x4), K1: row-major host doubles
 * shared by the batch; rate: the interpolation rate of camd_point_cloud_grid.  mapx / mapy: f32 [h1][w1] planes, image
 * b at + b * map_stride (floats): where camera 1's pixel finds its colour in camera 2's image (feed them to
 * camd_remap_u8(..., CAMD_INTER_LINEAR), camera.py:341), -1 where nothing landed.  keys_ws: batch * w1 * h1 * 8 bytes,
 * owner_ws: batch * w1 * h1 * 4 bytes.  batch <= 65535; a sampling grid of >= 2^32 - 1 cells is CAMD_ERR_BAD_ARG.   */
int camd_reproject_remap(const double* depth2, int w2, int h2, size_t depth_stride, const double K2inv_host[9],
                         const double T_2in1_host[16], const double K1_host[9], double rate, int w1, int h1,
                         float* mapx, float* mapy, size_t map_stride, unsigned long long* keys_ws,
                         uint32_t* owner_ws, int batch, void* stream);
/* replaces utils.point_cloud_to_arr2d with values (utils.py:254-288, scatter in uvzs_to_arr2d :291-317): project with
 * K, round half-to-even to a pixel, the values row of the nearest point wins.  points: f64 rows of point_stride >= 3
 * doubles, n < 2^32 - 1; NaN / inf / out-of-image projections are dropped.
 * values: [n][channels] of value_type, channels >= 1, contiguous; out: [h][w][channels] of the same type; pixels
 * nobody reaches get bg_value cast to that type (for CAMD_VALUE_U8 it must be an integer in 0..255).
 * keys_ws: w * h * 8 bytes, owner_ws: w * h * 4 bytes.                                                            */
enum { CAMD_VALUE_F64 = 0, CAMD_VALUE_F32 = 1, CAMD_VALUE_U8 = 2, CAMD_VALUE_U16 = 3 /* depth of camd_vis_depth only */ };
int camd_point_cloud_to_arr2d(const double* points, size_t n, int point_stride, const double K_host[9], int w, int h,
                              const void* values, int channels, int value_type, double bg_value, void* out,
                              unsigned long long* keys_ws, uint32_t* owner_ws, void* stream);

/* ---- sparse samples <-> dense images (csrc/sparse.hip) ----------------------------------------------
 * The reference's utils.uvzs_to_arr2d / arr2d_to_uvzs / interpolate_uvzs (utils.py:291-415) and
 * epipolar_geometry.matched_xyz_normals_to_zs (:88-97).  uv: float64 rows of uv_stride >= 2 doubles (u, v, ...).
 *
 * replaces uvzs_to_arr2d: pixel = int32(round-half-even(u, v)); rows outside w x h (NaN / inf too) are dropped; of
 * several rows on one pixel the LARGEST row index wins (NumPy's fancy assignment).  values / out as in
 * camd_point_cloud_to_arr2d.  keep != 0: out is a caller's image updated in place (pixels nobody reaches are left
 * alone, bg_value is unused); keep == 0: they get bg_value.  owner_ws: w * h * 4 bytes.  n < 2^32 - 1.        */
int camd_uvzs_to_arr2d(const double* uv, size_t n, int uv_stride, int w, int h, const void* values, int channels,
                       int value_type, double bg_value, int keep, void* out, uint32_t* owner_ws, void* stream);
/* replaces arr2d_to_uvzs without a mask: rows[x * h + y] = (x, y, arr2d[y][x]) -- x outer, y inner, like
 * np.array([xs, ys, arr2d]).T.reshape(-1, 3).  arr2d and rows are 8-byte elements: float64, or int64 when as_int64.  */
int camd_arr2d_to_uvzs(const void* arr2d, int w, int h, int as_int64, void* rows, void* stream);
/* ... with a mask (bytes, non-zero = taken): the masked pixels in row-major order; *count (device) = how many;
 * rows beyond capacity are not written.  workspace: camd_arr2d_mask_workspace_bytes(h) bytes.                    */
size_t camd_arr2d_mask_workspace_bytes(int h);
int camd_arr2d_to_uvzs_masked(const void* arr2d, const uint8_t* mask, int w, int h, int as_int64, void* rows,
                              size_t capacity, unsigned long long* count, void* workspace, void* stream);
/* replaces interpolate_uvzs(inter_type="nearest", distance) (KDTree.query per pixel): samples are binned into the
 * integer cells (floor u, floor v); a pixel searches the cells within R = max(1, ceil(distance)) of it.
 * distance <= CAMD_NEAREST_MAX_RADIUS, else CAMD_ERR_UNSUPPORTED.  Three calls around ONE exclusive scan that the
 * caller provides (any scan: it is plumbing):
 *   camd_sparse_bin_grid  -> R and the bin grid bins_w x bins_h (= w + 2R - 1, h + 2R - 1)
 *   camd_sparse_bin_count -> counts[bins_w * bins_h] (cleared here)
 *   caller: start[0] = 0, start[c + 1] = start[c] + counts[c]  (bins_w * bins_h + 1 entries); cursor = copy of start
 *   camd_sparse_bin_fill  -> sorted_uv [capacity][2], sorted_idx [capacity], capacity >= start[last]; consumes cursor
 *   camd_nearest_fill     -> out[y][x] = float32(z[i]) of the sample i nearest to (x, y) in float64
 *                            sqrt(dx*dx + dy*dy) if that is < distance, else 0; equal distances: the LOWEST i.
 * z: [n] of z_type CAMD_VALUE_F64 / CAMD_VALUE_F32.  out_w x out_h != w x h: the image is the
 * cv2.resize(INTER_NEAREST) of the w x h fill times out_w / w (float32: * out_w, then / w), written once.
 * h, out_h <= 65535.                                                                                            */
enum { CAMD_NEAREST_MAX_RADIUS = 32 };
int camd_sparse_bin_grid(int w, int h, double distance, int* radius, int* bins_w, int* bins_h);
int camd_sparse_bin_count(const double* uv, size_t n, int uv_stride, int w, int h, double distance, uint32_t* counts,
                          void* stream);
int camd_sparse_bin_fill(const double* uv, size_t n, int uv_stride, int w, int h, double distance, uint32_t* cursor,
                         size_t capacity, double* sorted_uv, uint32_t* sorted_idx, void* stream);
int camd_nearest_fill(const double* sorted_uv, const uint32_t* sorted_idx, const uint32_t* start, const void* z,
                      int z_type, int w, int h, double distance, float* out, int out_w, int out_h, void* stream);
/* the plane fit of interpolate_uvzs(inter_type="lstsq"): sums[9] (device) = sum of uu, uv, u, vv, v, 1, uz, vz, z over
 * the n >= 1 samples, reduced in a fixed order (no float atomics: two runs give the same bits).
 * partials_ws: camd_plane_sums_blocks(n) * 9 doubles.  The caller solves the 3x3 system on the host.             */
int camd_plane_sums_blocks(size_t n);
int camd_plane_sums(const double* uv, int uv_stride, const void* z, int z_type, size_t n, double* partials_ws,
                    double* sums, void* stream);
/* out[y][x] = float32(x * a + y * b + c) in float64; h <= 65535 */
int camd_plane_eval(double a, double b, double c, int w, int h, float* out, void* stream);
/* replaces matched_xyz_normals_to_zs(uvs_to_xyz_noramls(uv1, K1), uvs_to_xyz_noramls(uv2, K2), T_1to2): per match the
 * least-squares (z1, z2) of [-R X1, X2] (z1, z2)^T = t, X = Kinv (u, v, 1).  uv1, uv2: [n][2] float64 contiguous.  */
int camd_matched_uvs_to_zs(const double* uv1, const double* uv2, size_t n, const double K1inv_host[9],
                           const double K2inv_host[9], const double T_1to2_host[16], double* zs1, double* zs2,
                           void* stream);

/* ---- pose from matched points: the epipolar path (csrc/epipolar.hip) -----------------------------------------
 * The device side of calibrating_amd/epipolar_geometry.py (the reference's epipolar_geometry.py, flow_utils.py and
 * ReconstructionExtrinsics.build_set2ds_by_flowds).  Integer atomics only and fixed-order float sums: identical calls
 * give identical bits.  uv rows: uv_type CAMD_VALUE_F64 / CAMD_VALUE_F32, uv_stride >= 2 elements (u, v, ...), n < 2^32 - 1.
 * A cell window is cells cu0 .. cu0 + cells_w - 1 by cv0 .. cv0 + cells_h - 1, at most 2^28 cells, stored U-MAJOR:
 * grid[(cu - cu0) * cells_h + (cv - cv0)].  *outside (device u64, cleared by the entry point) counts the rows that
 * fall outside the window (NaN / inf among them); the caller sizes the window from the data, so it must read 0.
 *
 * replaces np.unique(np.int32((uv / max_distance).round()), axis=0, return_index=True): cell = int32(rint(u / d)),
 * int32(rint(v / d)) -- the division in the rows' own type, half to even -- and first[cell] = the smallest row index
 * landing there, 0xFFFFFFFF where none does (first is cleared here).  max_distance > 0.                          */
int camd_cell_first_index(const void* uv, int uv_type, size_t n, int uv_stride, double max_distance, int cu0, int cv0,
                          int cells_w, int cells_h, uint32_t* first, unsigned long long* outside, void* stream);
/* ... return_counts=True instead, for max_distance = 1: population[cell] = how many rows land there (cleared here) */
int camd_cell_population(const void* uv, int uv_type, size_t n, int uv_stride, int cu0, int cv0, int cells_w, int cells_h,
                         uint32_t* population, unsigned long long* outside, void* stream);
/* replaces np.intersect1d of the two sorted cell lists: the cells set in both grids, as (first1, first2) pairs in
 * ascending (u cell, v cell) order -- u the major key, signed -- which is the linear order of the u-major grid.
 *   camd_cell_intersect_count -> colcount[cells_w]: shared cells per u column
 *   caller: start[0] = 0, start[c + 1] = start[c] + colcount[c]  (cells_w + 1 int64 entries; any scan: it is plumbing)
 *   camd_cell_intersect_emit  -> idx1 / idx2 [capacity] int64, *count (device u64) = start[cells_w]
 * Both launch ONE WORKGROUP PER u COLUMN (cells_w of them) and the scan has cells_w entries: sized for image-shaped
 * windows.  A window that is wide in u and short in v (up to 2^28 x 1) is computed correctly but costs up to 2^28
 * nearly empty workgroups.                                                                                       */
int camd_cell_intersect_count(const uint32_t* first1, const uint32_t* first2, int cells_w, int cells_h, uint32_t* colcount,
                              void* stream);
int camd_cell_intersect_emit(const uint32_t* first1, const uint32_t* first2, int cells_w, int cells_h, const long long* start,
                             long long* idx1, long long* idx2, size_t capacity, unsigned long long* count, void* stream);
/* replaces filter_overlap_uvs (epipolar_geometry.py:205-216): keep[i] = the pixel int32(rint(u, v)) of uv1[i] is hit by
 * no other row of uv1 AND the same for uv2[i] (population1 / population2: camd_cell_population of each set over one
 * window), then uvs[mask] -- the kept rows in their own order, dtype kept.
 *   camd_overlap_keep -> keep[n] bytes, blockcount[camd_overlap_blocks(n)]: kept rows per 256 rows
 *   caller: start[0] = 0, start[b + 1] = start[b] + blockcount[b]  (blocks + 1 int64 entries)
 *   camd_overlap_emit -> out1 / out2 [capacity][2] of uv_type, *count (device u64) = start[blocks]                */
int camd_overlap_blocks(size_t n);
int camd_overlap_keep(const void* uv1, const void* uv2, int uv_type, size_t n, int uv_stride, int cu0, int cv0, int cells_w,
                      int cells_h, const uint32_t* population1, const uint32_t* population2, uint8_t* keep,
                      uint32_t* blockcount, void* stream);
int camd_overlap_emit(const void* uv1, const void* uv2, int uv_type, size_t n, int uv_stride, const uint8_t* keep,
                      const long long* start, void* out1, void* out2, size_t capacity, unsigned long long* count, void* stream);
/* The cheirality test of EssentialMatrixStereo.__init__ (:121-130) for all four candidate poses in one pass: every
 * match is read once and solved for (z1, z2) under each T_1to2[c] (four 4x4 row-major host matrices, t already scaled
 * to the baseline) by the very function camd_matched_uvs_to_zs evaluates.  sums[c * 2 + 0 / 1] (device, 8 doubles) =
 * sum of zs1 / zs2 under candidate c; the caller divides by n.  uv1, uv2: [n][2] float64 contiguous, n >= 1.
 * REDUCTION SHAPE (no float atomics): G = camd_epipolar_sums_blocks(n) = clamp(ceil(n / 256), 1, 1024) workgroups of 256
 * threads; a thread adds its rows serially, at most m = ceil(n / (256 G)) terms; above that a binary tree of
 * d = 8 (workgroup) + 2 (four partials per thread of the final workgroup) + 8 (final workgroup) = 18 levels.
 * partials_ws: G * 8 doubles.                                                                                    */
int camd_epipolar_sums_blocks(size_t n);
int camd_epipolar_sums(const double* uv1, const double* uv2, size_t n, const double K1inv_host[9], const double K2inv_host[9],
                       const double T_1to2_host[64], double* partials_ws, double* sums, void* stream);
/* sums[0] (device) = sum of z[i], i < n (idx == NULL, n <= z_len) or of z[idx[i]] (idx: [n] int64) -- the numerator of
 * zs.mean() / zs[idx].mean() in align_scale_with (:189-191); sums[1] = how many idx[i] lie outside [0, z_len) (they add
 * nothing; must read 0).  Same reduction shape as camd_epipolar_sums: m = ceil(n / (256 G)), d = 18, G =
 * camd_vector_sum_blocks(n); partials_ws: G * 2 doubles.  n >= 1.                                                */
int camd_vector_sum_blocks(size_t n);
int camd_vector_sum(const double* z, size_t z_len, const long long* idx, size_t n, double* partials_ws, double* sums,
                    void* stream);
/* replaces the flow-to-matches step of build_set2ds_by_flowds (reconstruction_epipolar_geometry.py:276-282): for the
 * masked pixels (bytes, non-zero = taken) in row-major order uvs_from = ((x + 0.5) - 1e-8, (y + 0.5) - 1e-8) and
 * uvs_to = float64(flow) + uvs_from, both [capacity][2] float64.  flow_abs: [h][w][2] of flow_type.  *count (device u64)
 * = how many; rows beyond capacity are not written.  workspace: camd_arr2d_mask_workspace_bytes(h) bytes.         */
int camd_flow_to_matched_uvs(const void* flow_abs, int flow_type, const uint8_t* mask, int w, int h, double* uvs_from,
                             double* uvs_to, size_t capacity, unsigned long long* count, void* workspace, void* stream);
/* replaces flow_utils.flow_abs_to_normal: [h][w][2] -> float32 [2][h][w], float32(float64(flow) / (w, h))          */
int camd_flow_abs_to_normal(const void* flow_abs, int flow_type, int w, int h, float* flow_normal, void* stream);
/* replaces flow_utils.flow_normal_to_abs: [2][h][w] -> float64 [h][w][2], float64(flow) * (target_w, target_h)    */
int camd_flow_normal_to_abs(const void* flow_normal, int flow_type, int w, int h, double target_w, double target_h,
                            double* flow_abs, void* stream);
/* ---- flow_utils.warp_flow (csrc/flow.hip): an image moved through a normalised flow, no map in memory -----------------
 * flow: [batch][2][h][w] of flow_type (CAMD_VALUE_F64 / CAMD_VALUE_F32), x in units of w, y in units of h; image b's two
 * planes start at flow + b * flow_stride (elements) -- every image of a batch has its own flow.  Pixel (x, y) maps to
 * m = float64(x) + float64(flow_x) * float64(w), likewise y and h (NumPy's promotion of flow * [[[w]], [[h]]],
 * flow_utils.py:111-112): product and sum rounded once each in float64, never fused.  Images are u8 HWC, cn 1 or 3, with
 * the pitch / stride / batch conventions of camd_remap_u8; interp: CAMD_INTER_NEAREST / _LINEAR / _LANCZOS4, anything else
 * is CAMD_ERR_UNSUPPORTED.  CAMD_ERR_BAD_ARG: cn other than 1 or 3, a side >= 32768 (cv2.remap's short coordinates),
 * w * h > 2^31 - 1, batch > 65535.
 *
 * replaces flow_utils.py:127-129 (img2 given): cv2.remap(img2, float32(m_x), float32(m_y), interp), BORDER_CONSTANT 0, for
 * an img2 that already has the flow's size (the boxx.resize of :128 is camd_resize_linear_u8).  A pixel whose map * 32 is
 * NaN, infinite or beyond int32 is 0: cvRound on x86 sends it to a cell outside every image.                        */
int camd_warp_flow_backward_u8(const uint8_t* img2, int cn, size_t src_pitch, size_t src_stride, const void* flow,
                               int flow_type, size_t flow_stride, uint8_t* dst, int w, int h, size_t dst_pitch,
                               size_t dst_stride, int interp, int batch, void* stream);
/* replaces flow_utils.py:113-125 (img1 given): t = int32(round_half_even(m)); a source pixel with a non-zero flow
 * (-0.0 counts as zero) and a target inside w x h writes its own (x, y) into the identity map at t, the last writer in
 * row-major source order winning, then cv2.remap(img1, map, interp).  The map holds integers, so all three
 * interpolations copy the winning pixel of img1 (sw x sh, which need not be w x h), or give 0 where that position lies
 * outside img1.  Sources whose target is NaN, infinite or beyond int32 are skipped.  winner_ws: batch * w * h int32 of
 * scratch (set to -1 on the stream, then atomicMax of the source's y * w + x: the largest index IS the last writer, so
 * identical calls give identical bytes).                                                                           */
int camd_warp_flow_forward_u8(const uint8_t* img1, int sw, int sh, int cn, size_t src_pitch, size_t src_stride,
                              const void* flow, int flow_type, size_t flow_stride, uint8_t* dst, int w, int h,
                              size_t dst_pitch, size_t dst_stride, int interp, int32_t* winner_ws, int batch, void* stream);

/* ---- pictures (csrc/vis.hip; utils.py:463-575, 673-719): depth error, depth through a colour table, lined tiles ---------
 * Planes are packed: image b of a batch starts at b * w * h elements (pictures: * 3 bytes, RGB).  w * h < 2^31, batch <=
 * 65535.  Float64 arithmetic is NumPy's: every product, sum and quotient rounded once, nothing contracted.
 *
 * vis_depth_l1 runs in stages that share two planes, l1 (float64) and valid (uint8):
 *   camd_vis_l1_error    l1 = (re - gt) * valid, valid = (re != 0) & (gt != 0) (utils.py:512-513).  re / gt: value_type
 *                        CAMD_VALUE_F64 / _F32 (widened exactly); gt == NULL: the number gt_value everywhere.  With
 *                        bar_place != CAMD_BAR_NONE the colour bar np.linspace(-bar_max_l1 * 1.1, bar_max_l1 * 1.1, length)
 *                        is written over both planes (:519-548; bar_width = (h + w) / 100 in the reference; a bar wider than
 *                        the side it lies along is CAMD_ERR_BAD_ARG).  maxkey[batch]: the bits of each image's largest
 *                        |l1|, bar included.  *nonfinite: how many pixels had a NaN or an infinity in re or gt.
 *   camd_vis_l1_limit    limit[batch] (float64): CAMD_LIMIT_FIXED = value (> 0); CAMD_LIMIT_MAX = the maximum of |l1| (from
 *                        maxkey); CAMD_LIMIT_TOP = the |l1| at descending rank k = int(value * valid_num) among the valid
 *                        pixels (:556-561 with value = -max_l1 inside (0, 1); k is kept below valid_num), 1.0 for an image
 *                        without a valid pixel.  An exact radix select, 8 passes of 8 bits over the key's bit pattern,
 *                        state per image in workspace (camd_vis_l1_limit_workspace_bytes), nothing read back.
 *   camd_vis_l1_bar      the bar written from the limit ON THE DEVICE: max_l1=None with a colour bar, where the reference
 *                        raises (it negates None); defined as "resolve the limit without the bar, then paint it".
 *   camd_vis_l1_colour   :564-575: red l1 > 0, green l1 < 0, clip(0, limit) / limit * 0.9 + 0.1, masked, * 255, truncated;
 *                        with overexposed, |l1| > limit gives G, B = 255, 0 (positive) or R, B = 230, 230 (negative).  A
 *                        limit of 0 (0 / 0 in the reference) is defined as the normalised value 0.                  */
enum { CAMD_BAR_NONE = 0, CAMD_BAR_UP = 1, CAMD_BAR_DOWN = 2, CAMD_BAR_LEFT = 3, CAMD_BAR_RIGHT = 4 };
enum { CAMD_LIMIT_FIXED = 0, CAMD_LIMIT_MAX = 1, CAMD_LIMIT_TOP = 2 };
int camd_vis_l1_error(const void* re, const void* gt, double gt_value, int value_type, int w, int h, int batch, int bar_place,
                      int bar_width, double bar_max_l1, double* l1, uint8_t* valid, unsigned long long* maxkey,
                      unsigned int* nonfinite, void* stream);
size_t camd_vis_l1_limit_workspace_bytes(int batch);
int camd_vis_l1_limit(const double* l1, const uint8_t* valid, size_t npix, int batch, int mode, double value,
                      const unsigned long long* maxkey, void* workspace, double* limit, void* stream);
int camd_vis_l1_bar(double* l1, uint8_t* valid, int w, int h, int batch, int bar_place, int bar_width, const double* limit,
                    void* stream);
int camd_vis_l1_colour(const double* l1, const uint8_t* valid, size_t npix, int batch, const double* limit, int overexposed,
                       uint8_t* dst, void* stream);
/* vis_depth (utils.py:466-482; camera.py:317-319): d = depth / divisor (value_type CAMD_VALUE_F64 / _F32 / _U16; divisor 1
 * leaves it alone), zero = (d == 0), d clipped to [clip_lo, clip_hi] (+-infinity: no clip), n = (d - lo) / den, with
 * slicen != 0 n = (n * slicen) mod 1, index = uint8(n * scale), dst = table[index] (table: 256 x 3 bytes in device
 * memory), 0 where zero_mask and zero.  An index that is NaN (a constant image's 0 / 0) or outside 0 .. 255 is 0.
 * range_mode CAMD_RANGE_GIVEN: lo and den are the arguments; CAMD_RANGE_NORMA: lo = min, den = max - min;
 * CAMD_RANGE_MAX: lo = 0, den = max -- of keys[batch][2], which camd_vis_depth_range fills per image from the same d
 * (integer atomics on order-preserving keys: exact, no host read).                                                  */
enum { CAMD_RANGE_GIVEN = 0, CAMD_RANGE_NORMA = 1, CAMD_RANGE_MAX = 2 };
int camd_vis_depth_range(const void* depth, int value_type, size_t npix, int batch, double divisor, double clip_lo,
                         double clip_hi, unsigned long long* keys, void* stream);
int camd_vis_depth(const void* depth, int value_type, size_t npix, int batch, double divisor, double clip_lo, double clip_hi,
                   double lo, double den, const unsigned long long* keys, int range_mode, double slicen, double scale,
                   const uint8_t* table, int zero_mask, uint8_t* dst, void* stream);
/* vis_stereo (tiles = 2: img1 | img2) and vis_align (tiles = 4: img1 | img2 over img2 | img1) (utils.py:673-719).  Images
 * are packed u8, w x h, cn1 / cn2 = 1 (replicated) or 3.  rows[h] / cols[2 * w] (cols NULL: none): the colour index 0 .. 5
 * of the line through that row of a tile / that column of the mosaic, -1 for none; the host computes them in integers
 * as the reference's loop does; columns win.  Tile t of image b is written at dst + b * image_stride + t * tile_stride
 * with rows dst_pitch bytes apart.                                                                                 */
int camd_vis_lines(const uint8_t* img1, int cn1, const uint8_t* img2, int cn2, int w, int h, int batch, const int8_t* rows,
                   const int8_t* cols, int tiles, uint8_t* dst, size_t dst_pitch, size_t tile_stride, size_t image_stride,
                   void* stream);

/* ---- all triples of a multi-view reconstruction in one pass (csrc/epipolar.hip; reconstruction_epipolar_geometry.py) ----
 * The batched form of the three camd_cell_* steps above: many point sets / many pairs of grids per launch, chosen by
 * blockIdx.y from a table.  Tables are HOST arrays; every entry is checked here against grid_cells / ncols before it is
 * copied to the caller's device table (nsets / ntriples entries, 1 .. 65535) and used, so no table can index outside
 * the buffers given.  uv: [n][2] contiguous.  Integer atomics only: the bits are those of the single calls.         */
typedef struct camd_cell_set {
    const void* uv;                 /* device rows [n][2] of uv_type */
    unsigned long long n;           /* < 2^32 - 1 */
    unsigned long long grid_offset; /* where this set's cells_w * cells_h grid starts in grids, in cells */
    int uv_type, cu0, cv0, cells_w, cells_h, reserved;
} camd_cell_set;
typedef struct camd_cell_triple {
    unsigned long long grid_offset1, grid_offset2; /* the two grids (one window: cells_w x cells_h) */
    unsigned long long column_offset;              /* where its cells_w columns start in colcount / start */
    int cells_w, cells_h;
} camd_cell_triple;
/* bounds[(set * B + b) * 4 + 0..3] = min u, min v, max u, max v over the rows block b of B = camd_uv_bounds_blocks()
 * took (+inf / -inf where it took none, NaN where it met a NaN); the caller takes the minimum / maximum over b on the
 * host.  The window fields of the sets are not read.                                                              */
int camd_uv_bounds_blocks(void);
int camd_uv_bounds_batch(const camd_cell_set* sets_host, int nsets, camd_cell_set* sets_dev, double* bounds, void* stream);
/* camd_cell_first_index of every set into its own grid (grids: grid_cells uint32, cleared here; *outside as above)  */
int camd_cell_first_index_batch(const camd_cell_set* sets_host, int nsets, camd_cell_set* sets_dev, double max_distance,
                                uint32_t* grids, size_t grid_cells, unsigned long long* outside, void* stream);
/* camd_cell_intersect_count / _emit of every triple: colcount[column_offset + c] for c < cells_w; the caller scans ALL
 * ncols counts once (start: ncols + 1 int64, start[0] = 0); triple k's pairs are idx1 / idx2[start[column_offset] ..) and
 * counts[k] (device u64) = how many.  Triples' columns must not overlap and should tile [0, ncols).  One workgroup per
 * (u column, triple).                                                                                              */
int camd_cell_intersect_count_batch(const uint32_t* grids, size_t grid_cells, const camd_cell_triple* triples_host, int ntriples,
                                    camd_cell_triple* triples_dev, uint32_t* colcount, size_t ncols, void* stream);
int camd_cell_intersect_emit_batch(const uint32_t* grids, size_t grid_cells, const camd_cell_triple* triples_host, int ntriples,
                                   camd_cell_triple* triples_dev, const long long* start, size_t ncols, long long* idx1,
                                   long long* idx2, size_t capacity, unsigned long long* counts, void* stream);
/* The per-view depth rows of ReconstructionExtrinsics (:225-241), [rows_total][4] float64 = [u, v, z, other view]:
 * rows[row_offset + i] = [float64(uv[i][0]), float64(uv[i][1]), z[i], other_view] for i < n.  uv: [n][2] of uv_type.  */
int camd_uvzi_pack(const void* uv, int uv_type, const double* z, size_t n, double other_view, double* rows, size_t rows_total,
                   size_t row_offset, void* stream);
/* *sum (device) = sum of rows[row_offset + i][column], i < n, of a [rows_total][columns] float64 array: the numerator
 * of uvzis[:, 2].mean().  REDUCTION SHAPE: that of camd_vector_sum -- G = camd_column_sum_blocks(n) = clamp(ceil(n / 256),
 * 1, 1024) workgroups, m = ceil(n / (256 G)) serial terms per thread, d = 18 tree levels, block partials in index
 * order, no float atomics.  partials_ws: G doubles.  n >= 1.                                                       */
int camd_column_sum_blocks(size_t n);
int camd_column_sum(const double* rows, size_t rows_total, int columns, int column, size_t row_offset, size_t n,
                    double* partials_ws, double* sum, void* stream);
/* rows[row_offset + i][column] *= rate, i < n: one multiply per element (uvzis[:, 2] *= rate)                        */
int camd_column_scale(double* rows, size_t rows_total, int columns, int column, size_t row_offset, size_t n, double rate,
                      void* stream);

/* ---- matched points between the raw image and the pinhole model (csrc/points.hip) ----------------------------
 * What stands between a matcher, which sees the raw frames, and the epipolar path above, which takes pinhole pixels.
 * One lane per point; rows are read in place: `*_stride` elements of `*_type` CAMD_VALUE_F64 / CAMD_VALUE_F32 from one
 * row to the next, so (u, v) / (x, y, z) may be the leading columns of uvzs / uvzis / xyzuv rows.  n < 2^31; n == 0
 * launches nothing.  out: [n][2] contiguous, aligned to one row (2 elements), not overlapping the input.  K: 9 host
 * doubles; dist: ndist = 0, 4, 5, 8, 12 or 14 host doubles (k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4 tauX tauY); non-zero
 * tauX / tauY are refused with CAMD_ERR_UNSUPPORTED.  float64 inside, no contraction, every division rounded once.
 *
 * replaces cv2.undistortPoints(uvs, K, D) of Cam.undistort_points (camera.py:286; epipolar_geometry.py:285-288, 327 begins
 * with it), no R, no P: x = (u - cx) * (1 / fx), y alike; with ndist != 0, x0 = x and `iters` (1 .. 100; cv2 runs 5, it
 * has no epsilon test here) rounds of
 *   r2 = x*x + y*y;  icdist = (1 + ((k6*r2 + k5)*r2 + k4)*r2) / (1 + ((k3*r2 + k2)*r2 + k1)*r2)
 *   icdist < 0: the point keeps its start value and is iterated no further
 *   dX = 2*p1*x*y + p2*(r2 + 2*x*x) + s1*r2 + s2*r2*r2;  dY = p1*(r2 + 2*y*y) + 2*p2*x*y + s3*r2 + s4*r2*r2
 *   x = (x0 - dX) * icdist;  y = (y0 - dY) * icdist
 * The normalised point is rounded to uv_type -- cv2's hand-over -- and stored as out_type.  out_type |
 * CAMD_POINTS_PIXELS: it goes back to pixels of the undistorted camera first, value * fx + cx and value * fy + cy in
 * float64: the whole of camera.py:286-287 with out_type CAMD_VALUE_F64.                                            */
enum { CAMD_POINTS_PIXELS = 0x100 };
int camd_undistort_points(const void* uv, int uv_type, size_t n, int uv_stride, const double K[9], const double* dist,
                          int ndist, int iters, void* out, int out_type, void* stream);
/* replaces cv2.projectPoints(xyzs, rvec, tvec, K, D)[0] of Cam.project_points (camera.py:275-280), no Jacobians; R = the
 * matrix of rvec (9 host doubles, row-major), t: 3 host doubles.  X = R0*x + R1*y + R2*z + t0 summed left to right, Y, Z
 * alike; iz = Z ? 1 / Z : 1; the distortion polynomial of camd_distort_index_map on (X*iz, Y*iz); u = xd*fx + cx,
 * v = yd*fy + cy, stored in xyz_type.                                                                               */
int camd_project_points(const void* xyz, int xyz_type, size_t n, int xyz_stride, const double R[9], const double t[3],
                        const double K[9], const double* dist, int ndist, void* out, void* stream);

/* ---- the pose of a target from its detected points, every frame of a recording in one launch (csrc/pnp.hip) ----
 * replaces cv2.solvePnPGeneric(object_points, image_points[:, None], K, D) of Cam.perspective_n_point (camera.py:266-273):
 * UNPINNED against cv2.  One wavefront per frame, four frames per workgroup, no workgroup
 * barrier; a frame's outputs depend on its own rows only, so they are the same bits alone and at any place of a batch.
 *
 * The points: frame f owns rows start[f] .. start[f + 1] of `image` ([u, v], raw distorted pixels) and of `object`
 * ([x, y, z]); with object_shared the object rows are one block shared by every frame (one board), frame f reading its
 * first start[f + 1] - start[f] rows.  Rows are read in place, `*_stride` elements of `*_type` CAMD_VALUE_F64 /
 * CAMD_VALUE_F32 apart.  start: frames + 1 int64 ON THE DEVICE; a range outside image_rows / object_rows is not read (status
 * 2).  K, dist, ndist as in camd_project_points.  queue: the HIP stream the launch is queued on.             */
typedef struct camd_pnp_points {
    const void* object;
    const void* image;
    const long long* start;
    unsigned long long object_rows, image_rows;
    int object_type, image_type, object_stride, image_stride, object_shared, frames;
} camd_pnp_points;
/* A start pose per frame -> pose[f] = R (9, row-major), t (3): the normal matrix of the direct linear transform on
 * Hartley-normalised points (image points undistorted by camd_undistort_points' iteration, 10 rounds), reduced over the
 * wave; its null vector by inverse iteration; scale, sign (target in front) and Gram-Schmidt.  planar != 0: the 9 x 9
 * matrix of the homography, on the object points turned by `plane` (9 host doubles: the rotation that lays the target's
 * plane on z = const), >= 4 points; planar == 0: the 12 x 12 matrix of the projection matrix, >= 6 points.  A frame
 * that cannot be started (too few points, a non-finite coordinate, no null vector) gets NaN.                        */
int camd_pnp_init(const camd_pnp_points* points, const double K[9], const double* dist, int ndist, int planar,
                  const double plane[9], double* pose, void* queue);
/* Levenberg-Marquardt in float64 from pose0[f * pose0_stride] (pose0_stride 12, or 0: one start for all frames): the
 * residual is camd_project_points' pixel minus the observed one, the step a local perturbation R <- exp([w]x) R,
 * t <- t + d; (J^T J + lambda diag(J^T J)) delta = -J^T r by Cholesky, lambda = 1e-3 at the start, / 10 after a step
 * that lowers the cost, * 10 after one that does not.  It stops when |delta| < eps (|p| + eps), eps = 2^-52, |p|^2 =
 * 3 + |t|^2; when lambda leaves [1e-12, 1e12]; or after 100 evaluations.  Per frame: pose (as above), rms = sqrt(cost /
 * 2n), iterations (evaluations after the first), status: 0 ok, 1 fewer than min_points (>= 3) points, 2 a non-finite
 * coordinate, 3 singular (a pivot of the unit-diagonal J^T J below 1e-10, no finite start) or not stopped at the cap.
 * status != 0: pose and rms are NaN.  pose must not overlap pose0.                                                   */
int camd_pnp_refine(const camd_pnp_points* points, const double K[9], const double* dist, int ndist, int min_points,
                    const double* pose0, int pose0_stride, double* pose, double* rms, int* iterations, int* status, void* queue);

/* ---- a camera's intrinsics and every frame's pose from detected points (csrc/calibrate.hip) ----
 * replaces cv2.calibrateCamera of Cam.calibrate (camera.py:63-93) for fx fy cx cy | k1 k2 p1 p2 k3: UNPINNED against cv2
 * (DESIGN.md section 2, U29).  A float64 Levenberg-Marquardt on raw pixels over the nine shared unknowns and six per
 * frame (camd_pnp_refine's local pose update), solved through the Schur complement on the shared block; damping and
 * stopping as in camd_pnp_refine, on the joint step; a candidate is accepted when its cost is lower, or higher by at most 64
 * ulp of the cost (the rounding of the sums).  The points are a camd_pnp_points.  The frames of the joint problem
 * are `used`: used_n int32 frame indices ON THE DEVICE, rising; per-frame arrays of these calls have one row per USED
 * frame.  All sums over frames have a fixed order (a stride of 64 over the used frames, then a butterfly): the same
 * input gives the same bits on every run.
 *
 * state: CAMD_CALIB_STATE_DOUBLES device doubles, written by the caller before the first call:
 *   [CAMD_CALIB_LAMBDA] = 1e-3, [CAMD_CALIB_K .. + 9) = fx fy cx cy k1 k2 p1 p2 k3 of the start,
 *   [CAMD_CALIB_MASK .. + 9) = 1 for a free entry of the block and 0 for a fixed one, everything else 0.
 * After camd_calib_step: [CAMD_CALIB_DONE] != 0 when the iteration has ended (stopped by the rule, or 100 evaluations),
 * [CAMD_CALIB_ACCEPT] != 0 when the step was taken (then the next step needs camd_calib_linearise first).
 * After camd_calib_finish: [CAMD_CALIB_STATUS] 0 ok / 3 singular (a pivot of the unit-diagonal reduced matrix below 1e-10)
 * or not converged at the cap, [CAMD_CALIB_COST] the sum of squared residuals, [CAMD_CALIB_K .. + 9) the result.     */
#define CAMD_CALIB_STATE_DOUBLES 40
#define CAMD_CALIB_WORKSPACE_DOUBLES 136 /* per used frame: A 21, B 54, C 45, gp 6, gk 9, c 1 */
#define CAMD_CALIB_CANDIDATE_DOUBLES 16  /* per used frame: R 9, t 3, cost, |step|^2, |pose|^2, unused */
enum {
    CAMD_CALIB_DONE = 0, CAMD_CALIB_ACCEPT = 1, CAMD_CALIB_LAMBDA = 2, CAMD_CALIB_COST = 3, CAMD_CALIB_EVALUATIONS = 4,
    CAMD_CALIB_ITERATIONS = 5, CAMD_CALIB_STATUS = 6, CAMD_CALIB_CONVERGED = 7, CAMD_CALIB_K = 8, CAMD_CALIB_DK = 17,
    CAMD_CALIB_MASK = 26, CAMD_CALIB_SOLVED = 35, CAMD_CALIB_PIVOT = 36
};
/* The start: H[f] = the homography (9, row-major) from the target's plane -- the object points turned by `plane`, 9 host
 * doubles, their x and y -- to raw pixels, by camd_pnp_init's Hartley-normalised direct linear transform with an identity
 * camera and no lens; NaN for a frame of fewer than 4 points, with a non-finite coordinate or without a null vector.
 * H: frames x 9 device doubles.                                                                                    */
int camd_calib_homography(const camd_pnp_points* points, const double plane[9], double* H, void* queue);
/* The sums of every used frame at state's K and `poses` (used_n x 12: R, t) -> workspace (used_n x 136).          */
int camd_calib_linearise(const camd_pnp_points* points, const int* used, int used_n, double* state, double* poses,
                         double* workspace, void* queue);
/* One evaluation at state's lambda: the reduced system and the block's step; every frame's step, candidate pose and
 * cost (candidate: used_n x 16); accept (poses and state's K take the candidate) or reject; lambda; the stop flags.  */
int camd_calib_step(const camd_pnp_points* points, const int* used, int used_n, double* state, double* poses,
                    double* candidate, double* workspace, void* queue);
/* After the last linearisation: the status, the cost, and frame_error[u] = sqrt(sum |r|^2 / n) of every used frame.   */
int camd_calib_finish(const camd_pnp_points* points, const int* used, int used_n, double* state, double* workspace,
                      double* frame_error, void* queue);
/* The first `count` doubles of state -> out (host), after everything queued before; returns when they have arrived.  */
int camd_calib_read(const double* state, int count, double* out, void* queue);

/* ---- a rig's R, t and the board's pose in every frame from the points both cameras detected (csrc/stereo_calibrate.hip) ----
 * replaces cv2.stereoCalibrate(..., flags=CALIB_FIX_INTRINSIC) of Stereo.get_R_t_by_stereo_calibrate
 * (stereo_camera.py:95-123): UNPINNED against cv2.  Both cameras' K and D stay fixed.  A float64
 * Levenberg-Marquardt on raw pixels over the six unknowns of the rig (x2 = R x1 + t; R <- exp([w]x) R, t <- t + d) and
 * six per frame (the board in camera 1, camd_pnp_refine's local pose update), solved through the Schur complement on the
 * rig's block; damping, stopping and acceptance as in camd_calib_step.  The frames of the joint problem are `used`, as
 * in camd_calib_*.  The sums over frames have two levels of fixed order -- a lane per frame and a butterfly over the 64
 * frames of a workgroup, then one wavefront over the workgroups' partials in rising order --, without atomics: the same
 * input gives the same bits on every run.
 *
 * points1 / points2: the same object rows, start and frames; `image` (with its type and stride) is camera 1's / camera
 * 2's.  K, dist, ndist of each camera as in camd_project_points (host).  Device arrays: used (used_n int32, rising),
 * state (CAMD_STEREO_STATE_DOUBLES), poses (used_n x 12: R_i, t_i), candidate (used_n x CAMD_STEREO_CANDIDATE_DOUBLES),
 * workspace (used_n x CAMD_STEREO_WORKSPACE_DOUBLES), partials (ceil(used_n / 64) x CAMD_STEREO_PARTIAL_DOUBLES),
 * frame_error (used_n).
 *
 * state, written by the caller before the first call: [CAMD_STEREO_LAMBDA] = 1e-3, [CAMD_STEREO_RIG .. + 12) = R (9,
 * row-major), t (3) of the start, everything else 0.  Its first two places are camd_calib's and camd_calib_read reads it:
 * after camd_stereo_step [CAMD_STEREO_DONE] != 0 when the iteration has ended (stopped by the rule, or 100 evaluations),
 * [CAMD_STEREO_ACCEPT] != 0 when the step was taken (then the next step needs camd_stereo_linearise first, which also
 * moves every frame's candidate into `poses`).  After camd_stereo_finish: [CAMD_STEREO_STATUS] 0 ok / 3 singular (a pivot
 * of the unit-diagonal reduced matrix below 1e-10) or not converged at the cap, [CAMD_STEREO_COST] the sum of squared
 * residuals of both cameras, [CAMD_STEREO_RIG .. + 12) the result.                                                   */
#define CAMD_STEREO_STATE_DOUBLES 40
#define CAMD_STEREO_WORKSPACE_DOUBLES 91 /* per used frame: A 21, B 36, C 21, gp 6, gr 6, c 1 */
#define CAMD_STEREO_CANDIDATE_DOUBLES 16 /* per used frame: R 9, t 3, cost, |step|^2, |pose|^2, unused */
#define CAMD_STEREO_PARTIAL_DOUBLES 36   /* per 64 used frames: S 21, g 6, diag C 6, cost; frames that did not factor; unused */
enum {
    CAMD_STEREO_DONE = 0, CAMD_STEREO_ACCEPT = 1, CAMD_STEREO_LAMBDA = 2, CAMD_STEREO_COST = 3, CAMD_STEREO_EVALUATIONS = 4,
    CAMD_STEREO_ITERATIONS = 5, CAMD_STEREO_STATUS = 6, CAMD_STEREO_CONVERGED = 7, CAMD_STEREO_RIG = 8, CAMD_STEREO_STEP = 20,
    CAMD_STEREO_CANDIDATE = 26, CAMD_STEREO_SOLVED = 38, CAMD_STEREO_PIVOT = 39
};
typedef struct camd_stereo_rig {
    camd_pnp_points points1, points2;
    const double* K1;     /* 9 host doubles */
    const double* dist1;  /* ndist1 host doubles */
    const double* K2;
    const double* dist2;
    const int* used;
    double* state;
    double* poses;
    double* candidate;
    double* workspace;
    double* partials;
    double* frame_error;
    int ndist1, ndist2, used_n, reserved;
} camd_stereo_rig;
/* The sums of every used frame at state's rig and `poses` -> workspace; needs poses and candidate.                 */
int camd_stereo_linearise(const camd_stereo_rig* rig, void* queue);
/* One evaluation at state's lambda: every frame's reduced contribution and the partials; the rig's step and candidate;
 * every frame's step, candidate pose and cost in both cameras; accept (state's rig takes the candidate) or reject;
 * lambda; the stop flags.  Needs poses, candidate and partials.                                                     */
int camd_stereo_step(const camd_stereo_rig* rig, void* queue);
/* After the last linearisation: the status, the cost, and frame_error[u] = sqrt(sum (|r1|^2 + |r2|^2) / 2n) of every
 * used frame.  Needs partials and frame_error.                                                                     */
int camd_stereo_finish(const camd_stereo_rig* rig, void* queue);

/* ---- the poses of N views and a world point per match, refined together (csrc/bundle.hip) ----
 * The joint refinement after ReconstructionExtrinsics' propagation; the reference has none, the contract is this project's
 * (INTEGRATION.md section F).  3 <= views <= CAMD_BUNDLE_MAX_VIEWS; pair p = (a, b), a < b, owns rows pair_start[p] ..
 * pair_start[p + 1] of uv_a / uv_b ([matches][2] pinhole pixels of uv_type CAMD_VALUE_F64 / F32, read in place); every
 * match is one world point with two observations.  A float64 Levenberg-Marquardt on pixels over 3 unknowns per used match
 * and 6 per view (camd_pnp_refine's local update of the world-to-camera pose), solved through the Schur complement on the
 * views' block; damping, stopping and acceptance as in camd_calib_step; a candidate that puts a used point at z <= 0 in
 * either of its views is rejected.  Held: the pose of view [CAMD_BUNDLE_FIXED] and coordinate [CAMD_BUNDLE_AXIS] of the
 * world centre of view [CAMD_BUNDLE_ANCHOR].  All sums have a fixed order and there are no atomics.
 *
 * state (CAMD_BUNDLE_STATE_DOUBLES device doubles), written by the caller before camd_bundle_start: [LAMBDA] = 1e-3,
 * [FIXED], [ANCHOR], [AXIS], [LABEL + v] the number written for view v into the depth rows, [POSES + 12 v ..) = R (9,
 * row-major), t (3) of view v (x_cam = R x_world + t), [K + 4 v ..) = fx fy cx cy, everything else 0.  Its first places are
 * camd_calib's, read by camd_calib_read.
 *
 * camd_bundle_start: status[row] = 0 ok / 1 a non-finite coordinate / 2 the rays' midpoint is at z <= 0 in either view or
 * |d_a x d_b| < 0.03 for the unit rays / 3 (threshold >= 0 only) the midpoint's reprojection error exceeds `threshold`
 * pixels in either view; points[row] = the midpoint (NaN unless status 0); rowoff = the exclusive scan of the used rows of
 * every segment (segments + 1 entries; segment s owns seg_n[s] <= CAMD_BUNDLE_SEGMENT rows from seg_first[s], of ONE pair).
 * The caller reads rowoff, sizes the arrays below and makes chunk_table (chunks x 4 int32: pair, first used point, points
 * <= CAMD_BUNDLE_CHUNK, 0; a chunk never straddles two pairs; rising) and pair_chunk (pairs + 1).
 * camd_bundle_emit: the used rows, in their order, to uv_used_a / uv_used_b (used x 2 of uv_type), X (used x 3), src (used).
 * camd_bundle_step: one evaluation; afterwards [DONE], [ACCEPT] as in camd_stereo_step (nothing else is needed between steps).
 * camd_bundle_finish: [STATUS] 0 ok / 3 singular (a pivot of the undamped unit-diagonal reduced matrix below 1e-10, in
 * [PIVOT]) or not stopped at 100 evaluations, [COST], [COST0]; pair_error[p] = sqrt(cost_p / 2 n_p); points[src] = the
 * refined points; rows_a / rows_b (used x 4, or both NULL) = [u, v, z, label of the other view] of every used point in view
 * a / view b of its pair (camd_uvzi_pack's layout).                                                                     */
#define CAMD_BUNDLE_MAX_VIEWS 16
#define CAMD_BUNDLE_CHUNK 256
#define CAMD_BUNDLE_SEGMENT 1024
#define CAMD_BUNDLE_PARTIAL_DOUBLES 104 /* S_aa 21, S_bb 21, S_ba 36, g_a 6, g_b 6, diag U_a 6, diag U_b 6, cost, points that did not factor */
#define CAMD_BUNDLE_EVAL_DOUBLES 4      /* the candidate's cost, |dX|^2, |X|^2, points it puts behind a view */
#define CAMD_BUNDLE_STATE_DOUBLES 576
enum {
    CAMD_BUNDLE_DONE = 0, CAMD_BUNDLE_ACCEPT = 1, CAMD_BUNDLE_LAMBDA = 2, CAMD_BUNDLE_COST = 3, CAMD_BUNDLE_EVALUATIONS = 4,
    CAMD_BUNDLE_ITERATIONS = 5, CAMD_BUNDLE_STATUS = 6, CAMD_BUNDLE_CONVERGED = 7, CAMD_BUNDLE_SOLVED = 8, CAMD_BUNDLE_PIVOT = 9,
    CAMD_BUNDLE_FIXED = 10, CAMD_BUNDLE_ANCHOR = 11, CAMD_BUNDLE_AXIS = 12, CAMD_BUNDLE_COST0 = 13, CAMD_BUNDLE_LABEL = 16,
    CAMD_BUNDLE_POSES = 32, CAMD_BUNDLE_CANDIDATE = 224, CAMD_BUNDLE_STEP = 416, CAMD_BUNDLE_K = 512
};
typedef struct camd_bundle {
    const void* uv_a;
    const void* uv_b;
    const int* pair_views;       /* pairs x 2 */
    const long long* pair_start; /* pairs + 1 */
    const long long* seg_first;  /* segments */
    const int* seg_n;            /* segments */
    const int* chunk_table;      /* chunks x 4 */
    const long long* pair_chunk; /* pairs + 1 */
    int* status;                 /* matches */
    double* points;              /* matches x 3 */
    unsigned long long* rowoff;  /* segments + 1 */
    uint32_t* rowcount;          /* segments */
    void* uv_used_a;
    void* uv_used_b;
    double* X;
    double* candidate;           /* used x 3 */
    long long* src;              /* used */
    double* partials;            /* chunks x CAMD_BUNDLE_PARTIAL_DOUBLES */
    double* pair_blocks;         /* pairs x CAMD_BUNDLE_PARTIAL_DOUBLES */
    double* eval_partials;       /* chunks x CAMD_BUNDLE_EVAL_DOUBLES */
    double* eval_blocks;         /* pairs x CAMD_BUNDLE_EVAL_DOUBLES */
    double* state;
    double* pair_error;          /* pairs */
    double* rows_a;
    double* rows_b;
    double threshold;            /* pixels; < 0: none */
    long long matches, used;
    int uv_type, views, pairs, segments, chunks, reserved;
} camd_bundle;
/* max_pair_rows: the rows of the largest pair (the launch's width) */
int camd_bundle_start(const camd_bundle* bundle, long long max_pair_rows, void* queue);
int camd_bundle_emit(const camd_bundle* bundle, void* queue);
int camd_bundle_step(const camd_bundle* bundle, void* queue);
int camd_bundle_finish(const camd_bundle* bundle, void* queue);

/* ---- detected corners refined to sub-pixel, every corner of every frame in one launch (csrc/subpix.hip) ----
 * replaces cv2.cornerSubPix(gray, corners, win, zero_zone, criteria) of Chessboard.find_image_points (boards.py:163-169):
 * UNPINNED against cv2.  One wavefront per corner, four corners per workgroup, no workgroup
 * barrier; a corner's outputs depend on its own start and its frame only, so they are the same bits alone and anywhere in
 * a batch.
 *
 * gray: `frames` u8 images of w x h with the pitch / stride conventions of camd_remap_u8 (cn = 1).  corners: `rows` rows
 * [x, y] of corner_type CAMD_VALUE_F64 / CAMD_VALUE_F32, contiguous.  start == NULL: dense, frame f owns rows
 * f * (rows / frames) ... ; otherwise frames + 1 int64 ON THE DEVICE, rising, as camd_pnp_points.start: frame f owns rows
 * start[f] .. start[f + 1] and may own none.  The start rows live on the device and are not checked by the host: a row
 * that no frame owns (rows beyond start[frames], rows that do not rise) gets status bit 8, and rows that rise but are not
 * the caller's split give a corner to another frame -- the frame index always stays below `frames`, so no memory beyond
 * the images is read either way.  mask: (2 win_h + 1) * (2 win_w + 1) float32 weights ON THE DEVICE, made by
 * the caller (row i, column j: exp(-y^2) exp(-x^2) with y = (i - win_h) / win_h, x alike, in float32, zero over the zero
 * zone), so the kernel calls no exp.  max_iters 1 .. 100; eps >= 0 is the SQUARED step below which the iteration ends.
 *
 * Per corner, with cT = the start rounded to float32 and cI = cT:
 *   patch  (2 win_w + 3) x (2 win_h + 3) float32 samples around cI: cx = cI.x - (pw - 1) * 0.5f, ix = floor(cx), a = cx - ix,
 *          y alike with b; ((a11 p00 + a12 p01) + a21 p10) + a22 p11 with a11 = (1 - a)(1 - b), a12 = a (1 - b),
 *          a21 = (1 - a) b, a22 = a b in float32; source coordinates clamped to the image
 *   sums   in float64 over the window, pixel k = i * (2 win_w + 1) + j: tgx = right - left, tgy = lower - upper sample,
 *          m = mask[k]; gxx = tgx tgx m, gxy = tgx tgy m, gyy = tgy tgy m; px = j - win_w, py = i - win_h;
 *          a += gxx, b += gxy, c += gyy, bb1 += gxx px + gxy py, bb2 += gxy px + gyy py.  Pixel k belongs to lane
 *          k % 64, a lane adds its pixels in rising k, the lanes' sums meet in a butterfly (xor 1, 2, ... 32)
 *   solve  det = a c - b b; |det| <= DBL_EPSILON^2: stop (status bit 1).  scale = 1 / det;
 *          cI2.x = (float)(cI.x + c scale bb1 - b scale bb2), cI2.y = (float)(cI.y - b scale bb1 + a scale bb2);
 *          err = the squared float32 step, in float64; cI = cI2; outside [0, w) x [0, h): stop (bit 2)
 *   loop   while (++iter < max_iters && err > eps)
 *   revert |cI.x - cT.x| > win_w or |cI.y - cT.y| > win_h: the result is cT (bit 4)
 * A start that is not finite, lies outside [0, w) x [0, h) or belongs to no frame: status bit 8, the corner comes back as
 * it came and no pixel is read (cv2 asserts).  out: rows x 2 of corner_type (a float64 holds the float32 result exactly);
 * iterations: the patches sampled; status: the bits above, 0 = converged or stopped at max_iters.
 * CAMD_ERR_BAD_ARG: win <= 0, an image smaller than 2 win + 5 on a side (cv2's assertion); CAMD_ERR_UNSUPPORTED: a patch
 * beyond 4096 floats (half-sizes up to (30, 30) fit).  queue: the HIP stream the launch is queued on.                  */
int camd_corner_sub_pix(const uint8_t* gray, int w, int h, size_t pitch, size_t stride, int frames, const void* corners,
                        int corner_type, size_t rows, const long long* start, int win_w, int win_h, const float* mask,
                        int max_iters, double eps, void* out, int* iterations, int* status, void* queue);
/* replaces cv2.cvtColor(img, cv2.COLOR_BGR2GRAY) on u8 (boards.py:159): UNPINNED against cv2.
 * dst = (c0 * k0 + c1 * k1 + c2 * k2 + (1 << (shift - 1))) >> shift per pixel of a three-channel image, c0 the first byte
 * of the pixel; the weights are >= 0 and add up to 1 << shift (cv2 4.x, recalled: 3735, 19235, 9798 and 15 for B, G, R).
 * Batched; pitch / stride conventions of camd_remap_u8 (src cn = 3, dst cn = 1).                                      */
int camd_bgr_to_gray_u8(const uint8_t* src, int w, int h, size_t src_pitch, size_t src_stride, uint8_t* dst, size_t dst_pitch,
                        size_t dst_stride, int batch, int k0, int k1, int k2, int shift, void* queue);

/* ---- chessboard corners from the image alone (csrc/chessboard.hip) ----
 * Stands where the reference calls cv2.findChessboardCorners (boards.py:160) with a contract of its OWN, not cv2's
 * (INTEGRATION.md section J): three stages, every value an integer, restated in NumPy by tests/chessboard_ref.py.      */
#define CAMD_CHESS_CAPACITY 1024   /* candidates kept per frame */
#define CAMD_CHESS_MAX_CORNERS 512 /* across * down */
/* Stage 1.  gray: frames images of w x h uint8, rows `pitch` and images `stride` bytes apart.  response: frames * h * w
 * int16, dense; response_max: one int32 per frame.  With g the image and I[0 .. 15] = g(x + dx, y + dy) at (dx, dy) =
 * (5,0) (5,2) (4,4) (2,5) (0,5) (-2,5) (-4,4) (-5,2) (-5,0) (-5,-2) (-4,-4) (-2,-5) (0,-5) (2,-5) (4,-4) (5,-2):
 *   sr = sum n<4 |I[n] + I[n+8] - I[n+4] - I[n+12]|, dr = sum n<8 |I[n] - I[n+8]|, ring = sum I,
 *   local = g(x, y) + g(x-1, y) + g(x+1, y) + g(x, y-1) + g(x, y+1),  r = 5 sr - 5 dr - |5 ring - 16 local|
 * (the ChESS response times 5), r = 0 within 5 px of a border; -30600 <= r <= 10200.  response_max >= 0.             */
int camd_chess_response(const uint8_t* gray, int w, int h, size_t pitch, size_t stride, int frames, int16_t* response,
                        int* response_max, void* queue);
/* Stage 2.  Pixel p is a candidate when r(p) > 0, relative * r(p) >= response_max[frame], and within the
 * (2 nms_radius + 1)^2 window clipped to the image r(p) > r(q) for every q before p in pixel order and r(p) >= r(q) for
 * every q after it.  peaks: frames x CAMD_CHESS_CAPACITY x 2 int32 (x, y), a frame's candidates in pixel order (those
 * beyond the capacity are dropped, the entries beyond the count are not written); counts: the candidates of each frame
 * in full.  workspace: camd_chess_peaks_workspace_bytes(h, frames) device bytes, 8-aligned.  relative 1 .. 64,
 * nms_radius 1 .. 8, else CAMD_ERR_UNSUPPORTED.                                                                      */
size_t camd_chess_peaks_workspace_bytes(int h, int frames);
int camd_chess_peaks(const int16_t* response, const int* response_max, int w, int h, int frames, int relative, int nms_radius,
                     void* workspace, int* peaks, int* counts, void* queue);
/* Stage 3, one wavefront per frame.  status: 2 where counts > CAMD_CHESS_CAPACITY, 1 where counts < n = across * down,
 * else the lattice is grown -- int32 / int64 squared distances and cross products, ties to the lowest candidate index:
 *   seed s minimises |m p - sum p|^2 over the m candidates; a is the nearest to s, u = a - s; b the nearest to s with
 *   4 cross(u, b - s)^2 >= |u|^2 |b - s|^2, v = b - s (none: status 4).  s is cell (0, 0); breadth first in queue order,
 *   directions +i, -i, +j, -j: a neighbour cell that is still empty is predicted at p + step, step = p - (the cell
 *   behind p) if labelled, else the same-direction step between the labelled pair beside p -- cells (i, j-1),(i+di, j-1)
 *   then (i, j+1),(i+di, j+1) for +-i; (i-1, j),(i-1, j+dj) then (i+1, .) for +-j --, else +-u / +-v; the nearest
 *   unlabelled candidate c takes the cell when 4 |c - prediction|^2 <= |step|^2.  Growth ends when more than n are labelled.
 *   Found: exactly n labelled, filling a box of across x down or down x across.  Order: across fastest; of the labelings
 *   of that shape with cross(sum of row steps, sum of column steps) > 0 (y down) the one whose corner 0 has the lowest
 *   y * w + x.  Otherwise status 4.
 * corners: frames x n x 2 float32, integer-valued, NaN where status != 0.  across, down >= 2, n <= CAMD_CHESS_MAX_CORNERS,
 * w, h <= 16384, else CAMD_ERR_UNSUPPORTED.                                                                          */
int camd_chess_lattice(const int* peaks, const int* counts, int w, int h, int frames, int across, int down, float* corners,
                       int* status, void* queue);

/* ---- the inner corners of a ChArUco board by id, cut or partly covered boards included (csrc/charuco.hip) ----
 * Stands where the reference calls cv2.aruco.detectMarkers / interpolateCornersCharuco (boards.py:359-368) with a contract
 * of its OWN, every value an integer, restated in NumPy by tests/charuco_ref.py.  peaks and
 * counts are camd_chess_peaks' of the same frames; gray as for camd_chess_response.  One wavefront per frame.
 *   Board: squares_x x squares_y squares, the top-left one black; markers of s x s bits plus a black ring of one cell,
 *   marker_num / marker_den of a square wide, centred in the squares with x % 2 != y % 2, their ids ascending from
 *   first_id in row-major order; dictionary_words[id]: bit (r, c) of weight 2^(s*s - 1 - (r*s + c)), 1 = white.  Inner
 *   corner y * (squares_x - 1) + x lies between squares (x, y) and (x + 1, y + 1).
 *   Lattice: seeds in order of |m p - sum p|^2; a seed's steps are u to one of its 16 nearest peaks and v to one of the 16
 *   nearest with 4 cross(u, v)^2 >= |u|^2 |v|^2, the first pair (u outermost) whose fourth corner has a peak within
 *   min(|u|, |v|) / 4 and in whose cell a marker of the board decodes; u, v swapped where cross(u, v) < 0.  Breadth first
 *   as camd_chess_lattice, a peak accepted within an eighth of the step, labels -15 .. 15, at most 320.
 *   Decode: sample (a, b) of the (s + 2)^2 lies at the bilinear blend of the cell's corners with weights A / D, D =
 *   2 den (s + 2), A[a] = den (s + 2) + num (2 a + 1 - (s + 2)), rounded to a pixel; its value is the sum of the 3 x 3
 *   pixels there; a bit is 1 where 2 value > lo + hi of the cell's extremes, hi - lo >= 9 * 40; the ring is all 0; the
 *   s*s bits turned 0 .. 3 quarter turns (np.rot90) against every id: the least (errors, id, turn) within max_bit_errors.
 *   Vote: a marker fixes the turn and the offset of lattice against board; the one most markers cast (the lowest of
 *   equals) stands where at least min_markers cast it and no more cast another.  Else the lattice's peaks seed no more
 *   and the next seed is tried: 32 seeds scanned, 4 lattices grown.
 * corners: frames x n x 2 float32, n = (squares_x - 1) (squares_y - 1), integer-valued, NaN where unseen; marker_ids:
 * frames x squares_x squares_y int32, the id decoded in a square, -1 where none; status: 0 found, 1 counts < 5, 2 counts >
 * CAMD_CHESS_CAPACITY, 4 no seed cell, 8 no vote stood.  Outside the limits below CAMD_ERR_UNSUPPORTED.             */
#define CAMD_CHARUCO_MIN_SQUARES 3
#define CAMD_CHARUCO_MAX_SQUARES 16
#define CAMD_CHARUCO_MAX_RATIO_DEN 64
#define CAMD_CHARUCO_MAX_IDS 1024
int camd_charuco_detect(const int* peaks, const int* counts, const uint8_t* gray, int w, int h, size_t pitch, size_t stride,
                        int frames, int squares_x, int squares_y, int marker_num, int marker_den,
                        const unsigned long long* dictionary_words, int n_ids, int s, int first_id, int min_markers,
                        int max_bit_errors, float* corners, int* marker_ids, int* status, void* queue);
/* Every board of a SET in every frame, in one pass over one set of peaks (k_charuco_multi; restated by
 * tests/multiboard_ref.py).  A set: boards->n = B boards, 1 .. CAMD_CHARUCO_MAX_BOARDS, of the same squares, ratio and
 * dictionary, board b with markers first_id[b] .. first_id[b] + squares_x squares_y / 2 - 1; the ranges lie inside the
 * dictionary and apart from each other, else CAMD_ERR_UNSUPPORTED.  `boards` is read on the host at the call.
 *   Seeds in camd_charuco_detect's order; a peak labelled in any lattice grown so far, accepted or not, seeds no more (it
 *   still counts as scanned).  A seed cell qualifies by a marker of a board not yet found.  Growth as above, over the peaks
 *   no accepted lattice holds.  Every decoded marker of a board not yet found casts (board, turn, offset); the accept rule
 *   is the one above on the winning triple (of equals the lowest board, then turn, then offset).  The winner's board is
 *   found and its rows are written; else the lattice's peaks seed no more and the seed cell's board counts as tried.
 *   The loop ends when every board is found, the seeds run out, 32 B seeds are scanned or 4 B lattices are grown.
 *   With B = 1: camd_charuco_detect bit for bit.
 * corners: frames x B x n x 2 float32; marker_ids: frames x B x squares_x squares_y int32; status: frames x B int32 -- 0
 * found; 1, 2 (the frame's, as above) for every board; else 8 for a board that was tried, 4 for the rest.
 * RANGE: the CAMD_CHESS_CAPACITY candidates are per FRAME, not per board, and the markers' own X-junctions count towards
 * them: a frame in which all the boards together leave more has status 2 for every board.                           */
#define CAMD_CHARUCO_MAX_BOARDS 8
typedef struct camd_charuco_boards {
    int n;
    int first_id[CAMD_CHARUCO_MAX_BOARDS];
} camd_charuco_boards;
int camd_charuco_detect_multi(const int* peaks, const int* counts, const uint8_t* gray, int w, int h, size_t pitch, size_t stride,
                              int frames, int squares_x, int squares_y, int marker_num, int marker_den,
                              const unsigned long long* dictionary_words, int n_ids, int s, const camd_charuco_boards* boards,
                              int min_markers, int max_bit_errors, float* corners, int* marker_ids, int* status, void* queue);

/* ---- stand-alone ArUco markers by id (csrc/markers.hip) ----
 * Stands where the reference calls cv2.aruco.detectMarkers (boards.py:280, 551) with a contract of its OWN (INTEGRATION.md
 * section J; UNPINNED against cv2), integers from the image to the coarse corners, restated in
 * NumPy by tests/markers_ref.py.  Images: frames of w x h, w, h <= 16384, frames * h < 2^31.  Outside a limit named below:
 * CAMD_ERR_UNSUPPORTED, before the device is touched.
 * Stage 1.  S(p): the sum of gray over the (2 block_radius + 1)^2 window about p clipped to the image, A(p): the pixels of
 * that part.  mask (frames * h * w uint8, dense) is 1 iff (gray(p) + offset) * A(p) < S(p).  block_radius 1 .. 32, offset
 * -255 .. 255.  The inside of a black area wider than the window is NOT dark: a large marker leaves a hollow ring.       */
int camd_dark_mask(const uint8_t* gray, int w, int h, size_t pitch, size_t stride, int frames, int block_radius, int offset,
                   uint8_t* mask, void* queue);
/* Stage 2.  labels (frames * h * w int32, dense): the least y * w + x of a pixel's 4-connected component of mask != 0, -1
 * where mask == 0.  The result does not depend on the order in which threads meet.                                      */
int camd_label_components(const uint8_t* mask, int w, int h, int frames, int* labels, void* queue);
/* Stage 3.  A component is a candidate when both sides of its bounding box lie in [min_side, max_side] and the box does
 * not touch the image's outermost pixel frame.  candidates: frames x CAMD_MARKER_CAPACITY x 6 int32 (root, x0, y0, x1, y1,
 * pixels), a frame's candidates in the pixel order of their roots (those beyond the capacity are dropped, the entries
 * beyond the count are not written); counts: the candidates of each frame in full; status: 2 where counts >
 * CAMD_MARKER_CAPACITY, else 0.  4 <= min_side <= max_side <= 1024.  workspace: camd_marker_candidates_workspace_bytes
 * device bytes (16 per pixel and a little), 16-aligned.                                                                 */
#define CAMD_MARKER_CAPACITY 1024 /* candidates kept per frame */
size_t camd_marker_candidates_workspace_bytes(int w, int h, int frames);
int camd_marker_candidates(const int* labels, int w, int h, int frames, int min_side, int max_side, void* workspace,
                           int* candidates, int* counts, int* status, void* queue);
/* Stages 4 to 6, one wavefront per candidate.  Over the pixels of the candidate's box that carry its label, ties to the
 * least pixel index throughout: a maximises |2 p - (box min + box max)|^2, b maximises |p - a|^2, c and d have the greatest
 * and the least cross(b - a, p - a).  Rejected: cross 0 at c or d, a, d, b, c not strictly convex, or a side shorter than
 * min_side.  quads: frames x CAMD_MARKER_CAPACITY x 4 x 2 int32, the corners a, d, b, c -- clockwise in image coordinates
 * (x right, y down) --, -1 where rejected or beyond the count.  Decode as camd_charuco_detect's with the marker filling the
 * quadrilateral (ratio 1 / 1): corner 0 is the cell's origin, 1 one step along i, 3 along j.  id_turn: frames x
 * CAMD_MARKER_CAPACITY int32, id << 2 | turn or -1.  Per (frame, id) the candidate with the least (errors, index) stands:
 * best (frames x n_ids uint32 scratch) = errors << 10 | index.  seen: frames x n_ids uint8; corners: frames x n_ids x 4 x 2
 * float32, corner j = quad corner (j + turn) % 4 -- the marker's own top-left, top-right, bottom-right, bottom-left --, NaN
 * where unseen.  They are centres of dark pixels: about half a pixel INSIDE the printed outline.  A frame whose count is
 * above the capacity has no markers.  s 4 .. 8, n_ids 1 .. CAMD_CHARUCO_MAX_IDS, max_bit_errors 0 .. s*s, frames <= 65535. */
int camd_marker_decode(const uint8_t* gray, int w, int h, size_t pitch, size_t stride, int frames, const int* labels,
                       const int* candidates, const int* counts, int min_side, const unsigned long long* dictionary_words,
                       int n_ids, int s, int max_bit_errors, int* quads, int* id_turn, unsigned* best, uint8_t* seen,
                       float* corners, void* queue);

/* ---- the variance of the Laplacian, a picture's sharpness (csrc/sharpness.hip) ----
 * Stands where the reference calls cv2.Laplacian(gray, cv2.CV_64F).var() (reconstruction_with_board.py:9-12); UNPINNED
 * against cv2.  L(x, y) = g(x-1, y) + g(x+1, y) + g(x, y-1) + g(x, y+1) - 4 g(x, y), a
 * neighbour outside the image mirrored about the border pixel (reflect-101: -1 -> 1, w -> w - 2).  sums: frames x 2 int64,
 * S1 = sum L and S2 = sum L^2 over a frame -- exact integers, so the order of the sum does not show; the variance is
 * (N S2 - S1^2) / N^2 with N = w h, formed by the caller (N S2 leaves 64 bits at 4K).  gray: frames images of w x h uint8,
 * rows `pitch` and images `stride` bytes apart.  w, h >= 2 (the mirror needs a second pixel), w h <= 2^31.            */
int camd_laplacian_sums(const uint8_t* gray, int w, int h, size_t pitch, size_t stride, int frames, long long* sums, void* queue);

/* ---- sparse samples filled by their plane inside their convex hull, batched over frames (csrc/hull.hip) ----
 * Stands where the reference's interpolate_uvzs(..., constrained_type="convex_hull") calls cv2.convexHull and
 * cv2.drawContours (utils.py:364-367) with a mask contract of its OWN (UNPINNED against cv2,
 * DESIGN.md section 2, U33).  A row (u, v, z) is VALID when u, v are finite, z is finite and not 0 and
 * |rint(u)|, |rint(v)| <= 2^20; its pixel is (int32(rint(u)), int32(rint(v))), half to even.  Pixel (x, y) is INSIDE iff the
 * integer point lies in the closed convex hull of the valid rows' pixels; pixels outside the image take part in the hull.
 * Only integers decide that: int64 cross products, int64 floor / ceil divisions.                                      */
#define CAMD_HULL_MAX_POINTS 4096 /* rows of one frame, and the largest vertex_capacity */
/* Stage A, one wavefront per frame, no workgroup barrier; a frame's record depends on its own rows only.
 * uv: `rows` float64 rows of uv_stride >= 2 doubles; z: `rows` values of z_type CAMD_VALUE_F64 / _F32, or NULL (every z
 * counts as 1: the mask alone).  start == NULL: frame f owns rows f * (rows / frames) ...; otherwise frames + 1 int64 ON
 * THE DEVICE, rising, as camd_pnp_points.start.  A range that leaves the rows or is longer than vertex_capacity is read
 * nowhere and counts as a frame without rows.  keep_last_per_pixel: rows whose pixel is outside w x h are dropped, and of
 * several valid rows on one pixel only the highest row index takes part, in the hull and in the fit (what a scatter
 * through camd_uvzs_to_arr2d leaves).  w, h are used for that only.
 *   hull   gift wrapping from the lowest (x, y); the next vertex is the candidate r for which cross(q - p, r - p) < 0
 *          against every other q, the farther one of collinear candidates: a total order, so the vertex set is unique.
 *          vertices: frames x vertex_capacity x 2 int32 (x, y), the first hull_counts[f] of a frame are written.
 *   plane  sums of uu, uv, u, vv, v, 1, uz, vz, z over the rows that take part, unrounded float64: row i belongs to lane
 *          i % 64, a lane adds its rows in rising i, the lanes meet in a butterfly (xor 1, 2, ... 32); then with
 *          mu = su / n, mv, mz alike: cuu = suu - su mu, cvv = svv - sv mv, cuv = suv - su mv, cuz = suz - su mz,
 *          cvz = svz - sv mz, det = cuu cvv - cuv cuv, a = (cuz cvv - cvz cuv) / det, b = (cvz cuu - cuz cuv) / det,
 *          c = mz - a mu - b mv.  abc: frames x 3 float64.
 *   status 1: no row takes part (hull_counts 0, abc NaN); 2: fewer than three rows or !(det > 1e-9 cuu cvv), i.e.
 *          1 - corr(u, v)^2 <= 1e-9: abc NaN; 4: a row with finite u, v and a valid z beyond 2^20 was left out.        */
int camd_hull_fit(const double* uv, int uv_stride, const void* z, int z_type, size_t rows, const long long* start, int frames,
                  int w, int h, int keep_last_per_pixel, int vertex_capacity, int* vertices, int* hull_counts, double* abc,
                  int* status, void* queue);
/* Stage B.  out: frames x h x w float32, every pixel written once: inside, float32(x * a + y * b + c) evaluated as
 * camd_plane_eval does, with a, b, c read from abc ON THE DEVICE (a caller may have overwritten them); outside, 0.
 * reciprocal != 0: 1.0f / that instead (IEEE division: +inf outside).  Row y is inside from
 * max(0, min ceil(crossing)) to min(w - 1, max floor(crossing)) over the hull's edges that reach the row.
 * zero_frames: NULL, or `frames` bytes ON THE DEVICE: a frame whose byte is not 0 is written as zeros throughout,
 * whatever `reciprocal` says (the frames of a recording that show no board).  queue: the HIP stream of the launch.    */
int camd_hull_fill(const int* vertices, const int* hull_counts, const double* abc, int vertex_capacity, int frames, int w, int h,
                   int reciprocal, const uint8_t* zero_frames, float* out, void* queue);
/* The mask alone from the same spans: frames x h x w uint8, 1 inside, 0 outside.                                       */
int camd_hull_mask(const int* vertices, const int* hull_counts, int vertex_capacity, int frames, int w, int h, uint8_t* out,
                   void* queue);

/* ---- a LiDAR cloud as a dense depth image: projection, the hull of any number of samples, the nearest sample inside it
 *      (csrc/lidar.hip) ----
 * The device side of xyzs_to_dense_depth in the reference's example/calibrate_lidar2cam_by_PnP/calibrate_lidar2cam_pnp.py:13-42.
 *
 * a. The cloud's rows inside the image.  xyz: n points (n < 2^31) of xyz_type CAMD_VALUE_F64 / _F32, xyz_stride >= 3 elements
 * apart (a column view of a wider array is read in place).  T: NULL or 16 host doubles (4 x 4, row-major); K: 9 host doubles,
 * all of them used; lens distortion takes no part.  Per point, in float64, every product and sum rounded on its own:
 *   X' = ((T[r][0] x + T[r][1] y) + T[r][2] z) + T[r][3]      (r = 0, 1, 2; without T: X' = X)
 *   p[r] = (K[r][0] X' + K[r][1] Y') + K[r][2] Z',   u = p0 / p2,   v = p1 / p2
 * and the point is KEPT iff p2 > 0, u >= 0, v >= 0, u < w and v < h (a NaN or an infinity fails a comparison).  stages is
 * 1 (count), 2 (emit) or 3 (both):
 *   count  counters[0] = the kept points, counters[1] = the points with p2 > 0 (uint64, on the device), and the workspace
 *          (camd_cloud_workspace_bytes(n) bytes, 8-aligned) is left ready for an emit of the same arguments;
 *   emit   rows[k] = (u * rate, v * rate, Z') float64 of the k-th kept point, in input order (the compaction of compact.hpp
 *          over rows of a fixed number of points); slots at or beyond `capacity` are not written.
 * Between the two a caller may read counters[1] back and choose `rate` from it.                                          */
size_t camd_cloud_workspace_bytes(size_t n);
int camd_cloud_to_uvzs(const void* xyz, int xyz_type, size_t n, int xyz_stride, const double* T, const double K[9], int w, int h,
                       double rate, int stages, double* rows, size_t capacity, unsigned long long* counters, void* workspace,
                       void* queue);
/* b. The convex hull of ANY number of samples, under camd_hull_fit's mask contract.  A sample (u, v) has the pixel
 * (int32(rint(u)), int32(rint(v))), half to even, when u, v are finite and |rint| <= 2^20; beyond that it is left out and
 * status bit 4 is set.  A point set and its per-row extremes have the same hull:
 *   camd_hull_row_range  range[0], range[1] = the lowest and the highest pixel row of the samples (INT_MAX, INT_MIN when
 *                        none has a pixel), range[2] = the status bits; 3 int32 on the device.
 *   camd_hull_extremes   table: rows x 2 int32, (xmin, xmax) of the samples on pixel row y0 + r, (INT_MAX, INT_MIN) where
 *                        there is none -- integer atomicMin / atomicMax, the same bits on every run; samples on other rows take
 *                        no part.  candidates: the non-empty rows' (xmin, y), (xmax, y) as float64 rows of 2, in rising y,
 *                        min before max (room for 2 * rows of them); *count = their number; *status as above.
 * The candidates go to camd_hull_fit with z = NULL: at most CAMD_HULL_MAX_POINTS of them as one frame, more as consecutive
 * chunks of that many (the frames of one call with `start`), whose surviving vertices, concatenated in frame order, are the
 * candidates of the next round.  uv: n float64 rows, uv_stride >= 2 doubles apart; 1 <= rows <= 2^21 + 1, |y0| <= 2^20.  */
int camd_hull_row_range(const double* uv, int uv_stride, size_t n, int* range, void* queue);
int camd_hull_extremes(const double* uv, int uv_stride, size_t n, int y0, int rows, int* table, double* candidates,
                       unsigned long long* count, int* status, void* queue);
/* c. camd_nearest_fill restricted to ONE hull record (vertices, hull_counts[0], vertex_capacity as camd_hull_fit leaves them):
 * out[y][x] (h x w float32) = what camd_nearest_fill gives for the same bins where the pixel lies in the row's closed span
 * (camd_hull_fill's), 0 elsewhere -- without a search there.  z: the samples' values, z_stride elements apart.            */
int camd_nearest_fill_in_hull(const double* sorted_uv, const uint32_t* sorted_idx, const uint32_t* start, const void* z, int z_type,
                              size_t z_stride, int w, int h, double distance, const int* vertices, const int* hull_counts,
                              int vertex_capacity, float* out, void* queue);

/* ---- sparse samples filled by their thin-plate spline, batched over frames (csrc/spline.hip) ----
 * The device side of the reference's interpolate_uvzs(inter_type="rbf"): scipy.interpolate.Rbf(u, v, z,
 * function="thin_plate", smooth=s) evaluated at every pixel (utils.py:373-388).  float64 throughout, every product and sum
 * rounded on its own, in the order given here; tests/spline_ref.py restates each stage.
 *   phi(dx, dy) = r == 0 ? 0 : (r * r) * log(r)   with r = sqrt(dx * dx + dy * dy)
 * The frames' rows follow one another in one array; start: frames + 1 int64 ON THE DEVICE, rising, frame f owns rows
 * start[f] .. start[f + 1].  A range that leaves the rows or is longer than `capacity` is read nowhere and counts as a frame
 * without rows.  capacity (1 .. CAMD_SPLINE_MAX_POINTS) is the leading dimension of every frame's matrix and weights;
 * 1 <= frames <= 65535.  A frame's numbers depend on its own rows only.                                                  */
#define CAMD_SPLINE_MAX_POINTS 1024 /* rows of one frame: what one workgroup factors */
#define CAMD_SPLINE_NO_SAMPLE 1     /* status: the frame has no row (nothing else is written for it) */
#define CAMD_SPLINE_SINGULAR 2      /* status: a zero or non-finite pivot; the frame's weights are NaN */
#define CAMD_SPLINE_NON_FINITE 4    /* status: a non-finite z or matrix entry; the frame's weights are NaN */
/* 1. A: frames x capacity x capacity; of frame f with n rows the leading n x n are written:
 *   A[i][j] = A[j][i] = phi(u_i - u_j, v_i - v_j) for j < i (computed once, stored twice),   A[i][i] = 0 - smooth.
 * uvz: rows of uvz_stride >= 2 doubles, u and v the first two.                                                           */
int camd_spline_assemble(const double* uvz, int uvz_stride, size_t rows, const long long* start, int frames, int capacity,
                         double smooth, double* A, void* queue);
/* 2. A w = z of every frame, one workgroup per frame, A factored IN PLACE (it is destroyed).  z: the frame's right-hand
 * sides, z_stride doubles apart (uvz + 2 with uvz_stride).  Gaussian elimination with partial pivoting: at step k the pivot
 * row is the i >= k with the largest |A[i][k]|, of equal ones the lowest; rows k and p are exchanged; for i > k:
 *   m = A[i][k] / A[k][k],   A[i][j] = A[i][j] - m * A[k][j] (j > k),   b[i] = b[i] - m * b[k]
 * then, k = n - 1 ... 0:   w[k] = b[k] / A[k][k],   b[i] = b[i] - A[i][k] * w[k] (i < k).
 * weights: frames x capacity, the first n of a frame are written; status: frames int32, 0 or one CAMD_SPLINE_* value.    */
int camd_spline_solve(const double* z, int z_stride, size_t rows, const long long* start, int frames, int capacity, double* A,
                      double* weights, int* status, void* queue);
/* 3. out: frames x out_h x out_w float64, every pixel written once:
 *   out[y][x] = sum over i = 0 .. n - 1, in that order, of  w_i * phi(x * grid_step - u_i, y * grid_step - v_i)   (s = s + t)
 * mask: NULL, or frames x out_h x out_w uint8: where it is 0 the pixel is written 0.0 and nothing is evaluated.          */
int camd_spline_eval(const double* uvz, int uvz_stride, size_t rows, const long long* start, int frames, int capacity,
                     const double* weights, const uint8_t* mask, int out_w, int out_h, int grid_step, double* out, void* queue);
/* out (frames x out_h x out_w) = cv2.resize(INTER_NEAREST) of (src * out_w) / w, src frames x h x w float64: pixel (X, Y)
 * reads (min(floor(X * ifx), w - 1), min(floor(Y * ify), h - 1)) with ifx = 1 / (out_w / w) -- what the reference's
 * FeatureMatchingAsStereoMatching does to its coarse disparity (stereo_matching.py:139-140).                             */
int camd_spline_upsize(const double* src, int w, int h, int frames, double* out, int out_w, int out_h, void* queue);

/* ---- the essential matrix of matched pixels by RANSAC over 8-point samples (csrc/essential.hip) ----
 * The device side of epipolar_geometry.find_essential_matrix.  A contract of this library's OWN: cv2.findEssentialMat is
 * not restated (UNPINNED); tests/essential_ref.py restates every stage in NumPy, bit for bit.
 * Shared by the three entries: uv1, uv2 are [n][stride] of uv_type (CAMD_VALUE_F64 / _F32; stride >= 2 elements, u and v
 * the first two of a row), read in place, 8 <= n < 2^31, FINITE (the caller checks; a sample that meets a non-finite
 * value is marked).  K1inv, K2inv: inv(K) as 9 host doubles.  The rays of match i are, each product and sum rounded,
 *   a[r] = (K1inv[3r] u1 + K1inv[3r + 1] v1) + K1inv[3r + 2],   b[r] likewise from K2inv and (u2, v2)
 * and its row of the 8-point system is row[3 j + k] = a[k] * b[j] (row . e = b^T E a with E = e as 3 x 3, row-major).
 * A match is an INLIER of e below threshold2 (the squared threshold, on the rays) when, with
 *   p[r] = (e[3r] a0 + e[3r + 1] a1) + e[3r + 2] a2,   q[c] = (e[c] b0 + e[3 + c] b1) + e[6 + c] b2   (c = 0, 1),
 *   num = (b0 p0 + b1 p1) + b2 p2,   den = ((p0 p0 + p1 p1) + q0 q0) + q1 q1:   num * num < threshold2 * den
 * -- its squared Sampson error num^2 / den compared without the division; a zero or non-finite e has no inliers.
 *
 * Stage 1.  Hypothesis h < hypotheses (1 .. 2^20) draws 8 DISTINCT rows: key = the output of splitmix64 from the state
 * `seed`; the hypothesis' stream starts at the state splitmix64 gives as OUTPUT from the state key ^ h; draw k is
 * floor(z n / 2^64) of the stream's next output z, drawn again while it repeats one of the draws before it (after 1024
 * repeats of one draw: the smallest index not drawn yet).  Nothing is shared between hypotheses: hypothesis h is the same
 * whatever `hypotheses` is.  M = sum over the 8 rows, in the order drawn, of row^T row (packed lower triangle, 45 sums);
 * e = the null vector by six rounds of inverse iteration on M + 1e-13 tr(M) I (the routine the PnP start uses), of unit
 * norm, its entry of the largest magnitude (the first of equals) positive.  A sample is MARKED, its e all zero, when e is
 * not finite, the Cholesky factorisation fails, or more than one pivot of it lies below 1e-10 tr(M): the matches leave
 * more than one null direction (coincident or otherwise degenerate ones) and determine no matrix.
 * samples: [hypotheses][8] int32, Es: [hypotheses][9] float64, both on the device.  One lane per hypothesis.           */
int camd_essential_hypotheses(const void* uv1, const void* uv2, int uv_type, size_t n, int uv1_stride, int uv2_stride,
                              const double K1inv[9], const double K2inv[9], unsigned long long seed, int hypotheses, int* samples,
                              double* Es, void* queue);
/* Stage 2.  counts[h] (device int32, cleared here) = the inliers of Es[h] among all n matches: a lane owns four matches
 * and walks the hypotheses, the counts are added by ballot, popcount and integer atomics (exact in any order).
 * winner (device, 11 doubles): [0 .. 8] the e of the largest count, ties to the LOWEST index, [9] that index, [10] its count. */
int camd_essential_score(const void* uv1, const void* uv2, int uv_type, size_t n, int uv1_stride, int uv2_stride,
                         const double K1inv[9], const double K2inv[9], const double* Es, int hypotheses, double threshold2,
                         int* counts, double* winner, void* queue);
/* Stage 3, for ONE matrix E (9 doubles ON THE DEVICE): mask[i] (n bytes) = 1 where match i is an inlier, and
 * sums (device, 46 doubles): sums[p (p + 1) / 2 + q] = sum over the inliers of row[p] * row[q] (q <= p < 9), sums[45] =
 * their number.  REDUCTION SHAPE: that of camd_epipolar_sums -- G = camd_essential_moments_blocks(n) = clamp(ceil(n / 256),
 * 1, 1024) workgroups, thread t of workgroup g adds rows 256 g + t, + 256 G, ... in that order, d = 18 tree levels, no
 * float atomics.  partials_ws: G * 46 doubles.                                                                       */
int camd_essential_moments_blocks(size_t n);
int camd_essential_moments(const void* uv1, const void* uv2, int uv_type, size_t n, int uv1_stride, int uv2_stride,
                           const double K1inv[9], const double K2inv[9], const double* E, double threshold2, uint8_t* mask,
                           double* partials_ws, double* sums, void* queue);
/* The same three stages for MANY pairs of views, one launch a stage (the device side of find_essential_matrices).  uv_a, uv_b:
 * [m][stride] as above, 1 <= m < 2^31, the pairs' rows one after the other.  pair_table (device, [pairs][21] doubles): pair p's
 * [0], [1] = its first row and its number of rows as int64 BIT PATTERNS, [2 .. 10] = inv(K) of the view uv_a shows, [11 .. 19] =
 * of the view uv_b shows, [20] = its threshold2.  A record that leaves the m rows is skipped by every kernel.  Pair p's outputs
 * are, bit for bit, what the single entries give for its rows alone: sample indices are local to the pair, every pair runs the
 * streams of `seed`, and the kernels' bodies are the single entries' own.
 * Stage 1: samples [pairs][hypotheses][8], Es [pairs][hypotheses][9]; a pair of fewer than 8 rows gets samples -1 and Es 0.  */
int camd_essential_batch_hypotheses(const void* uv_a, const void* uv_b, int uv_type, size_t m, int uv_a_stride, int uv_b_stride,
                                    const double* pair_table, int pairs, unsigned long long seed, int hypotheses, int* samples,
                                    double* Es, void* queue);
/* Stage 2: counts [pairs][hypotheses] int32 (cleared here), winner [pairs][11].  block_table (device, [blocks][4] int32,
 * 16-aligned): workgroup b owns rows 1024 g .. 1024 g + 1023 of pair block_table[b] = (pair, g, -, -), so no workgroup reads two
 * pairs; pairs of fewer than 8 rows have no workgroup and keep count 0.  lds_sum != 0: the four waves' counts of a hypothesis are
 * added in LDS and ONE atomic per (workgroup, hypothesis) reaches memory; 0: one per wave.  The counts are the same either way. */
int camd_essential_batch_score(const void* uv_a, const void* uv_b, int uv_type, size_t m, int uv_a_stride, int uv_b_stride,
                               const double* pair_table, int pairs, const int* block_table, int blocks, const double* Es,
                               int hypotheses, int lds_sum, int* counts, double* winner, void* queue);
/* Stage 3 for one matrix per pair, E + pair * E_stride (device), of the pairs the tables name: block_table[b] = (pair, g, G, -)
 * makes workgroup b the g-th of the G = camd_essential_moments_blocks(rows of the pair) that sum the pair, its partials the b-th 46
 * of partials_ws ([blocks][46]); final_table[f] = (pair, the pair's first workgroup, G, -) sums them into sums[pair] ([pairs][46]).
 * mask: the ONE [m] array; rows and sums of pairs no table names are left as they are.                                    */
int camd_essential_batch_moments(const void* uv_a, const void* uv_b, int uv_type, size_t m, int uv_a_stride, int uv_b_stride,
                                 const double* pair_table, int pairs, const int* block_table, int blocks, const int* final_table,
                                 int finals, const double* E, int E_stride, uint8_t* mask, double* partials_ws, double* sums,
                                 void* queue);

/* ---- keypoints, binary descriptors and a brute-force Hamming matcher: matches from two pictures (csrc/features.hip) ----
 * A contract of this library's OWN, NOT cv2.ORB / cv2.BFMatcher (UNPINNED):
 * integers end to end, every tie defined, restated in NumPy by tests/features_ref.py.  gray: frames images of w x h uint8,
 * rows `pitch` and images `stride` bytes apart; w, h <= 16384, frames * h < 2^31, else CAMD_ERR_UNSUPPORTED.
 * Stage A, the score.  ring[0 .. 15] = g(x + dx, y + dy) at (dx, dy) = (0,-3) (1,-3) (2,-2) (3,-1) (3,0) (3,1) (2,2) (1,3)
 * (0,3) (-1,3) (-2,2) (-3,1) (-3,0) (-3,-1) (-2,-2) (-1,-3); d[i] = ring[i] - g(x, y);
 *   score = max over the 16 starts s of max(min d[s .. s + 8], -max d[s .. s + 8]) (indices mod 16), and 0 if that is below
 *   `threshold` (1 .. 255) or the pixel lies within CAMD_FEATURE_BORDER of an image edge.  score: frames * h * w uint8, dense. */
#define CAMD_FEATURE_BORDER 16
int camd_feature_score(const uint8_t* gray, int w, int h, size_t pitch, size_t stride, int frames, int threshold, uint8_t* score,
                       void* queue);
/* Stage A, the keypoints.  key(p) = score(p) << 32 | (0xFFFFFFFF - (y * w + x)) as u64; p is a PEAK when score(p) != 0 (and p
 * lies CAMD_FEATURE_BORDER inside the image, whatever the plane says) and key(p) is the largest of its 3 x 3 neighbourhood.
 * The blocks of cell x cell pixels (cell 4 .. 64) are aligned at pixel (0, 0); a block's keypoint is its peak of the largest
 * key.  capacity = ceil(h / cell) * ceil(w / cell).  xy: frames x capacity x 2 int32 (x, y), scores: frames x capacity int32,
 * a frame's keypoints in row-major order of their blocks (the entries beyond the count are not written); counts: frames
 * int32.  workspace: camd_feature_keypoints_workspace_bytes device bytes, 8-aligned.                                   */
size_t camd_feature_keypoints_workspace_bytes(int w, int h, int frames, int cell);
int camd_feature_keypoints(const uint8_t* score, int w, int h, int frames, int cell, void* workspace, int* xy, int* scores,
                           int* counts, void* queue);
/* Stage B, one wavefront per keypoint, no workgroup barrier; a keypoint's outputs depend on its own pixels only.  xy, counts
 * as above with `capacity` slots per frame (any capacity >= 1); slots at or beyond counts[f] are left as they are.
 *   bin   m10 = sum dx g(x + dx, y + dy), m01 = sum dy g(x + dx, y + dy) over dx^2 + dy^2 <= 13^2 (int32);  the bin is the
 *         k in 0 .. 31 that maximises m10 C[k] + m01 S[k] in int64, the lowest of equals, C[k] = rint(16384 cos(2 pi k / 32)),
 *         S[k] = C[(k + 24) % 32]
 *   box   B(p) = the sum of g over the 5 x 5 window about p
 *   bits  pattern: 32 x 256 x 4 int8 ON THE DEVICE, 4-aligned: (x1, y1, x2, y2) of test i at rotation k, each clamped to
 *         -14 .. 14 when read; bit i = B(x + x1, y + y1) < B(x + x2, y + y2) with the tests of rotation `bin`
 * descriptors: frames x capacity x 32 uint8, 8-aligned, bit r of byte b = test 8 b + r; bins: frames x capacity int32.
 * A point nearer than CAMD_FEATURE_BORDER to an edge reads nothing: its descriptor is zero and its bin -1.             */
int camd_feature_describe(const uint8_t* gray, int w, int h, size_t pitch, size_t stride, int frames, const int* xy, const int* counts,
                          int capacity, const int8_t* pattern, uint8_t* descriptors, int* bins, void* queue);
/* Stage C, the search, both ways in one launch.  Two sets of descriptors (they may be the same): desc frames x capacity x
 * 32 uint8, 16-aligned, counts frames int32 (clamped to 0 .. capacity).  pairs: npairs x 2 int32 ON THE DEVICE, (frame of
 * set 1, frame of set 2); a frame outside its set counts as empty.  For query row q of the first frame, over the train rows
 * t of the second in rising t: distance d = the differing bits; d < d_best: d_second = d_best, d_best = d, best = t; else
 * d < d_second: d_second = d -- so best has the smallest (d, t) and d_second is the smallest d among the other rows, 257
 * where there is none.  best12: npairs x capacity1 int32 (-1 beyond the count or without a train row), dist12: npairs x
 * capacity1 x 2 int32 (d_best, d_second; 257 likewise); best21, dist21: the same with the roles swapped, npairs x
 * capacity2.  1 .. 65535 pairs, npairs * capacity < 2^30.                                                              */
int camd_feature_search(const uint8_t* desc1, const int* counts1, int frames1, int capacity1, const uint8_t* desc2, const int* counts2,
                        int frames2, int capacity2, const int* pairs, int npairs, int* best12, int* dist12, int* best21, int* dist21,
                        void* queue);
/* Stage C, the filter.  Query q of pair p is KEPT when d_best <= max_distance (0 .. 256), d_best * ratio_den <= ratio_num *
 * d_second (1 <= num <= den <= 2^20) and, with cross_check != 0, best21[p][best12[p][q]] == q.  matches: npairs x capacity1 x 2
 * int32 (q, best), distances: npairs x capacity1 int32, a pair's kept queries in rising q by the shared ordered compaction
 * (the entries beyond the count are not written); match_counts: npairs int32.  workspace:
 * camd_feature_filter_workspace_bytes device bytes, 8-aligned.                                                         */
size_t camd_feature_filter_workspace_bytes(int npairs);
int camd_feature_filter(const int* counts1, int frames1, int capacity1, int capacity2, const int* pairs, int npairs, const int* best12,
                        const int* dist12, const int* best21, int max_distance, int ratio_num, int ratio_den, int cross_check,
                        void* workspace, int* matches, int* distances, int* match_counts, void* queue);

#ifdef __cplusplus
}
#endif
#endif
