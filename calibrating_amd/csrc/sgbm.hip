// sgbm.hip -- Semi-Global Block Matching for gfx950 (MI355X), bit-exact with cv2.StereoSGBM
// (modes MODE_SGBM, MODE_HH, MODE_HH4 and MODE_SGBM_3WAY) at equal parameters.
//
// Replaces the cv2.StereoSGBM_create(...).compute(left, right) call of the reference
// (/root/reference/calibrating/stereo_matching.py:48-58,63).  Not a port of OpenCV's row-incremental
// CPU loop: the algorithm is re-stated in a data-parallel form (SURVEY.md Appendix A / DESIGN.md):
//
//   k_cost         (sgbm_cost.hpp) calcPixelCostBT + blockSize x blockSize box sum + P2 -> C[y][x][d] in ONE pass:
//                  lanes = columns, the workgroup walks rows; horizontal sum by wave-wide DPP shifts, vertical sum as a
//                  register ring.  The default for blockSize <= 11.
//   k_hsum, k_vsum (sgbm_split.hpp) the two-pass form of the same (round 1): BT + horizontal box sum into an intermediate volume,
//                  then the vertical box sum + P2.  Kept for blockSize 13 / 15 and as an A/B reference (CAMD_COST_SPLIT).
//   k_band         (sgbm_band.hpp) fused aggregation: four directions per pass + WTA in the last
//   k_scan         (sgbm_scan.hpp) one aggregation direction as independent line scans from a zero border state;
//                  a line is owned by a 2..16-lane group (2*NR disparities per lane, packed u16x2),
//                  neighbours d-1 / d+1 by DPP row shifts, min over d by a DPP butterfly
//   k_wta          winner-take-all, uniqueness, sub-pixel parabola, right-view map via LDS
//                  atomicMin on (cost << 16 | 0xFFFF - d), left-right check; one workgroup per row
//   k_median3 / speckle (post.hip)
//
// All volumes are [pair][y][x][Dp] int16 with Dp = LANES*2*NR >= D (NR packed u16x2 registers per lane); entries
// d >= D carry MAX_COST.
#include "common.hpp"

#include <cstdlib>
#include <cstring>
#include <new>

namespace camd {

static constexpr uint32_t SENT_PK = 0x7fff7fffu;  // MAX_COST in both halves
static constexpr int MAX_COST = 32767;
static constexpr int CAMD_MULTI_MAX_BATCH = 8;  // concurrent-direction path: npaths volumes for up to 8 pairs per call

struct Geom {
    int W, H, cn;          // image
    int minD, D, Dp;       // disparity range, padded
    int minX1, W1;         // cost coordinates: x_img = x + minX1
    int SW2;               // box radius
    int P1, P2, uniq, d12; // normalised parameters
    int ftzero;
    int lanes, nr;         // line-group shape: a lane holds nr packed registers = 2*nr disparities, Dp = lanes*2*nr
    int mode, npaths;
    uint32_t uniq_magic;   // floor(2^32 / (100 - uniq)) + 1, or 0 when 100 - uniq == 1 (band WTA)
    int speckleWindowSize, speckleRange;
};

}  // namespace camd
#include "sgbm_split.hpp"
#include "sgbm_cost.hpp"
#include "sgbm_scan.hpp"
#include "sgbm_band.hpp"
#include "sgbm_exact.hpp"
namespace camd {

// defined in post.hip
int launch_median3(const int16_t* src, size_t src_pitch_e, size_t src_stride_e, int16_t* dst,
                   size_t dst_pitch_e, size_t dst_stride_e, int w, int h, int batch, hipStream_t st);
int launch_speckle(int16_t* img, size_t pitch_e, size_t stride_e, int w, int h, int new_val, int max_size,
                   int max_diff, void* ws, size_t ws_bytes, int batch, hipStream_t st, bool* clean);
size_t speckle_ws_bytes(int w, int h, int batch);

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
enum Stage { ST_COST = 0, ST_HSUM, ST_VSUM, ST_SCAN, ST_SCAN2, ST_WTA, ST_POST, ST_SPECKLE, ST_COUNT };
// "cost" = the fused cost kernel (then hsum / vsum are empty), "hsum" + "vsum" = the split pair (then cost is empty);
// "scan" = the aggregation launches; on the band path the last pass is timed separately as "scan_last"
static const char* kStageNames[ST_COUNT] = {"cost", "hsum", "vsum", "scan", "scan_last", "wta", "median", "speckle"};

}  // namespace camd

struct camd_sgbm {
    camd::Geom g;         // the image
    camd::Geom ga;        // what the aggregation kernels see: g, or (MODE_SGBM_3WAY) one stripe of at most ga.H rows
    camd::CostRanges cr;  // row ranges of the cost volume: the image, or the 3WAY stripes (each a "virtual pair")
    int stripe_sz;        // 3WAY: rows a stripe owns
    int16_t* rawv;        // 3WAY: raw disparity per virtual pair [max_batch * cr.n][ga.H][W]
    uint32_t* cost_ovf;   // per volume: the wrapping cost kernel saw a value too close to 32767 (two-stage saturating build)
    uint32_t* cost_neg;   // per volume: C holds a value below P2 -> outside the packed-u16 regime (sgbm_exact.hpp)
    bool may_overflow;    // the parameters allow an int16 overflow of the box sums at all
    int exact_cap;        // 1: flagged volumes take the exact path (Lx allocated, CAMD_OPT_EXACT on); 0: they are refused
    int32_t* Lx;          // exact path: npaths per-direction volumes of int L values for ONE flagged volume
    int way3_simd_lanes;  // 3WAY winner-take-all tie rule: 8 = cv2's SSE / NEON builds (default), 1 = scalar build
    camd_sgbm_params params;
    int max_batch;
    size_t vol_elems;     // per pair, int16 elements of one volume
    size_t raw_stride, rawv_stride;  // int16 elements between the raw disparity images of consecutive pairs / 3WAY stripes
    size_t speckle_bytes; // size of speckle_ws
    uint16_t *C, *S;      // S doubles as the hsum buffer before aggregation
    int16_t* raw;         // [max_batch][H][W] disparity before median
    void* speckle_ws;
    bool speckle_clean;   // every parent entry of speckle_ws is -1 (post.hip keeps it so from call to call)
    hipStream_t speckle_stream;  // ... by the kernels of the last call, which ran on this stream
    // band-wavefront path (sgbm_band.hpp)
    bool band_ok;         // geometry supported by k_band instantiations
    int path;             // 0 = band passes (default when band_ok), 1 = one k_scan per direction
    int keep_S;           // band path: also store S in the final pass (stage-wise parity hook)
    int cost_path;        // CAMD_COST_*
    int saturate;         // U7: 1 = C saturates like OpenCV's CV_SIMD build (default), 0 = wraps like the scalar build
    int phases;           // CAMD_OPT_PHASES (experimental): bit 0 = build the cost volume, bit 1 = first aggregation pass,
                          // bit 2 = last pass + winner-take-all + post filters (default 7 = everything)
    int nbands, nchunks;
    size_t erec_stride;
    unsigned long long* E;
    uint32_t *flags, *ticket, *err, *keys;
    uint32_t* xbar;       // grid-barrier counter of the exact path's persistent kernel (sgbm_exact.hpp)
    int num_cus;          // compute units of the device the handle lives on
    int persist_cost, persist_row;  // CAMD_OPT_RESIDENT (experimental): workgroups per CU of k_cost_persist / k_band_row_persist, 0 = off
    uint32_t* err_host;   // pinned mirror of *err, refreshed by an async copy after every band-path compute
    int16_t* d1;
    uint32_t epoch;
    uint16_t* Smulti;     // concurrent-direction path: npaths volumes for smulti_cap pairs (allocated in create / set_option)
    int smulti_cap;
    int last_batch;
    bool profiling;
    hipEvent_t ev[camd::ST_COUNT + 1];
    bool ev_ok;
};

namespace camd {

static int normalise(const camd_sgbm_params* p, int width, int height, int cn, Geom* g)
{
    if (!p) { set_error("params is NULL"); return CAMD_ERR_BAD_ARG; }
    if (width <= 0 || height <= 0 || (cn != 1 && cn != 3)) {
        set_error("need width, height > 0 and 1 or 3 channels (got %d x %d x %d)", width, height, cn);
        return CAMD_ERR_BAD_ARG;
    }
    if (p->numDisparities <= 0) { set_error("numDisparities must be > 0"); return CAMD_ERR_BAD_ARG; }
    if (p->mode < CAMD_MODE_SGBM || p->mode > CAMD_MODE_HH4) {
        set_error("mode %d unknown (MODE_SGBM=0, MODE_HH=1, MODE_SGBM_3WAY=2, MODE_HH4=3)", p->mode);
        return CAMD_ERR_BAD_ARG;
    }
    memset(g, 0, sizeof(*g));
    g->W = width; g->H = height; g->cn = cn;
    g->minD = p->minDisparity; g->D = p->numDisparities;
    int maxD = g->minD + g->D;
    g->minX1 = maxD > 0 ? maxD : 0;
    int maxX1 = width + (g->minD < 0 ? g->minD : 0);
    g->W1 = maxX1 - g->minX1;
    g->uniq = p->uniquenessRatio >= 0 ? p->uniquenessRatio : 10;
    g->uniq_magic = (g->uniq <= 98) ? (uint32_t)((1ull << 32) / (unsigned)(100 - g->uniq) + 1) : 0u;
    g->d12 = p->disp12MaxDiff > 0 ? p->disp12MaxDiff : 1;
    g->P1 = p->P1 > 0 ? p->P1 : 2;
    int P2 = p->P2 > 0 ? p->P2 : 5;
    g->P2 = P2 > g->P1 + 1 ? P2 : g->P1 + 1;
    int bs = p->blockSize > 0 ? p->blockSize : 5;
    g->SW2 = bs / 2;
    if (p->mode == CAMD_MODE_SGBM_3WAY && p->blockSize <= 0) g->SW2 = 1;  // cv2's 3-way loop: SADWindowSize > 0 ? /2 : 1
    g->ftzero = (p->preFilterCap > 15 ? p->preFilterCap : 15) | 1;
    g->mode = p->mode;
    g->npaths = p->mode == CAMD_MODE_HH ? 8 : (p->mode == CAMD_MODE_HH4 ? 4 : (p->mode == CAMD_MODE_SGBM_3WAY ? 3 : 5));
    g->speckleWindowSize = p->speckleWindowSize;
    g->speckleRange = p->speckleRange;
    if (2 * g->SW2 + 1 > HSUM_RING) {
        set_error("blockSize %d > %d not implemented", bs, HSUM_RING - 1);
        return CAMD_ERR_UNSUPPORTED;
    }
    // (P2: cv2's rule of thumb 32 * cn * blockSize^2 is 21600 at block 15 RGB; the fuzz covers the range up to the
    // limit -- in the last few per cent below 32767 the exact int path meets narrowings it does not restate)
    if (g->P2 > CAMD_MAX_P2 || g->ftzero > CAMD_MAX_FTZERO) {
        set_error("P2 = %d / preFilterCap = %d outside the int16 regime the kernels implement", g->P2,
                  p->preFilterCap);
        return CAMD_ERR_UNSUPPORTED;
    }
    if (g->W1 > 0 && g->W1 <= g->SW2) {
        // cv2's first box sum reads pixel-cost columns 0..SW2 without clamping to width1-1: with fewer
        // columns than that it reads memory it never wrote, so there is no reference answer to match
        set_error("only %d matchable columns for blockSize %d: cv2.StereoSGBM's result is undefined there "
                  "(needs width - numDisparities > blockSize / 2)", g->W1, bs);
        return CAMD_ERR_UNSUPPORTED;
    }
    if (g->D > 512) { set_error("numDisparities %d > 512 not implemented", g->D); return CAMD_ERR_UNSUPPORTED; }
    // Layout of a pixel's disparity vector: `lanes` lanes x `nr` packed registers (2 disparities each).  With 16 lanes a
    // register more per lane is 32 disparities, so numDisparities in (64, 256] is padded to the next multiple of 32 --
    // the reference's 218 to 224, not to 256 (round 5; before, nr was a multiple of 4: 128 / 256 / 384 / 512) -- and every
    // kernel moves and computes that much less.  MODE_SGBM_3WAY keeps whole groups of 8 disparities per lane (its
    // 8-slot tie rule is evaluated per lane), as does everything beyond 256.
    if (g->D > 64) {
        g->lanes = 16;
        g->nr = (g->D <= 256 && p->mode != CAMD_MODE_SGBM_3WAY) ? (g->D + 31) / 32 : 4 * ((g->D + 127) / 128);
    }
    else if (g->D > 32) { g->lanes = 8; g->nr = 4; }
    else if (g->D > 16) { g->lanes = 4; g->nr = 4; }
    else { g->lanes = 2; g->nr = 4; }
    g->Dp = g->lanes * 2 * g->nr;
    return CAMD_OK;
}

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Row ranges of the cost volume and the geometry the aggregation kernels see.  MODE_SGBM_3WAY: cv2's four fixed row
// stripes (oracle/sgbm_ref.c compute_disparity_3way), each with its warm-up overlap, each a "virtual pair".
static int cost_ranges(const Geom& g, int block_size_raw, CostRanges* cr, int* stripe_sz, int* max_rows)
{
    if (g.mode != CAMD_MODE_SGBM_3WAY) {
        cr->n = 1;
        cr->start[0] = 0; cr->rows[0] = g.H;
        for (int i = 1; i < 4; i++) { cr->start[i] = 0; cr->rows[i] = 0; }
        *stripe_sz = g.H;
        *max_rows = g.H;
        return CAMD_OK;
    }
    const int ns = 4, sz = div_up(g.H, ns), ov = (block_size_raw / 2 + 1) + div_up(sz, 10);
    cr->n = ns;
    *stripe_sz = sz;
    *max_rows = 0;
    for (int s = 0; s < ns; s++) {
        int a = s * sz - ov, b = (s + 1) * sz < g.H ? (s + 1) * sz : g.H;
        if (s > 0 && s * sz < g.H && a < 0) {
            set_error("image height %d too small for MODE_SGBM_3WAY with blockSize %d (a stripe of %d rows needs a warm-up "
                      "of %d rows above it)", g.H, block_size_raw, sz, ov);
            return CAMD_ERR_UNSUPPORTED;
        }
        a = a < 0 ? 0 : (a > g.H ? g.H : a);
        cr->start[s] = a;
        cr->rows[s] = b > a ? b - a : 0;
        if (cr->rows[s] > *max_rows) *max_rows = cr->rows[s];
    }
    return CAMD_OK;
}

// U7: an int16 overflow of the box sums is possible at all only beyond this bound
static bool params_may_overflow(const Geom& g)
{
    const long long K = 2 * g.SW2 + 1;
    return K * K * g.cn * (2 * g.ftzero + 63) + g.P2 > 32767;
}

// work of one pair in units of one 1080p / D=128 volume
static double pair_work(const Geom& g) { return ((double)g.H * g.W1 * g.Dp) / (1080.0 * 1792.0 * 128.0); }
static double auto_concurrent_limit(const Geom& g) { return g.mode == CAMD_MODE_HH ? 8.0 : 4.0; }
// The band passes win on throughput once their workgroups -- bands x (virtual) pairs -- fill the chip; below that
// the wavefront of a pass fills and drains over a mostly idle GPU and the line scans win (concurrently into their own
// volumes while there is room for them, one launch per direction otherwise).  Measured crossovers (r03_batch_sweep,
// tools/gpu_mid_d_paths.sh, tools/gpu_small_d_paths.sh, tools/gpu_get_depth_sweep.py): 1080p D=128 between 3 and 4
// pairs (117 / 156 workgroups), MODE_HH at 8 (312); 720p D=128 8 pairs (208) band +29 %; 720p D=64 8 pairs (104)
// scans +19 %; 4K D=64 2 pairs (78) scans.  The two-wavefront modes need about twice as many.
static int band_fill_workgroups(const Geom& g) { return (g.mode == CAMD_MODE_HH || g.mode == CAMD_MODE_HH4) ? 300 : 150; }
// largest batch the AUTO rule sends down the concurrent-direction path (it needs npaths volumes per pair): the
// batches whose band passes would not fill the chip; at least one pair, at most CAMD_MULTI_MAX_BATCH
static int auto_concurrent_pairs(const Geom& g, bool band_ok, int max_batch, int nbands)
{
    int cap = max_batch < CAMD_MULTI_MAX_BATCH ? max_batch : CAMD_MULTI_MAX_BATCH;
    int n;
    if (band_ok && nbands > 0) n = (band_fill_workgroups(g) - 1) / nbands;  // pairs with fewer workgroups than that
    else n = (int)(auto_concurrent_limit(g) / pair_work(g));                   // no band instantiation (D > 256)
    if (n < 1) n = 1;
    return n < cap ? n : cap;
}

// The band passes are instantiated for 16 lanes x {1,2} vectors and 8 / 4 / 2 lanes x 1 vector per pixel (every
// numDisparities up to 256); their inline winner-take-all (not used by MODE_SGBM_3WAY, which decides its winners in
// k_wta) covers uniquenessRatio <= 99.
static bool band_supported(const Geom& g)
{
    const bool shape = g.W1 > 0 && g.nr <= 8;  // (lanes < 16 always come with nr == 4)
    return shape && (g.mode == CAMD_MODE_SGBM_3WAY || g.uniq <= 99);
}

// One kernel instantiation per line-group shape (lanes, nr): M(LANES, NR) for the handle's shape.  16 lanes take
// nr = 3 .. 8 (numDisparities up to 256 in steps of 32), 12 and 16 (up to 384 / 512, scan kernels only).
#define CAMD_FOR_SHAPE(g, M)                      \
    do {                                          \
        if ((g).lanes == 2) M(2, 4);              \
        else if ((g).lanes == 4) M(4, 4);         \
        else if ((g).lanes == 8) M(8, 4);         \
        else switch ((g).nr) {                    \
            case 3: M(16, 3); break;              \
            case 4: M(16, 4); break;              \
            case 5: M(16, 5); break;              \
            case 6: M(16, 6); break;              \
            case 7: M(16, 7); break;              \
            case 8: M(16, 8); break;              \
            case 12: M(16, 12); break;            \
            default: M(16, 16);                   \
        }                                         \
    } while (0)
// the same for the band passes (nr <= 8; band_supported)
#define CAMD_FOR_BAND_SHAPE(g, M)                 \
    do {                                          \
        if ((g).lanes == 2) M(2, 4);              \
        else if ((g).lanes == 4) M(4, 4);         \
        else if ((g).lanes == 8) M(8, 4);         \
        else switch ((g).nr) {                    \
            case 3: M(16, 3); break;              \
            case 4: M(16, 4); break;              \
            case 5: M(16, 5); break;              \
            case 6: M(16, 6); break;              \
            case 7: M(16, 7); break;              \
            default: M(16, 8);                    \
        }                                         \
    } while (0)

static int invalid_disp(const Geom& g) { return (g.minD - 1) * 16; }  // cv2's INVALID_DISP_SCALED

// the eight directions in the order OpenCV adds them up (it matters once sums saturate with negative terms in play)
static const int kDirs8[8][2] = {{1, 0}, {1, 1}, {0, 1}, {-1, 1}, {-1, 0}, {1, -1}, {0, -1}, {-1, -1}};

// the directions of one launch (unused entries repeat the first); returns the longest direction's number of lines
static int fill_scan_dirs(const Geom& g, const int (*dirs)[2], int ndirs, size_t dir_stride, ScanDirs* sd)
{
    int maxlines = 0;
    for (int i = 0; i < 8; i++) {
        const int k = i < ndirs ? i : 0;
        sd->dx[i] = dirs[k][0];
        sd->dy[i] = dirs[k][1];
        sd->nlines[i] = sd->dy[i] == 0 ? g.H : (sd->dx[i] == 0 ? g.W1 : g.W1 + g.H - 1);
        if (i < ndirs && sd->nlines[i] > maxlines) maxlines = sd->nlines[i];
    }
    sd->dir_stride = dir_stride;
    return maxlines;
}

// ndirs directions in one launch (ndirs > 1 only with FIRST: each direction writes its own volume)
template <bool FIRST>
static int launch_scan(const camd_sgbm* h, const int (*dirs)[2], int ndirs, uint16_t* S, size_t dir_stride,
                       int batch, hipStream_t st)
{
    const Geom& g = h->ga;
    ScanDirs sd;
    const int maxlines = fill_scan_dirs(g, dirs, ndirs, dir_stride, &sd);
    dim3 grid(div_up((long long)maxlines * g.lanes, 256), batch, ndirs);
    const bool pad = g.Dp != g.D;
#define CAMD_SCAN(LN, NVV)                                                                                  \
    do {                                                                                                    \
        if (pad) hipLaunchKernelGGL((k_scan<LN, NVV, FIRST, true>), grid, dim3(256), 0, st, h->C, S, g, sd, \
                                    h->vol_elems);                                                          \
        else hipLaunchKernelGGL((k_scan<LN, NVV, FIRST, false>), grid, dim3(256), 0, st, h->C, S, g, sd,    \
                                h->vol_elems);                                                              \
    } while (0)
    CAMD_FOR_SHAPE(g, CAMD_SCAN);
#undef CAMD_SCAN
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

static int launch_wta(const camd_sgbm* h, const uint16_t* S, int nvol, size_t dir_stride, int16_t* disp,
                      size_t pitch_e, size_t stride_e, int batch, hipStream_t st)
{
    const Geom& g = h->ga;
    const int tie_lanes = g.mode == CAMD_MODE_SGBM_3WAY ? h->way3_simd_lanes : 0;
    dim3 grid(g.H, batch);
    size_t lds = (size_t)g.W * 6;
    lds = align_up(lds, 16);
#define CAMD_WTA(LN, NVV)                                                                       \
    hipLaunchKernelGGL((k_wta<LN, NVV>), grid, dim3(256), lds, st, S, disp, pitch_e, stride_e, g, \
                       h->vol_elems, nvol, dir_stride, tie_lanes)
    CAMD_FOR_SHAPE(g, CAMD_WTA);
#undef CAMD_WTA
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

// one band-wavefront pass over `batch` (virtual) pairs (sgbm_band.hpp): full = H, V, Dg, A of sweep (sx, sy);
// !full = the row-parallel H-only pass.  mode 0 writes S, 1 adds to S, 2 reads S and decides the winners.
static int launch_band(camd_sgbm* h, int sx, int sy, bool full, int mode, int batch, hipStream_t st, bool diag = true,
                       bool tie8 = false)
{
    const Geom& g = h->ga;
    BandArgs a;
    a.C = h->C; a.S = h->S; a.E = h->E; a.flags = h->flags; a.ticket = h->ticket; a.err = h->err;
    a.keys = h->keys; a.d1 = h->d1; a.vol_stride = h->vol_elems; a.erec_stride = h->erec_stride;
    a.sx = sx; a.sy = sy; a.nbands = h->nbands; a.nchunks = h->nchunks; a.npairs = batch;
    a.epoch = ++h->epoch;
    a.write_S = h->keep_S;
    CAMD_HIP(hipMemsetAsync(h->ticket, 0, 4, st));
    // full passes: one workgroup per (pair, band); the row-parallel pass: the batch's rows in runs of R (sgbm_band.hpp)
    dim3 grid(full ? h->nbands * batch : div_up((long long)batch * g.H, BAND_THREADS / g.lanes)), block(BAND_BLOCK);
    const bool pad = g.Dp != g.D;
    // (the shapes that exist since round 5, nr = 3 / 5 / 6 / 7, are instantiated in their padded form only: the
    // unpadded one merely skips two masking operations per register, and D = Dp is the rare case there)
#define CAMD_BAND(LN, NRR, FF, MM, DG)                                                                          \
    do {                                                                                                        \
        if (pad || (NRR) % 4 != 0) hipLaunchKernelGGL((k_band<LN, NRR, FF, MM, true, DG>), grid, block, 0, st, a, g); \
        else hipLaunchKernelGGL((k_band<LN, ((NRR) % 4 ? 4 : (NRR)), FF, MM, false, DG>), grid, block, 0, st, a, g);   \
    } while (0)
#define CAMD_BAND_F0T(LN, NRR) CAMD_BAND(LN, NRR, true, 0, true)
#define CAMD_BAND_F2T(LN, NRR) CAMD_BAND(LN, NRR, true, 2, true)
#define CAMD_BAND_F0F(LN, NRR) CAMD_BAND(LN, NRR, true, 0, false)
#define CAMD_BAND_F2F(LN, NRR) CAMD_BAND(LN, NRR, true, 2, false)
#define CAMD_BAND_R2(LN, NRR) CAMD_BAND(LN, NRR, false, 2, true)
#define CAMD_BAND_R1(LN, NRR) CAMD_BAND(LN, NRR, false, 1, true)
    if (full && mode == 0 && diag) CAMD_FOR_BAND_SHAPE(g, CAMD_BAND_F0T);
    else if (full && mode == 2 && diag) CAMD_FOR_BAND_SHAPE(g, CAMD_BAND_F2T);
    else if (full && mode == 0) CAMD_FOR_BAND_SHAPE(g, CAMD_BAND_F0F);
    else if (full && mode == 2) CAMD_FOR_BAND_SHAPE(g, CAMD_BAND_F2F);
    else if (!full && mode == 2 && tie8) {
        // MODE_SGBM_3WAY: nr is a multiple of 4 (normalise)
#define CAMD_BAND_TIE(LN, NRR)                                                                                  \
    do {                                                                                                        \
        if (pad) hipLaunchKernelGGL((k_band<LN, NRR, false, 2, true, true, true>), grid, block, 0, st, a, g);   \
        else hipLaunchKernelGGL((k_band<LN, NRR, false, 2, false, true, true>), grid, block, 0, st, a, g);      \
    } while (0)
        if (g.lanes == 16 && g.nr == 4) CAMD_BAND_TIE(16, 4);
        else if (g.lanes == 16) CAMD_BAND_TIE(16, 8);
        else if (g.lanes == 8) CAMD_BAND_TIE(8, 4);
        else if (g.lanes == 4) CAMD_BAND_TIE(4, 4);
        else CAMD_BAND_TIE(2, 4);
#undef CAMD_BAND_TIE
    }
    else if (!full && mode == 2 && h->persist_row > 0 && g.lanes == 16 && g.nr == 4) {
        // CAMD_OPT_RESIDENT: a fixed number of resident workgroups, runs of rows by ticket (sgbm_band.hpp)
        const dim3 pgrid(h->persist_row * (h->num_cus > 0 ? h->num_cus : 256));
        if (pad) hipLaunchKernelGGL((k_band_row_persist<16, 4, true>), pgrid, block, 0, st, a, g);
        else hipLaunchKernelGGL((k_band_row_persist<16, 4, false>), pgrid, block, 0, st, a, g);
    }
    else if (!full && mode == 2) CAMD_FOR_BAND_SHAPE(g, CAMD_BAND_R2);
    else if (!full && mode == 1) CAMD_FOR_BAND_SHAPE(g, CAMD_BAND_R1);
    else { set_error("band pass (full %d, mode %d) not instantiated", (int)full, mode); return CAMD_ERR_UNSUPPORTED; }
#undef CAMD_BAND_F0T
#undef CAMD_BAND_F2T
#undef CAMD_BAND_F0F
#undef CAMD_BAND_F2F
#undef CAMD_BAND_R2
#undef CAMD_BAND_R1
#undef CAMD_BAND
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

// A flagged volume for which no exact workspace could be allocated: never hand back a silently different result --
// its disparities are written as invalid and the handle reports an error (err = 2).
__global__ __launch_bounds__(256) void k_poison_flagged(int16_t* __restrict__ raw, size_t stride_e, size_t n,
                                                        const uint32_t* __restrict__ neg, uint32_t* __restrict__ err,
                                                        int invalid)
{
    const int vp = blockIdx.y;
    if (!neg[vp]) return;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        raw[(size_t)vp * stride_e + i] = (int16_t)invalid;
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(err, 2u);
}

// the aggregation + winner-take-all in int arithmetic (sgbm_exact.hpp) of every FLAGGED (virtual) pair of the batch, in
// one launch that returns at once when nothing is flagged.  dst: the raw disparity image of (virtual) pair 0.
static int launch_exact(const camd_sgbm* h, int nvolumes, int16_t* dst, size_t stride_e, size_t n_e, hipStream_t st)
{
    const Geom& g = h->ga;
    static const int d_hh4[4][2] = {{0, 1}, {0, -1}, {1, 0}, {-1, 0}};   // v, ^, ->, <-  (oracle/sgbm_ref.c:532-607)
    static const int d_3way[3][2] = {{-1, 0}, {1, 0}, {0, 1}};           // (right + left) + top  (:789)
    const int (*dirs)[2] = g.mode == CAMD_MODE_HH4 ? d_hh4 : (g.mode == CAMD_MODE_SGBM_3WAY ? d_3way : kDirs8);
    const int nd = g.npaths;
    ScanDirs sd;
    fill_scan_dirs(g, dirs, nd, h->vol_elems, &sd);  // (dir_stride in int elements)
    const bool way3 = g.mode == CAMD_MODE_SGBM_3WAY;
    ExactArgs a;
    a.C = reinterpret_cast<const int16_t*>(h->C);
    a.Lx = h->Lx;
    a.dst = dst;
    a.vol_stride = h->vol_elems;
    a.dst_stride_e = stride_e;
    a.dst_pitch_e = (size_t)g.W;
    a.dst_n = n_e;
    a.neg = h->cost_neg;
    a.bar = h->xbar;
    a.err = h->err;
    a.nvol = nvolumes;
    a.nd = nd;
    a.tie_lanes = way3 ? h->way3_simd_lanes : 0;
    a.combine = g.mode == CAMD_MODE_HH4 ? 1 : (way3 ? 2 : 0);
    a.min_as_int = g.mode == CAMD_MODE_HH4 ? 1 : 0;
    a.invalid = invalid_disp(g);
    CAMD_HIP(hipMemsetAsync(h->xbar, 0, 4, st));
    const size_t lds = align_up((size_t)g.W * 6, 16);
    // One workgroup per compute unit and a hand-rolled grid barrier between the phases: the workgroups must all be
    // resident at once.  A cooperative launch makes the runtime check that (it refuses a grid that cannot be); where it is
    // refused or unsupported the plain launch runs with the barrier's bounded wait as the safety net (error bit 2).
    const dim3 grid(h->num_cus > 0 ? h->num_cus : 256);
    Geom gg = g;
    void* kargs[] = {(void*)&a, (void*)&gg, (void*)&sd};
#define CAMD_XALL(LN, NRR)                                                                                          \
    do {                                                                                                            \
        const void* fn = way3 ? (const void*)k_exact_all<LN, NRR, true> : (const void*)k_exact_all<LN, NRR, false>; \
        if (hipLaunchCooperativeKernel(fn, grid, dim3(256), kargs, lds, st) != hipSuccess) {                        \
            (void)hipGetLastError();                                                                                \
            if (way3) hipLaunchKernelGGL((k_exact_all<LN, NRR, true>), grid, dim3(256), lds, st, a, g, sd);         \
            else hipLaunchKernelGGL((k_exact_all<LN, NRR, false>), grid, dim3(256), lds, st, a, g, sd);             \
        }                                                                                                           \
    } while (0)
    CAMD_FOR_SHAPE(g, CAMD_XALL);
#undef CAMD_XALL
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

static size_t smulti_bytes(const Geom& g, size_t vol_elems, int pairs) { return (size_t)g.npaths * pairs * vol_elems * 2; }
static size_t lx_bytes(const Geom& g, size_t vol_elems) { return (size_t)g.npaths * vol_elems * 4; }

// Every device buffer of a handle in bytes (0 = the shape has no use for it) and the integers that size them: the ONE
// description of the workspace.  camd_sgbm_workspace_bytes reports its sum, camd_sgbm_create allocates from it.
struct WorkspacePlan {
    CostRanges cr;
    int stripe_sz, vrows;            // 3WAY: rows a stripe owns; rows of the tallest (virtual) pair
    size_t vol_elems;                // int16 elements of one volume
    size_t raw_stride, rawv_stride;  // int16 elements of one raw disparity image: a pair's, a 3WAY stripe's
    bool band_ok, may_overflow;
    int nbands, nchunks, smulti_cap;
    size_t erec_stride;
    size_t C, S;                     // one volume per (virtual) pair each
    size_t rawv, raw;                // raw disparity per 3WAY stripe / per pair
    size_t vol_flags;                // per volume: the near-overflow and the below-P2 word
    size_t ticket;                   // four words: band ticket, error word, the exact path's barrier, k_cost_persist's counter
    size_t speckle;
    size_t E, band_flags, keys, d1;  // band path: edge records, their flags, the winner-take-all state of every pixel
    size_t Smulti;                   // the latency path's per-direction volumes at the AUTO capacity (smulti_cap pairs)
    size_t Lx;                       // exact path: one set of per-direction int volumes
    // Where camd_sgbm_workspace_bytes has always reported something else than camd_sgbm_create allocates.  StereoSGBM's
    // handle cache (sgbm.py) evicts by the reported figure, so both sides stay as they are:
    size_t ticket_unreported;        // the report counts the first two of the four ticket words
    size_t rawv_unallocated;         // 3WAY without a matchable column (W1 <= 0): reported, but create allocates no volume
};

static int plan_workspace(const Geom& g, const camd_sgbm_params& p, int max_batch, WorkspacePlan* w)
{
    memset(w, 0, sizeof(*w));
    const int rc = cost_ranges(g, p.blockSize, &w->cr, &w->stripe_sz, &w->vrows);
    if (rc != CAMD_OK) return rc;
    const bool way3 = g.mode == CAMD_MODE_SGBM_3WAY, matchable = g.W1 > 0;
    const size_t w1 = matchable ? (size_t)g.W1 : 0, nvol = (size_t)max_batch * w->cr.n;  // volumes: one per (virtual) pair
    w->vol_elems = align_up((size_t)w->vrows * w1 * g.Dp * 2, 256) / 2;
    w->raw_stride = align_up((size_t)g.H * g.W * 2, 256) / 2;
    w->rawv_stride = align_up((size_t)w->vrows * g.W * 2, 256) / 2;
    w->C = w->S = nvol * w->vol_elems * 2;
    const size_t rawv = way3 ? nvol * w->rawv_stride * 2 : 0;
    w->rawv = matchable ? rawv : 0;
    w->rawv_unallocated = matchable ? 0 : rawv;
    w->raw = (size_t)max_batch * w->raw_stride * 2;
    w->vol_flags = nvol * 8;
    w->ticket = 16;
    w->ticket_unreported = 8;
    w->speckle = g.speckleWindowSize > 0 ? speckle_ws_bytes(g.W, g.H, max_batch) : 0;
    w->band_ok = band_supported(g);
    if (w->band_ok) {
        w->nbands = div_up(w->vrows, BAND_THREADS / g.lanes);  // bands of one (virtual) pair
        w->nchunks = div_up(g.W1, BAND_CHUNK);
        w->erec_stride = band_erec_stride(g.W1, g.lanes, (g.nr + 3) / 4);
        const size_t npix = nvol * w->vrows * g.W;
        w->E = nvol * w->nbands * w->erec_stride * 8;
        w->band_flags = nvol * w->nbands * w->nchunks * 4;
        w->keys = npix * 4;
        w->d1 = npix * 2;
    }
    // per-direction volumes: the latency path's (3WAY has none for its stripes), and one set of int volumes for the exact
    // aggregation where the parameters allow an int16 overflow of the cost volume (sgbm_exact.hpp)
    w->may_overflow = params_may_overflow(g);
    if (matchable) {
        w->smulti_cap = way3 ? 0 : auto_concurrent_pairs(g, w->band_ok, max_batch, w->nbands);
        w->Smulti = smulti_bytes(g, w->vol_elems, w->smulti_cap);
        if (w->may_overflow) w->Lx = lx_bytes(g, w->vol_elems);
    }
    return CAMD_OK;
}

#define CAMD_TRY(call) do { const int rc_ = (call); if (rc_ != CAMD_OK) return rc_; } while (0)

// profiling: the event that starts stage i (and ends stage i - 1); mark_rest closes every stage from i on as empty
static int mark(camd_sgbm* h, int i, hipStream_t st)
{
    if (h->profiling && h->ev_ok) CAMD_HIP(hipEventRecord(h->ev[i], st));
    return CAMD_OK;
}
static int mark_rest(camd_sgbm* h, int first, hipStream_t st)
{
    for (int i = first; i <= ST_COUNT; i++) CAMD_TRY(mark(h, i, st));
    return CAMD_OK;
}

// ---- the launch shape of k_cost ---------------------------------------------------------------------------------
// COST_CHUNKED: the wrapping kernel, rows in parallel chunks; COST_SATURATING: the saturating recurrence must start at
// row 0 (one chunk: few workgroups, a long walk); COST_RESIDENT: k_cost_persist (CAMD_OPT_RESIDENT), a fixed number of
// resident workgroups take the chunked kernel's items by ticket, in smaller row chunks so that the last items of the
// launch end together
enum CostForm { COST_CHUNKED, COST_SATURATING, COST_RESIDENT };
struct CostShape {
    int nw, ndblk, nstrips;       // waves per workgroup, disparity blocks of <= 128, strips of 64 - (K - 1) output columns
    int nchunks, rows_per_chunk;  // row chunks (rows per chunk in the longest range)
    size_t lds;
};
static CostShape cost_launch_shape(const camd_sgbm* h, int vbatch, CostForm form)
{
    const Geom& g = h->g;
    const int K = 2 * g.SW2 + 1, rows = h->ga.H;
    CostShape s;
    // waves per workgroup: one per 8 disparities, at least 4 (the staging needs up to 3 waves of lanes), at most
    // 8 for RGB (three 8-wave workgroups share a CU at 74 VGPRs: 17.5 instead of 20.2 ms per 64 pairs; a 16-wave
    // workgroup would have a CU to itself) and 16 for gray (fewer registers, and the staging per cell halves)
    const int maxw = g.cn == 3 ? CAMD_COST_MAX_WAVES_RGB : CAMD_COST_MAX_WAVES_GRAY;
    s.nw = g.Dp / COST_DL < 4 ? 4 : (g.Dp / COST_DL < maxw ? g.Dp / COST_DL : maxw);
    s.ndblk = div_up(g.Dp, s.nw * COST_DL);
    s.nstrips = div_up(g.W1, 64 - (K - 1));
    s.lds = cost_lds_bytes(g.cn, s.nw);
    int nchunks = 1;
    if (form != COST_SATURATING) {
        // row chunks: enough workgroups for ~32 rounds over the chip (resident: 24 items per resident workgroup)
        const long long per_chunk = (long long)s.nstrips * s.ndblk * vbatch;
        const int maxc = rows / 32 > 1 ? rows / 32 : 1;
        nchunks = form == COST_RESIDENT ? div_up(24LL * h->persist_cost * (h->num_cus > 0 ? h->num_cus : 256), per_chunk)
                                        : div_up(8192, per_chunk);
        nchunks = nchunks < 1 ? 1 : (nchunks > maxc ? maxc : nchunks);
        // Few workgroups (one or two pairs per call): the launch is a handful of rounds over the chip's places
        // (256 CUs x 3 eight-wave / 1 sixteen-wave workgroups), so the LAST round's fill decides: take the chunk
        // count that minimises rounds x (rows walked per workgroup, incl. the K-1 rows every chunk recomputes).
        // One 1080p RGB pair: 33 chunks = 1980 workgroups = 2.6 rounds of 37 rows -> 25 chunks = 1500 = 2 of 48.
        const long long places = 256LL * (s.nw <= 8 ? 3 : 1);
        if (form == COST_CHUNKED && per_chunk * nchunks < 6 * places) {
            long long best = -1;
            for (int nc = 1; nc <= maxc; nc++) {
                const long long cost = (long long)div_up(per_chunk * nc, places) * (div_up(rows, nc) + K - 1);
                if (best < 0 || cost < best) { best = cost; nchunks = nc; }
            }
        }
    }
    s.rows_per_chunk = div_up(rows, nchunks);
    s.nchunks = div_up(rows, s.rows_per_chunk);
    return s;
}

// one launch of the fused cost kernel over the call's vbatch volumes: the saturating or the wrapping recurrence; ovf /
// thresh: the two-stage build of a saturating volume (sgbm_cost.hpp)
static int launch_cost(camd_sgbm* h, const uint8_t* left, const uint8_t* right, size_t pitch, size_t image_stride,
                       int vbatch, bool sat_kernel, uint32_t* ovf, int thresh, hipStream_t st)
{
    const Geom& g = h->g;
    const int K = 2 * g.SW2 + 1;
    CostShape s = cost_launch_shape(h, vbatch, sat_kernel ? COST_SATURATING : COST_CHUNKED);
    // k_cost_persist is instantiated for the launches in which no wave leaves early and no per-volume early exit applies
    const bool resident = h->persist_cost > 0 && !sat_kernel && !ovf && h->cr.n == 1 && (K == 5 || K == 3) &&
                          g.D % (s.nw * COST_DL) == 0;
    if (resident) s = cost_launch_shape(h, vbatch, COST_RESIDENT);
    const dim3 grid(s.nstrips, s.nchunks * s.ndblk, vbatch), block(64 * s.nw);
    if (resident) {
        uint32_t* tk = h->ticket + 3;  // (zeroed by run_cost, before the launches)
        const int nx = s.nstrips, ny = s.nchunks * s.ndblk, nitems = nx * ny * vbatch;
        const dim3 pgrid(h->persist_cost * (h->num_cus > 0 ? h->num_cus : 256));
#define CAMD_COSTP(CNN, KK) hipLaunchKernelGGL((k_cost_persist<CNN, KK>), pgrid, block, s.lds, st, left, right, pitch, image_stride, \
                                               h->C, g, s.rows_per_chunk, s.nchunks, h->vol_elems, h->cr, tk, nx, ny, nitems)
        if (g.cn == 1) { if (K == 5) CAMD_COSTP(1, 5); else CAMD_COSTP(1, 3); }
        else { if (K == 5) CAMD_COSTP(3, 5); else CAMD_COSTP(3, 3); }
#undef CAMD_COSTP
        CAMD_LAUNCH_CHECK();
        return CAMD_OK;
    }
#define CAMD_COST(CNN, KK, SS)                                                                                          \
    hipLaunchKernelGGL((k_cost<CNN, KK, SS>), grid, block, s.lds, st, left, right, pitch, image_stride, h->C, g,        \
                       s.rows_per_chunk, s.nchunks, h->vol_elems, h->cr, ovf, thresh, h->cost_neg)
#define CAMD_COST_K(CNN)                                                                         \
    switch (K) {                                                                                 \
        case 1: CAMD_COST(CNN, 1, false); break;                                                 \
        case 3: CAMD_COST(CNN, 3, false); break;                                                 \
        case 5: if (sat_kernel) CAMD_COST(CNN, 5, true); else CAMD_COST(CNN, 5, false); break;   \
        case 7: if (sat_kernel) CAMD_COST(CNN, 7, true); else CAMD_COST(CNN, 7, false); break;   \
        case 9: if (sat_kernel) CAMD_COST(CNN, 9, true); else CAMD_COST(CNN, 9, false); break;   \
        default: if (sat_kernel) CAMD_COST(CNN, 11, true); else CAMD_COST(CNN, 11, false);       \
    }
    if (g.cn == 1) { CAMD_COST_K(1) } else { CAMD_COST_K(3) }
#undef CAMD_COST_K
#undef CAMD_COST
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

// the split pair (sgbm_split.hpp): BT + horizontal box sum into S, then the vertical box sum + P2 into C
static int launch_hsum(camd_sgbm* h, const uint8_t* left, const uint8_t* right, size_t pitch, size_t image_stride,
                       int batch, hipStream_t st)
{
    const Geom& g = h->g;
    int nseg = div_up(g.W1, HSUM_SEG), ndblk = div_up(g.Dp, 64);
    dim3 grid(nseg, g.H, batch), block(64 * ndblk);
    const int es = g.cn == 1 ? 4 : 12;
    const size_t maxr = HSUM_SEG + 2 * g.SW2 + ndblk * 64 + 2, maxl = HSUM_SEG + 2 * g.SW2 + 2;
    size_t lds = ((maxr + maxl) * es + (size_t)ndblk * (2 * g.SW2 + 1) * 64) * 4;
#define CAMD_HSUM(CNN, KK)                                                                                        \
    hipLaunchKernelGGL((k_hsum<CNN, KK>), grid, block, lds, st, left, right, pitch, image_stride, h->S, g, ndblk, \
                       h->vol_elems)
#define CAMD_HSUM_K(CNN)                                \
    switch (2 * g.SW2 + 1) {                            \
        case 1: CAMD_HSUM(CNN, 1); break;               \
        case 3: CAMD_HSUM(CNN, 3); break;               \
        case 5: CAMD_HSUM(CNN, 5); break;               \
        case 7: CAMD_HSUM(CNN, 7); break;               \
        case 9: CAMD_HSUM(CNN, 9); break;               \
        case 11: CAMD_HSUM(CNN, 11); break;             \
        default: CAMD_HSUM(CNN, 0);                     \
    }
    // measured: the register ring pays for gray (11.3 -> 9.5 ms per 64 pairs) but not for RGB, where the longer
    // unrolled body costs more than the two LDS operations it saves (20.2 -> 21.0 ms)
    if (g.cn == 1) { CAMD_HSUM_K(1) } else { CAMD_HSUM(3, 0); }
#undef CAMD_HSUM_K
#undef CAMD_HSUM
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}
static int launch_vsum(camd_sgbm* h, bool sat, int batch, hipStream_t st)
{
    const Geom& g = h->g;
    const int K = 2 * g.SW2 + 1;
    size_t rowv = (size_t)g.W1 * (g.Dp / 8);
    const uint4* hs4 = reinterpret_cast<const uint4*>(h->S);
    uint4* c4 = reinterpret_cast<uint4*>(h->C);
    const size_t ring_lds = (size_t)K * 256 * sizeof(uint4);
    if (sat) {
        // the saturating recurrence runs from row 0 down the whole column (LDS-ring kernel, any K)
        const dim3 vgrid(div_up((long long)rowv, 256), 1, batch);
        hipLaunchKernelGGL(k_vsum<true>, vgrid, dim3(256), ring_lds, st, hs4, c4, g, h->vol_elems / 8, g.H);
    } else {
        const dim3 vgrid(div_up((long long)rowv, 256), div_up(g.H, VSUM_ROWS), batch);
        switch (K) {
#define CAMD_VSUM(KK) case KK: hipLaunchKernelGGL((k_vsum_reg<KK>), vgrid, dim3(256), 0, st, hs4, c4, g, h->vol_elems / 8); break
            CAMD_VSUM(1); CAMD_VSUM(3); CAMD_VSUM(5); CAMD_VSUM(7); CAMD_VSUM(9); CAMD_VSUM(11);
#undef CAMD_VSUM
            default:
                hipLaunchKernelGGL(k_vsum<false>, vgrid, dim3(256), ring_lds, st, hs4, c4, g, h->vol_elems / 8, VSUM_ROWS);
        }
    }
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

// ---- stage 1: the matching cost volume C (stages "cost", "hsum", "vsum"; the caller has marked ST_COST) --------------
static int run_cost(camd_sgbm* h, const uint8_t* left, const uint8_t* right, size_t pitch, size_t image_stride, int batch,
                    hipStream_t st)
{
    const Geom& g = h->g;
    const int K = 2 * g.SW2 + 1;
    // U7: int16 overflow is possible at all only beyond params_may_overflow's bound; below it SAT == wrap
    const bool may_overflow = h->may_overflow;
    const bool sat = h->saturate && may_overflow;
    const bool way3 = g.mode == CAMD_MODE_SGBM_3WAY;
    const int vbatch = batch * h->cr.n;  // volumes this call fills (3WAY: four stripes per pair)
    const bool fused = K <= 11 && (h->cost_path != CAMD_COST_SPLIT || way3);
    const bool do_cost = (h->phases & 1) != 0;
    if (fused && do_cost) {
        // The saturating recurrence only differs from the wrapping one on images that drive a window sum to within one
        // horizontal sum of 32767, so where the true sums cannot wrap 16 bits the chunked wrapping kernel runs first and
        // flags the volumes that need the sequential kernel (sgbm_cost.hpp)
        const int tbound = K * g.cn * (2 * g.ftzero + 63);
        const bool two_stage = sat && (long long)K * tbound + g.P2 <= 65535;
        if (may_overflow) CAMD_HIP(hipMemsetAsync(h->cost_neg, 0, (size_t)vbatch * 4, st));
        if (h->persist_cost > 0) CAMD_HIP(hipMemsetAsync(h->ticket + 3, 0, 4, st));
        if (two_stage) {
            CAMD_HIP(hipMemsetAsync(h->cost_ovf, 0, (size_t)vbatch * 4, st));
            CAMD_TRY(launch_cost(h, left, right, pitch, image_stride, vbatch, false, h->cost_ovf, 32767 - tbound, st));
            CAMD_TRY(launch_cost(h, left, right, pitch, image_stride, vbatch, true, h->cost_ovf, -1, st));
        } else {
            CAMD_TRY(launch_cost(h, left, right, pitch, image_stride, vbatch, sat, nullptr, -1, st));
        }
    }
    CAMD_TRY(mark(h, ST_HSUM, st));
    if (!fused && do_cost) CAMD_TRY(launch_hsum(h, left, right, pitch, image_stride, batch, st));
    CAMD_TRY(mark(h, ST_VSUM, st));
    if (!fused && do_cost) CAMD_TRY(launch_vsum(h, sat, batch, st));
    // Volumes that hold a value below P2 are outside the regime of the packed-u16 aggregation kernels (sgbm_exact.hpp).
    // The saturating cost kernel reports them itself; behind the wrapping kernels and the split pair one more pass over
    // C finds them (only where the parameters allow an overflow at all)
    if (do_cost && may_overflow && !(fused && sat)) {
        if (!fused) CAMD_HIP(hipMemsetAsync(h->cost_neg, 0, (size_t)vbatch * 4, st));
        hipLaunchKernelGGL(k_flag_below, dim3(512, 1, vbatch), dim3(256), 0, st, reinterpret_cast<const int16_t*>(h->C),
                           h->ga, h->vol_elems, h->cr, h->cost_neg);
        CAMD_LAUNCH_CHECK();
    }
    return CAMD_OK;
}

// ---- the aggregation path of a call -----------------------------------------------------------------------------
// Fused band passes win on throughput (>= ~8 pairs per launch), concurrent per-direction scans on latency (a few pairs:
// every direction gets its own S volume and all of them run at once), sequential scans are the generic fallback.
// Measured at 1080p / D=128 (tools/gpu_batch_sweep.py, ms per pair): the concurrent scans win up to 4 pairs
// per call for 5 paths (3.1 / 2.4 / 2.0 against 6.8 / 3.7 / 2.2 through the band passes) and up to 8 pairs
// for 8 paths (3.6 ... 2.6 against 13.1 ... 2.9); from there on the band passes take over (1.36 / 1.87 at 16
// pairs, 0.98 / 1.14 at 64).
static int choose_path(const camd_sgbm* h, int batch)
{
    const Geom& g = h->g;
    const bool way3 = g.mode == CAMD_MODE_SGBM_3WAY;
    const long long band_wgs = (long long)h->nbands * batch * h->cr.n;  // workgroups of a full band pass
    int path = h->path;
    if (path == CAMD_PATH_AUTO) {
        // band passes when their workgroups fill the chip (band_fill_workgroups), else the concurrent scans
        if (h->band_ok && band_wgs >= band_fill_workgroups(g)) path = CAMD_PATH_BAND;
        else path = CAMD_PATH_CONCURRENT;
    }
    if (way3) {
        // no per-direction volumes for the stripes: band passes, or three line scans + k_wta.  The wavefront of a
        // band pass fills slowly, so for little work the scans win (ms per pair, scans / band, 1080p D=128: 2.1 / 4.2
        // for one pair, 1.65 / 1.38 for four; VGA D=64: 0.36 / 1.09 for one, 0.125 / 0.10 for sixteen)
        if (h->path == CAMD_PATH_AUTO) path = batch * pair_work(g) < 2.5 ? CAMD_PATH_SCAN : CAMD_PATH_BAND;
        else if (path != CAMD_PATH_SCAN) path = CAMD_PATH_BAND;
    }
    if (path == CAMD_PATH_BAND && !h->band_ok) path = CAMD_PATH_SCAN;
    // the per-direction volumes were sized in create / set_option: a larger batch takes the next best path -- the band
    // passes when they at least come close to filling the chip, else one scan launch per direction
    if (path == CAMD_PATH_CONCURRENT && batch > h->smulti_cap)
        path = (h->band_ok && (h->path != CAMD_PATH_AUTO || band_wgs >= 128)) ? CAMD_PATH_BAND : CAMD_PATH_SCAN;
    // At 4 or 2 lanes per pixel (numDisparities <= 32) a band is 112 or 224 rows high: an image has only a handful of
    // bands (tools/gpu_small_d_paths.sh, scans / band passes in pairs/s: 1080p D=32 8 pairs 1585 / 1294, 16 pairs
    // 1673 / 2202; VGA D=16 16 pairs 9980 / 6430, 64 pairs 17060 / 18530): same rule, the band passes from ~128
    // workgroups on
    if (h->path == CAMD_PATH_AUTO && path == CAMD_PATH_BAND && g.lanes <= 4 && band_wgs < 128) path = CAMD_PATH_SCAN;
    return path;
}

// 3WAY decides its winners inside the last band pass when that pass knows the tie rule in force: cv2's 8-slot rule
// for D % 8 == 0, or the scalar build's "smallest d" (the ordinary rule); otherwise k_wta does it afterwards
static bool way3_inline(const camd_sgbm* h) { return h->way3_simd_lanes == 1 || h->g.D % 8 == 0; }
// CAMD_OPT_PHASES without bit 2: the call ends behind the first band pass.  (The split between the two aggregation
// passes exists on the plain band path only; elsewhere bits 1 and 2 travel together)
static bool stops_before_last_pass(const camd_sgbm* h, int path)
{
    return path == CAMD_PATH_BAND && h->g.mode != CAMD_MODE_SGBM_3WAY && !(h->phases & 4);
}
static int launch_wta_init(camd_sgbm* h, const Geom& ga, int nimages, hipStream_t st)
{
    const size_t npix = (size_t)nimages * ga.H * ga.W;
    hipLaunchKernelGGL(k_wta_init, dim3(div_up((long long)npix, 256)), dim3(256), 0, st, h->keys, h->d1, npix, invalid_disp(ga));
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

// ---- stage 2: aggregation (stages "scan", "scan_last"; the caller has marked ST_SCAN) ---------------------------------
static int run_aggregation(camd_sgbm* h, int batch, int path, hipStream_t st)
{
    const Geom& g = h->g;
    const bool way3 = g.mode == CAMD_MODE_SGBM_3WAY;
    const int vbatch = batch * h->cr.n;
    if (path == CAMD_PATH_BAND && way3) {
        // the stripes are independent "virtual pairs": -> and v in one band pass, <- by the row-parallel pass
        if (way3_inline(h)) CAMD_TRY(launch_wta_init(h, h->ga, vbatch, st));
        CAMD_TRY(launch_band(h, +1, +1, true, 0, vbatch, st, false));
        CAMD_TRY(mark(h, ST_SCAN2, st));
        if (way3_inline(h)) CAMD_TRY(launch_band(h, -1, +1, false, 2, vbatch, st, true, h->way3_simd_lanes == 8));
        else CAMD_TRY(launch_band(h, -1, +1, false, 1, vbatch, st));
    } else if (path == CAMD_PATH_BAND) {
        // fused passes: every pass reads C once and touches S once for up to four directions
        if (h->phases & 2) {
            CAMD_TRY(launch_wta_init(h, g, batch, st));
            CAMD_TRY(launch_band(h, +1, +1, true, 0, batch, st, g.mode != CAMD_MODE_HH4));             // ->  v  [\.  ./]
        }
        CAMD_TRY(mark(h, ST_SCAN2, st));
        if (stops_before_last_pass(h, path)) return CAMD_OK;
        if (g.mode == CAMD_MODE_HH4) CAMD_TRY(launch_band(h, -1, -1, true, 2, batch, st, false));     // <-  ^ + WTA
        else if (g.mode == CAMD_MODE_HH) CAMD_TRY(launch_band(h, -1, -1, true, 2, batch, st));        // <-  ^  \^  /^ + WTA
        else CAMD_TRY(launch_band(h, -1, +1, false, 2, batch, st));                                   // <- + WTA
    } else {
        static const int dirs4[4][2] = {{1, 0}, {0, 1}, {-1, 0}, {0, -1}};  // MODE_SGBM_3WAY = the first three
        const int (*dirs)[2] = (g.mode == CAMD_MODE_HH4 || way3) ? dirs4 : kDirs8;
        if (path == CAMD_PATH_CONCURRENT) {
            CAMD_TRY(launch_scan<true>(h, dirs, g.npaths, h->Smulti, (size_t)h->smulti_cap * h->vol_elems, batch, st));
        } else {
            for (int i = 0; i < g.npaths; i++)
                CAMD_TRY(i == 0 ? launch_scan<true>(h, dirs + i, 1, h->S, 0, vbatch, st)
                                : launch_scan<false>(h, dirs + i, 1, h->S, 0, vbatch, st));
        }
        CAMD_TRY(mark(h, ST_SCAN2, st));  // (no separate last pass on the scan paths: zero-length stage)
    }
    return CAMD_OK;
}

// Volumes flagged as outside the u16 regime are aggregated again in int arithmetic (one launch for the batch that
// returns at once when nothing is flagged) and their raw disparities replaced; without that workspace they are
// written as invalid and reported.
static int redo_flagged(camd_sgbm* h, int16_t* dst, size_t stride_e, size_t n_e, int nvolumes, hipStream_t st)
{
    if (!h->may_overflow) return CAMD_OK;
    if (h->exact_cap) return launch_exact(h, nvolumes, dst, stride_e, n_e, st);
    hipLaunchKernelGGL(k_poison_flagged, dim3(64, nvolumes), dim3(256), 0, st, dst, stride_e, n_e, h->cost_neg, h->err,
                       invalid_disp(h->g));
    CAMD_LAUNCH_CHECK();
    CAMD_HIP(hipMemcpyAsync(h->err_host, h->err, 4, hipMemcpyDeviceToHost, st));
    return CAMD_OK;
}

static int launch_lrcheck(camd_sgbm* h, const Geom& ga, int16_t* out, size_t stride_e, int nimages, hipStream_t st)
{
    hipLaunchKernelGGL(k_lrcheck, dim3(div_up(div_up(ga.W, 2), 256), div_up(ga.H, LRCHECK_ROWS), nimages), dim3(256), 0, st, h->d1,
                       h->keys, out, (size_t)ga.W, stride_e, ga, h->err);
    CAMD_LAUNCH_CHECK();
    return CAMD_OK;
}

// ---- stage 3: the raw disparity of every pair in h->raw (stage "wta"; the caller has marked ST_WTA) -------------------
static int run_winners(camd_sgbm* h, int batch, int path, hipStream_t st)
{
    const Geom& g = h->g;
    const bool band = path == CAMD_PATH_BAND;
    if (g.mode == CAMD_MODE_SGBM_3WAY) {
        // winner-take-all + LR check per stripe row, then every image row is taken from the stripe that owns it
        const int vbatch = batch * h->cr.n;
        if (band && way3_inline(h)) CAMD_TRY(launch_lrcheck(h, h->ga, h->rawv, h->rawv_stride, vbatch, st));
        else CAMD_TRY(launch_wta(h, h->S, 1, 0, h->rawv, (size_t)g.W, h->rawv_stride, vbatch, st));
        CAMD_TRY(redo_flagged(h, h->rawv, h->rawv_stride, (size_t)h->ga.H * g.W, vbatch, st));
        hipLaunchKernelGGL(k_gather_stripes, dim3(div_up(g.W, 256), g.H, batch), dim3(256), 0, st, h->rawv, h->rawv_stride,
                           h->raw, h->raw_stride, g.W, g.H, h->stripe_sz, h->cr, band ? h->err : nullptr,
                           (h->may_overflow && !h->exact_cap) ? h->cost_neg : nullptr, invalid_disp(g));
        CAMD_LAUNCH_CHECK();
        if (band) CAMD_HIP(hipMemcpyAsync(h->err_host, h->err, 4, hipMemcpyDeviceToHost, st));
        return CAMD_OK;
    }
    if (band) {
        CAMD_TRY(launch_lrcheck(h, g, h->raw, h->raw_stride, batch, st));
        CAMD_HIP(hipMemcpyAsync(h->err_host, h->err, 4, hipMemcpyDeviceToHost, st));
    } else if (path == CAMD_PATH_CONCURRENT) {
        CAMD_TRY(launch_wta(h, h->Smulti, g.npaths, (size_t)h->smulti_cap * h->vol_elems, h->raw, (size_t)g.W, h->raw_stride, batch, st));
    } else {
        CAMD_TRY(launch_wta(h, h->S, 1, 0, h->raw, (size_t)g.W, h->raw_stride, batch, st));
    }
    return redo_flagged(h, h->raw, h->raw_stride, (size_t)g.H * g.W, batch, st);
}

// ---- stage 4: median and speckle filter into the caller's image (stages "median", "speckle"; ST_POST is marked) -------
static int run_post(camd_sgbm* h, int16_t* disp, size_t dpe, size_t dse, int batch, hipStream_t st)
{
    const Geom& g = h->g;
    CAMD_TRY(launch_median3(h->raw, g.W, h->raw_stride, disp, dpe, dse, g.W, g.H, batch, st));
    CAMD_TRY(mark(h, ST_SPECKLE, st));
    if (g.speckleWindowSize > 0) {
        // the "workspace is clean" invariant is established by the previous call's k_cc_apply, in stream order: a call
        // on another stream is not ordered behind it, so it clears the workspace itself (on its own stream)
        if (h->speckle_stream != st) { h->speckle_clean = false; h->speckle_stream = st; }
        CAMD_TRY(launch_speckle(disp, dpe, dse, g.W, g.H, invalid_disp(g), g.speckleWindowSize, 16 * g.speckleRange,
                                h->speckle_ws, h->speckle_bytes, batch, st, &h->speckle_clean));
    }
    return mark(h, ST_COUNT, st);
}

}  // namespace camd

using namespace camd;

extern "C" {

size_t camd_sgbm_workspace_bytes(const camd_sgbm_params* p, int width, int height, int channels,
                                 int max_batch)
{
    Geom g;
    WorkspacePlan w;
    if (normalise(p, width, height, channels, &g) != CAMD_OK || max_batch <= 0) return 0;
    if (plan_workspace(g, *p, max_batch, &w) != CAMD_OK) return 0;
    return w.C + w.S + w.rawv + w.raw + w.vol_flags + w.ticket + w.speckle + w.E + w.band_flags + w.keys + w.d1 + w.Smulti +
           w.Lx - w.ticket_unreported + w.rawv_unallocated;
}

int camd_sgbm_create(const camd_sgbm_params* p, int width, int height, int channels, int max_batch,
                     camd_sgbm** out)
{
    if (!out) { set_error("out is NULL"); return CAMD_ERR_BAD_ARG; }
    *out = nullptr;
    Geom g;
    int rc = normalise(p, width, height, channels, &g);
    if (rc != CAMD_OK) return rc;
    if (max_batch <= 0) { set_error("max_batch must be > 0"); return CAMD_ERR_BAD_ARG; }
    CAMD_NEED_DEVICE();
    WorkspacePlan w;
    rc = plan_workspace(g, *p, max_batch, &w);
    if (rc != CAMD_OK) return rc;
    if (g.mode == CAMD_MODE_SGBM_3WAY && 2 * g.SW2 + 1 > 11) {
        set_error("MODE_SGBM_3WAY is implemented for blockSize <= 11");
        return CAMD_ERR_UNSUPPORTED;
    }
    camd_sgbm* h = new (std::nothrow) camd_sgbm();
    if (!h) { set_error("out of host memory"); return CAMD_ERR_NOMEM; }
    memset(h, 0, sizeof(*h));
    h->g = g;
    h->params = *p;
    h->max_batch = max_batch;
    h->way3_simd_lanes = 8;
    h->cr = w.cr;
    h->stripe_sz = w.stripe_sz;
    h->ga = g;
    h->ga.H = w.vrows;
    h->vol_elems = w.vol_elems;
    h->raw_stride = w.raw_stride;
    h->rawv_stride = w.rawv_stride;
    h->speckle_bytes = w.speckle;
    h->may_overflow = w.may_overflow;
    h->band_ok = w.band_ok;
    h->nbands = w.nbands;
    h->nchunks = w.nchunks;
    h->erec_stride = w.erec_stride;
    h->path = 0;
    h->saturate = 1;
    h->phases = 7;
    h->epoch = 0;
    h->persist_cost = h->persist_row = 0;
    hipError_t e = hipSuccess;
    auto alloc = [&e](auto** ptr, size_t bytes) {  // (a buffer the plan sizes at 0 is not needed)
        if (e == hipSuccess && bytes) e = hipMalloc((void**)ptr, bytes);
    };
    alloc(&h->C, w.C);
    // the padded disparities d >= D of C hold P2 from here on: k_cost's all-padding waves do not write (sgbm_cost.hpp)
    // (complete before the handle is handed out: the first compute may run on a stream the null stream does not order)
    // Only a padded layout has such waves.  The fill runs on a stream of its own and only that stream is waited
    // for: no device-wide synchronisation, other streams keep running.
    if (e == hipSuccess && w.C && g.Dp != g.D) {
        hipStream_t fs = nullptr;
        e = hipStreamCreateWithFlags(&fs, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipMemsetD16Async(h->C, (unsigned short)g.P2, w.C / 2, fs);
        if (e == hipSuccess) e = hipStreamSynchronize(fs);
        if (fs) (void)hipStreamDestroy(fs);
    }
    // (S shifted against C by 256 B ... 1 MB so that the two streams of a pass do not touch the same offsets at the same
    // time: no difference, profiles/r06_s_offset.txt)
    alloc(&h->S, w.S);
    alloc(&h->rawv, w.rawv);
    alloc(&h->raw, w.raw);
    alloc(&h->cost_ovf, w.vol_flags);
    h->cost_neg = h->cost_ovf ? h->cost_ovf + w.vol_flags / 8 : nullptr;
    if (e == hipSuccess) e = hipMemset(h->cost_ovf, 0, w.vol_flags);
    alloc(&h->ticket, w.ticket);
    if (e == hipSuccess) e = hipMemset(h->ticket, 0, w.ticket);
    h->err = h->ticket ? h->ticket + 1 : nullptr;
    h->xbar = h->ticket ? h->ticket + 2 : nullptr;  // (ticket[3]: k_cost_persist's item counter)
    {
        int dev = 0, ncu = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess)
            h->num_cus = ncu;
        else
            (void)hipGetLastError();
    }
    if (e == hipSuccess) e = hipHostMalloc((void**)&h->err_host, 4, hipHostMallocDefault);
    if (e == hipSuccess) *h->err_host = 0;
    alloc(&h->speckle_ws, w.speckle);
    alloc(&h->E, w.E);
    alloc(&h->flags, w.band_flags);
    alloc(&h->keys, w.keys);
    alloc(&h->d1, w.d1);
    if (e == hipSuccess && w.band_flags) e = hipMemset(h->flags, 0, w.band_flags);
    // per-direction volumes, allocated last and allowed to fail: the latency path then has fewer pairs (or none: the
    // sequential scans take over), and without the one set the exact aggregation needs a flagged volume is refused
    // loudly (k_poison_flagged) instead
    if (e == hipSuccess) {
        int cap = w.smulti_cap;
        while (cap > 0) {
            if (hipMalloc((void**)&h->Smulti, smulti_bytes(g, h->vol_elems, cap)) == hipSuccess) break;
            (void)hipGetLastError();
            h->Smulti = nullptr;
            cap /= 2;
        }
        h->smulti_cap = cap;
        if (w.Lx) {
            if (hipMalloc((void**)&h->Lx, w.Lx) == hipSuccess) h->exact_cap = 1;
            else { (void)hipGetLastError(); h->Lx = nullptr; }
        }
    }
    if (e != hipSuccess) {
        set_error("workspace allocation failed: %s", hipGetErrorString(e));
        camd_sgbm_destroy(h);
        return e == hipErrorOutOfMemory ? CAMD_ERR_NOMEM : CAMD_ERR_HIP;
    }
    *out = h;
    return CAMD_OK;
}

// what the bits of the device-side error word mean (camd_sgbm_status / the next compute report them)
static const char* device_error_text(uint32_t e)
{
    static const char* kRefused =
        "a cost volume left the int16 regime of the aggregation kernels (values below P2 after an overflow of the box "
        "sums) and the handle has no workspace for the exact path; the disparities of that pair were written as invalid";
    static const char* kTimeout =
        "a band-wavefront pass timed out waiting for its upstream band; the disparities of that call were written as "
        "invalid";
    static const char* kBoth =
        "a band-wavefront pass timed out waiting for its upstream band (the disparities of that call were written as "
        "invalid) AND a cost volume left the int16 regime of the aggregation kernels with no workspace for the exact "
        "path (that pair was written as invalid)";
    static const char* kBarrier =
        "the exact int path's grid barrier timed out (its workgroups were not all resident at once -- e.g. on a stream "
        "restricted to few compute units while other kernels held them); the disparities of the flagged pairs were written "
        "as invalid";
    if (e & 4u) return kBarrier;
    return (e & 3u) == 3u ? kBoth : ((e & 2u) ? kRefused : kTimeout);
}

int camd_sgbm_destroy(camd_sgbm* h)
{
    if (!h) return CAMD_OK;
    if (h->ev_ok)
        for (int i = 0; i <= ST_COUNT; i++) (void)hipEventDestroy(h->ev[i]);
    (void)hipFree(h->C); (void)hipFree(h->S);
    (void)hipFree(h->raw); (void)hipFree(h->rawv); (void)hipFree(h->speckle_ws); (void)hipFree(h->cost_ovf);
    (void)hipFree(h->E); (void)hipFree(h->flags); (void)hipFree(h->ticket); (void)hipFree(h->keys);
    (void)hipFree(h->d1); (void)hipFree(h->Smulti); (void)hipFree(h->Lx);
    if (h->err_host) (void)hipHostFree(h->err_host);
    delete h;
    return CAMD_OK;
}

int camd_sgbm_query(const camd_sgbm* h, int* width1, int* D, int* Dp, int* minX1)
{
    if (!h) { set_error("handle is NULL"); return CAMD_ERR_BAD_ARG; }
    if (width1) *width1 = h->g.W1;
    if (D) *D = h->g.D;
    if (Dp) *Dp = h->g.Dp;
    if (minX1) *minX1 = h->g.minX1;
    return CAMD_OK;
}

int camd_sgbm_set_option(camd_sgbm* h, int option, int value)
{
    if (!h) { set_error("handle is NULL"); return CAMD_ERR_BAD_ARG; }
    if (option == CAMD_OPT_PATH && value >= CAMD_PATH_AUTO && value <= CAMD_PATH_CONCURRENT) {
        if (value == CAMD_PATH_CONCURRENT && h->g.W1 > 0) {
            // an explicit request may exceed what AUTO would use: grow the per-direction volumes here (an init-time
            // call), never inside the stream-ordered compute
            const int want = h->max_batch < CAMD_MULTI_MAX_BATCH ? h->max_batch : CAMD_MULTI_MAX_BATCH;
            if (want > h->smulti_cap) {
                CAMD_HIP(hipDeviceSynchronize());
                (void)hipFree(h->Smulti);
                h->Smulti = nullptr;
                h->smulti_cap = 0;
                hipError_t e = hipMalloc((void**)&h->Smulti, smulti_bytes(h->g, h->vol_elems, want));
                if (e != hipSuccess) {
                    (void)hipGetLastError();
                    set_error("no memory for %d x %d per-direction volumes", h->g.npaths, want);
                    return CAMD_ERR_NOMEM;
                }
                h->smulti_cap = want;
            }
        }
        h->path = value;
    }
    else if (option == CAMD_OPT_KEEP_S) h->keep_S = value != 0;
    else if (option == CAMD_OPT_COST && value >= CAMD_COST_AUTO && value <= CAMD_COST_SPLIT) h->cost_path = value;
    else if (option == CAMD_OPT_SATURATE) h->saturate = value != 0;
    else if (option == CAMD_OPT_3WAY_SIMD_LANES && (value == 1 || value == 8)) h->way3_simd_lanes = value;
    else if (option == CAMD_OPT_PHASES && value >= 1 && value <= 7) h->phases = value;
    else if (option == CAMD_OPT_RESIDENT && value >= 0 && (value >> 4) <= 4 && (value & 15) <= 4) {
        h->persist_cost = value >> 4;
        h->persist_row = value & 15;
    }
    else if (option == CAMD_OPT_EXACT) {
        if (value != 0 && !h->Lx && h->may_overflow) {
            // the workspace could not be had when the handle was made: try again rather than stay in refuse mode silently
            if (hipMalloc((void**)&h->Lx, lx_bytes(h->g, h->vol_elems)) != hipSuccess) {
                (void)hipGetLastError();
                h->Lx = nullptr;
                set_error("no memory for the exact path's %d per-direction int volumes; the handle keeps refusing flagged pairs",
                          h->g.npaths);
                return CAMD_ERR_NOMEM;
            }
        }
        h->exact_cap = (value != 0 && h->Lx) ? 1 : 0;
    }
    else { set_error("unknown option %d / value %d", option, value); return CAMD_ERR_BAD_ARG; }
    return CAMD_OK;
}

int camd_sgbm_status(camd_sgbm* h, void* stream)
{
    if (!h) { set_error("handle is NULL"); return CAMD_ERR_BAD_ARG; }
    if (!h->err) return CAMD_OK;
    uint32_t e = 0;
    CAMD_HIP(hipMemcpyAsync(&e, h->err, 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
    CAMD_HIP(hipStreamSynchronize((hipStream_t)stream));
    if (e) {
        CAMD_HIP(hipMemsetAsync(h->err, 0, 4, (hipStream_t)stream));
        if (h->err_host) *(volatile uint32_t*)h->err_host = 0;
        set_error("%s", device_error_text(e));
        return CAMD_ERR_HIP;
    }
    return CAMD_OK;
}

int camd_sgbm_set_profiling(camd_sgbm* h, int enable)
{
    if (!h) { set_error("handle is NULL"); return CAMD_ERR_BAD_ARG; }
    if (enable && !h->ev_ok) {
        for (int i = 0; i <= ST_COUNT; i++) CAMD_HIP(hipEventCreate(&h->ev[i]));
        h->ev_ok = true;
    }
    h->profiling = enable != 0;
    return CAMD_OK;
}
int camd_sgbm_num_stages(void) { return ST_COUNT; }
const char* camd_sgbm_stage_name(int i) { return i >= 0 && i < ST_COUNT ? kStageNames[i] : ""; }
int camd_sgbm_get_profile(camd_sgbm* h, float* ms, int n)
{
    if (!h || !ms) { set_error("NULL argument"); return CAMD_ERR_BAD_ARG; }
    if (!h->ev_ok || !h->profiling) { set_error("profiling not enabled"); return CAMD_ERR_BAD_ARG; }
    CAMD_HIP(hipEventSynchronize(h->ev[ST_COUNT]));
    for (int i = 0; i < n && i < ST_COUNT; i++) CAMD_HIP(hipEventElapsedTime(&ms[i], h->ev[i], h->ev[i + 1]));
    return CAMD_OK;
}

int camd_sgbm_compute(camd_sgbm* h, const uint8_t* left, const uint8_t* right, size_t pitch,
                      size_t image_stride, int16_t* disp, size_t disp_pitch, size_t disp_stride,
                      int batch, void* stream)
{
    if (!h || !left || !right || !disp) { set_error("NULL argument"); return CAMD_ERR_BAD_ARG; }
    const Geom& g = h->g;
    if (batch <= 0 || batch > h->max_batch) {
        set_error("batch %d outside [1, max_batch=%d]", batch, h->max_batch);
        return CAMD_ERR_BAD_ARG;
    }
    if (pitch < (size_t)g.W * g.cn || disp_pitch < (size_t)g.W * 2 || (disp_pitch & 1) || (disp_stride & 1)) {
        set_error("pitch too small or odd disparity pitch");
        return CAMD_ERR_BAD_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    // A device-side bounded wait that expired in an EARLIER call (its result was written as all-invalid by
    // k_lrcheck) is reported here without a synchronisation: the flag travels through a pinned mirror that an
    // async copy refreshes at the end of every band-path compute.
    if (h->err_host && *(volatile uint32_t*)h->err_host) {
        const uint32_t e = *(volatile uint32_t*)h->err_host;
        *(volatile uint32_t*)h->err_host = 0;
        CAMD_HIP(hipMemsetAsync(h->err, 0, 4, st));
        set_error("in an earlier compute on this handle: %s", device_error_text(e));
        return CAMD_ERR_HIP;
    }
    const size_t dpe = disp_pitch / 2, dse = disp_stride / 2;
    h->last_batch = batch;
    if (g.W1 <= 0) {
        // minX1 >= maxX1: everything is INVALID_DISP_SCALED; the median of a constant is the constant
        hipLaunchKernelGGL(k_fill_s16, dim3(div_up(g.W, 256), g.H, batch), dim3(256), 0, st, disp, dpe, dse,
                           g.W, g.H, invalid_disp(g));
        CAMD_LAUNCH_CHECK();
        return CAMD_OK;
    }

    CAMD_TRY(mark(h, ST_COST, st));
    CAMD_TRY(run_cost(h, left, right, pitch, image_stride, batch, st));
    // CAMD_OPT_PHASES: the caller runs the aggregation in a second call (another stream)
    if (!(h->phases & 6)) return mark_rest(h, ST_SCAN, st);
    const int path = choose_path(h, batch);
    CAMD_TRY(mark(h, ST_SCAN, st));
    CAMD_TRY(run_aggregation(h, batch, path, st));
    if (stops_before_last_pass(h, path)) return mark_rest(h, ST_WTA, st);
    CAMD_TRY(mark(h, ST_WTA, st));
    CAMD_TRY(run_winners(h, batch, path, st));
    CAMD_TRY(mark(h, ST_POST, st));
    return run_post(h, disp, dpe, dse, batch, st);
}

int camd_sgbm_debug_copy(camd_sgbm* h, int which, int index, void* dst, void* stream)
{
    if (!h || !dst) { set_error("NULL argument"); return CAMD_ERR_BAD_ARG; }
    if (index < 0 || index >= h->max_batch) { set_error("index out of range"); return CAMD_ERR_BAD_ARG; }
    const Geom& g = h->g;
    hipStream_t st = (hipStream_t)stream;
    if (which == 0 || which == 1) {
        if (g.mode == CAMD_MODE_SGBM_3WAY) {
            set_error("MODE_SGBM_3WAY keeps its volumes per stripe: only which = 2 (raw disparity) is available");
            return CAMD_ERR_UNSUPPORTED;
        }
        if (g.W1 <= 0) return CAMD_OK;
        const uint16_t* src = (which == 0 ? h->C : h->S) + (size_t)index * h->vol_elems;
        CAMD_HIP(hipMemcpyAsync(dst, src, (size_t)g.H * g.W1 * g.Dp * 2, hipMemcpyDeviceToDevice, st));
    } else if (which == 2) {
        CAMD_HIP(hipMemcpyAsync(dst, h->raw + (size_t)index * h->raw_stride, (size_t)g.H * g.W * 2,
                                hipMemcpyDeviceToDevice, st));
    } else {
        set_error("which must be 0 (C), 1 (S) or 2 (raw disparity)");
        return CAMD_ERR_BAD_ARG;
    }
    return CAMD_OK;
}

}  // extern "C"
