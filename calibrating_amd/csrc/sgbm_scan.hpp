// sgbm_scan.hpp -- the line-scan path (the latency path, and the generic fallback): how a lane moves its slice of a
// disparity vector (RegVec, ld_regs / st_regs, their LDS forms: shared with sgbm_band.hpp and sgbm_exact.hpp), k_scan = one
// aggregation direction as independent line scans, k_wta = winner-take-all + left-right check per row, and the two
// small kernels beside them.  Included by sgbm.hip (shares Geom, CostRanges, SENT_PK).
#pragma once

namespace camd {

// ------------------------------------------------------------------------------------------------
// k_scan: L_r along direction r = (dx, dy) for every line of the cost array, accumulated into S.
//   L(p,d) = C(p,d) + min(Lp[d], Lp[d-1]+P1, Lp[d+1]+P1, minLp+P2) - (minLp+P2),  Lp = L(p-r,.)
//   Lp = 0, minLp = 0 outside the array; Lp[-1] = Lp[D] = MAX_COST.
// A line is owned by LANES lanes; lane l holds d in [l*2*NR, (l+1)*2*NR) as NR packed u16 pairs.
// All arithmetic is u16: real values are in [0, 32767], MAX_COST + P1 does not wrap, and the final
// (C + m) - delta is exact modulo 2^16 (OpenCV's (CostType) cast).
// ------------------------------------------------------------------------------------------------
// directions of one launch: blockIdx.z selects the entry; with more than one entry every direction
// writes its own volume (Sv + z * dir_stride, FIRST only) so that all of them run concurrently
// ---- a lane's slice of a pixel's disparity vector: NR packed registers = 2*NR consecutive disparities = 4*NR bytes,
// 4-byte aligned (16-byte aligned, and moved as uint4, when NR % 4 == 0).  In LDS a lane's slice takes NQ = ceil(NR/4)
// 16-byte slots, the tail zero (lds_ld_regs / lds_st_regs below).
template <int NR> struct __attribute__((packed, aligned(4))) RegVec { uint32_t v[NR]; };
template <int NR>
__device__ __forceinline__ void ld_regs(const uint16_t* __restrict__ p, uint32_t (&dst)[NR])
{
    if constexpr (NR % 4 == 0) {
        const uint4* q = reinterpret_cast<const uint4*>(p);
#pragma unroll
        for (int v = 0; v < NR / 4; v++) {
            const uint4 w = q[v];
            dst[4 * v] = w.x; dst[4 * v + 1] = w.y; dst[4 * v + 2] = w.z; dst[4 * v + 3] = w.w;
        }
    } else {
        RegVec<NR> t;
        __builtin_memcpy(&t, p, sizeof(t));
#pragma unroll
        for (int k = 0; k < NR; k++) dst[k] = t.v[k];
    }
}
template <int NR>
__device__ __forceinline__ void st_regs(uint16_t* __restrict__ p, const uint32_t (&src)[NR])
{
    if constexpr (NR % 4 == 0) {
        uint4* q = reinterpret_cast<uint4*>(p);
#pragma unroll
        for (int v = 0; v < NR / 4; v++) q[v] = make_uint4(src[4 * v], src[4 * v + 1], src[4 * v + 2], src[4 * v + 3]);
    } else {
        RegVec<NR> t;
#pragma unroll
        for (int k = 0; k < NR; k++) t.v[k] = src[k];
        __builtin_memcpy(p, &t, sizeof(t));
    }
}
// streaming variants (global_load / global_store ... nt): the volumes are read and written once per pass.  Measured on the
// band passes (CAMD_BAND_NT, tools/history/gpu_r6_nt.sh) -- see sgbm_band.hpp
typedef uint32_t nt_u32x4 __attribute__((ext_vector_type(4)));
template <int NR>
__device__ __forceinline__ void ld_regs_nt(const uint16_t* __restrict__ p, uint32_t (&dst)[NR])
{
    if constexpr (NR % 4 == 0) {
        const nt_u32x4* q = reinterpret_cast<const nt_u32x4*>(p);
#pragma unroll
        for (int v = 0; v < NR / 4; v++) {
            const nt_u32x4 w = __builtin_nontemporal_load(q + v);
            dst[4 * v] = w.x; dst[4 * v + 1] = w.y; dst[4 * v + 2] = w.z; dst[4 * v + 3] = w.w;
        }
    } else {
        ld_regs<NR>(p, dst);
    }
}
template <int NR>
__device__ __forceinline__ void st_regs_nt(uint16_t* __restrict__ p, const uint32_t (&src)[NR])
{
    if constexpr (NR % 4 == 0) {
        nt_u32x4* q = reinterpret_cast<nt_u32x4*>(p);
#pragma unroll
        for (int v = 0; v < NR / 4; v++)
            __builtin_nontemporal_store(nt_u32x4{src[4 * v], src[4 * v + 1], src[4 * v + 2], src[4 * v + 3]}, q + v);
    } else {
        st_regs<NR>(p, src);
    }
}
// (k_scan / k_wta keep plain loads: with `nt` one 1080p pair took 1.89-1.90 instead of 1.79-1.88 ms -- the direction scans of ONE
// pair read the same C concurrently and want the L2 / MALL reuse; the band-pass series is profiles/r06_band_nt.txt)
template <int NR> __device__ __forceinline__ uint32_t reg_or0(const uint32_t (&a)[NR], int i) { return i < NR ? a[i < NR ? i : 0] : 0u; }
// LDS: slot v of lane `idx` lives at p[v * stride + idx] -- one PLANE per slot, so that consecutive lanes are 16 bytes
// apart in every ds_read_b128 / ds_write_b128 (lane-major slots, p[idx * NQ + v], put the lanes 32 bytes apart at
// NQ = 2: two-way bank conflicts in every exchange of the D > 128 band passes, 44 % of their LDS cycles in round 4)
template <int NR>
__device__ __forceinline__ void lds_ld_regs(const uint4* p, int idx, int stride, uint32_t (&dst)[NR])
{
#pragma unroll
    for (int v = 0; v < (NR + 3) / 4; v++) {
        const uint4 w = p[v * stride + idx];
        const uint32_t e[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (4 * v + k < NR) dst[4 * v + k] = e[k];
    }
}
template <int NR>
__device__ __forceinline__ void lds_st_regs(uint4* p, int idx, int stride, const uint32_t (&src)[NR])
{
#pragma unroll
    for (int v = 0; v < (NR + 3) / 4; v++)
        p[v * stride + idx] = make_uint4(reg_or0<NR>(src, 4 * v), reg_or0<NR>(src, 4 * v + 1), reg_or0<NR>(src, 4 * v + 2),
                                         reg_or0<NR>(src, 4 * v + 3));
}

struct ScanDirs {
    int dx[8], dy[8], nlines[8];
    size_t dir_stride;
};

template <int LANES, int NR, bool FIRST, bool PAD>
__global__ __launch_bounds__(256) void k_scan(const uint16_t* __restrict__ Cv, uint16_t* __restrict__ Sbase,
                                              Geom g, ScanDirs sd, size_t vol_stride)
{
    const int dx = sd.dx[blockIdx.z], dy = sd.dy[blockIdx.z], nlines = sd.nlines[blockIdx.z];
    uint16_t* __restrict__ Sv = Sbase + (size_t)blockIdx.z * sd.dir_stride;
    const int tid = blockIdx.x * 256 + threadIdx.x;
    const int line = tid / LANES, li = tid % LANES;
    if (line >= nlines) return;
    const int pair = blockIdx.y;
    const int W1 = g.W1, H = g.H;

    // start pixel and length of this line
    int x0, y0;
    if (dy == 0) {
        y0 = line;
        x0 = dx > 0 ? 0 : W1 - 1;
    } else {
        const int ys = dy > 0 ? 0 : H - 1;
        if (dx == 0 || line < W1) {
            x0 = line;
            y0 = ys;
        } else {
            x0 = dx > 0 ? 0 : W1 - 1;
            int k = line - W1 + 1;  // 1..H-1
            y0 = dy > 0 ? k : H - 1 - k;
        }
    }
    int len;
    {
        int lx = dx == 0 ? (1 << 30) : (dx > 0 ? W1 - x0 : x0 + 1);
        int ly = dy == 0 ? (1 << 30) : (dy > 0 ? H - y0 : y0 + 1);
        len = min(lx, ly);
    }
    const size_t off = (size_t)pair * vol_stride + ((size_t)y0 * W1 + x0) * g.Dp + (size_t)li * (2 * NR);
    const ptrdiff_t step = ((ptrdiff_t)dy * W1 + dx) * (ptrdiff_t)g.Dp;
    const uint16_t* cp = Cv + off;
    uint16_t* sp = Sv + off;

    uint32_t keep[NR], sent[NR];
    if (PAD) {
#pragma unroll
        for (int k = 0; k < NR; k++) {
            int d0 = li * 2 * NR + 2 * k;
            uint32_t kp = (d0 < g.D ? 0xffffu : 0u) | (d0 + 1 < g.D ? 0xffff0000u : 0u);
            keep[k] = kp;
            sent[k] = ~kp & SENT_PK;
        }
    }

    const uint32_t P1pk = dup16((uint32_t)g.P1), P2pk = dup16((uint32_t)g.P2);
    uint32_t Lp[NR];
#pragma unroll
    for (int k = 0; k < NR; k++) Lp[k] = 0;
    uint32_t delta = P2pk;  // minLp = 0
    uint32_t edge_lo = SENT_PK, edge_hi = SENT_PK;

    // A line is a dependent chain (every pixel needs the previous one), so with one pair per call the kernel is
    // latency-bound: the C (and S) vectors of the next PF-1 pixels are kept in flight in a register ring.  The
    // loop is unrolled by PF so the ring never moves, and the loads are unconditional (clamped to the line's last
    // pixel) so that the compiler can wait with counted vmcnt(N) instead of draining the ring every step.
    constexpr int PF = NR <= 4 ? 8 : (NR <= 8 ? 4 : 2);
    uint32_t cr[PF][NR], sr[FIRST ? 1 : PF][NR];
#pragma unroll
    for (int u = 0; u < PF - 1; u++) {
        const ptrdiff_t o = (ptrdiff_t)min(u, len - 1) * step;
        ld_regs<NR>(cp + o, cr[u]);
        if (!FIRST) ld_regs<NR>(sp + o, sr[u]);
    }
    for (int i0 = 0; i0 < len; i0 += PF) {
#pragma unroll
        for (int u = 0; u < PF; u++) {
            const int i = i0 + u;
            {
                const ptrdiff_t o = (ptrdiff_t)min(i + PF - 1, len - 1) * step;
                ld_regs<NR>(cp + o, cr[(u + PF - 1) % PF]);
                if (!FIRST) ld_regs<NR>(sp + o, sr[(u + PF - 1) % PF]);
            }
            if (i < len) {
                const uint32_t(&c)[NR] = cr[u];
                // neighbours across lanes: d-1 of my first element, d+1 of my last element
                // (edge_lo / edge_hi persist: the lane a row shift leaves untouched keeps its MAX_COST sentinel)
                edge_lo = dpp_mov<DPP_ROW_SHR1>(edge_lo, Lp[NR - 1]);
                edge_hi = dpp_mov<DPP_ROW_SHL1>(edge_hi, Lp[0]);
                uint32_t prev_last = edge_lo, next_first = edge_hi;
                if (LANES < 16) {
                    if (li == 0) prev_last = SENT_PK;
                    if (li == LANES - 1) next_first = SENT_PK;
                }
                // m[k] = (Lp[2k-1], Lp[2k]) ; m[k+1] = (Lp[2k+1], Lp[2k+2])
                uint32_t m[NR + 1];
                m[0] = alignbit16(Lp[0], prev_last);
#pragma unroll
                for (int k = 1; k < NR; k++) m[k] = alignbit16(Lp[k], Lp[k - 1]);
                m[NR] = alignbit16(next_first, Lp[NR - 1]);

                uint32_t L[NR];
                uint32_t mn = SENT_PK;
#pragma unroll
                for (int k = 0; k < NR; k++) {
                    // C + min(Lp, t, delta) - delta  ==  C - max(delta - min(Lp, t), 0)   (mod 2^16): one op less
                    uint32_t t = pk_add_u16(pk_min_u16(m[k], m[k + 1]), P1pk);
                    uint32_t l = pk_sub_u16(c[k], pk_subsat_u16(delta, pk_min_u16(Lp[k], t)));
                    if (PAD) l = (l & keep[k]) | sent[k];
                    L[k] = l;
                    mn = pk_min_u16(mn, l);
                }
                mn = group_min_pk_u16<LANES>(mn);
                mn = pk_min_u16(mn, alignbit16(mn, mn));  // both halves = min over all d
                delta = pk_add_u16(mn, P2pk);

                uint32_t s[NR];
#pragma unroll
                for (int k = 0; k < NR; k++) {
                    s[k] = FIRST ? L[k] : pk_addsat_i16(sr[FIRST ? 0 : u][k], L[k]);
                    Lp[k] = L[k];
                }
                st_regs<NR>(sp + (ptrdiff_t)i * step, s);
            }
        }
    }
}


// ------------------------------------------------------------------------------------------------
// k_wta: one workgroup per image row.  Per cost column x (a LANES-lane group each):
//   minS / bestDisp (smallest d attaining it), uniqueness test, sub-pixel parabola,
//   right-view map disp2 by LDS atomicMin on (minS << 16 | 0xFFFF - d)  [ties keep the larger d,
//   i.e. the larger x, which OpenCV visits first], then the left-right check of the row.
// ------------------------------------------------------------------------------------------------
static constexpr uint32_t KEY_INIT = 0x7fff0000u;

// EXACT (sgbm_exact.hpp): Sv points at nvol per-direction volumes of int L values (before narrowing); they are added
// up in OpenCV's grouping and with each mode's own narrowing -- combine 0: saturate(L0 + L1 + L2 + L3) of the int
// values, then saturate(that + the rest) (computeDisparitySGBM); 1: one saturating add per volume, in order, of
// (CostType)L (computeDisparitySGBM_HH4); 2: the same of saturate(L) (the 3-way loop) -- and every total is carried
// as S + 32768 in an unsigned half, so that all comparisons below order the same way; `bias` turns them back into
// values where the arithmetic needs them.
// (the body of k_wta for row y of pair `pair`; the persistent exact kernel of sgbm_exact.hpp calls it row after row)
template <int LANES, int NR, bool EXACT>
__device__ __forceinline__ void wta_row(const uint16_t* __restrict__ Sv, int16_t* __restrict__ disp,
                                        size_t disp_pitch_e, size_t disp_stride_e, const Geom& g,
                                        size_t vol_stride, int nvol, size_t dir_stride, int tie_lanes,
                                        int combine, int y, int pair)
{
    constexpr int bias = EXACT ? 32768 : 0;
    constexpr uint32_t key_init = EXACT ? 0xffff0000u : KEY_INIT;
    constexpr int max_cost_b = MAX_COST + bias;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t* keys = reinterpret_cast<uint32_t*>(smem);          // [W]
    int16_t* d1row = reinterpret_cast<int16_t*>(keys + g.W);     // [W]
    constexpr int GROUPS = 256 / LANES;
    const int li = threadIdx.x % LANES, grp = threadIdx.x / LANES;
    const int INVALID_SCALED = (g.minD - 1) * 16;

    for (int x = threadIdx.x; x < g.W; x += 256) {
        keys[x] = key_init;
        d1row[x] = (int16_t)INVALID_SCALED;
    }
    __syncthreads();

    const uint16_t* Srow = Sv + (size_t)pair * vol_stride + ((size_t)y * g.W1) * g.Dp + (size_t)li * (2 * NR);
    const int dbase = li * 2 * NR;
    for (int x = grp; x < g.W1; x += GROUPS) {
        uint32_t s[NR];
        if (!EXACT) {
            ld_regs<NR>(Srow + (size_t)x * g.Dp, s);
            // concurrent-direction path: S = saturating sum of the per-direction volumes
            for (int dv = 1; dv < nvol; dv++) {
                uint32_t q[NR];
                ld_regs<NR>(Srow + (size_t)dv * dir_stride + (size_t)x * g.Dp, q);
#pragma unroll
                for (int k = 0; k < NR; k++) s[k] = pk_addsat_i16(s[k], q[k]);
            }
        } else {
            // (dir_stride and the row offsets count int elements here)
            const int32_t* Lrow = reinterpret_cast<const int32_t*>(Sv) + ((size_t)y * g.W1 + x) * g.Dp + (size_t)li * (2 * NR);
            int tot[2 * NR], part[2 * NR];
#pragma unroll
            for (int e = 0; e < 2 * NR; e++) tot[e] = part[e] = 0;
            for (int dv = 0; dv <= nvol; dv++) {
                // close the running group before volume dv joins: after every volume in the sequential modes, at the
                // group boundary (after the first four volumes) and at the end in combine 0
                if (dv > 0 && (combine != 0 || dv == 4 || dv == nvol)) {
#pragma unroll
                    for (int e = 0; e < 2 * NR; e++) {
                        const int t = tot[e] + part[e];
                        tot[e] = t < -32768 ? -32768 : (t > 32767 ? 32767 : t);
                        part[e] = 0;
                    }
                }
                if (dv == nvol) break;
                const int2* pv = reinterpret_cast<const int2*>(Lrow + (size_t)dv * dir_stride);  // 8-byte aligned: li * 2NR ints
#pragma unroll
                for (int v = 0; v < NR; v++) {
                    const int2 q = pv[v];
                    const int w[2] = {q.x, q.y};
#pragma unroll
                    for (int k = 0; k < 2; k++) {
                        const int L = w[k];
                        part[2 * v + k] += combine == 0 ? L : (combine == 1 ? (int)(int16_t)L
                                                                             : (L < -32768 ? -32768 : (L > 32767 ? 32767 : L)));
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < NR; k++)
                s[k] = (uint32_t)(tot[2 * k] + bias) | ((uint32_t)(tot[2 * k + 1] + bias) << 16);
        }
        // (S << 16 | d) minimum: smallest S, then smallest d
        uint32_t key = 0xffffffffu;
#pragma unroll
        for (int k = 0; k < NR; k++) {
            int d0 = dbase + 2 * k;
            uint32_t lo = s[k] & 0xffffu, hi = s[k] >> 16;
            if (d0 < g.D) key = min(key, (lo << 16) | (uint32_t)d0);
            if (d0 + 1 < g.D) key = min(key, (hi << 16) | (uint32_t)(d0 + 1));
        }
        key = group_min_u32<LANES>(key);
        int minS = (int)(key >> 16), best = (int)(key & 0xffffu);
        if (NR % 4 == 0 && tie_lanes == 8) {  // (MODE_SGBM_3WAY keeps layouts of whole groups of 8 per lane: normalise())
            // MODE_SGBM_3WAY as OpenCV's CV_SIMD build decides ties (oracle/sgbm_ref.c way3_winner): the disparities
            // below E are scanned 8 at a time, every one of the 8 lane slots keeps the LAST d that attains its minimum,
            // the winner is the smallest of those positions among the slots that hold the global minimum; the scalar
            // tail [E, D) only wins with a strictly smaller total.  A lane owns whole groups of 8 consecutive d here, so
            // element e of every group is slot e.
            const int E = (g.D % 8 == 0) ? g.D : 8 * ((g.D - 1) / 8);
            uint32_t m1 = 0xffffu, ktail = 0xffffffffu;
#pragma unroll
            for (int k = 0; k < NR; k++) {
                const int d0 = dbase + 2 * k;
                const uint32_t lo = s[k] & 0xffffu, hi = s[k] >> 16;
                if (d0 < E) m1 = min(m1, lo); else if (d0 < g.D) ktail = min(ktail, (lo << 16) | (uint32_t)d0);
                if (d0 + 1 < E) m1 = min(m1, hi); else if (d0 + 1 < g.D) ktail = min(ktail, (hi << 16) | (uint32_t)(d0 + 1));
            }
            m1 = group_min_u32<LANES>(m1);
            ktail = group_min_u32<LANES>(ktail);
            uint32_t pos = 0xffffffffu;
#pragma unroll
            for (int e = 0; e < 8; e++) {
                uint32_t last = 0;  // 1 + the largest d of slot e (in this lane) whose total is the minimum
#pragma unroll
                for (int v = 0; v < NR / 4; v++) {
                    const int k = 4 * v + e / 2, d = dbase + 8 * v + e;
                    const uint32_t val = (e & 1) ? (s[k] >> 16) : (s[k] & 0xffffu);
                    if (d < E && val == m1) last = (uint32_t)d + 1;
                }
                last = group_max_u32<LANES>(last);
                if (last) pos = min(pos, last - 1);
            }
            if (E > 0 && (ktail >> 16) >= m1) { minS = (int)m1; best = (int)pos; }
            else { minS = (int)(ktail >> 16); best = (int)(ktail & 0xffffu); }
        }
        // uniqueness + the neighbours of the winner
        uint32_t flags = 0, sm = 0, spv = 0;
        const int thr = (minS - bias) * 100, mul = 100 - g.uniq;
#pragma unroll
        for (int k = 0; k < NR; k++) {
            int d0 = dbase + 2 * k;
            int lo = (int)(s[k] & 0xffffu) - bias, hi = (int)(s[k] >> 16) - bias;
            if (d0 < g.D) {
                if (lo * mul < thr && abs(best - d0) > 1) flags = 1;
                if (d0 == best - 1) sm = s[k] & 0xffffu;
                if (d0 == best + 1) spv = s[k] & 0xffffu;
            }
            if (d0 + 1 < g.D) {
                if (hi * mul < thr && abs(best - d0 - 1) > 1) flags = 1;
                if (d0 + 1 == best - 1) sm = s[k] >> 16;
                if (d0 + 1 == best + 1) spv = s[k] >> 16;
            }
        }
        // the two neighbours as 16-bit fields (each set by at most one lane; a field left at zero is never used)
        const uint32_t packed = group_or_u32<LANES>((sm << 16) | spv);
        flags = group_or_u32<LANES>(flags);
        if (li == 0 && minS < max_cost_b && !flags) {
            const int Sm = (int)(packed >> 16) - bias, Sp = (int)(packed & 0xffffu) - bias;
            int d = best;
            int x2 = x + g.minX1 - d - g.minD;
            atomicMin(&keys[x2], ((uint32_t)minS << 16) | (uint32_t)(0xffff - d));
            minS -= bias;
            if (0 < d && d < g.D - 1) {
                int denom2 = max(Sm + Sp - 2 * minS, 1);
                d = d * 16 + ((Sm - Sp) * 16 + denom2) / (denom2 * 2);  // C division truncates
            } else
                d *= 16;
            d1row[x + g.minX1] = (int16_t)(d + g.minD * 16);
        }
    }
    __syncthreads();

    int16_t* out = disp + (size_t)pair * disp_stride_e + (size_t)y * disp_pitch_e;
    const int maxX1 = g.minX1 + g.W1;
    for (int x = threadIdx.x; x < g.W; x += 256) {
        int d1 = d1row[x];
        if (x >= g.minX1 && x < maxX1 && d1 != INVALID_SCALED) {
            int _d = d1 >> 4, d_ = (d1 + 15) >> 4;
            int _x = x - _d, x_ = x - d_;
            bool bad = true;
            if (0 <= _x && _x < g.W) {
                uint32_t k = keys[_x];
                // untouched entries hold INVALID_DISP_SCALED and are compared unscaled (OpenCV quirk)
                int v = k == key_init ? INVALID_SCALED : (int)(0xffffu - (k & 0xffffu)) + g.minD;
                bad = v >= g.minD && abs(v - _d) > g.d12;
            } else
                bad = false;
            if (bad) {
                if (0 <= x_ && x_ < g.W) {
                    uint32_t k = keys[x_];
                    int v = k == key_init ? INVALID_SCALED : (int)(0xffffu - (k & 0xffffu)) + g.minD;
                    bad = v >= g.minD && abs(v - d_) > g.d12;
                } else
                    bad = false;
            }
            if (bad) d1 = INVALID_SCALED;
        }
        out[x] = (int16_t)d1;
    }
}

template <int LANES, int NR>
__global__ __launch_bounds__(256) void k_wta(const uint16_t* __restrict__ Sv, int16_t* __restrict__ disp,
                                             size_t disp_pitch_e, size_t disp_stride_e, Geom g,
                                             size_t vol_stride, int nvol, size_t dir_stride, int tie_lanes)
{
    wta_row<LANES, NR, false>(Sv, disp, disp_pitch_e, disp_stride_e, g, vol_stride, nvol, dir_stride, tie_lanes, 0,
                              (int)blockIdx.x, (int)blockIdx.y);
}

__global__ void k_fill_s16(int16_t* p, size_t pitch_e, size_t stride_e, int W, int H, int value)
{
    int x = blockIdx.x * 256 + threadIdx.x;
    if (x < W) p[(size_t)blockIdx.z * stride_e + (size_t)blockIdx.y * pitch_e + x] = (int16_t)value;
}

// MODE_SGBM_3WAY: rows of the final raw disparity come from the stripe that owns them
__global__ __launch_bounds__(256) void k_gather_stripes(const int16_t* __restrict__ rawv, size_t rawv_stride_e,
                                                        int16_t* __restrict__ raw, size_t raw_stride_e, int W, int H,
                                                        int stripe_sz, CostRanges cr, const uint32_t* __restrict__ err,
                                                        const uint32_t* __restrict__ refused, int invalid)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, pair = blockIdx.z;
    if (x >= W) return;
    const int s = min(y / stripe_sz, cr.n - 1);
    // a band pass that gave up waiting (sgbm_band.hpp) must not hand back plausible garbage: like k_lrcheck (bit 0 of
    // the error word); and a pair with ANY refused stripe (`refused`: the per-volume below-P2 flags, passed only when
    // there is no exact path to redo them) is invalid as a whole, as the header promises -- not just that stripe's rows
    bool bad = err && (*err & 1u);
    if (refused)
        for (int k = 0; k < cr.n; k++) bad |= refused[pair * cr.n + k] != 0;
    raw[(size_t)pair * raw_stride_e + (size_t)y * W + x] =
        bad ? (int16_t)invalid : rawv[(size_t)(pair * cr.n + s) * rawv_stride_e + (size_t)(y - cr.start[s]) * W + x];
}

}  // namespace camd
