// sgbm_split.hpp -- the two-pass form of the matching cost (round 1): k_hsum = calcPixelCostBT + horizontal box sum into an
// intermediate volume, k_vsum / k_vsum_reg = the vertical box sum + P2.  Kept for blockSize 13 / 15 and as an A/B
// reference (CAMD_COST_SPLIT); sgbm_cost.hpp builds the same volume in one pass.  Included by sgbm.hip (shares Geom).
#pragma once

namespace camd {

// ------------------------------------------------------------------------------------------------
// k_hsum: Hs[y][x][d] = sum_{dx=-SW2..SW2} pix(y, clamp(x+dx, 0, W1-1), d)   (u16, wraps like
// OpenCV's CostType), pix = sum over channels of min(c0, c1) [gradient] + min(c0, c1) >> 2 [raw].
// ------------------------------------------------------------------------------------------------
static constexpr int HSUM_SEG = 128;   // cost columns per workgroup
static constexpr int HSUM_RING = 16;   // ring slots (>= 2*SW2+1), per lane, in LDS

// One workgroup = one row y, cost columns [xs, xe), ALL disparities: wave w owns d in [64w, 64w+64).
// The right-image operands of the row segment are staged once in LDS (entry = one right pixel,
// CN*3 dwords padded to a multiple of 16 bytes); lane j of wave w reads entry (c - clo) + last - d for
// cost column c, so every step costs three ds_read_b128 (RGB) instead of VALU shifts.  The left-image
// operands are wave-uniform scalar loads.
// KT = the box width 2*SW2+1 when it is one of the instantiated sizes: the per-lane ring of the last KT column
// costs then lives in registers (the step loop is unrolled by 2*KT so every slot index is static);
// KT = 0: any width, ring in LDS.
template <int CN, int KT>
__global__ __launch_bounds__(512) void k_hsum(const uint8_t* __restrict__ left,
                                              const uint8_t* __restrict__ right, size_t pitch,
                                              size_t image_stride, uint16_t* __restrict__ Hs, Geom g,
                                              int ndblk, size_t vol_stride)
{
    constexpr int ES = CN == 1 ? 4 : 12;  // dwords per staged pixel
    extern __shared__ __attribute__((aligned(16))) uint32_t hs_lds[];
    const int lane = threadIdx.x & 63, dblk = threadIdx.x >> 6;
    const int y = blockIdx.y, pair = blockIdx.z;
    const int xs = blockIdx.x * HSUM_SEG, xe = min(xs + HSUM_SEG, g.W1);
    const int d = dblk * 64 + lane;
    const int K = 2 * g.SW2 + 1;
    const int clo = max(xs - g.SW2, 0), chi = min(xe - 1 + g.SW2, g.W1 - 1);
    const int last = ndblk * 64 - 1;
    const int ncols = (chi - clo) + ndblk * 64;          // right-image entries
    const int nleft = chi - clo + 1;                      // left-image entries (cost columns clo..chi)
    const int colbase = clo + g.minX1 - g.minD - last;    // right-image column of entry 0
    const int maxr = HSUM_SEG + 2 * g.SW2 + ndblk * 64 + 2, maxl = HSUM_SEG + 2 * g.SW2 + 2;
    uint32_t* stage = hs_lds;                              // [maxr][ES]  right operands (+1 halo entry each side)
    uint32_t* lstage = stage + (size_t)maxr * ES;          // [maxl][ES]  left operands  (+1 halo entry each side)
    uint32_t* ring = lstage + (size_t)maxl * ES + (size_t)dblk * K * 64;  // [ndblk][K][64]

    // ---- fused calcPixelCostBT preprocessing: planes p = (clipped x-Sobel | raw << 16) of the image
    // columns this segment touches, then per entry (p, min(p,(p+l)/2,(p+r)/2), max(...)).  Columns 0 and
    // W-1 of every plane hold ftzero; at the image edge the missing neighbour is p itself.
    // Phase 1 writes p into slot 0 of every entry (halo included), phase 2 reads the neighbours' slot 0.
    const uint32_t ftz2 = (uint32_t)g.ftzero | ((uint32_t)g.ftzero << 16);
    auto plane = [&](const uint8_t* img, int col, int c) -> uint32_t {
        if (col <= 0 || col >= g.W - 1) return ftz2;  // also covers columns outside the image (unused d)
        const uint8_t* r0 = img + (size_t)y * pitch + (size_t)col * CN + c;
        const uint8_t* rm = img + (size_t)(y > 0 ? y - 1 : y) * pitch + (size_t)col * CN + c;
        const uint8_t* rp = img + (size_t)(y < g.H - 1 ? y + 1 : y) * pitch + (size_t)col * CN + c;
        int gq = ((int)r0[CN] - (int)r0[-CN]) * 2 + ((int)rm[CN] - (int)rm[-CN]) + ((int)rp[CN] - (int)rp[-CN]);
        gq = min(max(gq, -g.ftzero), g.ftzero) + g.ftzero;
        return (uint32_t)gq | ((uint32_t)r0[0] << 16);
    };
    const uint8_t* imgR = right + (size_t)pair * image_stride;
    const uint8_t* imgL = left + (size_t)pair * image_stride;
    for (int e = threadIdx.x; e < ncols + 2; e += blockDim.x)
#pragma unroll
        for (int c = 0; c < CN; c++) stage[e * ES + c * 3] = plane(imgR, colbase - 1 + e, c);
    for (int e = threadIdx.x; e < nleft + 2; e += blockDim.x)
#pragma unroll
        for (int c = 0; c < CN; c++) lstage[e * ES + c * 3] = plane(imgL, clo + g.minX1 - 1 + e, c);
    if (KT == 0)
        for (int s = 0; s < K; s++) ring[s * 64 + lane] = 0;
    __syncthreads();
    auto finish = [&](uint32_t* dst, int e, int col) {  // entry e >= 1 holds image column col
#pragma unroll
        for (int c = 0; c < CN; c++) {
            uint32_t u = dst[e * ES + c * 3], l = dst[(e - 1) * ES + c * 3], r = dst[(e + 1) * ES + c * 3];
            uint32_t ul = col > 0 ? pk_lshr_u16(pk_add_u16(u, l), 0x00010001u) : u;
            uint32_t ur = col < g.W - 1 ? pk_lshr_u16(pk_add_u16(u, r), 0x00010001u) : u;
            dst[e * ES + c * 3 + 1] = pk_min_u16(pk_min_u16(ul, ur), u);
            dst[e * ES + c * 3 + 2] = pk_max_u16(pk_max_u16(ul, ur), u);
        }
    };
    for (int i = threadIdx.x; i < ncols; i += blockDim.x) finish(stage, i + 1, colbase + i);
    for (int i = threadIdx.x; i < nleft; i += blockDim.x) finish(lstage, i + 1, clo + g.minX1 + i);
    __syncthreads();
    const uint4* lent = reinterpret_cast<const uint4*>(lstage) + (ES / 4);  // skip the halo entry

    uint16_t* __restrict__ out = Hs + (size_t)pair * vol_stride + ((size_t)y * g.W1) * g.Dp + d;
    if (d >= g.Dp) return;  // lanes beyond the padded range only helped with the staging (no barrier follows)
    const uint32_t vmask = d < g.D ? 0xffffu : 0u;  // padded disparities D <= d < Dp are written as 0
    const uint4* ent = reinterpret_cast<const uint4*>(stage) + (size_t)(last - d + 1) * (ES / 4);

    // Software pipeline: the operands of step t+1 (three ds_read_b128 + the scalar loads of the left
    // pixel) are issued before the arithmetic of step t; two operand sets alternate (loop unrolled by 2).
    struct Ops { uint32_t V[CN], V0[CN], V1[CN], U[CN], U0[CN], U1[CN]; };
    auto fetch = [&](int t, Ops& o) {
        const int ct = min(max(t, 0), g.W1 - 1);  // clamped virtual column (box sum replicates the border)
        const uint4* e = ent + (size_t)(ct - clo) * (ES / 4);
        if (CN == 1) {
            uint4 a = e[0];
            o.V[0] = a.x; o.V0[0] = a.y; o.V1[0] = a.z;
        } else {
            uint4 a = e[0], b = e[1], c = e[2];
            o.V[0] = a.x; o.V0[0] = a.y; o.V1[0] = a.z;
            o.V[1 % CN] = a.w; o.V0[1 % CN] = b.x; o.V1[1 % CN] = b.y;
            o.V[2 % CN] = b.z; o.V0[2 % CN] = b.w; o.V1[2 % CN] = c.x;
        }
        const uint4* q = lent + (size_t)(ct - clo) * (ES / 4);
        if (CN == 1) {
            uint4 a = q[0];
            o.U[0] = a.x; o.U0[0] = a.y; o.U1[0] = a.z;
        } else {
            uint4 a = q[0], b = q[1], c = q[2];
            o.U[0] = a.x; o.U0[0] = a.y; o.U1[0] = a.z;
            o.U[1 % CN] = a.w; o.U0[1 % CN] = b.x; o.U1[1 % CN] = b.y;
            o.U[2 % CN] = b.z; o.U0[2 % CN] = b.w; o.U1[2 % CN] = c.x;
        }
    };
    uint32_t run = 0;
    const int t0 = xs - g.SW2, t1 = xe - 1 + g.SW2;
    // cost of one column for this lane's disparity (operands already fetched)
    auto column_cost = [&](const Ops& o) -> uint32_t {
        uint32_t acc = 0;
#pragma unroll
        for (int c = 0; c < CN; c++) {
            // c0 = max(0, u - v1, v0 - u), c1 = max(0, v - u1, u0 - v): at most one term of each pair is
            // non-zero, so OR of the saturating differences is their max
            uint32_t a = pk_subsat_u16(o.U[c], o.V1[c]) | pk_subsat_u16(o.V0[c], o.U[c]);
            uint32_t b = pk_subsat_u16(o.V[c], o.U1[c]) | pk_subsat_u16(o.U0[c], o.V[c]);
            uint32_t m = pk_min_u16(a, b);
            m = pk_lshr_u16(m, 0x00020000u);  // raw plane: cost >> 2
            acc = __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2_t, m),
                                         __builtin_bit_cast(u16x2_t, 0x00010001u), acc, false);
        }
        return acc;
    };
    auto emit = [&](int t) {
        const int xo = t - g.SW2;
        if (xo >= xs)
            out[(size_t)xo * g.Dp] = (uint16_t)(run & vmask);  // one unconditional store: no exec juggling
    };
    Ops A, B;
    fetch(t0, A);
    if (KT > 0) {
        uint32_t rr[KT > 0 ? KT : 1];
#pragma unroll
        for (int j = 0; j < (KT > 0 ? KT : 1); j++) rr[j] = 0;
        for (int t = t0; t <= t1; t += 2 * KT) {
#pragma unroll
            for (int j = 0; j < 2 * KT; j++) {
                if (t + j <= t1) {  // uniform
                    const Ops& o = (j & 1) ? B : A;
                    fetch(min(t + j + 1, t1), (j & 1) ? A : B);
                    const uint32_t acc = column_cost(o);
                    run += acc - rr[j % (KT > 0 ? KT : 1)];
                    rr[j % (KT > 0 ? KT : 1)] = acc;
                    emit(t + j);
                }
            }
        }
    } else {
        int slot = 0;
        auto step = [&](int t, const Ops& o, Ops& nxt) {
            fetch(min(t + 1, t1), nxt);
            const uint32_t old = ring[slot * 64 + lane];
            const uint32_t acc = column_cost(o);
            ring[slot * 64 + lane] = acc;
            slot = slot + 1 == K ? 0 : slot + 1;
            run += acc - old;
            emit(t);
        };
        for (int t = t0; t <= t1; t += 2) {
            step(t, A, B);
            if (t + 1 <= t1) step(t + 1, B, A);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// k_vsum: C[y][x][d] = P2 + sum_{dy=-SH2..SH2} Hs[clamp(y+dy,0,H-1)][x][d]   (u16 wrap)
// One thread = 8 consecutive d (16 bytes) of one column, walking VSUM_ROWS rows downwards with a running
// sum: C(y) = C(y-1) + Hs(y+SH2) - Hs(y-SH2-1).  The K = 2*SH2+1 rows inside the window live in a
// thread-private LDS ring, so every Hs row is read once per row segment (plus K-1 halo rows) whatever the
// row pitch is -- a per-row kernel that re-reads its K rows only gets them from L2 when vertically
// adjacent workgroups happen to land on the same XCD (true for W1 = 1792, false for W1 = 1793).
// ------------------------------------------------------------------------------------------------
static constexpr int VSUM_ROWS = 64;

// SAT: the saturating recurrence of OpenCV's CV_SIMD build (see sgbm_cost.hpp); then one block walks ALL rows.
template <bool SAT>
__global__ __launch_bounds__(256) void k_vsum(const uint4* __restrict__ Hs, uint4* __restrict__ C, Geom g,
                                              size_t vol_stride16, int rows_per_block)
{
    extern __shared__ uint4 vring[];  // [K][256]
    const size_t rowv = (size_t)g.W1 * (g.Dp / 8);  // uint4 per row
    const size_t i0 = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool ok = i0 < rowv;
    const size_t i = ok ? i0 : rowv - 1;
    const bool first_col = i < (size_t)(g.Dp / 8);  // cost column 0
    const int pair = blockIdx.z, H = g.H, SH2 = g.SW2, K = 2 * SH2 + 1;
    const int y0 = blockIdx.y * rows_per_block, y1 = min(y0 + rows_per_block, H);
    const uint4* base = Hs + (size_t)pair * vol_stride16 + i;
    uint4* out = C + (size_t)pair * vol_stride16 + i;
    auto ld = [&](int yy) -> uint4 { return base[(size_t)min(max(yy, 0), H - 1) * rowv]; };
    auto add = [&](uint32_t a, uint32_t b) { return SAT ? pk_addsat_i16(a, b) : pk_add_u16(a, b); };
    auto upd = [&](uint32_t a, uint32_t v, uint32_t o, bool add_first) {
        if (!SAT) return pk_sub_u16(pk_add_u16(a, v), o);
        return add_first ? pk_subsat_i16(pk_addsat_i16(a, v), o) : pk_addsat_i16(pk_subsat_i16(a, o), v);
    };
    const uint32_t p2 = dup16((uint32_t)g.P2);
    uint4 acc = make_uint4(p2, p2, p2, p2);
    for (int j = 0; j < K; j++) {
        uint4 v = ld(y0 - SH2 + j);
        vring[j * 256 + threadIdx.x] = v;
        acc.x = add(acc.x, v.x); acc.y = add(acc.y, v.y);
        acc.z = add(acc.z, v.z); acc.w = add(acc.w, v.w);
    }
    if (ok) out[(size_t)y0 * rowv] = acc;
    int slot = 0;  // ring position of the oldest row (y - SH2 - 1 of the next output row)
    uint4 nx[4];   // rows y+SH2 .. y+3+SH2 in flight
#pragma unroll
    for (int u = 0; u < 4; u++) nx[u] = ld(y0 + 1 + u + SH2);
    for (int y = y0 + 1; y < y1; y += 4) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (y + u < y1) {
                const uint4 v = nx[u];
                nx[u] = ld(y + u + 4 + SH2);
                const uint4 o = vring[slot * 256 + threadIdx.x];
                vring[slot * 256 + threadIdx.x] = v;
                slot = slot + 1 == K ? 0 : slot + 1;
                const bool af = first_col && y + u + SH2 < H;  // OpenCV's order in column 0 while the entering row exists
                acc.x = upd(acc.x, v.x, o.x, af); acc.y = upd(acc.y, v.y, o.y, af);
                acc.z = upd(acc.z, v.z, o.z, af); acc.w = upd(acc.w, v.w, o.w, af);
                if (ok) out[(size_t)(y + u) * rowv] = acc;
            }
        }
    }
}

// Register-ring variant for the common block sizes (K = 2*SH2+1 known at compile time): no LDS at all, so
// its workgroups can share a CU with the LDS-hungry cost kernel of another stream.
template <int K>
__global__ __launch_bounds__(256) void k_vsum_reg(const uint4* __restrict__ Hs, uint4* __restrict__ C, Geom g,
                                                  size_t vol_stride16)
{
    constexpr int SH2 = K / 2;
    const size_t rowv = (size_t)g.W1 * (g.Dp / 8);
    const size_t i0 = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool ok = i0 < rowv;
    const size_t i = ok ? i0 : rowv - 1;
    const int pair = blockIdx.z, H = g.H;
    const int y0 = blockIdx.y * VSUM_ROWS, y1 = min(y0 + VSUM_ROWS, H);
    const uint4* base = Hs + (size_t)pair * vol_stride16 + i;
    uint4* out = C + (size_t)pair * vol_stride16 + i;
    auto ld = [&](int yy) -> uint4 { return base[(size_t)min(max(yy, 0), H - 1) * rowv]; };
    const uint32_t p2 = dup16((uint32_t)g.P2);
    uint4 acc = make_uint4(p2, p2, p2, p2);
    uint4 ring[K];  // slot j: row y0 - SH2 + j, later replaced in rotation (static indices: the loop steps by K)
#pragma unroll
    for (int j = 0; j < K; j++) {
        ring[j] = ld(y0 - SH2 + j);
        acc.x = pk_add_u16(acc.x, ring[j].x); acc.y = pk_add_u16(acc.y, ring[j].y);
        acc.z = pk_add_u16(acc.z, ring[j].z); acc.w = pk_add_u16(acc.w, ring[j].w);
    }
    if (ok) out[(size_t)y0 * rowv] = acc;
    for (int y = y0 + 1; y < y1; y += K) {
        uint4 nv[K];
#pragma unroll
        for (int j = 0; j < K; j++) nv[j] = ld(y + j + SH2);  // unconditional (clamped): issued back to back
#pragma unroll
        for (int j = 0; j < K; j++) {
            const uint4 v = nv[j], o = ring[j];
            ring[j] = v;
            acc.x = pk_sub_u16(pk_add_u16(acc.x, v.x), o.x); acc.y = pk_sub_u16(pk_add_u16(acc.y, v.y), o.y);
            acc.z = pk_sub_u16(pk_add_u16(acc.z, v.z), o.z); acc.w = pk_sub_u16(pk_add_u16(acc.w, v.w), o.w);
            if (ok && y + j < y1) out[(size_t)(y + j) * rowv] = acc;
        }
    }
}

}  // namespace camd
