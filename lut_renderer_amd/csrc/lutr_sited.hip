// lutr_sited.hip -- gfx950 kernels of the sited chroma contract: the fused YUV -> RGB -> lut3d ->
// RGB -> YUV chain with bilinear chroma up-sampling ahead of the LUT and a sited [1 2 1] / [1 1] down-sampling after it,
// instead of the replicate-then-block-mean of lutr_kernels.hip.  4:2:0 and 4:2:2 only: 4:4:4 and `replicate` never
// reach this file (lutr_apply_yuv_sited delegates them to lutr_apply_yuv).
//
// Work split.  A wave owns a segment of chroma columns (kSitedNcl per lane) and walks down a strip of kSitedStrip chroma
// rows of one frame.  Every lane computes the LUT of the luma columns 2cx and 2cx+1 of its chroma columns cx.
//   - Horizontally co-sited down-sampling (left, topleft) also needs luma column 2cx-1: it comes from the lane to the left
//     (__shfl_up).  Lane 0 of a wave is a halo lane: it computes the column group left of the segment and stores nothing,
//     so segments overlap by one lane (1/64 more blends) instead of every lane recomputing its left column.
//   - Vertically co-sited down-sampling (topleft, 4:2:0) needs luma row 2j-1: the wave carries the horizontally filtered
//     sums of the odd row of block row j-1 into row j; only the first row of a strip is computed as a halo (1/33 more).
//   - Up-sampling reads chroma rows j-1 .. j+1 (clamped to the plane); the filtered rows are carried down the strip, so each
//     chroma row is loaded once per wave.
// All coordinates clamp to the frame, so odd heights, a one-pixel frame and the halos at the frame edge need no special case,
// and source rows outside the row shard [row0, row0 + rows) are read from the full frame (only the shard is written).
//
// Two instances of the one kernel, chosen by the launcher from the layout:
//   V = 1 (k_yuv_sited_vec): equal input and output container widths, a width that is a multiple of 4, positive strides and
//     planes aligned to the lane's access.  A lane's 4 luma samples of a row are one 8-byte (16-bit containers) or 4-byte
//     (8-bit) access, its 2 chroma samples one 4- or 2-byte access; stores are non-temporal.  The chroma taps k-1 and k+2
//     around the lane's pair come from the neighbouring lanes (__shfl_up / __shfl_down; lanes at a wave's edge load them).
//   V = 0 (k_yuv_sited): samples addressed one by one -- any alignment, negative or padded strides, odd widths, 8- or
//     16-bit containers on either side.
//
// Compiled with -ffp-contract=off like every strict kernel: the weighted sums are exact integers in fp32, the rest is the
// arithmetic of lutr_device.h.
#include "lutr_device.h"
#include "lutr_launch.h"

namespace lutr {

namespace {

constexpr int kSitedStrip = 16;    // chroma rows per wave
constexpr int kSitedNcl = 2;       // chroma columns per lane (the vector instance's accesses assume 2)
static_assert(kSitedNcl == 2, "the vector instance moves 4 luma / 2 chroma samples per lane and row");

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// C' of the contract: the chroma code after the optional range/depth prologue
__device__ __forceinline__ float cprime(const YuvConsts &K, float v)
{
    return K.pre != 0.0f ? clip_floor(fma_(K.pc, v, K.pcb), K.pre_max) : v;
}

// Horizontal up-sampling weights (quarters) at luma column 2c + d from the chroma samples cs[c] (k-1), cs[c+1] (k), cs[c+2]
// (k+1): co-sited 4 | 2 2, interstitial 1 3 | 3 1.
template <int COX>
__device__ __forceinline__ float h_up(const float *cs, int d)
{
    if (COX) return d ? 2.0f * cs[1] + 2.0f * cs[2] : 4.0f * cs[1];
    return d ? 3.0f * cs[1] + cs[2] : cs[0] + 3.0f * cs[1];
}

// one chroma row, horizontally up-sampled at the lane's luma columns: [chroma column][even / odd luma column]
struct HRow {
    float b[kSitedNcl][2], r[kSitedNcl][2];
};

// Lane geometry: first chroma column cx0 (negative for the halo lane of a frame's first segment), its clamped form cxl (the vector
// instance's accesses; lanes past the frame read the last pair and store nothing), and the scalar instance's clamped luma columns.
struct Lane {
    int lane, cx0, cxl, wc;
    int xs[kSitedNcl][2];
};

// The lane's chroma samples k-1 .. k+2 of one row (clamped to [0, wc-1]), after the prologue.
template <int V, int W>
__device__ __forceinline__ void chroma_taps(const YuvConsts &K, const uint8_t *row, const Lane &ln, int wide, float (&cs)[kSitedNcl + 2])
{
    if constexpr (V) {
        float v0, v1;
        if constexpr (W) {
            const uint32_t w = *(const uint32_t *)(row + (long long)ln.cxl * 2);
            v0 = (float)(w & 0xffffu); v1 = (float)(w >> 16);
        } else {
            const uint32_t w = *(const uint16_t *)(row + ln.cxl);
            v0 = (float)(w & 0xffu); v1 = (float)(w >> 8);
        }
        v0 = cprime(K, v0); v1 = cprime(K, v1);
        float l = __shfl_up(v1, 1, 64), r = __shfl_down(v0, 1, 64);     // every lane shuffles; edges are fixed below
        if (ln.lane == 0 && ln.cx0 > 0) l = cprime(K, ld_sample(row, ln.cx0 - 1, W));
        if (ln.lane == 63 && ln.cx0 + kSitedNcl < ln.wc) r = cprime(K, ld_sample(row, ln.cx0 + kSitedNcl, W));
        if (ln.cx0 <= 0) l = v0;
        if (ln.cx0 + kSitedNcl >= ln.wc) r = v1;
        cs[0] = l; cs[1] = v0; cs[2] = v1; cs[3] = r;
    } else {
        // the scalar instance: chroma columns of the lane's (clamped) luma columns
        const int k0 = ln.xs[0][0] >> 1;
        cs[0] = cprime(K, ld_sample(row, max(k0 - 1, 0), wide));
#pragma unroll
        for (int i = 1; i < kSitedNcl + 2; i++) cs[i] = cprime(K, ld_sample(row, min(k0 + i - 1, ln.wc - 1), wide));
    }
}

template <int COX, int V, int W>
__device__ __forceinline__ void load_hrow(const YuvConsts &K, const uint8_t *rb, const uint8_t *rr, const Lane &ln, int wide, HRow &o)
{
    float cb[kSitedNcl + 2], cr[kSitedNcl + 2];
    chroma_taps<V, W>(K, rb, ln, wide, cb);
    chroma_taps<V, W>(K, rr, ln, wide, cr);
#pragma unroll
    for (int c = 0; c < kSitedNcl; c++)
#pragma unroll
        for (int d = 0; d < 2; d++) {
            if constexpr (V) {
                o.b[c][d] = h_up<COX>(cb + c, d);
                o.r[c][d] = h_up<COX>(cr + c, d);
            } else {
                // clamped columns: take the taps of the column's own chroma index and parity (odd widths, the halo lane)
                const int x = ln.xs[c][d], i = (x >> 1) - (ln.xs[0][0] >> 1);
                o.b[c][d] = h_up<COX>(cb + i, x & 1);
                o.r[c][d] = h_up<COX>(cr + i, x & 1);
            }
        }
}

// S = wa * A + wb * B per sample (exact: integer weights, integer sums below 2^21)
__device__ __forceinline__ void vmix(HRow &s, float wa, const HRow &a, float wb, const HRow &b)
{
#pragma unroll
    for (int c = 0; c < kSitedNcl; c++)
#pragma unroll
        for (int d = 0; d < 2; d++) {
            s.b[c][d] = wa * a.b[c][d] + wb * b.b[c][d];
            s.r[c][d] = wa * a.r[c][d] + wb * b.r[c][d];
        }
}

// One luma row of the lane: up-sampled chroma S (scaled by inv = 1 / Wsum), stage 1, lut3d, and Y stored when `yout` is set.
// Returns the LUT outputs of the row's pixels.
template <int INTERP, int V, int W>
__device__ __forceinline__ void do_row(const LutConsts &L, const GFetch &f, const YuvConsts &K, const uint8_t *yrow, uint8_t *yout,
                                       const Lane &ln, const bool (&st)[kSitedNcl][2], const HRow &s, float inv, int win, int wout,
                                       Rgb (&o)[kSitedNcl][2])
{
    float yv[kSitedNcl][2];
    if constexpr (V) {
        if constexpr (W) {
            const uint2 v = *(const uint2 *)(yrow + (long long)ln.cxl * 4);
            const uint32_t w[2] = {v.x, v.y};
#pragma unroll
            for (int i = 0; i < 4; i++) yv[i >> 1][i & 1] = word_sample<1>(w, i);
        } else {
            const uint32_t w[1] = {*(const uint32_t *)(yrow + (long long)ln.cxl * 2)};
#pragma unroll
            for (int i = 0; i < 4; i++) yv[i >> 1][i & 1] = word_sample<0>(w, i);
        }
    } else {
#pragma unroll
        for (int c = 0; c < kSitedNcl; c++)
#pragma unroll
            for (int d = 0; d < 2; d++) yv[c][d] = ld_sample(yrow, ln.xs[c][d], win);
    }
    uint32_t yo[2] = {0u, 0u};
#pragma unroll
    for (int c = 0; c < kSitedNcl; c++)
#pragma unroll
        for (int d = 0; d < 2; d++) {
            const float cb = s.b[c][d] * inv - K.coff, cr = s.r[c][d] * inv - K.coff;
            Chroma ch;
            ch.rv = K.krv * cr;
            ch.gv = fma_(K.kgu, cb, K.kgv * cr);
            ch.bu = K.kbu * cb;
            const Rgb q = yuv_to_rgb(K, yv[c][d], ch);
            o[c][d] = lut3d_px<INTERP>(L, f, q.r, q.g, q.b);
            if (yout) {
                const float y = rgb_to_y(K, o[c][d]);
                if constexpr (V) word_put<W>(yo, 2 * c + d, y);
                else if (st[c][d]) st_sample(yout, ln.xs[c][d], wout, y);
            }
        }
    if constexpr (V) {
        if (yout && st[0][0]) {
            if constexpr (W) st_words<2, true>(yout + (long long)ln.cxl * 4, yo);       // luma column 2 cxl
            else st_words<1, true>(yout + (long long)ln.cxl * 2, yo);
        }
    }
}

// Horizontal down-sampling of one row: co-sited 1 2 1 over luma columns 2cx-1, 2cx, 2cx+1 (the first from the lane to
// the left for the lane's first chroma column; column 0 itself at the frame's left edge), interstitial 1 1 over 2cx, 2cx+1.
// Every lane executes the shuffles.
template <int COX>
__device__ __forceinline__ void h_down(const Lane &ln, const Rgb (&o)[kSitedNcl][2], Rgb (&h)[kSitedNcl])
{
    Rgb left;
    if (COX) {
        left.r = __shfl_up(o[kSitedNcl - 1][1].r, 1, 64);
        left.g = __shfl_up(o[kSitedNcl - 1][1].g, 1, 64);
        left.b = __shfl_up(o[kSitedNcl - 1][1].b, 1, 64);
        if (ln.cx0 == 0) left = o[0][0];          // tap 2*0-1 clamps onto column 0
    }
#pragma unroll
    for (int c = 0; c < kSitedNcl; c++) {
        if (COX) {
            const Rgb &l = c ? o[c - 1][1] : left;
            h[c].r = l.r + 2.0f * o[c][0].r + o[c][1].r;
            h[c].g = l.g + 2.0f * o[c][0].g + o[c][1].g;
            h[c].b = l.b + 2.0f * o[c][0].b + o[c][1].b;
        } else {
            h[c].r = o[c][0].r + o[c][1].r;
            h[c].g = o[c][0].g + o[c][1].g;
            h[c].b = o[c][0].b + o[c][1].b;
        }
    }
}

template <int V, int W>
__device__ __forceinline__ void store_chroma(const YuvConsts &K, uint8_t *ob, uint8_t *orr, const Lane &ln, const bool (&cst)[kSitedNcl],
                                             int wout, const Rgb (&s)[kSitedNcl])
{
    if constexpr (V) {
        if (!cst[0]) return;
        uint32_t wb[1] = {0u}, wr[1] = {0u};
#pragma unroll
        for (int c = 0; c < kSitedNcl; c++) {
            word_put<W>(wb, c, rgb_to_cb(K, s[c].r, s[c].g, s[c].b));
            word_put<W>(wr, c, rgb_to_cr(K, s[c].r, s[c].g, s[c].b));
        }
        if constexpr (W) {
            st_words<1, true>(ob + (long long)ln.cxl * 2, wb);
            st_words<1, true>(orr + (long long)ln.cxl * 2, wr);
        } else {
            __builtin_nontemporal_store((uint16_t)wb[0], (uint16_t *)(ob + ln.cxl));
            __builtin_nontemporal_store((uint16_t)wr[0], (uint16_t *)(orr + ln.cxl));
        }
    } else {
#pragma unroll
        for (int c = 0; c < kSitedNcl; c++)
            if (cst[c]) {
                st_sample(ob, ln.cx0 + c, wout, rgb_to_cb(K, s[c].r, s[c].g, s[c].b));
                st_sample(orr, ln.cx0 + c, wout, rgb_to_cr(K, s[c].r, s[c].g, s[c].b));
            }
    }
}

}  // namespace

// CSY: 1 = 4:2:0, 0 = 4:2:2.  COX / COY: chroma co-sited with luma horizontally / vertically (else interstitial).
// V: 1 = the vector instance with W = 16-bit containers (in and out), 0 = the scalar instance (W unused, widths at run time).
template <int CSY, int COX, int COY, int INTERP, int V, int W>
__global__ __launch_bounds__(256) void k_yuv_sited(LutConsts L, YuvConsts K, PlaneSet P, FrameGeom G, int win, int wout)
{
    const GFetch f(L);
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int Wd = G.w, H = G.h, wc = (Wd + 1) >> 1, hc = (H + (1 << CSY) - 1) >> CSY;
    const int cr0 = G.row0 >> CSY, cr1 = (G.row0 + G.rows + (1 << CSY) - 1) >> CSY;
    constexpr int kLanes = COX ? 63 : 64;                 // lanes that store; lane 0 is the halo lane when COX
    const int seg_w = kLanes * kSitedNcl;
    const int nseg = (wc + seg_w - 1) / seg_w, nstrip = (cr1 - cr0 + kSitedStrip - 1) / kSitedStrip;
    if (wave >= (long long)nseg * nstrip * G.nframes) return;          // whole waves only: the shuffles need every lane
    const int seg = (int)(wave % nseg);
    const long long t = wave / nseg;
    const int strip = (int)(t % nstrip);
    const long long fr = t / nstrip;
    const int js = cr0 + strip * kSitedStrip, je = min(js + kSitedStrip, cr1);

    Lane ln;
    ln.lane = lane;
    ln.wc = wc;
    ln.cx0 = seg * seg_w + (lane - (COX ? 1 : 0)) * kSitedNcl;
    ln.cxl = clampi(ln.cx0, 0, wc - kSitedNcl);           // vector instance: wc is a multiple of kSitedNcl there
    const bool lane_st = !COX || lane > 0;
    bool yst[kSitedNcl][2], cst[kSitedNcl];
#pragma unroll
    for (int c = 0; c < kSitedNcl; c++) {
        const int cx = ln.cx0 + c;
        ln.xs[c][0] = clampi(2 * cx, 0, Wd - 1);
        ln.xs[c][1] = clampi(2 * cx + 1, 0, Wd - 1);
        cst[c] = lane_st && cx >= 0 && cx < wc;
        yst[c][0] = cst[c];
        yst[c][1] = cst[c] && 2 * cx + 1 < Wd;
    }

    const uint8_t *sy = P.s[0] + fr * P.sfs[0], *sb = P.s[1] + fr * P.sfs[1], *sr = P.s[2] + fr * P.sfs[2];
    uint8_t *dy = P.d[0] + fr * P.dfs[0], *db = P.d[1] + fr * P.dfs[1], *dr = P.d[2] + fr * P.dfs[2];
    auto crow = [&](const uint8_t *base, int plane, int r) { return base + (long long)r * P.ss[plane]; };
    auto store_c = [&](int j, const Rgb (&s)[kSitedNcl]) {
        store_chroma<V, W>(K, db + (long long)j * P.ds[1], dr + (long long)j * P.ds[2], ln, cst, wout, s);
    };
    Rgb o[kSitedNcl][2], ha[kSitedNcl], hb[kSitedNcl], acc[kSitedNcl];

    if (CSY == 0) {
        // 4:2:2: the vertical axis is not subsampled (weight 1); Wsum = 4
        for (int j = js; j < je; j++) {
            HRow hcur;
            load_hrow<COX, V, W>(K, crow(sb, 1, j), crow(sr, 2, j), ln, win, hcur);
            do_row<INTERP, V, W>(L, f, K, sy + (long long)j * P.ss[0], dy + (long long)j * P.ds[0], ln, yst, hcur, 0.25f, win, wout, o);
            h_down<COX>(ln, o, ha);
            store_c(j, ha);
        }
        return;
    }

    // 4:2:0: chroma rows j-1, j, j+1 (clamped) carried down the strip; Wsum = 16
    HRow hp, hcur, hn, s;
    load_hrow<COX, V, W>(K, crow(sb, 1, max(js - 1, 0)), crow(sr, 2, max(js - 1, 0)), ln, win, hp);
    load_hrow<COX, V, W>(K, crow(sb, 1, min(js, hc - 1)), crow(sr, 2, min(js, hc - 1)), ln, win, hcur);
    if (COY) {
        // halo: luma row 2js-1 (row 0 at the top edge), odd: chroma 2 C[js-1] + 2 C[js]; its filtered row seeds the carry
        vmix(s, 2.0f, hp, 2.0f, hcur);
        do_row<INTERP, V, W>(L, f, K, sy + (long long)max(2 * js - 1, 0) * P.ss[0], nullptr, ln, yst, s, 0.0625f, win, wout, o);
        h_down<COX>(ln, o, acc);
    }
    for (int j = js; j < je; j++) {
        const int jn = min(j + 1, hc - 1);
        load_hrow<COX, V, W>(K, crow(sb, 1, jn), crow(sr, 2, jn), ln, win, hn);
        const int ya = 2 * j, yb = min(2 * j + 1, H - 1);
        // even row 2j: co-sited 4 C[j], interstitial C[j-1] + 3 C[j]
        if (COY) vmix(s, 4.0f, hcur, 0.0f, hcur);
        else vmix(s, 1.0f, hp, 3.0f, hcur);
        do_row<INTERP, V, W>(L, f, K, sy + (long long)ya * P.ss[0], dy + (long long)ya * P.ds[0], ln, yst, s, 0.0625f, win, wout, o);
        h_down<COX>(ln, o, ha);
        if (yb != ya) {
            // odd row 2j+1: co-sited 2 C[j] + 2 C[j+1], interstitial 3 C[j] + C[j+1]
            if (COY) vmix(s, 2.0f, hcur, 2.0f, hn);
            else vmix(s, 3.0f, hcur, 1.0f, hn);
            do_row<INTERP, V, W>(L, f, K, sy + (long long)yb * P.ss[0], dy + (long long)yb * P.ds[0], ln, yst, s, 0.0625f, win, wout, o);
            h_down<COX>(ln, o, hb);
        } else {
            // odd height, last block row: tap 2j+1 clamps onto row 2j
#pragma unroll
            for (int c = 0; c < kSitedNcl; c++) hb[c] = ha[c];
        }
#pragma unroll
        for (int c = 0; c < kSitedNcl; c++) {
            if (COY) {
                // 1 2 1 over rows 2j-1, 2j, 2j+1
                Rgb v;
                v.r = acc[c].r + 2.0f * ha[c].r + hb[c].r;
                v.g = acc[c].g + 2.0f * ha[c].g + hb[c].g;
                v.b = acc[c].b + 2.0f * ha[c].b + hb[c].b;
                acc[c] = hb[c];
                ha[c] = v;
            } else {
                ha[c].r += hb[c].r; ha[c].g += hb[c].g; ha[c].b += hb[c].b;
            }
        }
        store_c(j, ha);
        hp = hcur;
        hcur = hn;
    }
}

// The vector instance's layout: every plane of src and dst aligned to the lane's access (4 luma samples, 2 chroma samples),
// positive strides, and frame strides that keep the alignment.
const char *launch_yuv_sited(hipStream_t st, const LutConsts &L, const YuvConsts &K, const PlaneSet &P, const FrameGeom &G,
                             int din, int dout, int csy, int loc, int mode)
{
    const int win = din > 8, wout = dout > 8;
    // 4:2:2 has no subsampled vertical axis, so topleft and left are the same filter and share the left instances
    const int cox = loc != LUTR_CHROMA_CENTER, coy = csy && loc == LUTR_CHROMA_TOPLEFT;
    const long long wc = (G.w + 1) >> 1, bh = 1 << csy;
    const long long crows = (G.row0 + G.rows + bh - 1) / bh - G.row0 / bh;
    const long long seg_w = (cox ? 63 : 64) * kSitedNcl;
    const long long waves = (wc + seg_w - 1) / seg_w * ((crows + kSitedStrip - 1) / kSitedStrip) * G.nframes;
    const long long blocks = (waves + 3) / 4;
    if (blocks > 0x7fffffffll) return nullptr;
    const dim3 grid((unsigned)blocks), block(256);
    bool vec = win == wout && G.w % (2 * kSitedNcl) == 0 &&
               (mode == LUTR_INTERP_NEAREST || mode == LUTR_INTERP_TRILINEAR || mode == LUTR_INTERP_TETRAHEDRAL);
    const long long ya = 2 * kSitedNcl * (win ? 2 : 1), ca = kSitedNcl * (win ? 2 : 1);
    const bool batch = G.nframes > 1;
    for (int c = 0; c < 3 && vec; c++) {
        const long long a = c ? ca : ya;
        vec = planes_ok(P, c, a, batch, kStrideAny, false);
    }
#define SITED_CASE(CSY, COX, COY, I, NAME) \
    if (csy == CSY && cox == COX && coy == COY && mode == I) { \
        if (vec && win) { \
            hipLaunchKernelGGL((k_yuv_sited<CSY, COX, COY, I, 1, 1>), grid, block, 0, st, L, K, P, G, win, wout); \
            return "k_yuv_sited_vec<16," NAME "," #I ">"; \
        } \
        if (vec) { \
            hipLaunchKernelGGL((k_yuv_sited<CSY, COX, COY, I, 1, 0>), grid, block, 0, st, L, K, P, G, win, wout); \
            return "k_yuv_sited_vec<8," NAME "," #I ">"; \
        } \
        hipLaunchKernelGGL((k_yuv_sited<CSY, COX, COY, I, 0, 0>), grid, block, 0, st, L, K, P, G, win, wout); \
        return "k_yuv_sited<" NAME "," #I ">"; \
    }
#define SITED_SCALAR(CSY, COX, COY, I, NAME) \
    if (csy == CSY && cox == COX && coy == COY && mode == I) { \
        hipLaunchKernelGGL((k_yuv_sited<CSY, COX, COY, I, 0, 0>), grid, block, 0, st, L, K, P, G, win, wout); \
        return "k_yuv_sited<" NAME "," #I ">"; \
    }
#define SITED_MODES(CSY, COX, COY, NAME) \
    SITED_CASE(CSY, COX, COY, 0, NAME) SITED_CASE(CSY, COX, COY, 1, NAME) SITED_CASE(CSY, COX, COY, 2, NAME) \
    SITED_SCALAR(CSY, COX, COY, 3, NAME) SITED_SCALAR(CSY, COX, COY, 4, NAME)
    SITED_MODES(1, 1, 0, "420,left") SITED_MODES(1, 0, 0, "420,center") SITED_MODES(1, 1, 1, "420,topleft")
    SITED_MODES(0, 1, 0, "422,left") SITED_MODES(0, 0, 0, "422,center")
#undef SITED_MODES
#undef SITED_SCALAR
#undef SITED_CASE
    return nullptr;
}

}  // namespace lutr
