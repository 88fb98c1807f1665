// lutr_kernels.hip -- gfx950 (MI355X / CDNA4) kernels of the 3D-LUT apply engine.
//
// What they replace: the per-pixel loops of FFmpeg's lut3d filter (and the scalers
// around it) that the reference invokes through
//   /root/reference/src/lut_renderer/ffmpeg.py:246   lut3d=file=...:interp=...
//   /root/reference/src/lut_renderer/ffmpeg.py:212-236, :304-310  scale= / format=
// Semantics: SURVEY.md Appendix A (lut3d) and DESIGN.md "YUV contract".
//
// Compiled with -ffp-contract=off: every product and sum of the lut3d restatement
// rounds separately, in FFmpeg's scalar C order, so results are bit-identical to the
// CPU oracle.  Fused multiply-adds appear only where written as __builtin_fmaf.
//
// This is gather + lerp: no MFMA.  The bound is HBM (6 B/px for yuv420p10le in+out)
// and, before that, VALU issue; see DESIGN.md "Kernels".
#include <cstdlib>

#include "lutr_device.h"
#include "lutr_launch.h"

namespace lutr {

// ================================================================= generic kernels
// Any depth 8..16, any strides/alignment, odd sizes, all five modes.  One thread per
// pixel (RGB) or per chroma block (YUV).  This is the ragged-input path, not the fast one.

__global__ __launch_bounds__(256) void k_rgb_generic(LutConsts L, PlaneSet P, FrameGeom G, int wide, int mode)
{
    const GFetch f(L);
    const long long total = (long long)G.w * G.rows * G.nframes;
    for (long long u = blockIdx.x * 256ll + threadIdx.x; u < total; u += (long long)gridDim.x * 256ll) {
        const int x = (int)(u % G.w);
        const long long t = u / G.w;
        const int y = G.row0 + (int)(t % G.rows);
        const long long fr = t / G.rows;
        const float g = ld_sample(src_row(P, 0, fr, y), x, wide);
        const float b = ld_sample(src_row(P, 1, fr, y), x, wide);
        const float r = ld_sample(src_row(P, 2, fr, y), x, wide);
        const Rgb o = lut3d_px_rt(mode, L, f, r, g, b);
        st_sample(dst_row(P, 0, fr, y), x, wide, o.g);
        st_sample(dst_row(P, 1, fr, y), x, wide, o.b);
        st_sample(dst_row(P, 2, fr, y), x, wide, o.r);
    }
}

// (the block walk, the block body and the sink: lutr_device.h, shared with k_yuv_float of the dither path)
__global__ __launch_bounds__(256) void k_yuv_generic(LutConsts L, YuvConsts K, PlaneSet P, FrameGeom G,
                                                     int win, int wout, int csx, int csy, int mode)
{
    const GFetch f(L);
    PlaneSink sink{K, P, wout};
    for_each_block(G, csx, csy, false, [&](long long fr, int cx, int cy) { yuv_block(L, f, K, P, G, fr, cx, cy, win, csx, csy, mode, sink); });
}

// ================================================================= vector kernels, global gather
// The low-latency path of small launches (and the A/B reference of the LDS window).  kVecBytes bytes per plane row and thread:
// 4 px (16-bit containers) or 8 px (8-bit); kVecBytes and vec_bytes<WIN, WOUT>(): lutr_device.h.
template <int WIDE, int INTERP>
__global__ __launch_bounds__(256) void k_rgb_vec(LutConsts L, PlaneSet P, FrameGeom G)
{
    constexpr int PXT = kVecBytes / (WIDE ? 2 : 1), NW = kVecBytes / 4;
    const GFetch f(L);
    const unsigned uw = (unsigned)G.w / PXT;
    const unsigned total = uw * (unsigned)G.rows * (unsigned)G.nframes;
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u >= total) return;
    const unsigned xu = u % uw, t = u / uw;
    const int y = G.row0 + (int)(t % (unsigned)G.rows);
    const long long fr = t / (unsigned)G.rows;
    const long long xo = (long long)xu * kVecBytes;
    uint32_t gw[NW], bw[NW], rw[NW], go[NW], bo[NW], ro[NW];
#pragma unroll
    for (int k = 0; k < NW; k++) { go[k] = 0; bo[k] = 0; ro[k] = 0; }
    ld_words<NW>(gw, src_row(P, 0, fr, y) + xo);
    ld_words<NW>(bw, src_row(P, 1, fr, y) + xo);
    ld_words<NW>(rw, src_row(P, 2, fr, y) + xo);
#pragma unroll
    for (int i = 0; i < PXT; i++) {
        const Rgb o = lut3d_px<INTERP>(L, f, word_sample<WIDE>(rw, i), word_sample<WIDE>(gw, i),
                                       word_sample<WIDE>(bw, i));
        word_put<WIDE>(go, i, o.g);
        word_put<WIDE>(bo, i, o.b);
        word_put<WIDE>(ro, i, o.r);
    }
    st_words<NW, true>(dst_row(P, 0, fr, y) + xo, go);
    st_words<NW, true>(dst_row(P, 1, fr, y) + xo, bo);
    st_words<NW, true>(dst_row(P, 2, fr, y) + xo, ro);
}

// The fused vector kernels (this one and those of lutr_xsub.hip, lutr_rgb2yuv.hip, lutr_rgbf.hip, lutr_semi.hip) keep their frame
// -- unit preamble, row addresses, fence, output stage -- written out: hipcc's schedule follows the order of the source, and each
// shared form tried (src_row / dst_row, a fence helper, an output-stage struct, k_yuv_vec as the equal-layout instance of
// k_yuv_xsub_vec's body) moved instructions in some instance.  tools/device_asm_diff.sh is the check for any change to them.
template <int WIN, int WOUT, int CSX, int CSY, int INTERP>
__global__ __launch_bounds__(256) void k_yuv_vec(LutConsts L, YuvConsts K, PlaneSet P, FrameGeom G)
{
    constexpr int VB = vec_bytes<WIN, WOUT>();
    constexpr int PXT = VB / (WIN ? 2 : 1);               // luma samples per thread per row
    constexpr int YWI = VB / 4, YWO = PXT * (WOUT ? 2 : 1) / 4;   // luma words per thread per row, in / out
    constexpr int BH = 1 << CSY, BW = 1 << CSX;
    constexpr int NC = PXT >> CSX;                        // chroma samples per thread
    constexpr int CWI = NC * (WIN ? 2 : 1) / 4, CWO = NC * (WOUT ? 2 : 1) / 4;
    static_assert(CWI >= 1 && CWO >= 1 && YWO >= 1, "a thread must own whole words");
    const GFetch f(L);
    const unsigned uw = (unsigned)G.w / PXT;
    const unsigned ub = (unsigned)G.rows >> CSY;
    const unsigned total = uw * ub * (unsigned)G.nframes;
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u >= total) return;
    const unsigned xu = u % uw, t = u / uw;
    const int cy = (G.row0 >> CSY) + (int)(t % ub);
    const long long fr = t / ub;
    const long long xi = (long long)xu * VB, xo = (long long)xu * (YWO * 4), cxi = (long long)xu * (CWI * 4), cxo = (long long)xu * (CWO * 4);

    uint32_t yw[BH][YWI], cbw[CWI], crw[CWI];
    uint32_t yo[BH][YWO], cbo[CWO], cro[CWO];
#pragma unroll
    for (int dy = 0; dy < BH; dy++) {
        ld_words<YWI>(yw[dy], P.s[0] + fr * P.sfs[0] + (long long)(cy * BH + dy) * P.ss[0] + xi);
#pragma unroll
        for (int k = 0; k < YWO; k++) yo[dy][k] = 0;
    }
    ld_words<CWI>(cbw, P.s[1] + fr * P.sfs[1] + (long long)cy * P.ss[1] + cxi);
    ld_words<CWI>(crw, P.s[2] + fr * P.sfs[2] + (long long)cy * P.ss[2] + cxi);
#pragma unroll
    for (int k = 0; k < CWO; k++) { cbo[k] = 0; cro[k] = 0; }

#pragma unroll
    for (int j = 0; j < NC; j++) {
        const Chroma c = chroma_terms(K, word_sample<WIN>(cbw, j), word_sample<WIN>(crw, j));
        float rs = 0.f, gs = 0.f, bs = 0.f;
#pragma unroll
        for (int dy = 0; dy < BH; dy++) {
#pragma unroll
            for (int dx = 0; dx < BW; dx++) {
                const int i = j * BW + dx;
                const Rgb q = yuv_to_rgb(K, word_sample<WIN>(yw[dy], i), c);
                const Rgb o = lut3d_px<INTERP>(L, f, q.r, q.g, q.b);
                rs += o.r; gs += o.g; bs += o.b;
                word_put<WOUT>(yo[dy], i, rgb_to_y(K, o));
            }
        }
        word_put<WOUT>(cbo, j, rgb_to_cb(K, rs, gs, bs));
        word_put<WOUT>(cro, j, rgb_to_cr(K, rs, gs, bs));
        // Zero-instruction fence: without it hipcc hoists the coordinates and taps of every chroma block of the
        // thread to the top (256 VGPRs, one wave per SIMD); with it blocks are emitted one after the other.
#pragma unroll
        for (int dy = 0; dy < BH; dy++) {
#pragma unroll
            for (int k = 0; k < YWI; k++) asm volatile("" : "+v"(yw[dy][k]));
#pragma unroll
            for (int k = 0; k < YWO; k++) asm volatile("" : "+v"(yo[dy][k]));
        }
#pragma unroll
        for (int k = 0; k < CWI; k++) asm volatile("" : "+v"(cbw[k]), "+v"(crw[k]));
#pragma unroll
        for (int k = 0; k < CWO; k++) asm volatile("" : "+v"(cbo[k]), "+v"(cro[k]));
    }
#pragma unroll
    for (int dy = 0; dy < BH; dy++)
        st_words<YWO>(P.d[0] + fr * P.dfs[0] + (long long)(cy * BH + dy) * P.ds[0] + xo, yo[dy]);
    st_words<CWO>(P.d[1] + fr * P.dfs[1] + (long long)cy * P.ds[1] + cxo, cbo);
    st_words<CWO>(P.d[2] + fr * P.dfs[2] + (long long)cy * P.ds[2] + cxo, cro);
}

// ================================================================= launchers
// (layout predicates, grid sizing and the small-job boundary: lutr_launch.h)
const char *launch_rgb(hipStream_t st, int variant, const LutConsts &L, const PlaneSet &P,
                       const FrameGeom &G, int depth, int mode, unsigned *stats, unsigned *queue)
{
    // a prelut (.csp shaper): the round-3 tube kernels read one (three coordinate tables, 8- and 10-bit data); the round-1 tile kernel does not
    const bool tiles = L.pre == nullptr;
    const int wide = depth > 8;
    const int pxt = wide ? 8 : 16;
    const long long px = (long long)G.w * G.rows * G.nframes;
    bool vec_ok = vec_mode(mode) &&
                  G.w % pxt == 0 && units_fit(px / pxt);
    for (int c = 0; c < 3 && vec_ok; c++)
        vec_ok = planes_ok(P, c, 16, G.nframes > 1, kStrideTile, false);
    if (variant == VAR_GENERIC) vec_ok = false;
    // which LDS kernel would take the launch decides where "small" ends: the tube kernels have the two-level queue (33 Mpx), round 1's kernel not (70)
    const Rgb2Policy pol = rgb2_policy();
    const bool tube_first = pol != RGB2_OFF && (pol == RGB2_ALL || !tiles || mode != LUTR_INTERP_TRILINEAR);
    if ((tiles || depth <= 10) && vec_ok && ((variant == VAR_AUTO && !small_job(px, tube_first ? kSmallQueueMpx : kSmallTileMpx)) || variant == VAR_VEC_LDS)) {
        // round 3: the tube kernels (lutr_rgb2.hip) take the planes in (R, G, B) order; gbrp is (G, B, R)
        // Policy (profiles/r03_exp21_planar_rgb_tube_vs_round1.txt): with the two-level chunk queue the tube kernel wins every 4-tap and
        // nearest launch (gbrp10le tetrahedral 8 / 16 / 128 frames 359 / 412 / 432 vs 282 / 353 / 427 Gpx/s, gbrp 519 / 583 / 637 vs
        // 379 / 447 / 593, gbrp nearest 885 = 0.66 of the peak); trilinear's eight 16-byte taps stay on round 1's kernel, which is
        // 16-20 % faster there at 128 frames.  LUTR_RGB2=all sends everything it can take to the tube kernels, =0 nothing.
        if (tube_first) {
            const PlaneSet Q = gbrp_to_rgb(P);
            const char *name = wide ? launch_rgb_tube_ly1(st, L, Q, G, depth, mode, 0, stats, queue)
                                    : launch_rgb_tube_ly0(st, L, Q, G, depth, mode, 0, stats, queue);
            if (name) return name;
        }
        if (tiles) return launch_rgb_tile(st, L, P, G, depth, mode, stats, queue);
        if (variant == VAR_VEC_LDS) variant = VAR_VEC_GLOBAL;          // a prelut the tube kernels could not take (layout): vector kernels
    }
    if (!tiles && variant == VAR_VEC_LDS) variant = VAR_VEC_GLOBAL;
    // A ragged width on aligned (padded) rows: the fast kernel takes the columns up to the last multiple of
    // its unit, the scalar kernel the few that remain (each pixel is independent, so any split is exact).
    const int wv = G.w / pxt * pxt;
    if (tiles && variant == VAR_AUTO && !vec_ok && wv > 0 && wv < G.w && !small_job(px, kSmallTileMpx) &&
        vec_mode(mode) &&
        units_fit((long long)wv * G.rows * G.nframes / pxt) &&
        planes_ok(P, 0, 16, G.nframes > 1, kStrideTile, false) && planes_ok(P, 1, 16, G.nframes > 1, kStrideTile, false) &&
        planes_ok(P, 2, 16, G.nframes > 1, kStrideTile, false)) {
        FrameGeom Gv = G, Ge = G;
        Gv.w = wv;
        Ge.w = G.w - wv;
        const long long eb = (long long)wv * (wide ? 2 : 1);
        const PlaneSet Pe = advance_planes(P, eb, eb, eb, eb);
        const char *name = launch_rgb_tile(st, L, P, Gv, depth, mode, stats, queue);
        hipLaunchKernelGGL(k_rgb_generic, dim3(stride_grid("k_rgb_generic", (long long)Ge.w * G.rows * G.nframes, kGridStrideCap)), dim3(256), 0, st,
                           L, Pe, Ge, wide, mode);
        return name;
    }
    if (!vec_ok) {
        if (variant == VAR_VEC_GLOBAL || variant == VAR_VEC_LDS) return nullptr;
        // grid-stride; enough blocks to fill 256 CUs x 8
        hipLaunchKernelGGL(k_rgb_generic, dim3(stride_grid("k_rgb_generic", px, kGridStrideCap)), dim3(256), 0, st, L, P, G, wide, mode);
        return "k_rgb_generic";
    }
    const dim3 grid(grid_for(px / (kVecBytes / (wide ? 2 : 1)))), block(256);
#define RGB_CASE(W, I) \
    if (wide == W && mode == I) { \
        hipLaunchKernelGGL((k_rgb_vec<W, I>), grid, block, 0, st, L, P, G); \
        return "k_rgb_vec<" #W "," #I ">"; \
    }
    RGB_CASE(0, 0) RGB_CASE(0, 1) RGB_CASE(0, 2)
    RGB_CASE(1, 0) RGB_CASE(1, 1) RGB_CASE(1, 2)
#undef RGB_CASE
    return nullptr;
}

// Round-2 tile kernels (lutr_tile2.hip): input and output depth are independent there, so source planes are checked
// against the input unit (16 bytes of luma, the matching chroma bytes) and destination planes against the output unit.
static const char *try_tile2(hipStream_t st, const LutConsts &L, const YuvConsts &K, const PlaneSet &P, const FrameGeom &G,
                             int din, int dout, int lut_depth, int csx, int csy, int mode, bool fast, unsigned *stats, unsigned *queue)
{
    // a prelut: only one that is the same non-decreasing shaper on the three channels (LutConsts::pre_shared) and only up to 10 bit (the
    // coordinate table); anything else stays on the generic / vector kernels
    const char *nop = getenv("LUTR_NO_TILE2_PRELUT");
    if (getenv("LUTR_NO_TILE2") || (L.pre && (!L.pre_shared || lut_depth > 10 || (nop && nop[0] != '0')))) return nullptr;
    const int win = din > 8, wout = dout > 8, pxt = win ? 8 : 16, bh = 1 << csy;
    if (!vec_mode(mode)) return nullptr;
    if (G.w % pxt || G.row0 % bh || G.rows % bh || (csx == 0 && csy == 1)) return nullptr;
    if (!units_fit((long long)(G.w / pxt) * (G.rows >> csy) * G.nframes)) return nullptr;
    const long long yi = 16, yo = (long long)pxt * (wout ? 2 : 1), ci = (long long)(pxt >> csx) * (win ? 2 : 1),
                    co = (long long)(pxt >> csx) * (wout ? 2 : 1);
    const bool batch = G.nframes > 1;
    for (int c = 0; c < 3; c++)
        if (!plane_ok(P.s[c], P.ss[c], P.sfs[c], c ? ci : yi, batch, kStrideTile2, true) ||
            !plane_ok(P.d[c], P.ds[c], P.dfs[c], c ? co : (yo > 16 ? 16 : yo), batch, kStrideTile2, true))
            return nullptr;
#define T2_TRY(tag) return launch_yuv_tile2_##tag(st, L, K, P, G, din, dout, lut_depth, csx, csy, mode, fast, stats, queue)
    const int key = win * 1000 + wout * 100 + csx * 10 + csy;
    switch (key) {
    case 11:   T2_TRY(w00_c11);
    case 10:   T2_TRY(w00_c10);
    case 0:    T2_TRY(w00_c00);
    case 1111: T2_TRY(w11_c11);
    case 1110: T2_TRY(w11_c10);
    case 1100: T2_TRY(w11_c00);
    case 1011: T2_TRY(w10_c11);
    case 1010: T2_TRY(w10_c10);
    case 1000: T2_TRY(w10_c00);
    }
#undef T2_TRY
    return nullptr;
}

const char *launch_yuv(hipStream_t st, int variant, const LutConsts &L, const YuvConsts &K,
                       const PlaneSet &P, const FrameGeom &G, int din, int dout, int lut_depth, int csx, int csy, int mode,
                       bool fast, unsigned *stats, unsigned *queue)
{
    const int win = din > 8, wout = dout > 8;
    const int pxt = win ? 8 : 16;
    const int bh = 1 << csy;
    if (L.pre && !(L.pre_shared && lut_depth <= 10) && variant == VAR_VEC_LDS) variant = VAR_VEC_GLOBAL;   // a prelut the tile kernels cannot take
    if (variant == VAR_VEC_LDS || (variant == VAR_AUTO && !small_job((long long)G.w * G.rows * G.nframes, kSmallQueueMpx))) {
        if (const char *name = try_tile2(st, L, K, P, G, din, dout, lut_depth, csx, csy, mode, fast, stats, queue)) return name;
        if (variant == VAR_VEC_LDS) return nullptr;          // asked for the tile kernels, and they cannot take this call
    }
    const long long cbytes = (long long)(pxt >> csx) * (win ? 2 : 1);      // chroma bytes per thread
    bool vec_ok = vec_mode(mode) &&
                  win == wout && G.w % pxt == 0 && G.row0 % bh == 0 && G.rows % bh == 0 &&
                  !(csx == 0 && csy == 1) &&
                  units_fit((long long)(G.w / pxt) * (G.rows >> csy) * G.nframes);
    for (int c = 0; c < 3 && vec_ok; c++) vec_ok = planes_ok(P, c, c ? cbytes : 16, G.nframes > 1, kStrideTile, false);
    if (variant == VAR_GENERIC) vec_ok = false;
    // ragged width on aligned (padded) rows: tile kernel up to the last whole unit, scalar kernel for the rest
    // (the split falls on a chroma-block boundary: the unit is 8 or 16 luma samples wide)
    const int wv = G.w / pxt * pxt;
    if (variant == VAR_AUTO && wv > 0 && wv < G.w && !small_job((long long)G.w * G.rows * G.nframes, kSmallQueueMpx)) {
        FrameGeom Gv = G, Ge = G;
        Gv.w = wv;
        Ge.w = G.w - wv;
        if (const char *name = try_tile2(st, L, K, P, Gv, din, dout, lut_depth, csx, csy, mode, fast, stats, queue)) {
            const long long bsi = win ? 2 : 1, bso = wout ? 2 : 1;
            const PlaneSet Pe = advance_planes(P, wv * bsi, (wv >> csx) * bsi, wv * bso, (wv >> csx) * bso);
            hipLaunchKernelGGL(k_yuv_generic, dim3(block_grid("k_yuv_generic", Ge.w, G.rows, G.nframes, csx, csy)), dim3(256), 0, st, L, K, Pe, Ge,
                               win, wout, csx, csy, mode);
            return name;
        }
    }
    // 10-bit (or deeper) source written as 8 bit: the vector kernel with 16-byte luma units
    if (!vec_ok && variant != VAR_GENERIC && win == 1 && wout == 0 &&
        vec_mode(mode) &&
        G.w % 8 == 0 && G.row0 % bh == 0 && G.rows % bh == 0 && !(csx == 0 && csy == 1) &&
        units_fit((long long)(G.w / 8) * (G.rows >> csy) * G.nframes) &&
        plane_ok(P.s[0], P.ss[0], P.sfs[0], 16, G.nframes > 1, kStrideTile2, true) &&
        plane_ok(P.d[0], P.ds[0], P.dfs[0], 8, G.nframes > 1, kStrideTile2, true) &&
        plane_ok(P.s[1], P.ss[1], P.sfs[1], 16 >> csx, G.nframes > 1, kStrideTile2, true) &&
        plane_ok(P.d[1], P.ds[1], P.dfs[1], 8 >> csx, G.nframes > 1, kStrideTile2, true) &&
        plane_ok(P.s[2], P.ss[2], P.sfs[2], 16 >> csx, G.nframes > 1, kStrideTile2, true) &&
        plane_ok(P.d[2], P.ds[2], P.dfs[2], 8 >> csx, G.nframes > 1, kStrideTile2, true)) {
        const dim3 grid(grid_for((long long)(G.w / 8) * (G.rows >> csy) * G.nframes)), block(256);
#define YUV10_CASE(X, Y, I) \
        if (csx == X && csy == Y && mode == I) { \
            hipLaunchKernelGGL((k_yuv_vec<1, 0, X, Y, I>), grid, block, 0, st, L, K, P, G); \
            return "k_yuv_vec<10," #X "," #Y "," #I ">"; \
        }
#define YUV10_FMT(X, Y) YUV10_CASE(X, Y, 0) YUV10_CASE(X, Y, 1) YUV10_CASE(X, Y, 2)
        YUV10_FMT(1, 1) YUV10_FMT(1, 0) YUV10_FMT(0, 0)
#undef YUV10_FMT
#undef YUV10_CASE
    }
    if (!vec_ok) {
        if (variant == VAR_VEC_GLOBAL || variant == VAR_VEC_LDS) return nullptr;
        hipLaunchKernelGGL(k_yuv_generic, dim3(block_grid("k_yuv_generic", G.w, G.rows, G.nframes, csx, csy)), dim3(256), 0, st, L, K, P, G, win,
                           wout, csx, csy, mode);
        return "k_yuv_generic";
    }
    const long long units = (long long)(G.w / (kVecBytes / (win ? 2 : 1))) * (G.rows >> csy) * G.nframes;
    const dim3 grid(grid_for(units)), block(256);
#define YUV_CASE(W, X, Y, I) \
    if (win == W && csx == X && csy == Y && mode == I) { \
        hipLaunchKernelGGL((k_yuv_vec<W, W, X, Y, I>), grid, block, 0, st, L, K, P, G); \
        return "k_yuv_vec<" #W "," #X "," #Y "," #I ">"; \
    }
#define YUV_FMT(W, X, Y) YUV_CASE(W, X, Y, 0) YUV_CASE(W, X, Y, 1) YUV_CASE(W, X, Y, 2)
    YUV_FMT(0, 1, 1) YUV_FMT(0, 1, 0) YUV_FMT(0, 0, 0)
    YUV_FMT(1, 1, 1) YUV_FMT(1, 1, 0) YUV_FMT(1, 0, 0)
#undef YUV_FMT
#undef YUV_CASE
    return nullptr;
}

}  // namespace lutr
