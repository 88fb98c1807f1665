// lutr_yuv2rgb.hip -- gfx950 kernels of the fused pass for YUV sources with an RGB output.
//
// What they replace: a chain the reference never emits but ffmpeg runs for every image-sequence or preview delivery of a camera
// file,
//   lut3d=file=...:interp=...,format=<rgb fmt>
// on a planar YUV frame: format negotiation puts lut3d at the RGB format's depth, so the frame is converted to integer RGB at
// that depth, goes through the lattice and is stored as it is.  The contract is a composition of pinned pieces: the first two
// stages of 3.2 / 3.8 (each source chroma sample replicated over its INPUT block, YUV -> integer RGB at lut_depth through
// chroma_terms / yuv_to_rgb) and 3.1 (lut3d on integer RGB at that depth).  There is no RGB -> YUV stage and no chroma mean.
// mode = -1 leaves the LUT out: the converted codes are stored.
//
// The destination travels in PlaneSet::d as three component streams in R, G, B order (lutr_internal.h RgbLayout), like the
// source of lutr_rgb2yuv.hip: planar gbrp, or one packed image whose fourth component, if any, is written K.max_l (opaque).
//
// One source, two kinds of translation unit (Makefile MIX_RULE), like lutr_rgb2yuv.hip:
//   without LUTR_Y2R_WI   the generic kernel and the launcher
//   LUTR_Y2R_WI / _WO     the vector kernels of one container mix (8 -> 8, 16 -> 16, 16 -> 8): 3 layouts x 3 destination kinds x 4 modes
#include "lutr_device.h"
#include "lutr_launch.h"

namespace lutr {

#ifdef LUTR_Y2R_WI
// ================================================================= vector kernel, global gather
// union_vec_unit's input side (whole-dword loads, 8 luma samples per thread and row, 2^ICSY rows per thread, chroma_terms once
// per input chroma sample, lattice taps gathered from L1/L2) with k_packed_vec's output side.  NC = 1: three planes; 3 | 4: one
// packed image (8 pixels = 6, 8, 12 or 16 dwords per row).  The component order of a packed destination is a wave-uniform argument.

template <int WIN, int ICSX, int ICSY, int NC, int WOUT, int INTERP>
__global__ __launch_bounds__(256) void k_yuv2rgb_vec(LutConsts L, YuvConsts K, PlaneSet P, FrameGeom G, RgbLayout Y)
{
    constexpr int PXT = 8;                                        // luma samples per thread per row
    constexpr int YWI = PXT * (WIN ? 2 : 1) / 4;                  // luma words in per thread per row
    constexpr int CWI = (PXT >> ICSX) * (WIN ? 2 : 1) / 4;        // chroma words in per thread
    constexpr int BW = 1 << ICSX, BH = 1 << ICSY;                 // the input chroma block
    constexpr int NB = PXT / BW;                                  // blocks per thread
    constexpr int SWO = PXT * (WOUT ? 2 : 1) / 4;                 // dwords of 8 samples of one component out
    constexpr int NWO = (NC == 1 ? 3 : NC) * SWO;                 // destination dwords per thread per row
    static_assert(NB >= 1 && CWI >= 1 && YWI >= 1 && SWO >= 1, "a thread must own whole words");
    const GFetch f(L);
    const unsigned uw = (unsigned)G.w / PXT;
    const unsigned ub = (unsigned)G.rows >> ICSY;
    const unsigned total = uw * ub * (unsigned)G.nframes;
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u >= total) return;
    const unsigned xu = u % uw, t = u / uw;
    const int y0 = ((G.row0 >> ICSY) + (int)(t % ub)) * BH;       // first luma row of the thread
    const long long fr = t / ub;
    const uint32_t amax = (uint32_t)K.max_l;                      // the fourth component of a packed destination: opaque

    uint32_t yw[BH][YWI], cbw[CWI], crw[CWI];
    uint32_t out[BH][NWO];
#pragma unroll
    for (int dy = 0; dy < BH; dy++) {
        ld_words<YWI>(yw[dy], P.s[0] + fr * P.sfs[0] + (long long)(y0 + dy) * P.ss[0] + (long long)xu * (YWI * 4));
#pragma unroll
        for (int k = 0; k < NWO; k++) out[dy][k] = 0;
    }
    {
        const long long r = (long long)(y0 >> ICSY), cx = (long long)xu * (CWI * 4);
        ld_words<CWI>(cbw, P.s[1] + fr * P.sfs[1] + r * P.ss[1] + cx);
        ld_words<CWI>(crw, P.s[2] + fr * P.sfs[2] + r * P.ss[2] + cx);
    }

#pragma unroll
    for (int j = 0; j < NB; j++) {
        const Chroma c = chroma_terms(K, word_sample<WIN>(cbw, j), word_sample<WIN>(crw, j));
#pragma unroll
        for (int dy = 0; dy < BH; dy++) {
#pragma unroll
            for (int dx = 0; dx < BW; dx++) {
                const int i = j * BW + dx;
                const Rgb q = yuv_to_rgb(K, word_sample<WIN>(yw[dy], i), c);
                Rgb o;
                if constexpr (INTERP < 0) o = q;
                else o = lut3d_px<INTERP>(L, f, q.r, q.g, q.b);
                y2r_put<WOUT, NC>(out[dy], i, o, Y, amax);
            }
        }
        // Zero-instruction fence (k_yuv_vec's): keeps hipcc from hoisting the coordinates and taps of every block of the thread
        // to the top; with it the blocks are emitted one after the other.
#pragma unroll
        for (int dy = 0; dy < BH; dy++) {
#pragma unroll
            for (int k = 0; k < YWI; k++) asm volatile("" : "+v"(yw[dy][k]));
#pragma unroll
            for (int k = 0; k < NWO; k++) asm volatile("" : "+v"(out[dy][k]));
        }
#pragma unroll
        for (int k = 0; k < CWI; k++) asm volatile("" : "+v"(cbw[k]), "+v"(crw[k]));
    }
#pragma unroll
    for (int dy = 0; dy < BH; dy++) {
        if constexpr (NC == 1) {
#pragma unroll
            for (int k = 0; k < 3; k++)
                st_words<SWO>(P.d[k] + fr * P.dfs[k] + (long long)(y0 + dy) * P.ds[k] + (long long)xu * (SWO * 4), out[dy] + k * SWO);
        } else {
            uint32_t *dp = (uint32_t *)(P.d[0] + fr * P.dfs[0] + (long long)(y0 + dy) * P.ds[0]) + (size_t)xu * NWO;
#pragma unroll
            for (int k = 0; k < NWO; k++) dp[k] = out[dy][k];
        }
    }
}

// The vector kernels of this translation unit's container mix; the layout checks are the caller's (launch_yuv2rgb).
const char *LUTR_CAT(LUTR_CAT(launch_yuv2rgb_vec_w, LUTR_Y2R_WI), LUTR_Y2R_WO)(hipStream_t st, const LutConsts &L, const YuvConsts &K,
                                                                                const PlaneSet &P, const RgbLayout &Y,
                                                                                const FrameGeom &G, int icsx, int icsy, int mode)
{
    constexpr int WI = LUTR_Y2R_WI, WO = LUTR_Y2R_WO;
    const long long units = (long long)(G.w / 8) * (G.rows >> icsy) * G.nframes;
    const dim3 grid((unsigned)((units + 255) / 256)), block(256);
#define Y2R_CASE(IX, IY, C, I, IN) \
    if (icsx == IX && icsy == IY && Y.step == C && mode == I) { \
        hipLaunchKernelGGL((k_yuv2rgb_vec<WI, IX, IY, C, WO, I>), grid, block, 0, st, L, K, P, G, Y); \
        return "k_yuv2rgb_vec<" LUTR_STR(LUTR_Y2R_WI) "," #IX "," #IY "," #C "," LUTR_STR(LUTR_Y2R_WO) "," IN ">"; \
    }
#define Y2R_DST(IX, IY, C) Y2R_CASE(IX, IY, C, -1, "nolut") Y2R_CASE(IX, IY, C, 0, "0") Y2R_CASE(IX, IY, C, 1, "1") Y2R_CASE(IX, IY, C, 2, "2")
#define Y2R_LAYOUT(IX, IY) Y2R_DST(IX, IY, 1) Y2R_DST(IX, IY, 3) Y2R_DST(IX, IY, 4)
    Y2R_LAYOUT(1, 1) Y2R_LAYOUT(1, 0) Y2R_LAYOUT(0, 0)
#undef Y2R_LAYOUT
#undef Y2R_DST
#undef Y2R_CASE
    return nullptr;
}

#else  // !LUTR_Y2R_WI
// ================================================================= generic kernel
// One thread per input chroma block: xsub_union_block (lutr_device.h) with a 4:4:4 "output layout", so that every pixel is a
// block of its own, and a sink that stores the pixel; any depth pair, stride or alignment, odd sizes, all five modes and the
// LUT-free form.  Only pixels inside the frame are written.
__global__ __launch_bounds__(256) void k_yuv2rgb_generic(LutConsts L, YuvConsts K, PlaneSet P, FrameGeom G, RgbLayout Y, int win,
                                                         int icsx, int icsy, int mode)
{
    const GFetch f(L);
    RgbSink sink{P, Y, K.max_l};
    for_each_block(G, icsx, icsy, false, [&](long long fr, int ux, int uy) {
        xsub_union_block(K, P, G, fr, ux, uy, win, icsx, icsy, 0, 0, sink, [&](long long, int, int, const Rgb &q) {
            return mode < 0 ? q : lut3d_px_rt(mode, L, f, q.r, q.g, q.b);
        });
    });
}

// ================================================================= launcher
const char *launch_yuv2rgb(hipStream_t st, int variant, const LutConsts &L, const YuvConsts &K, const PlaneSet &P,
                           const RgbLayout &Y, const FrameGeom &G, int din, int icsx, int icsy, int mode)
{
    const int win = din > 8, wout = Y.wide;
    const int bh = 1 << icsy;
    // the vector kernels' unit: 8 luma samples per row; an 8-bit source written as 16 bit has none
    const bool mix_ok = win == wout || (win && !wout);
    const long long bsi = win ? 2 : 1, bso = wout ? 2 : 1;
    const bool batch = G.nframes > 1;
    // the 3-component vector body knows R G B and B G R order only
    const bool order_ok = Y.step != 3 || (Y.go == 1 && ((Y.ro == 0 && Y.bo == 2) || (Y.ro == 2 && Y.bo == 0)));
    auto vec_fits = [&](const PlaneSet &Q, const FrameGeom &H) {
        if (!mix_ok || !order_ok || !(mode == -1 || vec_mode(mode))) return false;
        if (H.w % 8 || H.row0 % bh || H.rows % bh) return false;
        if (!units_fit((long long)(H.w / 8) * (H.rows / bh) * H.nframes)) return false;
        if (!plane_ok(Q.s[0], Q.ss[0], Q.sfs[0], 8 * bsi, batch, kStrideAny, false)) return false;
        for (int c = 1; c < 3; c++)
            if (!plane_ok(Q.s[c], Q.ss[c], Q.sfs[c], (8 >> icsx) * bsi, batch, kStrideAny, false)) return false;
        if (Y.step == 1) {
            for (int c = 0; c < 3; c++)
                if (!plane_ok(Q.d[c], Q.ds[c], Q.dfs[c], 8 * bso, batch, kStrideAny, false)) return false;
        } else if (!plane_ok(Q.d[0], Q.ds[0], Q.dfs[0], 4, batch, kStrideAny, false)) {
            return false;
        }
        return true;
    };
    auto vec = [&](const PlaneSet &Q, const FrameGeom &H) -> const char * {
        if (win && wout) return launch_yuv2rgb_vec_w11(st, L, K, Q, Y, H, icsx, icsy, mode);
        if (win) return launch_yuv2rgb_vec_w10(st, L, K, Q, Y, H, icsx, icsy, mode);
        return launch_yuv2rgb_vec_w00(st, L, K, Q, Y, H, icsx, icsy, mode);
    };
    auto generic = [&](const PlaneSet &Q, const FrameGeom &H) {
        hipLaunchKernelGGL(k_yuv2rgb_generic, dim3(block_grid("k_yuv2rgb_generic", H.w, H.rows, H.nframes, icsx, icsy)), dim3(256), 0, st, L, K, Q,
                           H, Y, win, icsx, icsy, mode);
        return "k_yuv2rgb_generic";
    };
    // (no LDS kernel for this path; the unit is 8 luma samples wide, whole chroma blocks)
    return launch_vec_or_generic(variant, P, G, 8, vec_fits, vec, generic, [&](int wv) {
        const long long db = (long long)wv * Y.step * bso;
        return advance_planes(P, wv * bsi, (wv >> icsx) * bsi, db, db);
    });
}
#endif  // LUTR_Y2R_WI

}  // namespace lutr
