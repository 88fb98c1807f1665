// lutr_rgb2yuv.hip -- gfx950 kernels of the fused pass for RGB sources with a YUV output.
//
// What they replace: the reference's chain on an RGB source (a PNG / TIFF / DPX sequence, an RGB screen recording):
//   lut3d=file=...:interp=...   directly on the RGB frame                 (ffmpeg.py:246)
//   format=<pix_fmt>            RGB -> YUV at the output depth and layout (ffmpeg.py:304-310)
// The contract is a composition of pinned pieces: 3.1 (lut3d on integer RGB at the source's depth) and the last stage of 3.2
// (integer RGB -> YUV; Y per pixel, each chroma sample from the sum of the LUT's integer RGB over its OUTPUT block, 1/n folded
// into cbr..crb; a partial block at an odd edge takes the edge column / row again).  mode = -1 leaves the LUT out: the source
// codes go straight to the output stage (stage 0 of the full-range composition, 3.9 point 6).
//
// The source arrives as three component streams in R, G, B order (lutr_internal.h RgbLayout): planar gbrp, or one packed image.
//
// One source, two kinds of translation unit (Makefile MIX_RULE), like lutr_xsub.hip:
//   without LUTR_R2Y_WI   the generic kernel, the unquantised pass of the dither path and the launcher
//   LUTR_R2Y_WI / _WO     the vector kernels of one container mix (8 -> 8, 16 -> 16, 16 -> 8): 3 source kinds x 3 layouts x 4 modes
#include "lutr_device.h"
#include "lutr_launch.h"

namespace lutr {

#ifdef LUTR_R2Y_WI
// ================================================================= vector kernel, global gather
// k_yuv_xsub_vec's structure with the input side replaced: whole-dword loads and stores, 8 luma samples per thread and row,
// 2^OCSY rows per thread, lattice taps gathered from L1/L2 (frame written out: see k_yuv_vec).  NC = 1: three planes; 3 | 4: one packed image (8 pixels = 6, 8, 12 or
// 16 dwords per row, unpacked as k_packed_vec does: r2y_pixel, lutr_device.h).  The component order of a packed source is a
// wave-uniform argument.

template <int WIN, int NC, int WOUT, int OCSX, int OCSY, int INTERP>
__global__ __launch_bounds__(256) void k_rgb2yuv_vec(LutConsts L, YuvConsts K, PlaneSet P, FrameGeom G, RgbLayout Y)
{
    constexpr int PXT = 8;                                        // luma samples per thread per row
    constexpr int SW = PXT * (WIN ? 2 : 1) / 4;                   // dwords of 8 samples of one component
    constexpr int NWI = (NC == 1 ? 3 : NC) * SW;                  // source dwords per thread per row
    constexpr int YWO = PXT * (WOUT ? 2 : 1) / 4;                 // luma words out per thread per row
    constexpr int BW = 1 << OCSX, BH = 1 << OCSY;                 // the output chroma block
    constexpr int NB = PXT / BW;                                  // blocks per thread
    constexpr int CWO = (PXT >> OCSX) * (WOUT ? 2 : 1) / 4;       // chroma words out per thread
    static_assert(NB >= 1 && CWO >= 1 && YWO >= 1, "a thread must own whole words");
    const GFetch f(L);
    const unsigned uw = (unsigned)G.w / PXT;
    const unsigned ub = (unsigned)G.rows >> OCSY;
    const unsigned total = uw * ub * (unsigned)G.nframes;
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u >= total) return;
    const unsigned xu = u % uw, t = u / uw;
    const int y0 = ((G.row0 >> OCSY) + (int)(t % ub)) * BH;       // first luma row of the thread
    const long long fr = t / ub;
    const long long xo = (long long)xu * (YWO * 4), cxo = (long long)xu * (CWO * 4);

    uint32_t in[BH][NWI];
    uint32_t yo[BH][YWO], cbo[CWO], cro[CWO];
#pragma unroll
    for (int dy = 0; dy < BH; dy++) {
        if constexpr (NC == 1) {
#pragma unroll
            for (int k = 0; k < 3; k++)
                ld_words<SW>(in[dy] + k * SW, P.s[k] + fr * P.sfs[k] + (long long)(y0 + dy) * P.ss[k] + (long long)xu * (SW * 4));
        } else {
            const uint32_t *sp = (const uint32_t *)(P.s[0] + fr * P.sfs[0] + (long long)(y0 + dy) * P.ss[0]) + (size_t)xu * NWI;
#pragma unroll
            for (int k = 0; k < NWI; k++) in[dy][k] = sp[k];
        }
#pragma unroll
        for (int k = 0; k < YWO; k++) yo[dy][k] = 0;
    }
#pragma unroll
    for (int k = 0; k < CWO; k++) { cbo[k] = 0; cro[k] = 0; }

#pragma unroll
    for (int j = 0; j < NB; j++) {
        float rs = 0.f, gs = 0.f, bs = 0.f;
#pragma unroll
        for (int dy = 0; dy < BH; dy++) {
#pragma unroll
            for (int dx = 0; dx < BW; dx++) {
                const int i = j * BW + dx;
                const Rgb q = r2y_pixel<WIN, NC>(in[dy], i, Y);
                Rgb o;
                if constexpr (INTERP < 0) o = q;
                else o = lut3d_px<INTERP>(L, f, q.r, q.g, q.b);
                rs += o.r; gs += o.g; bs += o.b;
                word_put<WOUT>(yo[dy], i, rgb_to_y(K, o));
            }
        }
        word_put<WOUT>(cbo, j, rgb_to_cb(K, rs, gs, bs));
        word_put<WOUT>(cro, j, rgb_to_cr(K, rs, gs, bs));
        // Zero-instruction fence (k_yuv_vec's): keeps hipcc from hoisting the coordinates and taps of every block of the thread
        // to the top; with it the blocks are emitted one after the other.
#pragma unroll
        for (int dy = 0; dy < BH; dy++) {
#pragma unroll
            for (int k = 0; k < NWI; k++) asm volatile("" : "+v"(in[dy][k]));
#pragma unroll
            for (int k = 0; k < YWO; k++) asm volatile("" : "+v"(yo[dy][k]));
        }
#pragma unroll
        for (int k = 0; k < CWO; k++) asm volatile("" : "+v"(cbo[k]), "+v"(cro[k]));
    }
#pragma unroll
    for (int dy = 0; dy < BH; dy++)
        st_words<YWO>(P.d[0] + fr * P.dfs[0] + (long long)(y0 + dy) * P.ds[0] + xo, yo[dy]);
    const long long r = (long long)(y0 >> OCSY);
    st_words<CWO>(P.d[1] + fr * P.dfs[1] + r * P.ds[1] + cxo, cbo);
    st_words<CWO>(P.d[2] + fr * P.dfs[2] + r * P.ds[2] + cxo, cro);
}

// The vector kernels of this translation unit's container mix; the layout checks are the caller's (launch_rgb2yuv).
const char *LUTR_CAT(LUTR_CAT(launch_rgb2yuv_vec_w, LUTR_R2Y_WI), LUTR_R2Y_WO)(hipStream_t st, const LutConsts &L, const YuvConsts &K,
                                                                                const PlaneSet &P, const RgbLayout &Y,
                                                                                const FrameGeom &G, int ocsx, int ocsy, int mode)
{
    constexpr int WI = LUTR_R2Y_WI, WO = LUTR_R2Y_WO;
    const long long units = (long long)(G.w / 8) * (G.rows >> ocsy) * G.nframes;
    const dim3 grid((unsigned)((units + 255) / 256)), block(256);
#define R2Y_CASE(C, OX, OY, I, IN) \
    if (Y.step == C && ocsx == OX && ocsy == OY && mode == I) { \
        hipLaunchKernelGGL((k_rgb2yuv_vec<WI, C, WO, OX, OY, I>), grid, block, 0, st, L, K, P, G, Y); \
        return "k_rgb2yuv_vec<" LUTR_STR(LUTR_R2Y_WI) "," #C "," LUTR_STR(LUTR_R2Y_WO) "," #OX "," #OY "," IN ">"; \
    }
#define R2Y_LAYOUT(C, OX, OY) R2Y_CASE(C, OX, OY, -1, "nolut") R2Y_CASE(C, OX, OY, 0, "0") R2Y_CASE(C, OX, OY, 1, "1") R2Y_CASE(C, OX, OY, 2, "2")
#define R2Y_SRC(C) R2Y_LAYOUT(C, 1, 1) R2Y_LAYOUT(C, 1, 0) R2Y_LAYOUT(C, 0, 0)
    R2Y_SRC(1) R2Y_SRC(3) R2Y_SRC(4)
#undef R2Y_SRC
#undef R2Y_LAYOUT
#undef R2Y_CASE
    return nullptr;
}

#else  // !LUTR_R2Y_WI
// ================================================================= generic kernels
// One thread per output chroma block; any depth, stride or alignment, odd sizes, all five modes and the LUT-free form.  A pixel
// outside the frame is the edge pixel again, so a partial block sums the edge column / row twice, like np.pad(mode="edge"); only
// pixels inside the planes are written.
template <class Sink>
__device__ __forceinline__ void r2y_block(const LutConsts &L, const GFetch &f, const PlaneSet &P, const RgbLayout &Y,
                                          const FrameGeom &G, long long fr, int cx, int cy, int ocsx, int ocsy, int mode, Sink &sink)
{
    const int obw = 1 << ocsx, obh = 1 << ocsy;
    float rs = 0.f, gs = 0.f, bs = 0.f;
    for (int dy = 0; dy < obh; dy++) {
        const int yy = cy * obh + dy;
        const int y = yy < G.h ? yy : G.h - 1;
        for (int dx = 0; dx < obw; dx++) {
            const int xx = cx * obw + dx;
            const int x = xx < G.w ? xx : G.w - 1;
            const int e = x * Y.step;
            const float r = ld_sample(src_row(P, 0, fr, y), e + Y.ro, Y.wide);
            const float g = ld_sample(src_row(P, 1, fr, y), e + Y.go, Y.wide);
            const float b = ld_sample(src_row(P, 2, fr, y), e + Y.bo, Y.wide);
            const Rgb o = mode < 0 ? Rgb{r, g, b} : lut3d_px_rt(mode, L, f, r, g, b);
            rs += o.r; gs += o.g; bs += o.b;
            if (yy < G.h && xx < G.w) sink.luma(fr, x, y, o);
        }
    }
    sink.chroma(fr, cx, cy, rs, gs, bs);
}

// (the walk over output blocks and the sinks: lutr_device.h)
__global__ __launch_bounds__(256) void k_rgb2yuv_generic(LutConsts L, YuvConsts K, PlaneSet P, FrameGeom G, RgbLayout Y, int wout,
                                                         int ocsx, int ocsy, int mode)
{
    const GFetch f(L);
    PlaneSink sink{K, P, wout};
    for_each_block(G, ocsx, ocsy, false, [&](long long fr, int cx, int cy) { r2y_block(L, f, P, Y, G, fr, cx, cy, ocsx, ocsy, mode, sink); });
}

__global__ __launch_bounds__(256) void k_rgb2yuv_float(LutConsts L, YuvConsts K, PlaneSet P, FrameGeom G, RgbLayout Y, FloatPlanes F,
                                                       int ocsx, int ocsy, int mode)
{
    const GFetch f(L);
    FloatSink sink(K, F, G, ocsx, ocsy);
    for_each_block(G, ocsx, ocsy, true, [&](long long fr, int cx, int cy) { r2y_block(L, f, P, Y, G, fr, cx, cy, ocsx, ocsy, mode, sink); });
}

const char *launch_rgb2yuv_dither(hipStream_t st, const LutConsts &L, const YuvConsts &K, const PlaneSet &P, const RgbLayout &Y,
                                  const FrameGeom &G, const FloatPlanes &F, int dout, int ocsx, int ocsy, int mode)
{
    hipLaunchKernelGGL(k_rgb2yuv_float, dim3(block_grid("k_rgb2yuv_float", G.w, G.h, G.nframes, ocsx, ocsy)), dim3(256), 0, st, L, K, P, G, Y, F,
                       ocsx, ocsy, mode);
    return launch_dither_ed(st, K, P, G, F, dout > 8, ocsx, ocsy) ? "k_rgb2yuv_float+k_dither_ed" : nullptr;
}

// blue-noise dither: the same walk with a DitherSink; rows of any shard, no scratch
__global__ __launch_bounds__(256) void k_rgb2yuv_bn_generic(LutConsts L, YuvConsts K, PlaneSet P, FrameGeom G, RgbLayout Y,
                                                            const float *__restrict__ bn, int wout, int ocsx, int ocsy, int mode)
{
    const GFetch f(L);
    DitherSink sink{K, P, wout, bn, 0, 0};
    for_each_block(G, ocsx, ocsy, false, [&](long long fr, int cx, int cy) { r2y_block(L, f, P, Y, G, fr, cx, cy, ocsx, ocsy, mode, sink); });
}

const char *launch_rgb2yuv_bn(hipStream_t st, int variant, const LutConsts &L, const YuvConsts &K, const PlaneSet &P,
                              const RgbLayout &Y, const FrameGeom &G, const float *bn, int dout, int ocsx, int ocsy, int mode)
{
    if (variant == VAR_VEC_GLOBAL || variant == VAR_VEC_LDS) return nullptr;
    hipLaunchKernelGGL(k_rgb2yuv_bn_generic, dim3(block_grid("k_rgb2yuv_bn_generic", G.w, G.rows, G.nframes, ocsx, ocsy)), dim3(256), 0, st, L, K,
                       P, G, Y, bn,
                       dout > 8, ocsx, ocsy, mode);
    return "k_rgb2yuv_bn_generic";
}

// ================================================================= launcher
const char *launch_rgb2yuv(hipStream_t st, int variant, const LutConsts &L, const YuvConsts &K, const PlaneSet &P,
                           const RgbLayout &Y, const FrameGeom &G, int dout, int ocsx, int ocsy, int mode)
{
    const int win = Y.wide, wout = dout > 8;
    const int bh = 1 << ocsy;
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
        if (Y.step == 1) {
            for (int c = 0; c < 3; c++)
                if (!plane_ok(Q.s[c], Q.ss[c], Q.sfs[c], 8 * bsi, batch, kStrideAny, false)) return false;
        } else if (!plane_ok(Q.s[0], Q.ss[0], Q.sfs[0], 4, batch, kStrideAny, false)) {
            return false;
        }
        if (!plane_ok(Q.d[0], Q.ds[0], Q.dfs[0], 8 * bso, batch, kStrideAny, false)) return false;
        for (int c = 1; c < 3; c++)
            if (!plane_ok(Q.d[c], Q.ds[c], Q.dfs[c], (8 >> ocsx) * bso, batch, kStrideAny, false)) return false;
        return true;
    };
    auto vec = [&](const PlaneSet &Q, const FrameGeom &H) -> const char * {
        if (win && wout) return launch_rgb2yuv_vec_w11(st, L, K, Q, Y, H, ocsx, ocsy, mode);
        if (win) return launch_rgb2yuv_vec_w10(st, L, K, Q, Y, H, ocsx, ocsy, mode);
        return launch_rgb2yuv_vec_w00(st, L, K, Q, Y, H, ocsx, ocsy, mode);
    };
    auto generic = [&](const PlaneSet &Q, const FrameGeom &H) {
        hipLaunchKernelGGL(k_rgb2yuv_generic, dim3(block_grid("k_rgb2yuv_generic", H.w, H.rows, H.nframes, ocsx, ocsy)), dim3(256), 0, st, L, K, Q,
                           H, Y, wout, ocsx, ocsy, mode);
        return "k_rgb2yuv_generic";
    };
    // (no LDS kernel for this path; the unit is 8 luma samples wide, whole chroma blocks)
    return launch_vec_or_generic(variant, P, G, 8, vec_fits, vec, generic, [&](int wv) {
        const long long sb = (long long)wv * Y.step * bsi;
        return advance_planes(P, sb, sb, wv * bso, (wv >> ocsx) * bso);
    });
}
#endif  // LUTR_R2Y_WI

}  // namespace lutr
