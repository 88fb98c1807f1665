// lutr_rgbf.hip -- gfx950 kernels for planar float RGB sources, gbrpf32.
//
// What they replace: the reference's chain on a float source (what ffmpeg decodes an OpenEXR sequence to):
//   lut3d=file=...:interp=...   vf_lut3d.c's planar-float path on the frame itself   (ffmpeg.py:246)
//   format=<pix_fmt>            float RGB -> YUV at the output depth and layout      (ffmpeg.py:304-310)
// Per pixel: sanitise the three floats by their bit pattern (NaN -> 0, +-inf -> +-FLT_MAX), the prelut per pixel when one is set
// (prelut_interp_1d_linear on the raw table), s = clip(x * (scale * (n - 1)), 0, n - 1), interp<mode>; the result is stored as it
// is (float output), or quantised to 16-bit codes with round-half-even and handed to 3.9's output stage at lut_depth 16 (YUV
// output).  Always strict arithmetic.  Float in, float out is pixelwise and may run in place.
//
// The source arrives as three planes in R, G, B order (PlaneSet::s; the C-ABI's gbrp order is turned by gbrp_to_rgb).
//
// One source, two kinds of translation unit (Makefile), like lutr_rgb2yuv.hip:
//   without LUTR_RGBF_WO   the float -> float kernels, the generic kernels, the unquantised pass of the dither path, the launchers
//   LUTR_RGBF_WO = 0 | 1   the fused float -> YUV vector kernels of one output container: 3 layouts x 4 modes
#include <cfloat>

#include "lutr_device.h"
#include "lutr_launch.h"

namespace lutr {

// ================================================================= the pixel
// vf_lut3d.c's sanitizef: decided on the bits (the library is built with -fno-honor-nans: a comparison may be compiled away)
__device__ __forceinline__ float sanitizef(float v)
{
    const uint32_t u = __float_as_uint(v);
    if ((u & 0x7f800000u) == 0x7f800000u) {
        if (u & 0x007fffffu) return 0.0f;
        return (u & 0x80000000u) ? -FLT_MAX : FLT_MAX;
    }
    return v;
}

// FFmpeg's prelut_interp_1d_linear on channel c
__device__ __forceinline__ float prelut_px(const FloatPre &Q, int c, float x)
{
    const int last = Q.size - 1;
    const float t = med3((x - Q.min[c]) * Q.scale[c], 0.0f, (float)last);
    const int prev = (int)t;
    const int next = prev + 1 < last ? prev + 1 : last;
    const float *tab = Q.tab + (size_t)c * Q.size;
    return lerpf(tab[prev], tab[next], t - (float)prev);
}

// lattice coordinates of one sanitised pixel
__device__ __forceinline__ void rgbf_coords(const LutConsts &L, const FloatPre &Q, float r, float g, float b, float *s)
{
    float x[3] = {sanitizef(r), sanitizef(g), sanitizef(b)};
    if (Q.tab) {
#pragma unroll
        for (int c = 0; c < 3; c++) x[c] = prelut_px(Q, c, x[c]);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) s[c] = med3(x[c] * L.sc[c], 0.0f, L.lut_max);
}

template <int INTERP, class F>
__device__ __forceinline__ Rgb rgbf_px(const LutConsts &L, const FloatPre &Q, const F &f, float r, float g, float b)
{
    float s[3];
    rgbf_coords(L, Q, r, g, b, s);
    return interp<INTERP>(f, s[0], s[1], s[2]);
}

template <class F>
__device__ __forceinline__ Rgb rgbf_px_rt(int mode, const LutConsts &L, const FloatPre &Q, const F &f, float r, float g, float b)
{
    switch (mode) {
    case LUTR_INTERP_NEAREST:   return rgbf_px<LUTR_INTERP_NEAREST>(L, Q, f, r, g, b);
    case LUTR_INTERP_TRILINEAR: return rgbf_px<LUTR_INTERP_TRILINEAR>(L, Q, f, r, g, b);
    case LUTR_INTERP_PYRAMID:   return rgbf_px<LUTR_INTERP_PYRAMID>(L, Q, f, r, g, b);
    case LUTR_INTERP_PRISM:     return rgbf_px<LUTR_INTERP_PRISM>(L, Q, f, r, g, b);
    default:                    return rgbf_px<LUTR_INTERP_TETRAHEDRAL>(L, Q, f, r, g, b);
    }
}

// float -> the 16-bit code swscale's planar-float reader makes of it: round half to even, then clip (held as a float)
__device__ __forceinline__ float quant16(float v) { return med3(__builtin_rintf(v * 65535.0f), 0.0f, 65535.0f); }
__device__ __forceinline__ Rgb quant16(const Rgb &v) { return Rgb{quant16(v.r), quant16(v.g), quant16(v.b)}; }

// mode < 0: no lut3d -- sanitise and quantise only
template <int INTERP, class F>
__device__ __forceinline__ Rgb rgbf_codes(const LutConsts &L, const FloatPre &Q, const F &f, float r, float g, float b)
{
    if constexpr (INTERP < 0) return quant16(Rgb{sanitizef(r), sanitizef(g), sanitizef(b)});
    else return quant16(rgbf_px<INTERP>(L, Q, f, r, g, b));
}

#ifdef LUTR_RGBF_WO
// ================================================================= fused float -> YUV vector kernel, global gather
// k_rgb2yuv_vec's structure with the input side replaced: a thread owns 8 luma samples by 2^OCSY rows, loads them as two dwordx4
// per plane and row, and stores whole dwords of Y, Cb and Cr.  (Frame written out: see k_yuv_vec.)
template <int WOUT, int OCSX, int OCSY, int INTERP>
__global__ __launch_bounds__(256) void k_rgbf2yuv_vec(LutConsts L, FloatPre Q, YuvConsts K, PlaneSet P, FrameGeom G)
{
    constexpr int PXT = 8;                                        // luma samples per thread per row
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

    float in[BH][3][PXT];
    uint32_t yo[BH][YWO], cbo[CWO], cro[CWO];
#pragma unroll
    for (int dy = 0; dy < BH; dy++) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float4 *sp = (const float4 *)(P.s[k] + fr * P.sfs[k] + (long long)(y0 + dy) * P.ss[k] + (long long)xu * (PXT * 4));
            const float4 a = sp[0], b = sp[1];
            in[dy][k][0] = a.x; in[dy][k][1] = a.y; in[dy][k][2] = a.z; in[dy][k][3] = a.w;
            in[dy][k][4] = b.x; in[dy][k][5] = b.y; in[dy][k][6] = b.z; in[dy][k][7] = b.w;
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
                const Rgb o = rgbf_codes<INTERP>(L, Q, f, in[dy][0][i], in[dy][1][i], in[dy][2][i]);
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
            for (int k = 0; k < 3; k++) {
#pragma unroll
                for (int i = 0; i < PXT; i++) asm volatile("" : "+v"(in[dy][k][i]));
            }
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

// The vector kernels of this translation unit's output container; the layout checks are the caller's (launch_rgbf2yuv).
const char *LUTR_CAT(launch_rgbf2yuv_vec_w, LUTR_RGBF_WO)(hipStream_t st, const LutConsts &L, const FloatPre &Q, const YuvConsts &K,
                                                         const PlaneSet &P, const FrameGeom &G, int ocsx, int ocsy, int mode)
{
    constexpr int WO = LUTR_RGBF_WO;
    const long long units = (long long)(G.w / 8) * (G.rows >> ocsy) * G.nframes;
    const dim3 grid((unsigned)((units + 255) / 256)), block(256);
#define RGBF_CASE(OX, OY, I, IN) \
    if (ocsx == OX && ocsy == OY && mode == I) { \
        hipLaunchKernelGGL((k_rgbf2yuv_vec<WO, OX, OY, I>), grid, block, 0, st, L, Q, K, P, G); \
        return "k_rgbf2yuv_vec<" LUTR_STR(LUTR_RGBF_WO) "," #OX "," #OY "," IN ">"; \
    }
#define RGBF_LAYOUT(OX, OY) RGBF_CASE(OX, OY, -1, "nolut") RGBF_CASE(OX, OY, 0, "0") RGBF_CASE(OX, OY, 1, "1") RGBF_CASE(OX, OY, 2, "2")
    RGBF_LAYOUT(1, 1) RGBF_LAYOUT(1, 0) RGBF_LAYOUT(0, 0)
#undef RGBF_LAYOUT
#undef RGBF_CASE
    return nullptr;
}

#else  // !LUTR_RGBF_WO
// ================================================================= float -> float vector kernel, global gather
// A thread owns 4 pixels of a row: one dwordx4 load per plane, lattice taps gathered from L1/L2, one dwordx4 store per plane.
// The thread reads its pixels before it writes them and no other thread touches them: src == dst is fine.
template <int INTERP>
__global__ __launch_bounds__(256) void k_rgbf_vec(LutConsts L, FloatPre Q, PlaneSet P, FrameGeom G)
{
    const GFetch f(L);
    const unsigned uw = (unsigned)G.w / 4;
    const unsigned total = uw * (unsigned)G.rows * (unsigned)G.nframes;
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u >= total) return;
    const unsigned xu = u % uw, t = u / uw;
    const long long y = G.row0 + (int)(t % (unsigned)G.rows), fr = t / (unsigned)G.rows;
    float in[3][4], out[3][4];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float4 v = *(const float4 *)(P.s[k] + fr * P.sfs[k] + y * P.ss[k] + (long long)xu * 16);
        in[k][0] = v.x; in[k][1] = v.y; in[k][2] = v.z; in[k][3] = v.w;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const Rgb o = rgbf_px<INTERP>(L, Q, f, in[0][i], in[1][i], in[2][i]);
        out[0][i] = o.r; out[1][i] = o.g; out[2][i] = o.b;
    }
#pragma unroll
    for (int k = 0; k < 3; k++)
        *(float4 *)(P.d[k] + fr * P.dfs[k] + y * P.ds[k] + (long long)xu * 16) = make_float4(out[k][0], out[k][1], out[k][2], out[k][3]);
}

// ================================================================= generic kernels
// float -> float, one thread per pixel: any 4-byte aligned layout, negative strides, all five modes
__global__ __launch_bounds__(256) void k_rgbf_generic(LutConsts L, FloatPre Q, PlaneSet P, FrameGeom G, int mode)
{
    const GFetch f(L);
    const long long total = (long long)G.w * G.rows * G.nframes;
    for (long long u = blockIdx.x * 256ll + threadIdx.x; u < total; u += (long long)gridDim.x * 256ll) {
        const int x = (int)(u % G.w);
        const long long t = u / G.w;
        const long long y = G.row0 + (int)(t % G.rows), fr = t / G.rows;
        const float r = ((const float *)src_row(P, 0, fr, y))[x];
        const float g = ((const float *)src_row(P, 1, fr, y))[x];
        const float b = ((const float *)src_row(P, 2, fr, y))[x];
        const Rgb o = rgbf_px_rt(mode, L, Q, f, r, g, b);
        ((float *)dst_row(P, 0, fr, y))[x] = o.r;
        ((float *)dst_row(P, 1, fr, y))[x] = o.g;
        ((float *)dst_row(P, 2, fr, y))[x] = o.b;
    }
}

// float -> YUV by output chroma blocks (r2y_block's walk, lutr_rgb2yuv.hip): a pixel outside the frame is the edge pixel again
template <class Sink>
__device__ __forceinline__ void rgbf_block(const LutConsts &L, const FloatPre &Q, const GFetch &f, const PlaneSet &P,
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
            const float r = ((const float *)src_row(P, 0, fr, y))[x];
            const float g = ((const float *)src_row(P, 1, fr, y))[x];
            const float b = ((const float *)src_row(P, 2, fr, y))[x];
            const Rgb o = mode < 0 ? rgbf_codes<-1>(L, Q, f, r, g, b) : quant16(rgbf_px_rt(mode, L, Q, f, r, g, b));
            rs += o.r; gs += o.g; bs += o.b;
            if (yy < G.h && xx < G.w) sink.luma(fr, x, y, o);
        }
    }
    sink.chroma(fr, cx, cy, rs, gs, bs);
}

// (the walk over output blocks and the sinks: lutr_device.h)
__global__ __launch_bounds__(256) void k_rgbf2yuv_generic(LutConsts L, FloatPre Q, YuvConsts K, PlaneSet P, FrameGeom G, int wout,
                                                          int ocsx, int ocsy, int mode)
{
    const GFetch f(L);
    PlaneSink sink{K, P, wout};
    for_each_block(G, ocsx, ocsy, false, [&](long long fr, int cx, int cy) { rgbf_block(L, Q, f, P, G, fr, cx, cy, ocsx, ocsy, mode, sink); });
}

// the dither path's pass 1: unquantised Y, Cb, Cr of whole frames
__global__ __launch_bounds__(256) void k_rgbf2yuv_float(LutConsts L, FloatPre Q, YuvConsts K, PlaneSet P, FrameGeom G, FloatPlanes F,
                                                        int ocsx, int ocsy, int mode)
{
    const GFetch f(L);
    FloatSink sink(K, F, G, ocsx, ocsy);
    for_each_block(G, ocsx, ocsy, true, [&](long long fr, int cx, int cy) { rgbf_block(L, Q, f, P, G, fr, cx, cy, ocsx, ocsy, mode, sink); });
}

// blue-noise dither: the same walk with a DitherSink; rows of any shard, no scratch
__global__ __launch_bounds__(256) void k_rgbf2yuv_bn_generic(LutConsts L, FloatPre Q, YuvConsts K, PlaneSet P, FrameGeom G,
                                                             const float *__restrict__ bn, int wout, int ocsx, int ocsy, int mode)
{
    const GFetch f(L);
    DitherSink sink{K, P, wout, bn, 0, 0};
    for_each_block(G, ocsx, ocsy, false, [&](long long fr, int cx, int cy) { rgbf_block(L, Q, f, P, G, fr, cx, cy, ocsx, ocsy, mode, sink); });
}

// ================================================================= launchers
const char *launch_rgbf(hipStream_t st, int variant, const LutConsts &L, const FloatPre &Q, const PlaneSet &P, const FrameGeom &G,
                        int mode)
{
    const bool batch = G.nframes > 1;
    auto vec_fits = [&](const PlaneSet &S, const FrameGeom &H) {
        if (!vec_mode(mode) || H.w % 4) return false;
        if (!units_fit((long long)(H.w / 4) * H.rows * H.nframes)) return false;
        for (int c = 0; c < 3; c++)
            if (!planes_ok(S, c, 16, batch, kStrideAny, false)) return false;
        return true;
    };
    auto vec = [&](const PlaneSet &S, const FrameGeom &H) -> const char * {
        const dim3 grid(grid_for((long long)(H.w / 4) * H.rows * H.nframes)), block(256);
        switch (mode) {
        case LUTR_INTERP_NEAREST:   hipLaunchKernelGGL(k_rgbf_vec<LUTR_INTERP_NEAREST>, grid, block, 0, st, L, Q, S, H); return "k_rgbf_vec<0>";
        case LUTR_INTERP_TRILINEAR: hipLaunchKernelGGL(k_rgbf_vec<LUTR_INTERP_TRILINEAR>, grid, block, 0, st, L, Q, S, H); return "k_rgbf_vec<1>";
        default:                    hipLaunchKernelGGL(k_rgbf_vec<LUTR_INTERP_TETRAHEDRAL>, grid, block, 0, st, L, Q, S, H); return "k_rgbf_vec<2>";
        }
    };
    auto generic = [&](const PlaneSet &S, const FrameGeom &H) {
        hipLaunchKernelGGL(k_rgbf_generic, dim3(stride_grid("k_rgbf_generic", (long long)H.w * H.rows * H.nframes, kGridStrideCap)), dim3(256), 0,
                           st, L, Q,
                           S, H, mode);
        return "k_rgbf_generic";
    };
    // (no LDS kernel for this path; the unit is 4 pixels wide)
    return launch_vec_or_generic(variant, P, G, 4, vec_fits, vec, generic, [&](int wv) {
        return advance_planes(P, (long long)wv * 4, (long long)wv * 4, (long long)wv * 4, (long long)wv * 4);
    });
}

const char *launch_rgbf2yuv_dither(hipStream_t st, const LutConsts &L, const FloatPre &Q, const YuvConsts &K, const PlaneSet &P,
                                   const FrameGeom &G, const FloatPlanes &F, int dout, int ocsx, int ocsy, int mode)
{
    hipLaunchKernelGGL(k_rgbf2yuv_float, dim3(block_grid("k_rgbf2yuv_float", G.w, G.h, G.nframes, ocsx, ocsy)), dim3(256), 0, st, L, Q, K, P, G, F,
                       ocsx, ocsy, mode);
    return launch_dither_ed(st, K, P, G, F, dout > 8, ocsx, ocsy) ? "k_rgbf2yuv_float+k_dither_ed" : nullptr;
}

const char *launch_rgbf2yuv_bn(hipStream_t st, int variant, const LutConsts &L, const FloatPre &Q, const YuvConsts &K,
                               const PlaneSet &P, const FrameGeom &G, const float *bn, int dout, int ocsx, int ocsy, int mode)
{
    if (variant == VAR_VEC_GLOBAL || variant == VAR_VEC_LDS) return nullptr;
    hipLaunchKernelGGL(k_rgbf2yuv_bn_generic, dim3(block_grid("k_rgbf2yuv_bn_generic", G.w, G.rows, G.nframes, ocsx, ocsy)), dim3(256), 0, st, L, Q,
                       K, P, G, bn,
                       dout > 8, ocsx, ocsy, mode);
    return "k_rgbf2yuv_bn_generic";
}

const char *launch_rgbf2yuv(hipStream_t st, int variant, const LutConsts &L, const FloatPre &Q, const YuvConsts &K, const PlaneSet &P,
                            const FrameGeom &G, int dout, int ocsx, int ocsy, int mode)
{
    const int wout = dout > 8;
    const int bh = 1 << ocsy;
    const long long bso = wout ? 2 : 1;
    const bool batch = G.nframes > 1;
    auto vec_fits = [&](const PlaneSet &S, const FrameGeom &H) {
        if (!(mode == -1 || vec_mode(mode))) return false;
        if (H.w % 8 || H.row0 % bh || H.rows % bh) return false;
        if (!units_fit((long long)(H.w / 8) * (H.rows / bh) * H.nframes)) return false;
        for (int c = 0; c < 3; c++)
            if (!plane_ok(S.s[c], S.ss[c], S.sfs[c], 16, batch, kStrideAny, false)) return false;
        if (!plane_ok(S.d[0], S.ds[0], S.dfs[0], 8 * bso, batch, kStrideAny, false)) return false;
        for (int c = 1; c < 3; c++)
            if (!plane_ok(S.d[c], S.ds[c], S.dfs[c], (8 >> ocsx) * bso, batch, kStrideAny, false)) return false;
        return true;
    };
    auto vec = [&](const PlaneSet &S, const FrameGeom &H) -> const char * {
        return wout ? launch_rgbf2yuv_vec_w1(st, L, Q, K, S, H, ocsx, ocsy, mode) : launch_rgbf2yuv_vec_w0(st, L, Q, K, S, H, ocsx, ocsy, mode);
    };
    auto generic = [&](const PlaneSet &S, const FrameGeom &H) {
        hipLaunchKernelGGL(k_rgbf2yuv_generic, dim3(block_grid("k_rgbf2yuv_generic", H.w, H.rows, H.nframes, ocsx, ocsy)), dim3(256), 0, st, L, Q,
                           K, S, H, wout, ocsx, ocsy, mode);
        return "k_rgbf2yuv_generic";
    };
    // (no LDS kernel for this path; the unit is 8 luma samples wide, whole chroma blocks)
    return launch_vec_or_generic(variant, P, G, 8, vec_fits, vec, generic, [&](int wv) {
        return advance_planes(P, (long long)wv * 4, (long long)wv * 4, wv * bso, (wv >> ocsx) * bso);
    });
}
#endif  // LUTR_RGBF_WO

}  // namespace lutr
