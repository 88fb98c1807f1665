// lutr_premul.hip -- gfx950 kernels for premultiplied alpha: unpremultiply, lut3d, premultiply in one pass.
//
// What they add: a non-linear LUT on premultiplied colour is wrong wherever 0 < alpha < 1 (look(a * c) is not a * look(c)), and
// the two steps that mend it sit between stages that live inside the fused kernels.  Integer YUV (yuva* sources), per luma
// position with `a` the source's alpha code there, Ma = 2^din - 1, Ml = 2^lut_depth - 1:
//   q   = YUV -> integer RGB at the LUT depth            (3.2; chroma replicated over its INPUT block)
//   S   = min(Ml, floor((q * Ma + floor(a / 2)) / a))    a > 0; S = q for a == 0       (exact integers)
//   o   = lut3d(S)  truncated and clipped to [0, Ml]     (3.1; all five modes, a .csp prelut taken)
//   P   = floor((o * a + floor(Ma / 2)) / Ma)
//   out = integer RGB -> YUV from P                      (3.2 / 3.8; chroma = mean over its OUTPUT block)
// The unit of work is 3.8's union block for every pair of layouts, the equal ones included.  The alpha plane of the output is
// lutr_alpha_plane's (3.16), launched by the caller after this pass.
// Float RGB (gbrapf32le), per pixel with t = clamp(a, 0, 1) (NaN -> 0 on its bits):
//   S = sanitize(sanitize(c) / t) for t > 0, sanitize(c) for t == 0;  out = lut3d_float(S) * t   (3.10's path in between)
//
// One source, two kinds of translation unit (Makefile MIX_RULE):
//   without LUTR_PM_WI   the generic kernels, the float kernels and the launchers
//   LUTR_PM_WI / _WO     the YUV vector kernels of one container mix (8 -> 8, 16 -> 16, 16 -> 8): 9 layout pairs x 3 modes
#include <cfloat>
#include <string>

#include "lutr_device.h"
#include "lutr_launch.h"

namespace lutr {

// ================================================================= the integer pixel
// unpremultiply, lut3d, premultiply on the integer RGB codes q (held as floats, like everywhere); a = the alpha code, <= M.ma
template <class Lut>
__device__ __forceinline__ Rgb premul_px(const PremulConsts &M, uint32_t a, const Rgb &q, Lut lut)
{
    // one reciprocal serves the three divisions of the pixel (v_rcp_f32 is good to 1 ulp, div_q16 allows 2)
    UnpremulPx u;
    u.den = a ? a : M.ma;
    u.half = a >> 1;
    u.lim = mad24(M.ml, u.den, 0u);
    u.rcp = __builtin_amdgcn_rcpf((float)u.den);
    const float sr = (float)unpremul_code((uint32_t)q.r, u, M.ma);
    const float sg = (float)unpremul_code((uint32_t)q.g, u, M.ma);
    const float sb = (float)unpremul_code((uint32_t)q.b, u, M.ma);
    const Rgb o = lut(sr, sg, sb);
    Rgb p;
    p.r = (float)premul_code((uint32_t)o.r, a, M.ma, M.din);
    p.g = (float)premul_code((uint32_t)o.g, a, M.ma, M.din);
    p.b = (float)premul_code((uint32_t)o.b, a, M.ma, M.din);
    return p;
}

__device__ __forceinline__ uint32_t umin_(uint32_t a, uint32_t b) { return a < b ? a : b; }

#ifdef LUTR_PM_WI
// ================================================================= vector kernel, global gather
template <int WIDE>
__device__ __forceinline__ uint32_t word_code(const uint32_t *w, int i)
{
    if constexpr (WIDE) return (w[i >> 1] >> ((i & 1) * 16)) & 0xffffu;
    else return (w[i >> 2] >> ((i & 3) * 8)) & 0xffu;
}

// union_vec_unit's structure (lutr_device.h) without the dither offsets: whole-word loads and stores, the union block walk,
// taps gathered from L1 / L2.  The thread's alpha words are loaded beside its luma words (BH rows, the same word count); the two
// integer steps sit around lut3d_px.
template <int WIN, int WOUT, int ICSX, int ICSY, int OCSX, int OCSY, int INTERP>
__global__ __launch_bounds__(256) void k_yuva_premul_vec(LutConsts L, YuvConsts K, PremulConsts M, PremulPlanes PP, FrameGeom G)
{
    constexpr int VB = vec_bytes<WIN, WOUT>();
    constexpr int PXT = VB / (WIN ? 2 : 1);                       // luma samples per thread per row
    constexpr int YWI = VB / 4, YWO = PXT * (WOUT ? 2 : 1) / 4;   // luma (and alpha) words per thread per row, in / out
    constexpr int CSX = cmax(ICSX, OCSX), CSY = cmax(ICSY, OCSY);
    constexpr int BW = 1 << CSX, BH = 1 << CSY;                   // the union block
    constexpr int NB = PXT / BW;                                  // union blocks per thread
    constexpr int IRH = BH >> ICSY, ORH = BH >> OCSY;             // chroma rows per thread, in / out
    constexpr int IBX = BW >> ICSX, OBX = BW >> OCSX;             // chroma samples per union block and row, in / out
    constexpr int CWI = (PXT >> ICSX) * (WIN ? 2 : 1) / 4, CWO = (PXT >> OCSX) * (WOUT ? 2 : 1) / 4;
    static_assert(NB >= 1 && CWI >= 1 && CWO >= 1 && YWO >= 1, "a thread must own whole words");
    const PlaneSet &P = PP.p;
    const GFetch f(L);
    const unsigned uw = (unsigned)G.w / PXT;
    const unsigned ub = (unsigned)G.rows >> CSY;
    const unsigned total = uw * ub * (unsigned)G.nframes;
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u >= total) return;
    const unsigned xu = u % uw, t = u / uw;
    const int y0 = ((G.row0 >> CSY) + (int)(t % ub)) * BH;        // first luma row of the thread
    const long long fr = t / ub;
    const long long xi = (long long)xu * VB, xo = (long long)xu * (YWO * 4), cxi = (long long)xu * (CWI * 4),
                    cxo = (long long)xu * (CWO * 4);

    uint32_t yw[BH][YWI], aw[BH][YWI], cbw[IRH][CWI], crw[IRH][CWI];
    uint32_t yo[BH][YWO], cbo[ORH][CWO], cro[ORH][CWO];
#pragma unroll
    for (int dy = 0; dy < BH; dy++) {
        ld_words<YWI>(yw[dy], P.s[0] + fr * P.sfs[0] + (long long)(y0 + dy) * P.ss[0] + xi);
        ld_words<YWI>(aw[dy], PP.a.a + fr * PP.a.afs + (long long)(y0 + dy) * PP.a.as + xi);
#pragma unroll
        for (int k = 0; k < YWO; k++) yo[dy][k] = 0;
    }
#pragma unroll
    for (int iy = 0; iy < IRH; iy++) {
        const long long r = (long long)((y0 >> ICSY) + iy);
        ld_words<CWI>(cbw[iy], P.s[1] + fr * P.sfs[1] + r * P.ss[1] + cxi);
        ld_words<CWI>(crw[iy], P.s[2] + fr * P.sfs[2] + r * P.ss[2] + cxi);
    }
#pragma unroll
    for (int oy = 0; oy < ORH; oy++)
#pragma unroll
        for (int k = 0; k < CWO; k++) { cbo[oy][k] = 0; cro[oy][k] = 0; }

#pragma unroll
    for (int j = 0; j < NB; j++) {
        Chroma c[IRH][IBX];
#pragma unroll
        for (int iy = 0; iy < IRH; iy++)
#pragma unroll
            for (int ix = 0; ix < IBX; ix++)
                c[iy][ix] = chroma_terms(K, word_sample<WIN>(cbw[iy], j * IBX + ix), word_sample<WIN>(crw[iy], j * IBX + ix));
        float rs[ORH][OBX], gs[ORH][OBX], bs[ORH][OBX];
#pragma unroll
        for (int oy = 0; oy < ORH; oy++)
#pragma unroll
            for (int ox = 0; ox < OBX; ox++) { rs[oy][ox] = 0.f; gs[oy][ox] = 0.f; bs[oy][ox] = 0.f; }
#pragma unroll
        for (int dy = 0; dy < BH; dy++) {
#pragma unroll
            for (int dx = 0; dx < BW; dx++) {
                const int i = j * BW + dx;
                const Rgb q = yuv_to_rgb(K, word_sample<WIN>(yw[dy], i), c[dy >> ICSY][dx >> ICSX]);
                const uint32_t a = umin_(word_code<WIN>(aw[dy], i), M.ma);
                const Rgb o = premul_px(M, a, q, [&](float r, float g, float b) { return lut3d_px<INTERP>(L, f, r, g, b); });
                rs[dy >> OCSY][dx >> OCSX] += o.r; gs[dy >> OCSY][dx >> OCSX] += o.g; bs[dy >> OCSY][dx >> OCSX] += o.b;
                word_put<WOUT>(yo[dy], i, rgb_to_y(K, o));
            }
        }
#pragma unroll
        for (int oy = 0; oy < ORH; oy++)
#pragma unroll
            for (int ox = 0; ox < OBX; ox++) {
                const int i = j * OBX + ox;
                word_put<WOUT>(cbo[oy], i, rgb_to_cb(K, rs[oy][ox], gs[oy][ox], bs[oy][ox]));
                word_put<WOUT>(cro[oy], i, rgb_to_cr(K, rs[oy][ox], gs[oy][ox], bs[oy][ox]));
            }
        // Zero-instruction fence (k_yuv_vec's): keeps hipcc from hoisting the coordinates and taps of every union block of the
        // thread to the top; with it the blocks are emitted one after the other.
#pragma unroll
        for (int dy = 0; dy < BH; dy++) {
#pragma unroll
            for (int k = 0; k < YWI; k++) asm volatile("" : "+v"(yw[dy][k]), "+v"(aw[dy][k]));
#pragma unroll
            for (int k = 0; k < YWO; k++) asm volatile("" : "+v"(yo[dy][k]));
        }
#pragma unroll
        for (int iy = 0; iy < IRH; iy++)
#pragma unroll
            for (int k = 0; k < CWI; k++) asm volatile("" : "+v"(cbw[iy][k]), "+v"(crw[iy][k]));
#pragma unroll
        for (int oy = 0; oy < ORH; oy++)
#pragma unroll
            for (int k = 0; k < CWO; k++) asm volatile("" : "+v"(cbo[oy][k]), "+v"(cro[oy][k]));
    }
#pragma unroll
    for (int dy = 0; dy < BH; dy++)
        st_words<YWO>(P.d[0] + fr * P.dfs[0] + (long long)(y0 + dy) * P.ds[0] + xo, yo[dy]);
#pragma unroll
    for (int oy = 0; oy < ORH; oy++) {
        const long long r = (long long)((y0 >> OCSY) + oy);
        st_words<CWO>(P.d[1] + fr * P.dfs[1] + r * P.ds[1] + cxo, cbo[oy]);
        st_words<CWO>(P.d[2] + fr * P.dfs[2] + r * P.ds[2] + cxo, cro[oy]);
    }
}

// The vector kernels of this translation unit's container mix; the layout checks are the caller's (launch_yuva_premul).
const char *LUTR_CAT(LUTR_CAT(launch_yuva_premul_vec_w, LUTR_PM_WI), LUTR_PM_WO)(hipStream_t st, const LutConsts &L, const YuvConsts &K,
                                                                                 const PremulConsts &M, const PremulPlanes &P,
                                                                                 const FrameGeom &G, int icsx, int icsy, int ocsx,
                                                                                 int ocsy, int mode)
{
    constexpr int WI = LUTR_PM_WI, WO = LUTR_PM_WO;
    constexpr int PXT = vec_bytes<WI, WO>() / (WI ? 2 : 1);
    const int bh = 1 << cmax(icsy, ocsy);
    const long long units = (long long)(G.w / PXT) * (G.rows / bh) * G.nframes;
    const dim3 grid((unsigned)((units + 255) / 256)), block(256);
#define PM_CASE(IX, IY, OX, OY, I) \
    if (icsx == IX && icsy == IY && ocsx == OX && ocsy == OY && mode == I) { \
        hipLaunchKernelGGL((k_yuva_premul_vec<WI, WO, IX, IY, OX, OY, I>), grid, block, 0, st, L, K, M, P, G); \
        return "k_yuva_premul_vec<" LUTR_STR(LUTR_PM_WI) "," LUTR_STR(LUTR_PM_WO) "," #IX "," #IY "," #OX "," #OY "," #I ">"; \
    }
#define PM_PAIR(IX, IY, OX, OY) PM_CASE(IX, IY, OX, OY, 0) PM_CASE(IX, IY, OX, OY, 1) PM_CASE(IX, IY, OX, OY, 2)
    PM_PAIR(1, 1, 1, 1) PM_PAIR(1, 1, 1, 0) PM_PAIR(1, 1, 0, 0)
    PM_PAIR(1, 0, 1, 1) PM_PAIR(1, 0, 1, 0) PM_PAIR(1, 0, 0, 0)
    PM_PAIR(0, 0, 1, 1) PM_PAIR(0, 0, 1, 0) PM_PAIR(0, 0, 0, 0)
#undef PM_PAIR
#undef PM_CASE
    return nullptr;
}

#else  // !LUTR_PM_WI
// ================================================================= generic kernel, integer YUV
// One thread per union block; any depth, stride or alignment, odd sizes, all five modes.  xsub_union_block's walk (lutr_device.h)
// with the alpha code of each pixel: a pixel outside the frame is the edge pixel again (its luma, its chroma and its alpha); only
// pixels and chroma samples inside the planes are written.
__global__ __launch_bounds__(256) void k_yuva_premul_generic(LutConsts L, YuvConsts K, PremulConsts M, PremulPlanes PP, FrameGeom G,
                                                             int win, int wout, int icsx, int icsy, int ocsx, int ocsy, int mode)
{
    const PlaneSet &P = PP.p;
    const GFetch f(L);
    PlaneSink sink{K, P, wout};
    const int csx = cmax(icsx, ocsx), csy = cmax(icsy, ocsy);
    const int bw = 1 << csx, bh = 1 << csy, obw = 1 << ocsx, obh = 1 << ocsy;
    const int cwo = (G.w + obw - 1) >> ocsx, cho = (G.h + obh - 1) >> ocsy;
    for_each_block(G, csx, csy, false, [&](long long fr, int ux, int uy) {
        for (int oy = 0; oy < bh; oy += obh) {
            for (int ox = 0; ox < bw; ox += obw) {
                float rs = 0.f, gs = 0.f, bs = 0.f;
                for (int dy = 0; dy < obh; dy++) {
                    const int yy = uy * bh + oy + dy;
                    const int y = yy < G.h ? yy : G.h - 1;
                    for (int dx = 0; dx < obw; dx++) {
                        const int xx = ux * bw + ox + dx;
                        const int x = xx < G.w ? xx : G.w - 1;
                        const float cbv = ld_sample(src_row(P, 1, fr, y >> icsy), x >> icsx, win);
                        const float crv = ld_sample(src_row(P, 2, fr, y >> icsy), x >> icsx, win);
                        const float yv = ld_sample(src_row(P, 0, fr, y), x, win);
                        const uint8_t *arow = PP.a.a + fr * PP.a.afs + (long long)y * PP.a.as;
                        const uint32_t a = umin_(win ? ((const uint16_t *)arow)[x] : arow[x], M.ma);
                        const Rgb q = yuv_to_rgb(K, yv, chroma_terms(K, cbv, crv));
                        const Rgb o = premul_px(M, a, q, [&](float r, float g, float b) { return lut3d_px_rt(mode, L, f, r, g, b); });
                        rs += o.r; gs += o.g; bs += o.b;
                        if (yy < G.h && xx < G.w) sink.luma(fr, x, y, o);
                    }
                }
                const int ocx = (ux * bw + ox) >> ocsx, ocy = (uy * bh + oy) >> ocsy;
                if (ocx < cwo && ocy < cho) sink.chroma(fr, ocx, ocy, rs, gs, bs);
            }
        }
    });
}

// ================================================================= launcher, integer YUV
const char *launch_yuva_premul(hipStream_t st, int variant, const LutConsts &L, const YuvConsts &K, const PremulPlanes &P,
                               const FrameGeom &G, int din, int dout, int lut_depth, int icsx, int icsy, int ocsx, int ocsy, int mode)
{
    const int win = din > 8, wout = dout > 8;
    const int csx = cmax(icsx, ocsx), csy = cmax(icsy, ocsy), bh = 1 << csy;
    PremulConsts M;
    M.ma = (1u << din) - 1u;
    M.ml = (1u << lut_depth) - 1u;
    M.din = din;
    // the vector kernels' unit: 8 bytes of luma and of alpha per row (16 for a 16-bit source written as 8 bit); 8 -> 16 bit has none
    const bool mix_ok = win == wout || (win && !wout);
    const int pxt = (win && !wout) ? 8 : (win ? 4 : 8);
    const long long bsi = win ? 2 : 1, bso = wout ? 2 : 1;
    const bool batch = G.nframes > 1;
    int ran = 0;                                 // bit 0: a vector kernel was launched, bit 1: the generic one
    auto vec_fits = [&](const PremulPlanes &R, const FrameGeom &H) {
        const PlaneSet &Q = R.p;
        if (!mix_ok || !vec_mode(mode)) return false;
        if (H.w % pxt || H.row0 % bh || H.rows % bh) return false;
        if (!units_fit((long long)(H.w / pxt) * (H.rows / bh) * H.nframes)) return false;
        if (!plane_ok(Q.s[0], Q.ss[0], Q.sfs[0], pxt * bsi, batch, kStrideAny, false) || !plane_ok(Q.d[0], Q.ds[0], Q.dfs[0], pxt * bso, batch, kStrideAny, false))
            return false;
        if (!plane_ok(R.a.a, R.a.as, R.a.afs, pxt * bsi, batch, kStrideAny, false)) return false;    // aligned and dense like luma
        for (int c = 1; c < 3; c++)
            if (!plane_ok(Q.s[c], Q.ss[c], Q.sfs[c], (pxt >> icsx) * bsi, batch, kStrideAny, false) ||
                !plane_ok(Q.d[c], Q.ds[c], Q.dfs[c], (pxt >> ocsx) * bso, batch, kStrideAny, false))
                return false;
        return true;
    };
    auto vec = [&](const PremulPlanes &R, const FrameGeom &H) -> const char * {
        ran |= 1;
        if (win && wout) return launch_yuva_premul_vec_w11(st, L, K, M, R, H, icsx, icsy, ocsx, ocsy, mode);
        if (win) return launch_yuva_premul_vec_w10(st, L, K, M, R, H, icsx, icsy, ocsx, ocsy, mode);
        return launch_yuva_premul_vec_w00(st, L, K, M, R, H, icsx, icsy, ocsx, ocsy, mode);
    };
    auto generic = [&](const PremulPlanes &R, const FrameGeom &H) {
        ran |= 2;
        hipLaunchKernelGGL(k_yuva_premul_generic, dim3(block_grid("k_yuva_premul_generic", H.w, H.rows, H.nframes, csx, csy)), dim3(256), 0, st, L,
                           K, M, R, H,
                           win, wout, icsx, icsy, ocsx, ocsy, mode);
        return "k_yuva_premul_generic";
    };
    // (no LDS-window kernel for this path; the unit is 4 or 8 luma samples wide, whole union blocks)
    const char *name = launch_vec_or_generic(variant, P, G, pxt, vec_fits, vec, generic, [&](int wv) {
        PremulPlanes R = P;
        R.p = advance_planes(P.p, wv * bsi, (wv >> icsx) * bsi, wv * bso, (wv >> ocsx) * bso);
        R.a.a += wv * bsi;
        return R;
    });
    if (!name || ran != 3) return name;
    // a ragged width split between the two kernels: both are named
    static thread_local std::string both;
    both = std::string(name) + "+k_yuva_premul_generic";
    return both.c_str();
}

// ================================================================= the float pixel
// (3.10's pixel, as lutr_rgbf.hip has it: sanitise on the bits, the prelut per pixel on the raw table, the lattice coordinates)
__device__ __forceinline__ float pm_sanitizef(float v)
{
    const uint32_t u = __float_as_uint(v);
    if ((u & 0x7f800000u) == 0x7f800000u) {
        if (u & 0x007fffffu) return 0.0f;
        return (u & 0x80000000u) ? -FLT_MAX : FLT_MAX;
    }
    return v;
}

__device__ __forceinline__ float pm_prelut_px(const FloatPre &Q, int c, float x)
{
    const int last = Q.size - 1;
    const float t = med3((x - Q.min[c]) * Q.scale[c], 0.0f, (float)last);
    const int prev = (int)t;
    const int next = prev + 1 < last ? prev + 1 : last;
    const float *tab = Q.tab + (size_t)c * Q.size;
    return lerpf(tab[prev], tab[next], t - (float)prev);
}

// t = clamp(a, 0, 1); NaN -> 0, decided on the bits (the library is built with -fno-honor-nans)
__device__ __forceinline__ float pm_alpha_t(float a)
{
    const uint32_t u = __float_as_uint(a);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0.0f;
    return a > 0.0f ? fminf(a, 1.0f) : 0.0f;                      // (-0 and everything below: +0)
}

// One pixel: S = sanitize(c) / t (one correctly rounded fp32 division: plain `/` under the build's flags, subnormals kept), an
// overflow to +-inf sanitised to +-FLT_MAX; the float lut3d path; one fp32 multiply by t.
template <int INTERP, class F>
__device__ __forceinline__ Rgb rgbaf_premul_px(const LutConsts &L, const FloatPre &Q, const F &f, float r, float g, float b, float a)
{
    const float t = pm_alpha_t(a);
    float x[3] = {pm_sanitizef(r), pm_sanitizef(g), pm_sanitizef(b)};
    if (t > 0.0f) {
#pragma unroll
        for (int c = 0; c < 3; c++) x[c] = pm_sanitizef(x[c] / t);
    }
    if (Q.tab) {
#pragma unroll
        for (int c = 0; c < 3; c++) x[c] = pm_prelut_px(Q, c, x[c]);
    }
    float s[3];
#pragma unroll
    for (int c = 0; c < 3; c++) s[c] = med3(x[c] * L.sc[c], 0.0f, L.lut_max);
    const Rgb o = interp<INTERP>(f, s[0], s[1], s[2]);
    return Rgb{o.r * t, o.g * t, o.b * t};
}

template <class F>
__device__ __forceinline__ Rgb rgbaf_premul_px_rt(int mode, const LutConsts &L, const FloatPre &Q, const F &f, float r, float g,
                                                  float b, float a)
{
    switch (mode) {
    case LUTR_INTERP_NEAREST:   return rgbaf_premul_px<LUTR_INTERP_NEAREST>(L, Q, f, r, g, b, a);
    case LUTR_INTERP_TRILINEAR: return rgbaf_premul_px<LUTR_INTERP_TRILINEAR>(L, Q, f, r, g, b, a);
    case LUTR_INTERP_PYRAMID:   return rgbaf_premul_px<LUTR_INTERP_PYRAMID>(L, Q, f, r, g, b, a);
    case LUTR_INTERP_PRISM:     return rgbaf_premul_px<LUTR_INTERP_PRISM>(L, Q, f, r, g, b, a);
    default:                    return rgbaf_premul_px<LUTR_INTERP_TETRAHEDRAL>(L, Q, f, r, g, b, a);
    }
}

// ================================================================= float vector kernel, global gather
// k_rgbf_vec's structure (lutr_rgbf.hip) with the alpha plane as a fourth source stream: a thread owns 4 pixels of a row, one
// dwordx4 load per stream, one dwordx4 store per colour plane.  The thread reads its pixels before it writes them and no other
// thread touches them: src == dst is fine.
template <int INTERP>
__global__ __launch_bounds__(256) void k_rgbaf_premul_vec(LutConsts L, FloatPre Q, PremulPlanes PP, FrameGeom G)
{
    const PlaneSet &P = PP.p;
    const GFetch f(L);
    const unsigned uw = (unsigned)G.w / 4;
    const unsigned total = uw * (unsigned)G.rows * (unsigned)G.nframes;
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u >= total) return;
    const unsigned xu = u % uw, t = u / uw;
    const long long y = G.row0 + (int)(t % (unsigned)G.rows), fr = t / (unsigned)G.rows;
    float in[4][4], out[3][4];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float4 v = *(const float4 *)(P.s[k] + fr * P.sfs[k] + y * P.ss[k] + (long long)xu * 16);
        in[k][0] = v.x; in[k][1] = v.y; in[k][2] = v.z; in[k][3] = v.w;
    }
    {
        const float4 v = *(const float4 *)(PP.a.a + fr * PP.a.afs + y * PP.a.as + (long long)xu * 16);
        in[3][0] = v.x; in[3][1] = v.y; in[3][2] = v.z; in[3][3] = v.w;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const Rgb o = rgbaf_premul_px<INTERP>(L, Q, f, in[0][i], in[1][i], in[2][i], in[3][i]);
        out[0][i] = o.r; out[1][i] = o.g; out[2][i] = o.b;
    }
#pragma unroll
    for (int k = 0; k < 3; k++)
        *(float4 *)(P.d[k] + fr * P.dfs[k] + y * P.ds[k] + (long long)xu * 16) = make_float4(out[k][0], out[k][1], out[k][2], out[k][3]);
}

// ================================================================= float generic kernel
// one thread per pixel: any 4-byte aligned layout, negative strides, all five modes
__global__ __launch_bounds__(256) void k_rgbaf_premul_generic(LutConsts L, FloatPre Q, PremulPlanes PP, FrameGeom G, int mode)
{
    const PlaneSet &P = PP.p;
    const GFetch f(L);
    const long long total = (long long)G.w * G.rows * G.nframes;
    for (long long u = blockIdx.x * 256ll + threadIdx.x; u < total; u += (long long)gridDim.x * 256ll) {
        const int x = (int)(u % G.w);
        const long long t = u / G.w;
        const long long y = G.row0 + (int)(t % G.rows), fr = t / G.rows;
        const float r = ((const float *)src_row(P, 0, fr, y))[x];
        const float g = ((const float *)src_row(P, 1, fr, y))[x];
        const float b = ((const float *)src_row(P, 2, fr, y))[x];
        const float a = ((const float *)(PP.a.a + fr * PP.a.afs + y * PP.a.as))[x];
        const Rgb o = rgbaf_premul_px_rt(mode, L, Q, f, r, g, b, a);
        ((float *)dst_row(P, 0, fr, y))[x] = o.r;
        ((float *)dst_row(P, 1, fr, y))[x] = o.g;
        ((float *)dst_row(P, 2, fr, y))[x] = o.b;
    }
}

// ================================================================= launcher, float RGB
const char *launch_rgbaf_premul(hipStream_t st, int variant, const LutConsts &L, const FloatPre &Q, const PremulPlanes &P,
                                const FrameGeom &G, int mode)
{
    const bool batch = G.nframes > 1;
    int ran = 0;
    auto vec_fits = [&](const PremulPlanes &R, const FrameGeom &H) {
        if (!vec_mode(mode) || H.w % 4) return false;
        if (!units_fit((long long)(H.w / 4) * H.rows * H.nframes)) return false;
        for (int c = 0; c < 3; c++)
            if (!planes_ok(R.p, c, 16, batch, kStrideAny, false)) return false;
        return plane_ok(R.a.a, R.a.as, R.a.afs, 16, batch, kStrideAny, false);
    };
    auto vec = [&](const PremulPlanes &R, const FrameGeom &H) -> const char * {
        ran |= 1;
        const dim3 grid(grid_for((long long)(H.w / 4) * H.rows * H.nframes)), block(256);
        switch (mode) {
        case LUTR_INTERP_NEAREST:   hipLaunchKernelGGL(k_rgbaf_premul_vec<LUTR_INTERP_NEAREST>, grid, block, 0, st, L, Q, R, H); return "k_rgbaf_premul_vec<0>";
        case LUTR_INTERP_TRILINEAR: hipLaunchKernelGGL(k_rgbaf_premul_vec<LUTR_INTERP_TRILINEAR>, grid, block, 0, st, L, Q, R, H); return "k_rgbaf_premul_vec<1>";
        default:                    hipLaunchKernelGGL(k_rgbaf_premul_vec<LUTR_INTERP_TETRAHEDRAL>, grid, block, 0, st, L, Q, R, H); return "k_rgbaf_premul_vec<2>";
        }
    };
    auto generic = [&](const PremulPlanes &R, const FrameGeom &H) {
        ran |= 2;
        hipLaunchKernelGGL(k_rgbaf_premul_generic, dim3(stride_grid("k_rgbaf_premul_generic", (long long)H.w * H.rows * H.nframes, kGridStrideCap)),
                           dim3(256), 0, st,
                           L, Q, R, H, mode);
        return "k_rgbaf_premul_generic";
    };
    // (no LDS kernel for this path; the unit is 4 pixels wide)
    const char *name = launch_vec_or_generic(variant, P, G, 4, vec_fits, vec, generic, [&](int wv) {
        PremulPlanes R = P;
        R.p = advance_planes(P.p, (long long)wv * 4, (long long)wv * 4, (long long)wv * 4, (long long)wv * 4);
        R.a.a += (long long)wv * 4;
        return R;
    });
    if (!name || ran != 3) return name;
    static thread_local std::string both;
    both = std::string(name) + "+k_rgbaf_premul_generic";
    return both.c_str();
}
#endif  // LUTR_PM_WI

}  // namespace lutr
