// lutr_device.h -- device-side pieces shared by the gfx950 gather kernels (lutr_kernels.hip, lutr_packed.hip, lutr_sited.hip,
// lutr_dither.hip, lutr_xsub.hip, lutr_bnd.hip, lutr_rgb2yuv.hip, lutr_rgbf.hip, lutr_semi.hip): the lut3d per-pixel restatement (SURVEY.md
// Appendix A.3-A.5), the YUV contract (DESIGN.md "YUV contract"), little sample/word accessors, the block walk, block
// body and output sinks of the by-block generic kernels, the vector kernels' unit size, and the unit, vector body and
// generic walk of the paths that work by union blocks (UnionUnit, union_vec_unit, xsub_union_block).
//
// Everything here rounds exactly like FFmpeg's scalar C (-ffp-contract=off; fused
// multiply-adds only where written as __builtin_fmaf).
#pragma once

#include "lutr_internal.h"

namespace lutr {

// ---------------------------------------------------------------- small math
constexpr int cmax(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ float med3(float a, float lo, float hi) { return __builtin_amdgcn_fmed3f(a, lo, hi); }
__device__ __forceinline__ float max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }
__device__ __forceinline__ float min3(float a, float b, float c) { return fminf(fminf(a, b), c); }
__device__ __forceinline__ float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// ---------------------------------------------------------------- lattice access
// Global-memory gather (served by L1 / the XCD's L2: a 33^3 padded lattice is 629 KB).
struct GFetch {
    const float4 *__restrict__ lat;
    float fr, fg;   // node strides as floats: n1*n1, n1 (blue stride is 1)
    int   sr, sg;   // the same as ints
    __device__ __forceinline__ explicit GFetch(const LutConsts &L)
        : lat(L.lat), fr((float)(L.n1 * L.n1)), fg((float)L.n1), sr(L.n1 * L.n1), sg(L.n1) {}
    // integer math: n1^3 reaches 2^24 at N = 256, one step past what fp32 holds exactly
    __device__ __forceinline__ int index(float pr, float pg, float pb) const
    {
        return ((int)pr * sg + (int)pg) * sg + (int)pb;
    }
    __device__ __forceinline__ float4 ld(int i) const { return lat[i]; }
};

// ---------------------------------------------------------------- lut3d core
struct Rgb { float r, g, b; };

__device__ __forceinline__ float lerpf(float v0, float v1, float f) { return v0 + (v1 - v0) * f; }

// FFmpeg's NEAR(x) = (int)(x + .5) adds a DOUBLE .5 to the float coordinate, so the sum is exact and the result is
// floor(x) + (frac(x) >= 1/2).  frac(x) = x - floor(x) is exact in fp32, which makes this form bit-identical without
// double arithmetic (floorf(x + .5f) is not: for x = k + 0.49999997 the float sum rounds up to k + 1).
__device__ __forceinline__ float near_f(float s)
{
    const float p = floorf(s);
    return (s - p >= .5f) ? p + 1.0f : p;
}

template <class F>
__device__ __forceinline__ Rgb interp_nearest(const F &f, float sr, float sg, float sb)
{
    const float4 c = f.ld(f.index(near_f(sr), near_f(sg), near_f(sb)));
    return Rgb{c.x, c.y, c.z};
}

template <class F>
__device__ __forceinline__ Rgb interp_trilinear(const F &f, float sr, float sg, float sb)
{
    const float pr = floorf(sr), pg = floorf(sg), pb = floorf(sb);
    const float dr = sr - pr, dg = sg - pg, db = sb - pb;
    const int i = f.index(pr, pg, pb);
    const float4 c000 = f.ld(i), c001 = f.ld(i + 1);
    const float4 c010 = f.ld(i + f.sg), c011 = f.ld(i + f.sg + 1);
    const float4 c100 = f.ld(i + f.sr), c101 = f.ld(i + f.sr + 1);
    const float4 c110 = f.ld(i + f.sr + f.sg), c111 = f.ld(i + f.sr + f.sg + 1);
    Rgb o;
#define TRI(ch) \
    { \
        const float c00 = lerpf(c000.ch, c100.ch, dr), c10 = lerpf(c010.ch, c110.ch, dr); \
        const float c01 = lerpf(c001.ch, c101.ch, dr), c11 = lerpf(c011.ch, c111.ch, dr); \
        const float c0 = lerpf(c00, c10, dg), c1 = lerpf(c01, c11, dg); \
        o_ = lerpf(c0, c1, db); \
    }
    float o_;
    TRI(x) o.r = o_;
    TRI(y) o.g = o_;
    TRI(z) o.b = o_;
#undef TRI
    return o;
}

// FFmpeg's six branches all evaluate (1-x)*c000 + (x-y)*cA + (y-z)*cB + z*c111 with
// (x,y,z) = (d.r,d.g,d.b) sorted descending, cA one step along x's axis and cB one more
// along y's.  Ties only change a tap whose weight is exactly 0, so for a finite lattice
// the max3/med3/min3 form below is bit-identical to the branchy original.
template <class F>
__device__ __forceinline__ Rgb interp_tetrahedral(const F &f, float sr, float sg, float sb)
{
    const float pr = floorf(sr), pg = floorf(sg), pb = floorf(sb);
    const float dr = sr - pr, dg = sg - pg, db = sb - pb;
    const int i = f.index(pr, pg, pb);
    const float x = max3(dr, dg, db), y = med3(dr, dg, db), z = min3(dr, dg, db);
    const int oa = (dr == x) ? f.sr : ((dg == x) ? f.sg : 1);
    const int oz = (db == z) ? 1 : ((dg == z) ? f.sg : f.sr);
    const int o111 = f.sr + f.sg + 1;
    const float4 c0 = f.ld(i), c1 = f.ld(i + oa), c2 = f.ld(i + o111 - oz), c3 = f.ld(i + o111);
    const float w0 = 1.0f - x, w1 = x - y, w2 = y - z, w3 = z;
    Rgb o;
    o.r = w0 * c0.x + w1 * c1.x + w2 * c2.x + w3 * c3.x;
    o.g = w0 * c0.y + w1 * c1.y + w2 * c2.y + w3 * c3.y;
    o.b = w0 * c0.z + w1 * c1.z + w2 * c2.z + w3 * c3.z;
    return o;
}

// pyramid / prism (generic kernel only)
template <class F>
__device__ Rgb interp_pyramid(const F &f, float sr, float sg, float sb)
{
    const float pr = floorf(sr), pg = floorf(sg), pb = floorf(sb);
    const float dr = sr - pr, dg = sg - pg, db = sb - pb;
    const int i = f.index(pr, pg, pb);
    const float4 c000 = f.ld(i), c001 = f.ld(i + 1);
    const float4 c010 = f.ld(i + f.sg), c011 = f.ld(i + f.sg + 1);
    const float4 c100 = f.ld(i + f.sr), c101 = f.ld(i + f.sr + 1);
    const float4 c110 = f.ld(i + f.sr + f.sg), c111 = f.ld(i + f.sr + f.sg + 1);
    Rgb o;
#define PYR(ch, out) \
    if (dg > dr && db > dr) { \
        out = c000.ch + (c111.ch - c011.ch) * dr + (c010.ch - c000.ch) * dg + (c001.ch - c000.ch) * db + \
              (c011.ch - c001.ch - c010.ch + c000.ch) * dg * db; \
    } else if (dr > dg && db > dg) { \
        out = c000.ch + (c100.ch - c000.ch) * dr + (c111.ch - c101.ch) * dg + (c001.ch - c000.ch) * db + \
              (c101.ch - c001.ch - c100.ch + c000.ch) * dr * db; \
    } else { \
        out = c000.ch + (c100.ch - c000.ch) * dr + (c010.ch - c000.ch) * dg + (c111.ch - c110.ch) * db + \
              (c110.ch - c100.ch - c010.ch + c000.ch) * dr * dg; \
    }
    PYR(x, o.r) PYR(y, o.g) PYR(z, o.b)
#undef PYR
    return o;
}

template <class F>
__device__ Rgb interp_prism(const F &f, float sr, float sg, float sb)
{
    const float pr = floorf(sr), pg = floorf(sg), pb = floorf(sb);
    const float dr = sr - pr, dg = sg - pg, db = sb - pb;
    const int i = f.index(pr, pg, pb);
    const float4 c000 = f.ld(i), c001 = f.ld(i + 1);
    const float4 c010 = f.ld(i + f.sg), c011 = f.ld(i + f.sg + 1);
    const float4 c100 = f.ld(i + f.sr), c101 = f.ld(i + f.sr + 1);
    const float4 c110 = f.ld(i + f.sr + f.sg), c111 = f.ld(i + f.sr + f.sg + 1);
    Rgb o;
#define PRI(ch, out) \
    if (db > dr) { \
        out = c000.ch + (c001.ch - c000.ch) * db + (c101.ch - c001.ch) * dr + (c010.ch - c000.ch) * dg + \
              (c000.ch - c010.ch - c001.ch + c011.ch) * db * dg + \
              (c001.ch - c011.ch - c101.ch + c111.ch) * dr * dg; \
    } else { \
        out = c000.ch + (c101.ch - c100.ch) * db + (c100.ch - c000.ch) * dr + (c010.ch - c000.ch) * dg + \
              (c100.ch - c110.ch - c101.ch + c111.ch) * db * dg + \
              (c000.ch - c010.ch - c100.ch + c110.ch) * dr * dg; \
    }
    PRI(x, o.r) PRI(y, o.g) PRI(z, o.b)
#undef PRI
    return o;
}

template <int INTERP, class F>
__device__ __forceinline__ Rgb interp(const F &f, float sr, float sg, float sb)
{
    if constexpr (INTERP == LUTR_INTERP_NEAREST) return interp_nearest(f, sr, sg, sb);
    else if constexpr (INTERP == LUTR_INTERP_TRILINEAR) return interp_trilinear(f, sr, sg, sb);
    else if constexpr (INTERP == LUTR_INTERP_PYRAMID) return interp_pyramid(f, sr, sg, sb);
    else if constexpr (INTERP == LUTR_INTERP_PRISM) return interp_prism(f, sr, sg, sb);
    else return interp_tetrahedral(f, sr, sg, sb);
}

// One pixel of A.3.  In: integer codes held as floats.  Out: integer codes held as
// floats (truncation toward zero, then clip to [0, M], exactly av_clip_uintp2((int)(v*M))).
template <int INTERP, class F>
__device__ __forceinline__ Rgb lut3d_px(const LutConsts &L, const F &f, float rc, float gc, float bc)
{
    float sr, sg, sb;
    if (L.pre) {         // a prelut (cineSpace shaper): the host folded shaper, scale and clip into one coordinate per integer code
        sr = L.pre[(int)rc]; sg = L.pre[L.pre_stride + (int)gc]; sb = L.pre[2 * L.pre_stride + (int)bc];
    } else {
        const float xr = rc * L.scale_f, xg = gc * L.scale_f, xb = bc * L.scale_f;
        sr = med3(xr * L.sc[0], 0.0f, L.lut_max);
        sg = med3(xg * L.sc[1], 0.0f, L.lut_max);
        sb = med3(xb * L.sc[2], 0.0f, L.lut_max);
    }
    const Rgb v = interp<INTERP>(f, sr, sg, sb);
    Rgb o;
    o.r = med3(truncf(v.r * L.maxf), 0.0f, L.maxf);
    o.g = med3(truncf(v.g * L.maxf), 0.0f, L.maxf);
    o.b = med3(truncf(v.b * L.maxf), 0.0f, L.maxf);
    return o;
}

template <class F>
__device__ __forceinline__ Rgb lut3d_px_rt(int mode, const LutConsts &L, const F &f, float r, float g, float b)
{
    switch (mode) {
    case LUTR_INTERP_NEAREST:   return lut3d_px<LUTR_INTERP_NEAREST>(L, f, r, g, b);
    case LUTR_INTERP_TRILINEAR: return lut3d_px<LUTR_INTERP_TRILINEAR>(L, f, r, g, b);
    case LUTR_INTERP_PYRAMID:   return lut3d_px<LUTR_INTERP_PYRAMID>(L, f, r, g, b);
    case LUTR_INTERP_PRISM:     return lut3d_px<LUTR_INTERP_PRISM>(L, f, r, g, b);
    default:                    return lut3d_px<LUTR_INTERP_TETRAHEDRAL>(L, f, r, g, b);
    }
}

// lut3d_px from its scale step on, for a pixel that arrives as unit floats instead of integer codes (the ASC CDL's output,
// DESIGN.md 3.19): clip of the coordinates, blend, truncation toward zero and clip to [0, M] as above.  No prelut: a per-code
// table has nothing to index with.
template <int INTERP, class F>
__device__ __forceinline__ Rgb lut3d_unit(const LutConsts &L, const F &f, const Rgb &x)
{
    const float sr = med3(x.r * L.sc[0], 0.0f, L.lut_max);
    const float sg = med3(x.g * L.sc[1], 0.0f, L.lut_max);
    const float sb = med3(x.b * L.sc[2], 0.0f, L.lut_max);
    const Rgb v = interp<INTERP>(f, sr, sg, sb);
    Rgb o;
    o.r = med3(truncf(v.r * L.maxf), 0.0f, L.maxf);
    o.g = med3(truncf(v.g * L.maxf), 0.0f, L.maxf);
    o.b = med3(truncf(v.b * L.maxf), 0.0f, L.maxf);
    return o;
}

template <class F>
__device__ __forceinline__ Rgb lut3d_unit_rt(int mode, const LutConsts &L, const F &f, const Rgb &x)
{
    switch (mode) {
    case LUTR_INTERP_NEAREST:   return lut3d_unit<LUTR_INTERP_NEAREST>(L, f, x);
    case LUTR_INTERP_TRILINEAR: return lut3d_unit<LUTR_INTERP_TRILINEAR>(L, f, x);
    case LUTR_INTERP_PYRAMID:   return lut3d_unit<LUTR_INTERP_PYRAMID>(L, f, x);
    case LUTR_INTERP_PRISM:     return lut3d_unit<LUTR_INTERP_PRISM>(L, f, x);
    default:                    return lut3d_unit<LUTR_INTERP_TETRAHEDRAL>(L, f, x);
    }
}

// Stages A and B of the ASC CDL on one pixel of integer codes held as floats: the host's per-code table of
// clamp(x * slope + offset)^power per channel, then the saturation mix around Rec.709 luma -- every product and sum rounded on
// its own (this code is compiled without contraction).  mix = (C.sat != 1), decided once per kernel.
__device__ __forceinline__ Rgb cdl_px(const CdlConsts &C, bool mix, const Rgb &q)
{
    Rgb t;
    t.r = C.tab[(int)q.r];
    t.g = C.tab[C.stride + (int)q.g];
    t.b = C.tab[2 * C.stride + (int)q.b];
    if (mix) {
        const float l = (0.2126f * t.r + 0.7152f * t.g) + 0.0722f * t.b;
        t.r = med3(l + C.sat * (t.r - l), 0.0f, 1.0f);
        t.g = med3(l + C.sat * (t.g - l), 0.0f, 1.0f);
        t.b = med3(l + C.sat * (t.b - l), 0.0f, 1.0f);
    }
    return t;
}

// ---------------------------------------------------------------- YUV contract pieces
struct Chroma { float rv, gv, bu; };

__device__ __forceinline__ float clip_floor(float v, float hi) { return med3(floorf(v), 0.0f, hi); }

__device__ __forceinline__ Chroma chroma_terms(const YuvConsts &K, float cbv, float crv)
{
    if (K.pre != 0.0f) {
        cbv = clip_floor(fma_(K.pc, cbv, K.pcb), K.pre_max);
        crv = clip_floor(fma_(K.pc, crv, K.pcb), K.pre_max);
    }
    const float cb = cbv - K.coff, cr = crv - K.coff;
    Chroma c;
    c.rv = K.krv * cr;
    c.gv = fma_(K.kgu, cb, K.kgv * cr);
    c.bu = K.kbu * cb;
    return c;
}

__device__ __forceinline__ Rgb yuv_to_rgb(const YuvConsts &K, float yv, const Chroma &c)
{
    if (K.pre != 0.0f)
        yv = clip_floor(fma_(K.py, yv, K.pyb), K.pre_max);
    const float yy = fma_(K.ky, yv, K.yb);
    Rgb o;
    o.r = clip_floor(yy + c.rv, K.max_l);
    o.g = clip_floor(yy + c.gv, K.max_l);
    o.b = clip_floor(yy + c.bu, K.max_l);
    return o;
}

__device__ __forceinline__ float rgb_to_y(const YuvConsts &K, const Rgb &q)
{
    return clip_floor(fma_(K.cyr, q.r, fma_(K.cyg, q.g, fma_(K.cyb, q.b, K.yob))), K.max_o);
}

__device__ __forceinline__ float rgb_to_cb(const YuvConsts &K, float rs, float gs, float bs)
{
    return clip_floor(fma_(K.cbr, rs, fma_(K.cbg, gs, fma_(K.cbb, bs, K.cob))), K.max_o);
}

__device__ __forceinline__ float rgb_to_cr(const YuvConsts &K, float rs, float gs, float bs)
{
    return clip_floor(fma_(K.crr, rs, fma_(K.crg, gs, fma_(K.crb, bs, K.cob))), K.max_o);
}

// ---------------------------------------------------------------- sample access
__device__ __forceinline__ float ld_sample(const uint8_t *row, int x, int wide)
{
    return wide ? (float)((const uint16_t *)row)[x] : (float)row[x];
}

__device__ __forceinline__ void st_sample(uint8_t *row, int x, int wide, float v)
{
    const unsigned u = (unsigned)v;
    if (wide) ((uint16_t *)row)[x] = (uint16_t)u;
    else row[x] = (uint8_t)u;
}

// sample i of a little-endian word vector (i is a compile-time constant after unrolling)
template <int WIDE>
__device__ __forceinline__ float word_sample(const uint32_t *w, int i)
{
    if constexpr (WIDE) return (float)((w[i >> 1] >> ((i & 1) * 16)) & 0xffffu);
    else return (float)((w[i >> 2] >> ((i & 3) * 8)) & 0xffu);
}

template <int WIDE>
__device__ __forceinline__ void word_put(uint32_t *w, int i, float v)
{
    const uint32_t u = (uint32_t)v;
    if constexpr (WIDE) w[i >> 1] |= u << ((i & 1) * 16);
    else w[i >> 2] |= u << ((i & 3) * 8);
}

// sample i of a word vector whose 16-bit codes sit `shift` bits up in their container (p010le: 6): the shift rides in the
// bit-field extract that unpacks the sample anyway (the vector kernels of lutr_semi.hip and the semi form of lutr_stack.hip)
template <int WIDE>
__device__ __forceinline__ float word_code(const uint32_t *w, int i, unsigned shift)
{
    if constexpr (WIDE) return (float)__builtin_amdgcn_ubfe(w[i >> 1], (unsigned)(i & 1) * 16u + shift, 16u - shift);
    else return word_sample<0>(w, i);
}

template <int NW>
__device__ __forceinline__ void ld_words(uint32_t *w, const uint8_t *p)
{
    if constexpr (NW == 4) {
        const uint4 v = *(const uint4 *)p;
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else if constexpr (NW == 2) {
        const uint2 v = *(const uint2 *)p;
        w[0] = v.x; w[1] = v.y;
    } else {
        w[0] = *(const uint32_t *)p;
    }
}

// NT: non-temporal store.  Pays where the stores would otherwise push the lattice out of the caches: k_rgb_vec on small gbrp10le
// launches 253 -> 360 Gpx/s; the YUV and packed vector kernels do not gain (+-1 %) and keep plain stores.
template <int NW, bool NT = false>
__device__ __forceinline__ void st_words(uint8_t *p, const uint32_t *w)
{
    if constexpr (NT) {
        typedef unsigned nt4 __attribute__((ext_vector_type(4)));
        typedef unsigned nt2 __attribute__((ext_vector_type(2)));
        if constexpr (NW == 4) __builtin_nontemporal_store(nt4{w[0], w[1], w[2], w[3]}, (nt4 *)p);
        else if constexpr (NW == 2) __builtin_nontemporal_store(nt2{w[0], w[1]}, (nt2 *)p);
        else __builtin_nontemporal_store(w[0], (uint32_t *)p);
    } else {
        if constexpr (NW == 4) *(uint4 *)p = make_uint4(w[0], w[1], w[2], w[3]);
        else if constexpr (NW == 2) *(uint2 *)p = make_uint2(w[0], w[1]);
        else *(uint32_t *)p = w[0];
    }
}

// ---------------------------------------------------------------- RGB sources of the vector kernels (lutr_rgb2yuv.hip, lutr_rgbstack.hip)
// `in` holds the 8 pixels of a thread and row: planar (NC = 1) the 8 samples of R, of G and of B one after the other; packed
// (NC = 3 | 4) the 8 pixels as they lie in memory.

// component `off` (runtime, wave-uniform) of pixel i of a 4-component run
template <int WIDE>
__device__ __forceinline__ float r2y_comp4(const uint32_t *w, int i, int off)
{
    if constexpr (WIDE) {
        const unsigned long long pv = ((unsigned long long)w[2 * i + 1] << 32) | w[2 * i];
        return (float)(unsigned)((pv >> (off * 16)) & 0xffffull);
    } else {
        return (float)((w[i] >> (off * 8)) & 0xffu);
    }
}

template <int WIN, int NC>
__device__ __forceinline__ Rgb r2y_pixel(const uint32_t *in, int i, const RgbLayout &Y)
{
    constexpr int SW = 8 * (WIN ? 2 : 1) / 4;             // dwords of 8 samples of one plane
    if constexpr (NC == 1) {
        return Rgb{word_sample<WIN>(in, i), word_sample<WIN>(in + SW, i), word_sample<WIN>(in + 2 * SW, i)};
    } else if constexpr (NC == 3) {
        const float c0 = word_sample<WIN>(in, i * 3), c1 = word_sample<WIN>(in, i * 3 + 1), c2 = word_sample<WIN>(in, i * 3 + 2);
        const bool swap = Y.ro != 0;                      // bgr order
        return Rgb{swap ? c2 : c0, c1, swap ? c0 : c2};
    } else {
        return Rgb{r2y_comp4<WIN>(in, i, Y.ro), r2y_comp4<WIN>(in, i, Y.go), r2y_comp4<WIN>(in, i, Y.bo)};
    }
}

// ---------------------------------------------------------------- RGB destinations of the vector kernels (lutr_yuv2rgb.hip, lutr_y2rstack.hip)
// `out` holds the 8 pixels of a thread and row as `in` above does: planar the 8 samples of R, of G and of B; packed as in memory.

// pixel i of the thread's 8 into the output words of one row
template <int WOUT, int NC>
__device__ __forceinline__ void y2r_put(uint32_t *out, int i, const Rgb &o, const RgbLayout &Y, uint32_t amax)
{
    constexpr int SW = 8 * (WOUT ? 2 : 1) / 4;            // dwords of 8 samples of one plane
    if constexpr (NC == 1) {
        word_put<WOUT>(out, i, o.r);
        word_put<WOUT>(out + SW, i, o.g);
        word_put<WOUT>(out + 2 * SW, i, o.b);
    } else if constexpr (NC == 3) {
        const bool swap = Y.ro != 0;                      // bgr order
        word_put<WOUT>(out, i * 3 + 0, swap ? o.b : o.r);
        word_put<WOUT>(out, i * 3 + 1, o.g);
        word_put<WOUT>(out, i * 3 + 2, swap ? o.r : o.b);
    } else {
        const int ao = 6 - Y.ro - Y.go - Y.bo;
        if constexpr (WOUT) {
            const unsigned long long q = ((unsigned long long)amax << (ao * 16)) |
                                         ((unsigned long long)(unsigned)o.r << (Y.ro * 16)) |
                                         ((unsigned long long)(unsigned)o.g << (Y.go * 16)) |
                                         ((unsigned long long)(unsigned)o.b << (Y.bo * 16));
            out[2 * i] = (uint32_t)q;
            out[2 * i + 1] = (uint32_t)(q >> 32);
        } else {
            out[i] = (amax << (ao * 8)) | ((unsigned)o.r << (Y.ro * 8)) | ((unsigned)o.g << (Y.go * 8)) |
                     ((unsigned)o.b << (Y.bo * 8));
        }
    }
}

// ---------------------------------------------------------------- plane rows
template <class Y>
__device__ __forceinline__ const uint8_t *src_row(const PlaneSet &P, int c, long long fr, Y y)
{
    return P.s[c] + fr * P.sfs[c] + y * P.ss[c];
}

template <class Y>
__device__ __forceinline__ uint8_t *dst_row(const PlaneSet &P, int c, long long fr, Y y)
{
    return P.d[c] + fr * P.dfs[c] + y * P.ds[c];
}

// the RGB destination of the by-block generic kernels (lutr_yuv2rgb.hip, lutr_y2rstack.hip): a sink that stores the pixel
struct RgbSink {
    const PlaneSet &P;
    const RgbLayout &Y;
    float amax;
    __device__ __forceinline__ void luma(long long fr, int x, int y, const Rgb &o)
    {
        const int e = x * Y.step;
        st_sample(dst_row(P, 0, fr, y), e + Y.ro, Y.wide, o.r);
        st_sample(dst_row(P, 1, fr, y), e + Y.go, Y.wide, o.g);
        st_sample(dst_row(P, 2, fr, y), e + Y.bo, Y.wide, o.b);
        if (Y.step == 4) st_sample(dst_row(P, 0, fr, y), e + 6 - Y.ro - Y.go - Y.bo, Y.wide, amax);
    }
    __device__ __forceinline__ void chroma(long long, int, int, float, float, float) {}
};

// ---------------------------------------------------------------- by-block generic kernels: the walk and the output sinks
// Grid-stride walk of blocks of 2^csx x 2^csy luma samples, one thread per block: body(fr, cx, cy) for every block that touches
// rows row0 .. row0 + rows of the frame (whole_frames: all of it, the dither path's pass 1)
template <class Body>
__device__ __forceinline__ void for_each_block(const FrameGeom &G, int csx, int csy, bool whole_frames, Body body)
{
    const int cw = (G.w + (1 << csx) - 1) >> csx;
    const int cr0 = whole_frames ? 0 : G.row0 >> csy;
    const int crows = (((whole_frames ? G.h : G.row0 + G.rows) + (1 << csy) - 1) >> csy) - cr0;
    const long long total = (long long)cw * crows * G.nframes;
    for (long long u = blockIdx.x * 256ll + threadIdx.x; u < total; u += (long long)gridDim.x * 256ll) {
        const long long t = u / cw;
        body(t / crows, (int)(u % cw), cr0 + (int)(t % crows));
    }
}

// Where a generic kernel puts one output chroma block: luma() per pixel inside the frame, chroma() once with the block's R, G, B
// sums.  PlaneSink: the quantised planes.
struct PlaneSink {
    const YuvConsts &K;
    const PlaneSet &P;
    int wout;
    __device__ __forceinline__ void luma(long long fr, int x, int y, const Rgb &o)
    {
        st_sample(dst_row(P, 0, fr, y), x, wout, rgb_to_y(K, o));
    }
    __device__ __forceinline__ void chroma(long long fr, int cx, int cy, float rs, float gs, float bs)
    {
        st_sample(dst_row(P, 1, fr, cy), cx, wout, rgb_to_cb(K, rs, gs, bs));
        st_sample(dst_row(P, 2, fr, cy), cx, wout, rgb_to_cr(K, rs, gs, bs));
    }
};

// FloatSink: the dither path's pass 1 -- unquantised planes, densely packed per frame, chroma in the layout csx, csy
struct FloatSink {
    const YuvConsts &K;
    const FloatPlanes &F;
    const FrameGeom &G;
    int cw, ch;
    __device__ __forceinline__ FloatSink(const YuvConsts &K, const FloatPlanes &F, const FrameGeom &G, int csx, int csy)
        : K(K), F(F), G(G), cw((G.w + (1 << csx) - 1) >> csx), ch((G.h + (1 << csy) - 1) >> csy) {}
    __device__ __forceinline__ void luma(long long fr, int x, int y, const Rgb &o)
    {
        F.y[(fr * G.h + y) * G.w + x] = fma_(K.cyr, o.r, fma_(K.cyg, o.g, fma_(K.cyb, o.b, K.yob))) - 0.5f;
    }
    __device__ __forceinline__ void chroma(long long fr, int cx, int cy, float rs, float gs, float bs)
    {
        F.cb[(fr * ch + cy) * cw + cx] = fma_(K.cbr, rs, fma_(K.cbg, gs, fma_(K.cbb, bs, K.cob))) - 0.5f;
        F.cr[(fr * ch + cy) * cw + cx] = fma_(K.crr, rs, fma_(K.crg, gs, fma_(K.crb, bs, K.cob))) - 0.5f;
    }
};

// ---------------------------------------------------------------- blue-noise dither
// bn: the 64 x 64 table of offsets d = (2 rank - 4095) / 8192, row-major.  Sample (x, y) of output plane `plane` (0 = Y, 1 = Cb,
// 2 = Cr; the plane's own coordinates, counted from the top-left of the full frame) takes bn[(y + OY) & 63][(x + OX) & 63].  The x
// shifts are multiples of 8: an aligned run of up to 8 samples is contiguous in the table and never wraps.
__device__ __forceinline__ int bn_ox(int plane) { return plane == 0 ? 0 : (plane == 1 ? 24 : 40); }
__device__ __forceinline__ int bn_oy(int plane) { return plane == 0 ? 0 : (plane == 1 ? 37 : 11); }

__device__ __forceinline__ float bn_offset(const float *__restrict__ bn, int plane, int x, int y)
{
    return bn[(((y + bn_oy(plane)) & 63) << 6) | ((x + bn_ox(plane)) & 63)];
}

// the output stage with the offset in front of clip_floor: one fp32 add, rounded once (d = 0 gives rgb_to_y / _cb / _cr above)
__device__ __forceinline__ float rgb_to_y(const YuvConsts &K, const Rgb &q, float d)
{
    return clip_floor(fma_(K.cyr, q.r, fma_(K.cyg, q.g, fma_(K.cyb, q.b, K.yob))) + d, K.max_o);
}

__device__ __forceinline__ float rgb_to_cb(const YuvConsts &K, float rs, float gs, float bs, float d)
{
    return clip_floor(fma_(K.cbr, rs, fma_(K.cbg, gs, fma_(K.cbb, bs, K.cob))) + d, K.max_o);
}

__device__ __forceinline__ float rgb_to_cr(const YuvConsts &K, float rs, float gs, float bs, float d)
{
    return clip_floor(fma_(K.crr, rs, fma_(K.crg, gs, fma_(K.crb, bs, K.cob))) + d, K.max_o);
}

// DitherSink: PlaneSink with the table.  x0 / cx0: where column 0 of the planes lies in the frame (luma / output chroma samples;
// the generic tail of a column split starts to the right of the vector kernel's part); rows already count from the frame's top.
struct DitherSink {
    const YuvConsts &K;
    const PlaneSet &P;
    int wout;
    const float *__restrict__ bn;
    int x0, cx0;
    __device__ __forceinline__ void luma(long long fr, int x, int y, const Rgb &o)
    {
        st_sample(dst_row(P, 0, fr, y), x, wout, rgb_to_y(K, o, bn_offset(bn, 0, x0 + x, y)));
    }
    __device__ __forceinline__ void chroma(long long fr, int cx, int cy, float rs, float gs, float bs)
    {
        st_sample(dst_row(P, 1, fr, cy), cx, wout, rgb_to_cb(K, rs, gs, bs, bn_offset(bn, 1, cx0 + cx, cy)));
        st_sample(dst_row(P, 2, fr, cy), cx, wout, rgb_to_cr(K, rs, gs, bs, bn_offset(bn, 2, cx0 + cx, cy)));
    }
};

// One chroma block of the fused YUV pass (k_yuv_generic, k_yuv_float).  A pixel outside the frame is the edge pixel again (odd
// sizes: the edge column / row is summed twice); only pixels inside the frame are written.
template <class Sink>
__device__ __forceinline__ void yuv_block(const LutConsts &L, const GFetch &f, const YuvConsts &K, const PlaneSet &P,
                                          const FrameGeom &G, long long fr, int cx, int cy, int win, int csx, int csy, int mode,
                                          Sink &sink)
{
    const int bw = 1 << csx, bh = 1 << csy;
    const Chroma c = chroma_terms(K, ld_sample(src_row(P, 1, fr, cy), cx, win), ld_sample(src_row(P, 2, fr, cy), cx, win));
    float rs = 0.f, gs = 0.f, bs = 0.f;
    for (int dy = 0; dy < bh; dy++) {
        const int yy = cy * bh + dy;
        const int y = yy < G.h ? yy : G.h - 1;
        for (int dx = 0; dx < bw; dx++) {
            const int xx = cx * bw + dx;
            const int x = xx < G.w ? xx : G.w - 1;
            const Rgb q = yuv_to_rgb(K, ld_sample(src_row(P, 0, fr, y), x, win), c);
            const Rgb o = lut3d_px_rt(mode, L, f, q.r, q.g, q.b);
            rs += o.r; gs += o.g; bs += o.b;
            if (yy < G.h && xx < G.w) sink.luma(fr, x, y, o);
        }
    }
    sink.chroma(fr, cx, cy, rs, gs, bs);
}

// One union block of a pass that works by union blocks (the generic kernels of lutr_xsub.hip, lutr_bnd.hip,
// lutr_chain.hip, lutr_cdl.hip, lutr_l1d.hip and lutr_stack.hip).  The block is walked one OUTPUT
// chroma block at a time (its sum is then one set of three accumulators); every pixel reads the input chroma sample of its
// own input block and goes through px(fr, x, y, q) -> o, the family's stages on the codes q behind the YUV -> RGB stage.  A
// pixel outside the frame is the edge pixel again (its luma, its chroma and the (x, y) px sees), so a partial output block
// sums the edge column / row twice, like np.pad(mode="edge"); only pixels and chroma samples inside the planes are written.
template <class Sink, class Px>
__device__ __forceinline__ void xsub_union_block(const YuvConsts &K, const PlaneSet &P, const FrameGeom &G, long long fr, int ux,
                                                 int uy, int win, int icsx, int icsy, int ocsx, int ocsy, Sink &sink, Px px)
{
    const int bw = 1 << cmax(icsx, ocsx), bh = 1 << cmax(icsy, ocsy), obw = 1 << ocsx, obh = 1 << ocsy;
    const int cwo = (G.w + obw - 1) >> ocsx, cho = (G.h + obh - 1) >> ocsy;
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
                    const Rgb o = px(fr, x, y, yuv_to_rgb(K, yv, chroma_terms(K, cbv, crv)));
                    rs += o.r; gs += o.g; bs += o.b;
                    if (yy < G.h && xx < G.w) sink.luma(fr, x, y, o);
                }
            }
            const int ocx = (ux * bw + ox) >> ocsx, ocy = (uy * bh + oy) >> ocsy;
            if (ocx < cwo && ocy < cho) sink.chroma(fr, ocx, ocy, rs, gs, bs);
        }
    }
}

// A code inside a container at run-time width: sample x of `row`, `shift` bits up inside a 16-bit word (p010le, y210le: 6); the
// generic kernels of the semi-planar and packed 4:2:2 paths (lutr_semi.hip, lutr_pkyuv.hip).
__device__ __forceinline__ float ld_code(const uint8_t *row, long long x, int wide, int shift)
{
    return wide ? (float)(((const uint16_t *)row)[x] >> shift) : (float)row[x];
}

__device__ __forceinline__ void st_code(uint8_t *row, long long x, int wide, int shift, float v)
{
    const unsigned u = (unsigned)v;
    if (wide) ((uint16_t *)row)[x] = (uint16_t)(u << shift);
    else row[x] = (uint8_t)u;
}

// ---------------------------------------------------------------- vector kernels, global gather
// kVecBytes bytes per plane row and thread: with 16-byte accesses these kernels needed 256 VGPRs (one wave per SIMD); at 8 bytes
// they keep several waves per SIMD, which is what a gather wants.
constexpr int kVecBytes = 8;
// WIN / WOUT: 16-bit containers in / out.  A 10-bit source written as 8 bit (the reference's libx264 default,
// ffmpeg.py:287-302) takes 16 bytes of luma per thread and row so that its 8-bit chroma output is still a whole word.
template <int WIN, int WOUT> constexpr int vec_bytes() { return (WIN && !WOUT) ? 16 : kVecBytes; }


// ---------------------------------------------------------------- the vector body of every pass that works by union blocks (3.8)
// N offsets of one table row for the samples x .. x + N - 1 of a plane (x a multiple of min(N, 4); ox a multiple of 8): aligned
// 16-byte (8-byte for N = 2) loads, each inside one row of the table.
template <int N>
__device__ __forceinline__ void ld_bn(float *d, const float *__restrict__ row, int x, int ox)
{
    if constexpr (N >= 4) {
#pragma unroll
        for (int k = 0; k < N; k += 4) {
            const float4 v = *(const float4 *)(row + ((x + k + ox) & 63));
            d[k] = v.x; d[k + 1] = v.y; d[k + 2] = v.z; d[k + 3] = v.w;
        }
    } else {
        static_assert(N == 2, "a thread owns 2, 4 or 8 samples of a plane row");
        const float2 v = *(const float2 *)(row + ((x + ox) & 63));
        d[0] = v.x; d[1] = v.y;
    }
}

// One unit of a vector kernel that works by union blocks: the thread's share of a frame, VB bytes of luma per row
// (PXT samples), BH luma rows, NB union blocks side by side.  The input chroma rows (IRH) and output chroma rows (ORH) of the
// unit are separate word arrays.
template <int WIN, int WOUT, int ICSX, int ICSY, int OCSX, int OCSY>
struct UnionUnit {
    static constexpr int kWin = WIN, kWout = WOUT, kIcsx = ICSX, kIcsy = ICSY, kOcsx = OCSX, kOcsy = OCSY;
    static constexpr int VB = vec_bytes<WIN, WOUT>();
    static constexpr int PXT = VB / (WIN ? 2 : 1);                       // luma samples per thread per row
    static constexpr int YWI = VB / 4, YWO = PXT * (WOUT ? 2 : 1) / 4;   // luma words per thread per row, in / out
    static constexpr int CSX = cmax(ICSX, OCSX), CSY = cmax(ICSY, OCSY);
    static constexpr int BW = 1 << CSX, BH = 1 << CSY;                   // the union block
    static constexpr int NB = PXT / BW;                                  // union blocks per thread
    static constexpr int IRH = BH >> ICSY, ORH = BH >> OCSY;             // chroma rows per thread, in / out
    static constexpr int IBX = BW >> ICSX, OBX = BW >> OCSX;             // chroma samples per union block and row, in / out
    static constexpr int CWI = (PXT >> ICSX) * (WIN ? 2 : 1) / 4, CWO = (PXT >> OCSX) * (WOUT ? 2 : 1) / 4;
    static constexpr int CPX = PXT >> OCSX;                              // output chroma samples per thread per row
    static_assert(NB >= 1 && CWI >= 1 && CWO >= 1 && YWO >= 1, "a thread must own whole words");
    // the units of a launch: what a one-shot kernel compares its thread against and a grid-stride kernel walks up to
    static __device__ __forceinline__ unsigned count(const FrameGeom &G)
    {
        return ((unsigned)G.w / PXT) * ((unsigned)G.rows >> CSY) * (unsigned)G.nframes;
    }
};

// the same count on the host, for the launchers of one container mix (the layout checks are their callers')
template <int WI, int WO>
inline long long union_units(const FrameGeom &G, int icsy, int ocsy)
{
    constexpr int PXT = vec_bytes<WI, WO>() / (WI ? 2 : 1);
    return (long long)(G.w / PXT) * (G.rows >> cmax(icsy, ocsy)) * G.nframes;
}

// the nine pairs of chroma layouts (ICSX, ICSY, OCSX, OCSY) these kernels are instantiated for
#define LUTR_UNION_PAIRS(X) \
    X(1, 1, 1, 1) X(1, 1, 1, 0) X(1, 1, 0, 0) \
    X(1, 0, 1, 1) X(1, 0, 1, 0) X(1, 0, 0, 0) \
    X(0, 0, 1, 1) X(0, 0, 1, 0) X(0, 0, 0, 0)

// Unit u of a launch, whole: k_yuv_vec's structure (lutr_kernels.hip) -- whole-word loads and stores, lattice taps gathered from
// L1/L2 -- for every pair of layouts; the thread walks its union blocks one after the other.  px(q) -> o: the family's stages on
// the codes q of one pixel behind the YUV -> RGB stage.  The body of k_yuv_xsub_vec, k_yuv_bn_vec, k_yuv_chain_vec and
// k_yuv_cdl_vec; the kernel keeps how units are walked.  (k_yuv_l1d_vec and k_yuv_stack*_vec hold copies of it: DESIGN.md 3.8.)  BN
// (3.15): the offsets of the thread's output samples are loaded beside its source words, PXT floats per luma row, PXT >> OCSX
// per output chroma row and plane (the table, 16 KB, stays in L1 / L2); otherwise bn is not read.
template <class U, bool BN = false, class Px>
__device__ __forceinline__ void union_vec_unit(unsigned u, const YuvConsts &K, const PlaneSet &P, const FrameGeom &G, Px px,
                                               const float *__restrict__ bn = nullptr)
{
    constexpr int WIN = U::kWin, WOUT = U::kWout, ICSX = U::kIcsx, ICSY = U::kIcsy, OCSX = U::kOcsx, OCSY = U::kOcsy;
    constexpr int PXT = U::PXT, YWI = U::YWI, YWO = U::YWO, BW = U::BW, BH = U::BH, IRH = U::IRH, ORH = U::ORH, IBX = U::IBX,
                  OBX = U::OBX, CWI = U::CWI, CWO = U::CWO, CPX = U::CPX;
    const unsigned uw = (unsigned)G.w / PXT;
    const unsigned ub = (unsigned)G.rows >> U::CSY;
    const unsigned xu = u % uw, t = u / uw;
    const int y0 = ((G.row0 >> U::CSY) + (int)(t % ub)) * BH;     // first luma row of the thread
    const long long fr = t / ub;
    const long long xi = (long long)xu * U::VB, xo = (long long)xu * (YWO * 4), cxi = (long long)xu * (CWI * 4),
                    cxo = (long long)xu * (CWO * 4);

    uint32_t yw[BH][YWI], cbw[IRH][CWI], crw[IRH][CWI];
    uint32_t yo[BH][YWO], cbo[ORH][CWO], cro[ORH][CWO];
    float dy_[BH][BN ? PXT : 1], dcb[ORH][BN ? CPX : 1], dcr[ORH][BN ? CPX : 1];   // the offsets of the thread's output samples
#pragma unroll
    for (int dy = 0; dy < BH; dy++) {
        ld_words<YWI>(yw[dy], P.s[0] + fr * P.sfs[0] + (long long)(y0 + dy) * P.ss[0] + xi);
        if constexpr (BN) ld_bn<PXT>(dy_[dy], bn + (((y0 + dy + bn_oy(0)) & 63) << 6), (int)xu * PXT, bn_ox(0));
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
    for (int oy = 0; oy < ORH; oy++) {
        if constexpr (BN) {
            const int r = (y0 >> OCSY) + oy;
            ld_bn<CPX>(dcb[oy], bn + (((r + bn_oy(1)) & 63) << 6), (int)xu * CPX, bn_ox(1));
            ld_bn<CPX>(dcr[oy], bn + (((r + bn_oy(2)) & 63) << 6), (int)xu * CPX, bn_ox(2));
        }
#pragma unroll
        for (int k = 0; k < CWO; k++) { cbo[oy][k] = 0; cro[oy][k] = 0; }
    }

#pragma unroll
    for (int j = 0; j < U::NB; j++) {
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
                const Rgb o = px(yuv_to_rgb(K, word_sample<WIN>(yw[dy], i), c[dy >> ICSY][dx >> ICSX]));
                rs[dy >> OCSY][dx >> OCSX] += o.r; gs[dy >> OCSY][dx >> OCSX] += o.g; bs[dy >> OCSY][dx >> OCSX] += o.b;
                if constexpr (BN) word_put<WOUT>(yo[dy], i, rgb_to_y(K, o, dy_[dy][i]));
                else word_put<WOUT>(yo[dy], i, rgb_to_y(K, o));
            }
        }
#pragma unroll
        for (int oy = 0; oy < ORH; oy++)
#pragma unroll
            for (int ox = 0; ox < OBX; ox++) {
                const int i = j * OBX + ox;
                if constexpr (BN) {
                    word_put<WOUT>(cbo[oy], i, rgb_to_cb(K, rs[oy][ox], gs[oy][ox], bs[oy][ox], dcb[oy][i]));
                    word_put<WOUT>(cro[oy], i, rgb_to_cr(K, rs[oy][ox], gs[oy][ox], bs[oy][ox], dcr[oy][i]));
                } else {
                    word_put<WOUT>(cbo[oy], i, rgb_to_cb(K, rs[oy][ox], gs[oy][ox], bs[oy][ox]));
                    word_put<WOUT>(cro[oy], i, rgb_to_cr(K, rs[oy][ox], gs[oy][ox], bs[oy][ox]));
                }
            }
        // Zero-instruction fence (k_yuv_vec's): keeps hipcc from hoisting the coordinates and taps of every union block of the
        // thread to the top; with it the blocks are emitted one after the other.
#pragma unroll
        for (int dy = 0; dy < BH; dy++) {
#pragma unroll
            for (int k = 0; k < YWI; k++) asm volatile("" : "+v"(yw[dy][k]));
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

// ---------------------------------------------------------------- premultiplied alpha
// a * b + c for a, b below 2^24 and a sum below 2^32: v_mad_u32_u24, full rate (a 32-bit multiply is quarter rate)
__host__ __device__ __forceinline__ uint32_t mad24(uint32_t a, uint32_t b, uint32_t c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul24(a, b) + c;
#else
    return a * b + c;
#endif
}

// floor(num / den) for 1 <= den < 2^16 and a quotient below 2^16; rcp = 1 / den to within 2 ulp.  The fp32 estimate is off by
// less than 2^16 * (2^-24 + 2^-22) + 2^-8 < 2^-5 of the true ratio; biased up by 2^-5 its floor is the quotient or one above it,
// and one multiply-subtract decides.
__host__ __device__ __forceinline__ uint32_t div_q16(uint32_t num, uint32_t den, float rcp)
{
    const uint32_t q = (uint32_t)__builtin_fmaf((float)num, rcp, 0.03125f);
    const int32_t r = (int32_t)(num - mad24(q, den, 0u));
    return q + (uint32_t)(r >> 31);                               // r < 0: one too many
}

// What the three channels of a pixel share in the unpremultiply step.  den = a, or Ma for a == 0: floor(C * Ma / Ma) is the
// contract's S = C with no select.  lim = Ml * den: a numerator at or above it gives Ml.
struct UnpremulPx {
    uint32_t den, half, lim;
    float rcp;                       // 1 / den (v_rcp_f32: 1 ulp)
};

// S = min(Ml, floor((c * ma + floor(a / 2)) / a)) for a > 0, c for a == 0; c <= ml <= ma < 2^16 (the numerator stays below 2^32).
// The clamp goes first, on the numerator: floor(lim / den) is Ml exactly, and the division only sees quotients up to Ml.
__host__ __device__ __forceinline__ uint32_t unpremul_code(uint32_t c, const UnpremulPx &u, uint32_t ma)
{
    const uint32_t num = mad24(c, ma, u.half);
    return div_q16(num < u.lim ? num : u.lim, u.den, u.rcp);
}

// P = floor((c * a + floor(ma / 2)) / ma), ma = 2^d - 1, c and a up to ma: x / (2^d - 1) = (x + (x >> d) + 1) >> d for every
// x below 2^2d - 1, and x is at most ma * ma + ma / 2.
__host__ __device__ __forceinline__ uint32_t premul_code(uint32_t c, uint32_t a, uint32_t ma, int d)
{
    const uint32_t x = mad24(c, a, ma >> 1);
    return (x + (x >> d) + 1u) >> d;
}

}  // namespace lutr
