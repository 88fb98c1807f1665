// lutr_l1d.hip -- gfx950 kernels of a 1D LUT, alone or ahead of lut3d in the fused YUV pass.
//
// What they compute: ffmpeg's `lut1d=file=tech.cube,lut3d=file=look.cube` on the integer RGB the YUV -> RGB stage hands lut3d:
//   q    = YUV -> integer RGB at the LUT depth            (3.2; chroma replicated over its INPUT block)
//   q'_c = tab[c][q_c]                                     (the 1D LUT folded per integer code on the host: lutr_lut1d_table)
//   v    = lut3d on the codes q' (3.1), or q' itself       (INTERP none: lut1d alone)
//   out  = integer RGB -> YUV from v                       (3.2 / 3.8; chroma = mean over its OUTPUT block)
// The unit of work is 3.8's union block for every pair of layouts, the equal ones included.  The table is uint16, 3 x 2^depth
// entries: 1.5 / 6 / 24 KB at 8 / 10 / 12 bit.  The vector kernels walk their units with a grid stride, so that a workgroup can
// stage the table into LDS once (LDS = true) and amortise that over many 256-thread passes; LDS = false reads it from global
// memory through L1 like the CDL's table.  Both read the same entries: the bits do not depend on the choice.
//
// One source, two kinds of translation unit (Makefile MIX_RULE):
//   without LUTR_L1_WI   the generic kernel, the planar RGB kernels and the launchers
//   LUTR_L1_WI / _WO     the vector kernels of one container mix (8 -> 8, 16 -> 16, 16 -> 8): 9 layout pairs x 4 modes x 2 placements
#include "lutr_device.h"
#include "lutr_launch.h"

namespace lutr {

extern __shared__ uint32_t l1d_lds[];                             // the staged table: 3 * stride uint16 (LDS = true)

// The whole table into LDS, once per workgroup: 3 * stride uint16 = 3 * stride / 2 whole words (stride = 2^depth >= 256); the
// launcher sized the dynamic LDS to that.  Every thread of the workgroup must arrive here.
__device__ __forceinline__ void l1d_stage(const L1dConsts &C)
{
    const uint32_t *__restrict__ src = (const uint32_t *)C.tab;
    const int words = 3 * (C.stride >> 1);
    for (int i = threadIdx.x; i < words; i += 256) l1d_lds[i] = src[i];
    __syncthreads();
}

#ifdef LUTR_L1_WI
// ================================================================= vector kernel

template <bool LDS>
__device__ __forceinline__ Rgb l1d_px(const L1dConsts &C, const Rgb &q)
{
    const int ir = (int)q.r, ig = C.stride + (int)q.g, ib = 2 * C.stride + (int)q.b;
    Rgb t;
    if constexpr (LDS) {
        const uint16_t *s = (const uint16_t *)l1d_lds;
        t.r = (float)s[ir]; t.g = (float)s[ig]; t.b = (float)s[ib];
    } else {
        t.r = (float)C.tab[ir]; t.g = (float)C.tab[ig]; t.b = (float)C.tab[ib];
    }
    return t;
}

// union_vec_unit's structure (lutr_device.h), kept as this family's own copy: through the shared body a dozen instances lose a wave
// (DESIGN.md 3.8).  The uint16 lookup sits in front of the lattice, inside a
// grid-stride walk over the units: no thread leaves before the barrier behind the staging.
template <int WIN, int WOUT, int ICSX, int ICSY, int OCSX, int OCSY, int INTERP, bool LDS>
__global__ __launch_bounds__(256) void k_yuv_l1d_vec(LutConsts L, L1dConsts C, YuvConsts K, PlaneSet P, FrameGeom G)
{
    constexpr int VB = vec_bytes<WIN, WOUT>();
    constexpr int PXT = VB / (WIN ? 2 : 1);                       // luma samples per thread per row
    constexpr int YWI = VB / 4, YWO = PXT * (WOUT ? 2 : 1) / 4;   // luma words per thread per row, in / out
    constexpr int CSX = cmax(ICSX, OCSX), CSY = cmax(ICSY, OCSY);
    constexpr int BW = 1 << CSX, BH = 1 << CSY;                   // the union block
    constexpr int NB = PXT / BW;                                  // union blocks per thread
    constexpr int IRH = BH >> ICSY, ORH = BH >> OCSY;             // chroma rows per thread, in / out
    constexpr int IBX = BW >> ICSX, OBX = BW >> OCSX;             // chroma samples per union block and row, in / out
    constexpr int CWI = (PXT >> ICSX) * (WIN ? 2 : 1) / 4, CWO = (PXT >> OCSX) * (WOUT ? 2 : 1) / 4;
    static_assert(NB >= 1 && CWI >= 1 && CWO >= 1 && YWO >= 1, "a thread must own whole words");
    if constexpr (LDS) l1d_stage(C);
    const GFetch f(L);
    const unsigned uw = (unsigned)G.w / PXT;
    const unsigned ub = (unsigned)G.rows >> CSY;
    const unsigned total = uw * ub * (unsigned)G.nframes;
    for (unsigned u = blockIdx.x * 256u + threadIdx.x; u < total; u += gridDim.x * 256u) {
        const unsigned xu = u % uw, t = u / uw;
        const int y0 = ((G.row0 >> CSY) + (int)(t % ub)) * BH;    // first luma row of the thread
        const long long fr = t / ub;
        const long long xi = (long long)xu * VB, xo = (long long)xu * (YWO * 4), cxi = (long long)xu * (CWI * 4),
                        cxo = (long long)xu * (CWO * 4);

        uint32_t yw[BH][YWI], cbw[IRH][CWI], crw[IRH][CWI];
        uint32_t yo[BH][YWO], cbo[ORH][CWO], cro[ORH][CWO];
#pragma unroll
        for (int dy = 0; dy < BH; dy++) {
            ld_words<YWI>(yw[dy], P.s[0] + fr * P.sfs[0] + (long long)(y0 + dy) * P.ss[0] + xi);
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
                    const Rgb t1 = l1d_px<LDS>(C, q);
                    Rgb o;
                    if constexpr (INTERP == LUTR_INTERP_NONE) o = t1;
                    else o = lut3d_px<INTERP>(L, f, t1.r, t1.g, t1.b);
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
}

// The vector kernels of this translation unit's container mix; the layout checks are the caller's (launch_yuv_l1d).  The grid:
// with the table in LDS, eight workgroups a CU, each staging once and walking its share of the units; without, the usual cap.
const char *LUTR_CAT(LUTR_CAT(launch_yuv_l1d_vec_w, LUTR_L1_WI), LUTR_L1_WO)(hipStream_t st, const LutConsts &L, const L1dConsts &C,
                                                                              const YuvConsts &K, const PlaneSet &P,
                                                                              const FrameGeom &G, int icsx, int icsy, int ocsx,
                                                                              int ocsy, int mode, bool lds)
{
    constexpr int WI = LUTR_L1_WI, WO = LUTR_L1_WO;
    const dim3 grid(stride_grid("k_yuv_l1d_vec", union_units<WI, WO>(G, icsy, ocsy), lds ? (unsigned)device_cus() * 8u : kGridStrideCap)), block(256);
    const size_t lds_bytes = lds ? (size_t)3 * C.stride * sizeof(uint16_t) : 0;
#define L1_CASE(IX, IY, OX, OY, I) \
    if (icsx == IX && icsy == IY && ocsx == OX && ocsy == OY && mode == (I)) { \
        if (lds) hipLaunchKernelGGL((k_yuv_l1d_vec<WI, WO, IX, IY, OX, OY, I, true>), grid, block, lds_bytes, st, L, C, K, P, G); \
        else hipLaunchKernelGGL((k_yuv_l1d_vec<WI, WO, IX, IY, OX, OY, I, false>), grid, block, 0, st, L, C, K, P, G); \
        return "k_yuv_l1d_vec<" LUTR_STR(LUTR_L1_WI) "," LUTR_STR(LUTR_L1_WO) "," #IX "," #IY "," #OX "," #OY "," #I ">"; \
    }
#define L1_PAIR(IX, IY, OX, OY) L1_CASE(IX, IY, OX, OY, -1) L1_CASE(IX, IY, OX, OY, 0) L1_CASE(IX, IY, OX, OY, 1) L1_CASE(IX, IY, OX, OY, 2)
    LUTR_UNION_PAIRS(L1_PAIR)
#undef L1_PAIR
#undef L1_CASE
    return nullptr;
}

#else  // !LUTR_L1_WI
// ================================================================= generic kernel
// One thread per union block; any depth, stride or alignment, odd sizes, all five modes and none.  xsub_union_block's walk
// (lutr_device.h) with the table lookup in front of the lattice (read from global memory).
__global__ __launch_bounds__(256) void k_yuv_l1d_generic(LutConsts L, L1dConsts C, YuvConsts K, PlaneSet P, FrameGeom G, int win,
                                                         int wout, int icsx, int icsy, int ocsx, int ocsy, int mode)
{
    const GFetch f(L);
    PlaneSink sink{K, P, wout};
    for_each_block(G, cmax(icsx, ocsx), cmax(icsy, ocsy), false, [&](long long fr, int ux, int uy) {
        xsub_union_block(K, P, G, fr, ux, uy, win, icsx, icsy, ocsx, ocsy, sink, [&](long long, int, int, const Rgb &q) {
            Rgb o;
            o.r = (float)C.tab[(int)q.r];
            o.g = (float)C.tab[C.stride + (int)q.g];
            o.b = (float)C.tab[2 * C.stride + (int)q.b];
            if (mode != LUTR_INTERP_NONE) o = lut3d_px_rt(mode, L, f, o.r, o.g, o.b);
            return o;
        });
    });
}

// ================================================================= launcher of the fused pass
// LUTR_L1D_LDS=0 / 1: where the vector kernels read the table (tests and tools; unset: the measured default below).  A table above
// 24 KB (13 bit and deeper) is always read from global memory.  The default is the faster one on 64 UHD frames.
constexpr size_t kL1dLdsBytes = 24 * 1024;
constexpr bool kL1dLdsDefault = true;
static bool l1d_in_lds(const L1dConsts &C)
{
    if ((size_t)3 * C.stride * sizeof(uint16_t) > kL1dLdsBytes) return false;
    if (const char *e = getenv("LUTR_L1D_LDS")) {
        if (e[0] == '0' && !e[1]) return false;
        if (e[0] == '1' && !e[1]) return true;
    }
    return kL1dLdsDefault;
}

const char *launch_yuv_l1d(hipStream_t st, int variant, const LutConsts &L, const L1dConsts &C, const YuvConsts &K, const PlaneSet &P,
                           const FrameGeom &G, int din, int dout, int icsx, int icsy, int ocsx, int ocsy, int mode)
{
    const UnionLaunch U(G, din, dout, icsx, icsy, ocsx, ocsy);
    const bool lds = l1d_in_lds(C);
    auto vec = [&](const PlaneSet &Q, const FrameGeom &H) -> const char * {
        if (U.win && U.wout) return launch_yuv_l1d_vec_w11(st, L, C, K, Q, H, icsx, icsy, ocsx, ocsy, mode, lds);
        if (U.win) return launch_yuv_l1d_vec_w10(st, L, C, K, Q, H, icsx, icsy, ocsx, ocsy, mode, lds);
        return launch_yuv_l1d_vec_w00(st, L, C, K, Q, H, icsx, icsy, ocsx, ocsy, mode, lds);
    };
    auto generic = [&](const PlaneSet &Q, const FrameGeom &H, int) {
        hipLaunchKernelGGL(k_yuv_l1d_generic, dim3(U.generic_grid("k_yuv_l1d_generic", H)), dim3(256), 0, st, L, C, K, Q, H, U.win, U.wout,
                           icsx, icsy, ocsx, ocsy, mode);
        return "k_yuv_l1d_generic";
    };
    return launch_union(variant, P, G, U, mode == LUTR_INTERP_NONE || vec_mode(mode), vec, generic, "k_yuv_l1d_generic");
}

// ================================================================= lut1d alone on planar RGB
// plane i of gbrp (G, B, R) reads the table of channel 1, 2, 0
__device__ __forceinline__ int l1d_plane_channel(int i) { return i == 0 ? 1 : (i == 1 ? 2 : 0); }

// One thread per dword of a row, the three planes: whole-dword loads and stores, 4 (8 bit) or 2 (16 bit) samples each; a code above
// M in a 16-bit container takes T[M].  A sample is read and written by the same lane, so the planes may be the source's own.
// LDS: the table staged once per workgroup, as in k_yuv_l1d_vec (the walk is a grid stride already).
template <int WIDE, bool LDS>
__global__ __launch_bounds__(256) void k_rgb_l1d(L1dConsts C, PlaneSet P, FrameGeom G, unsigned maxi, int ww)
{
    if constexpr (LDS) l1d_stage(C);
    const long long total = (long long)ww * G.rows * G.nframes;
    for (long long u = blockIdx.x * 256ll + threadIdx.x; u < total; u += (long long)gridDim.x * 256ll) {
        const long long x4 = (u % ww) * 4, t = u / ww;
        const int y = G.row0 + (int)(t % G.rows);
        const long long fr = t / G.rows;
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const unsigned base = (unsigned)(l1d_plane_channel(i) * C.stride);
            auto tab = [&](unsigned code) -> uint32_t {
                if constexpr (LDS) return ((const uint16_t *)l1d_lds)[base + code];
                else return C.tab[base + code];
            };
            const uint32_t v = *(const uint32_t *)(src_row(P, i, fr, y) + x4);
            uint32_t o;
            if constexpr (WIDE) o = tab(min(v & 0xffffu, maxi)) | (tab(min(v >> 16, maxi)) << 16);
            else o = tab(v & 0xffu) | (tab((v >> 8) & 0xffu) << 8) | (tab((v >> 16) & 0xffu) << 16) | (tab(v >> 24) << 24);
            *(uint32_t *)(dst_row(P, i, fr, y) + x4) = o;
        }
    }
}

// One thread per pixel of the columns x0 .. w - 1: any stride or alignment
__global__ __launch_bounds__(256) void k_rgb_l1d_generic(L1dConsts C, PlaneSet P, FrameGeom G, unsigned maxi, int wide, int x0)
{
    const int wt = G.w - x0;
    const long long total = (long long)wt * G.rows * G.nframes;
    for (long long u = blockIdx.x * 256ll + threadIdx.x; u < total; u += (long long)gridDim.x * 256ll) {
        const int x = x0 + (int)(u % wt);
        const long long t = u / wt;
        const int y = G.row0 + (int)(t % G.rows);
        const long long fr = t / G.rows;
        for (int i = 0; i < 3; i++) {
            const uint16_t *__restrict__ tab = C.tab + l1d_plane_channel(i) * C.stride;
            const uint8_t *s = src_row(P, i, fr, y);
            uint8_t *d = dst_row(P, i, fr, y);
            if (wide) ((uint16_t *)d)[x] = tab[min((unsigned)((const uint16_t *)s)[x], maxi)];
            else d[x] = (uint8_t)tab[s[x]];
        }
    }
}

const char *launch_rgb_l1d(hipStream_t st, int variant, const L1dConsts &C, const PlaneSet &P, const FrameGeom &G, int depth)
{
    if (variant == VAR_VEC_LDS) return nullptr;
    const int wide = depth > 8, spw = wide ? 2 : 4;
    const unsigned maxi = (1u << depth) - 1u;
    const bool batch = G.nframes > 1;
    bool aligned = variant != VAR_GENERIC;
    for (int c = 0; c < 3; c++) aligned = aligned && planes_ok(P, c, 4, batch, kStrideAny, false);
    const int ww = aligned ? G.w / spw : 0, wv = ww * spw;
    if (variant == VAR_VEC_GLOBAL && wv != G.w) return nullptr;
    if (ww > 0) {
        const bool lds = l1d_in_lds(C);
        const unsigned grid = stride_grid("k_rgb_l1d", (long long)ww * G.rows * G.nframes, lds ? (unsigned)device_cus() * 8u : kGridStrideCap);
        const size_t lds_bytes = lds ? (size_t)3 * C.stride * sizeof(uint16_t) : 0;
        if (wide && lds) hipLaunchKernelGGL((k_rgb_l1d<1, true>), dim3(grid), dim3(256), lds_bytes, st, C, P, G, maxi, ww);
        else if (wide) hipLaunchKernelGGL((k_rgb_l1d<1, false>), dim3(grid), dim3(256), 0, st, C, P, G, maxi, ww);
        else if (lds) hipLaunchKernelGGL((k_rgb_l1d<0, true>), dim3(grid), dim3(256), lds_bytes, st, C, P, G, maxi, ww);
        else hipLaunchKernelGGL((k_rgb_l1d<0, false>), dim3(grid), dim3(256), 0, st, C, P, G, maxi, ww);
    }
    if (wv < G.w) {
        const unsigned grid = stride_grid("k_rgb_l1d_generic", (long long)(G.w - wv) * G.rows * G.nframes, kGridStrideCap);
        hipLaunchKernelGGL(k_rgb_l1d_generic, dim3(grid), dim3(256), 0, st, C, P, G, maxi, wide, wv);
    }
    if (wv == G.w) return wide ? "k_rgb_l1d<1>" : "k_rgb_l1d<0>";
    if (wv == 0) return "k_rgb_l1d_generic";
    return wide ? "k_rgb_l1d<1>+k_rgb_l1d_generic" : "k_rgb_l1d<0>+k_rgb_l1d_generic";
}
#endif  // LUTR_L1_WI

}  // namespace lutr
