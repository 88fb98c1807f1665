// lutr_cdl.hip -- gfx950 kernels of the fused YUV pass with an ASC CDL in front of lut3d.
//
// What they compute: the per-clip colour decision (slope, offset, power, saturation; ASC CDL v1.2) on the integer RGB the YUV ->
// RGB stage hands lut3d, then the shared show LUT, in one pass:
//   q   = YUV -> integer RGB at the LUT depth              (3.2; chroma replicated over its INPUT block)
//   T_c = tab[c][q_c]                                      (A: slope, offset, clamp and power folded per integer code on the host;
//                                                           no pow on the device)
//   o_c = med3(l + sat * (T_c - l), 0, 1)                  (B: l = (0.2126 T_R + 0.7152 T_G) + 0.0722 T_B; skipped when sat == 1)
//   v   = lut3d on the unit floats o, truncated and clipped to [0, M]   (C: 3.1 from the scale step on)
//   out = integer RGB -> YUV from v                        (3.2 / 3.8; chroma = mean over its OUTPUT block)
// The unit of work is 3.8's union block for every pair of layouts, the equal ones included.  The table is read from global memory
// through L1 like LutConsts::pre (12 KB at 10 bit, 768 KB at 16 bit).
//
// One source, two kinds of translation unit (Makefile MIX_RULE):
//   without LUTR_CD_WI   the generic kernel and the launcher
//   LUTR_CD_WI / _WO     the vector kernels of one container mix (8 -> 8, 16 -> 16, 16 -> 8): 9 layout pairs x 3 modes
#include "lutr_device.h"
#include "lutr_launch.h"

namespace lutr {

#ifdef LUTR_CD_WI
// ================================================================= vector kernel, global gather
// union_vec_unit (lutr_device.h), one unit per thread, with the table reads, the saturation mix and the lattice as its per-pixel
// stage: a pixel's three table reads are issued together, the lattice taps depend on them.
template <int WIN, int WOUT, int ICSX, int ICSY, int OCSX, int OCSY, int INTERP>
__global__ __launch_bounds__(256) void k_yuv_cdl_vec(LutConsts L, CdlConsts C, YuvConsts K, PlaneSet P, FrameGeom G)
{
    using U = UnionUnit<WIN, WOUT, ICSX, ICSY, OCSX, OCSY>;
    const GFetch f(L);
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u >= U::count(G)) return;
    const bool mix = C.sat != 1.0f;                               // a kernel argument: the branch is wave-uniform
    auto px = [=](const Rgb &q) __attribute__((always_inline)) { return lut3d_unit<INTERP>(L, f, cdl_px(C, mix, q)); };
    union_vec_unit<U>(u, K, P, G, px);
}

// The vector kernels of this translation unit's container mix; the layout checks are the caller's (launch_yuv_cdl).
const char *LUTR_CAT(LUTR_CAT(launch_yuv_cdl_vec_w, LUTR_CD_WI), LUTR_CD_WO)(hipStream_t st, const LutConsts &L, const CdlConsts &C,
                                                                              const YuvConsts &K, const PlaneSet &P,
                                                                              const FrameGeom &G, int icsx, int icsy, int ocsx,
                                                                              int ocsy, int mode)
{
    constexpr int WI = LUTR_CD_WI, WO = LUTR_CD_WO;
    const dim3 grid((unsigned)((union_units<WI, WO>(G, icsy, ocsy) + 255) / 256)), block(256);
#define CD_CASE(IX, IY, OX, OY, I) \
    if (icsx == IX && icsy == IY && ocsx == OX && ocsy == OY && mode == I) { \
        hipLaunchKernelGGL((k_yuv_cdl_vec<WI, WO, IX, IY, OX, OY, I>), grid, block, 0, st, L, C, K, P, G); \
        return "k_yuv_cdl_vec<" LUTR_STR(LUTR_CD_WI) "," LUTR_STR(LUTR_CD_WO) "," #IX "," #IY "," #OX "," #OY "," #I ">"; \
    }
#define CD_PAIR(IX, IY, OX, OY) CD_CASE(IX, IY, OX, OY, 0) CD_CASE(IX, IY, OX, OY, 1) CD_CASE(IX, IY, OX, OY, 2)
    LUTR_UNION_PAIRS(CD_PAIR)
#undef CD_PAIR
#undef CD_CASE
    return nullptr;
}

#else  // !LUTR_CD_WI
// ================================================================= generic kernel
// One thread per union block; any depth, stride or alignment, odd sizes, all five modes.  xsub_union_block's walk (lutr_device.h)
// with the CDL in front of the lattice.
__global__ __launch_bounds__(256) void k_yuv_cdl_generic(LutConsts L, CdlConsts C, YuvConsts K, PlaneSet P, FrameGeom G, int win,
                                                         int wout, int icsx, int icsy, int ocsx, int ocsy, int mode)
{
    const GFetch f(L);
    PlaneSink sink{K, P, wout};
    const bool mix = C.sat != 1.0f;
    for_each_block(G, cmax(icsx, ocsx), cmax(icsy, ocsy), false, [&](long long fr, int ux, int uy) {
        xsub_union_block(K, P, G, fr, ux, uy, win, icsx, icsy, ocsx, ocsy, sink, [&](long long, int, int, const Rgb &q) {
            return lut3d_unit_rt(mode, L, f, cdl_px(C, mix, q));
        });
    });
}

// ================================================================= launcher
const char *launch_yuv_cdl(hipStream_t st, int variant, const LutConsts &L, const CdlConsts &C, const YuvConsts &K, const PlaneSet &P,
                           const FrameGeom &G, int din, int dout, int icsx, int icsy, int ocsx, int ocsy, int mode)
{
    const UnionLaunch U(G, din, dout, icsx, icsy, ocsx, ocsy);
    auto vec = [&](const PlaneSet &Q, const FrameGeom &H) -> const char * {
        if (U.win && U.wout) return launch_yuv_cdl_vec_w11(st, L, C, K, Q, H, icsx, icsy, ocsx, ocsy, mode);
        if (U.win) return launch_yuv_cdl_vec_w10(st, L, C, K, Q, H, icsx, icsy, ocsx, ocsy, mode);
        return launch_yuv_cdl_vec_w00(st, L, C, K, Q, H, icsx, icsy, ocsx, ocsy, mode);
    };
    auto generic = [&](const PlaneSet &Q, const FrameGeom &H, int) {
        hipLaunchKernelGGL(k_yuv_cdl_generic, dim3(U.generic_grid("k_yuv_cdl_generic", H)), dim3(256), 0, st, L, C, K, Q, H, U.win, U.wout,
                           icsx, icsy, ocsx, ocsy, mode);
        return "k_yuv_cdl_generic";
    };
    return launch_union(variant, P, G, U, vec_mode(mode), vec, generic, "k_yuv_cdl_generic");
}
#endif  // LUTR_CD_WI

}  // namespace lutr
