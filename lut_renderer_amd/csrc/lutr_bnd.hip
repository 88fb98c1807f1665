// lutr_bnd.hip -- gfx950 kernels of the fused YUV pass with blue-noise dither in its output stage.
//
// A threshold dither: every output sample is quantised as clip(floor(c + d)) where c is the value the output stage hands to
// clip_floor without dither (3.2's fma chain, 0.5 included) and d in (-0.5, 0.5) comes from a 64 x 64 void-and-cluster table by the
// sample's position in its plane.  No scratch, no coupling between rows or frames: row shards and batches give the bits of the
// whole call.  Everything ahead of the add is 3.8's contract (lutr_xsub.hip) for all nine layout pairs, the three equal ones
// included, in strict arithmetic.
//
// One source, two kinds of translation unit (Makefile MIX_RULE):
//   without LUTR_BN_WI   the generic kernel and the launcher
//   LUTR_BN_WI / _WO     the vector kernels of one container mix (8 -> 8, 16 -> 16, 16 -> 8): 9 layout pairs x 3 modes
#include "lutr_device.h"
#include "lutr_launch.h"

namespace lutr {

#ifdef LUTR_BN_WI
// ================================================================= vector kernel, global gather
// k_yuv_xsub_vec with the offsets in the output stage (union_vec_unit's BN, lutr_device.h).  bn_vec takes the constants by value:
// handed on from the kernel's own arguments, hipcc schedules a dozen instances across a wave boundary.
template <class U, int INTERP>
__device__ __forceinline__ void bn_vec(LutConsts L, YuvConsts K, PlaneSet P, FrameGeom G, const float *__restrict__ bn)
{
    const GFetch f(L);
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u >= U::count(G)) return;
    auto px = [&](const Rgb &q) __attribute__((always_inline)) { return lut3d_px<INTERP>(L, f, q.r, q.g, q.b); };
    union_vec_unit<U, true>(u, K, P, G, px, bn);
}
template <int WIN, int WOUT, int ICSX, int ICSY, int OCSX, int OCSY, int INTERP>
__global__ __launch_bounds__(256) void k_yuv_bn_vec(LutConsts L, YuvConsts K, PlaneSet P, FrameGeom G, const float *__restrict__ bn)
{
    bn_vec<UnionUnit<WIN, WOUT, ICSX, ICSY, OCSX, OCSY>, INTERP>(L, K, P, G, bn);
}

// The vector kernels of this translation unit's container mix; the layout checks are the caller's (launch_yuv_bn).
const char *LUTR_CAT(LUTR_CAT(launch_yuv_bn_vec_w, LUTR_BN_WI), LUTR_BN_WO)(hipStream_t st, const LutConsts &L, const YuvConsts &K,
                                                                             const PlaneSet &P, const FrameGeom &G, const float *bn,
                                                                             int icsx, int icsy, int ocsx, int ocsy, int mode)
{
    constexpr int WI = LUTR_BN_WI, WO = LUTR_BN_WO;
    const dim3 grid((unsigned)((union_units<WI, WO>(G, icsy, ocsy) + 255) / 256)), block(256);
#define BN_CASE(IX, IY, OX, OY, I) \
    if (icsx == IX && icsy == IY && ocsx == OX && ocsy == OY && mode == I) { \
        hipLaunchKernelGGL((k_yuv_bn_vec<WI, WO, IX, IY, OX, OY, I>), grid, block, 0, st, L, K, P, G, bn); \
        return "k_yuv_bn_vec<" LUTR_STR(LUTR_BN_WI) "," LUTR_STR(LUTR_BN_WO) "," #IX "," #IY "," #OX "," #OY "," #I ">"; \
    }
#define BN_PAIR(IX, IY, OX, OY) BN_CASE(IX, IY, OX, OY, 0) BN_CASE(IX, IY, OX, OY, 1) BN_CASE(IX, IY, OX, OY, 2)
    LUTR_UNION_PAIRS(BN_PAIR)
#undef BN_PAIR
#undef BN_CASE
    return nullptr;
}

#else  // !LUTR_BN_WI
// ================================================================= generic kernel
// k_yuv_xsub_generic's walk and block body (lutr_device.h) with a DitherSink: any depth, stride or alignment, odd sizes, all five
// modes, 8 -> 16 bit.  x0: the frame column of the planes' column 0 (a whole number of union blocks).
__global__ __launch_bounds__(256) void k_yuv_bn_generic(LutConsts L, YuvConsts K, PlaneSet P, FrameGeom G, const float *__restrict__ bn,
                                                        int x0, int win, int wout, int icsx, int icsy, int ocsx, int ocsy, int mode)
{
    const GFetch f(L);
    DitherSink sink{K, P, wout, bn, x0, x0 >> ocsx};
    for_each_block(G, cmax(icsx, ocsx), cmax(icsy, ocsy), false, [&](long long fr, int ux, int uy) {
        xsub_union_block(K, P, G, fr, ux, uy, win, icsx, icsy, ocsx, ocsy, sink, [&](long long, int, int, const Rgb &q) {
            return lut3d_px_rt(mode, L, f, q.r, q.g, q.b);
        });
    });
}

// ================================================================= launcher
const char *launch_yuv_bn(hipStream_t st, int variant, const LutConsts &L, const YuvConsts &K, const PlaneSet &P, const FrameGeom &G,
                          const float *bn, int din, int dout, int icsx, int icsy, int ocsx, int ocsy, int mode)
{
    const UnionLaunch U(G, din, dout, icsx, icsy, ocsx, ocsy);
    auto vec = [&](const PlaneSet &Q, const FrameGeom &H) -> const char * {
        if (U.win && U.wout) return launch_yuv_bn_vec_w11(st, L, K, Q, H, bn, icsx, icsy, ocsx, ocsy, mode);
        if (U.win) return launch_yuv_bn_vec_w10(st, L, K, Q, H, bn, icsx, icsy, ocsx, ocsy, mode);
        return launch_yuv_bn_vec_w00(st, L, K, Q, H, bn, icsx, icsy, ocsx, ocsy, mode);
    };
    // the pattern is anchored to the frame: the generic kernel is told where its planes begin
    auto generic = [&](const PlaneSet &Q, const FrameGeom &H, int x0) {
        hipLaunchKernelGGL(k_yuv_bn_generic, dim3(U.generic_grid("k_yuv_bn_generic", H)), dim3(256), 0, st, L, K, Q, H, bn, x0, U.win,
                           U.wout, icsx, icsy, ocsx, ocsy, mode);
        return "k_yuv_bn_generic";
    };
    // k_yuv_xsub_vec's unit and conditions
    return launch_union(variant, P, G, U, vec_mode(mode), vec, generic);
}
#endif  // LUTR_BN_WI

}  // namespace lutr
