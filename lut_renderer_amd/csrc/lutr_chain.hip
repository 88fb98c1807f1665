// lutr_chain.hip -- gfx950 kernels of the fused YUV pass with TWO lut3d stages.
//
// What they replace: `lut3d=file=A:interp=ia,lut3d=file=B:interp=ib,format=<pix_fmt>` -- a technical LUT followed by a creative
// look.  Both lut3d instances negotiate the same RGB format, so the frame stays integer RGB at the LUT depth between them:
//   q0  = YUV -> integer RGB at the LUT depth             (3.2; chroma replicated over its INPUT block)
//   q1  = lut3d_A(q0)   truncated and clipped to [0, M]   (3.1; A's prelut, if it has one)
//   q2  = lut3d_B(q1)   B's own size and scale; the codes q1 enter B exactly as source codes enter A
//   out = integer RGB -> YUV from q2                      (3.2 / 3.8; chroma = mean over its OUTPUT block)
// The unit of work is 3.8's union block for every pair of layouts, the equal ones included.
//
// One source, two kinds of translation unit (Makefile MIX_RULE):
//   without LUTR_CH_WI   the generic kernel and the launcher
//   LUTR_CH_WI / _WO     the vector kernels of one container mix (8 -> 8, 16 -> 16, 16 -> 8): 9 layout pairs x 3 modes
#include "lutr_device.h"
#include "lutr_launch.h"

namespace lutr {

#ifdef LUTR_CH_WI
// ================================================================= vector kernel, global gather
// union_vec_unit (lutr_device.h), one unit per thread, with the two lattices as its per-pixel stage.  The second gather's
// coordinates are computed from the first one's truncated codes, so its taps are fetched after the first one's have been
// blended: a pixel holds one set of taps at a time.  One template mode serves both stages.
template <int WIN, int WOUT, int ICSX, int ICSY, int OCSX, int OCSY, int INTERP>
__global__ __launch_bounds__(256) void k_yuv_chain_vec(LutConsts L, LutConsts L2, YuvConsts K, PlaneSet P, FrameGeom G)
{
    using U = UnionUnit<WIN, WOUT, ICSX, ICSY, OCSX, OCSY>;
    const GFetch f(L), f2(L2);
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u >= U::count(G)) return;
    auto px = [=](const Rgb &q) __attribute__((always_inline)) {
        const Rgb m = lut3d_px<INTERP>(L, f, q.r, q.g, q.b);
        return lut3d_px<INTERP>(L2, f2, m.r, m.g, m.b);
    };
    union_vec_unit<U>(u, K, P, G, px);
}

// The vector kernels of this translation unit's container mix; the layout checks are the caller's (launch_yuv_chain).
const char *LUTR_CAT(LUTR_CAT(launch_yuv_chain_vec_w, LUTR_CH_WI), LUTR_CH_WO)(hipStream_t st, const LutConsts &L, const LutConsts &L2,
                                                                                const YuvConsts &K, const PlaneSet &P,
                                                                                const FrameGeom &G, int icsx, int icsy, int ocsx,
                                                                                int ocsy, int mode)
{
    constexpr int WI = LUTR_CH_WI, WO = LUTR_CH_WO;
    const dim3 grid((unsigned)((union_units<WI, WO>(G, icsy, ocsy) + 255) / 256)), block(256);
#define CH_CASE(IX, IY, OX, OY, I) \
    if (icsx == IX && icsy == IY && ocsx == OX && ocsy == OY && mode == I) { \
        hipLaunchKernelGGL((k_yuv_chain_vec<WI, WO, IX, IY, OX, OY, I>), grid, block, 0, st, L, L2, K, P, G); \
        return "k_yuv_chain_vec<" LUTR_STR(LUTR_CH_WI) "," LUTR_STR(LUTR_CH_WO) "," #IX "," #IY "," #OX "," #OY "," #I ">"; \
    }
#define CH_PAIR(IX, IY, OX, OY) CH_CASE(IX, IY, OX, OY, 0) CH_CASE(IX, IY, OX, OY, 1) CH_CASE(IX, IY, OX, OY, 2)
    LUTR_UNION_PAIRS(CH_PAIR)
#undef CH_PAIR
#undef CH_CASE
    return nullptr;
}

#else  // !LUTR_CH_WI
// ================================================================= generic kernel
// One thread per union block; any depth, stride or alignment, odd sizes, all five modes on either stage.  xsub_union_block's walk
// (lutr_device.h) with the second lattice behind the first.
__global__ __launch_bounds__(256) void k_yuv_chain_generic(LutConsts L, LutConsts L2, YuvConsts K, PlaneSet P, FrameGeom G, int win,
                                                           int wout, int icsx, int icsy, int ocsx, int ocsy, int mode, int mode2)
{
    const GFetch f(L), f2(L2);
    PlaneSink sink{K, P, wout};
    for_each_block(G, cmax(icsx, ocsx), cmax(icsy, ocsy), false, [&](long long fr, int ux, int uy) {
        xsub_union_block(K, P, G, fr, ux, uy, win, icsx, icsy, ocsx, ocsy, sink, [&](long long, int, int, const Rgb &q) {
            const Rgb m = lut3d_px_rt(mode, L, f, q.r, q.g, q.b);
            return lut3d_px_rt(mode2, L2, f2, m.r, m.g, m.b);
        });
    });
}

// ================================================================= launcher
const char *launch_yuv_chain(hipStream_t st, int variant, const LutConsts &L, const LutConsts &L2, const YuvConsts &K,
                             const PlaneSet &P, const FrameGeom &G, int din, int dout, int icsx, int icsy, int ocsx, int ocsy,
                             int mode, int mode2)
{
    const UnionLaunch U(G, din, dout, icsx, icsy, ocsx, ocsy);
    auto vec = [&](const PlaneSet &Q, const FrameGeom &H) -> const char * {
        if (U.win && U.wout) return launch_yuv_chain_vec_w11(st, L, L2, K, Q, H, icsx, icsy, ocsx, ocsy, mode);
        if (U.win) return launch_yuv_chain_vec_w10(st, L, L2, K, Q, H, icsx, icsy, ocsx, ocsy, mode);
        return launch_yuv_chain_vec_w00(st, L, L2, K, Q, H, icsx, icsy, ocsx, ocsy, mode);
    };
    auto generic = [&](const PlaneSet &Q, const FrameGeom &H, int) {
        hipLaunchKernelGGL(k_yuv_chain_generic, dim3(U.generic_grid("k_yuv_chain_generic", H)), dim3(256), 0, st, L, L2, K, Q, H, U.win,
                           U.wout, icsx, icsy, ocsx, ocsy, mode, mode2);
        return "k_yuv_chain_generic";
    };
    // the vector kernels have one mode for both stages
    return launch_union(variant, P, G, U, vec_mode(mode) && mode2 == mode, vec, generic, "k_yuv_chain_generic");
}
#endif  // LUTR_CH_WI

}  // namespace lutr
