// lutr_xsub.hip -- gfx950 kernels of the fused YUV pass with a chroma subsampling change.
//
// What they replace: the `format=<pix_fmt>` at the end of the reference's filter chain when the pixel format it picks
// has another subsampling than the source (ffmpeg.py:304-310; the ProRes 422 HQ master of ffmpeg.py:417-433 on a 4:2:0
// source, force_8bit's yuv420p on a 4:2:2 / 4:4:4 source).  The contract is 3.2's with the two chroma stages split:
//   up-sampling    each source chroma sample is replicated over its INPUT block (x >> icsx, y >> icsy)
//   down-sampling  each output chroma sample is the mean of the LUT's integer RGB over its OUTPUT block (1/n in cbr..crb,
//                  n = 2^(ocsx + ocsy); a partial block at an odd edge takes the edge column / row again)
// The unit of work is the union block, 2^max(icsx, ocsx) x 2^max(icsy, ocsy) luma samples: it holds whole input and whole
// output chroma blocks.
//
// One source, two kinds of translation unit (Makefile MIX_RULE):
//   without LUTR_XS_WI   the generic kernel, the unquantised pass of the dither path and the launcher
//   LUTR_XS_WI / _WO     the vector kernels of one container mix (8 -> 8, 16 -> 16, 16 -> 8): 6 layout pairs x 3 modes
#include "lutr_device.h"
#include "lutr_launch.h"

namespace lutr {

#ifdef LUTR_XS_WI
// ================================================================= vector kernel, global gather
// union_vec_unit (lutr_device.h) with the lattice as its per-pixel stage, one unit per thread
template <int WIN, int WOUT, int ICSX, int ICSY, int OCSX, int OCSY, int INTERP>
__global__ __launch_bounds__(256) void k_yuv_xsub_vec(LutConsts L, YuvConsts K, PlaneSet P, FrameGeom G)
{
    using U = UnionUnit<WIN, WOUT, ICSX, ICSY, OCSX, OCSY>;
    const GFetch f(L);
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u >= U::count(G)) return;
    auto px = [=](const Rgb &q) __attribute__((always_inline)) { return lut3d_px<INTERP>(L, f, q.r, q.g, q.b); };
    union_vec_unit<U>(u, K, P, G, px);
}

// The vector kernels of this translation unit's container mix; the layout checks are the caller's (launch_yuv_xsub).
const char *LUTR_CAT(LUTR_CAT(launch_yuv_xsub_vec_w, LUTR_XS_WI), LUTR_XS_WO)(hipStream_t st, const LutConsts &L, const YuvConsts &K,
                                                                               const PlaneSet &P, const FrameGeom &G, int icsx,
                                                                               int icsy, int ocsx, int ocsy, int mode)
{
    constexpr int WI = LUTR_XS_WI, WO = LUTR_XS_WO;
    const dim3 grid((unsigned)((union_units<WI, WO>(G, icsy, ocsy) + 255) / 256)), block(256);
#define XS_CASE(IX, IY, OX, OY, I) \
    if (icsx == IX && icsy == IY && ocsx == OX && ocsy == OY && mode == I) { \
        hipLaunchKernelGGL((k_yuv_xsub_vec<WI, WO, IX, IY, OX, OY, I>), grid, block, 0, st, L, K, P, G); \
        return "k_yuv_xsub_vec<" LUTR_STR(LUTR_XS_WI) "," LUTR_STR(LUTR_XS_WO) "," #IX "," #IY "," #OX "," #OY "," #I ">"; \
    }
#define XS_PAIR(IX, IY, OX, OY) XS_CASE(IX, IY, OX, OY, 0) XS_CASE(IX, IY, OX, OY, 1) XS_CASE(IX, IY, OX, OY, 2)
    // a subsampling change: the six unequal pairs of LUTR_UNION_PAIRS
    XS_PAIR(1, 1, 1, 0) XS_PAIR(1, 1, 0, 0)
    XS_PAIR(1, 0, 1, 1) XS_PAIR(1, 0, 0, 0)
    XS_PAIR(0, 0, 1, 1) XS_PAIR(0, 0, 1, 0)
#undef XS_PAIR
#undef XS_CASE
    return nullptr;
}

#else  // !LUTR_XS_WI
// ================================================================= generic kernels
// One thread per union block; any depth, stride or alignment, odd sizes, all five modes.
// (the walk over union blocks, the block body xsub_union_block and the sinks: lutr_device.h)
__global__ __launch_bounds__(256) void k_yuv_xsub_generic(LutConsts L, YuvConsts K, PlaneSet P, FrameGeom G, int win, int wout,
                                                          int icsx, int icsy, int ocsx, int ocsy, int mode)
{
    const GFetch f(L);
    PlaneSink sink{K, P, wout};
    for_each_block(G, cmax(icsx, ocsx), cmax(icsy, ocsy), false, [&](long long fr, int ux, int uy) {
        xsub_union_block(K, P, G, fr, ux, uy, win, icsx, icsy, ocsx, ocsy, sink, [&](long long, int, int, const Rgb &q) {
            return lut3d_px_rt(mode, L, f, q.r, q.g, q.b);
        });
    });
}

// the dither path's pass 1 (k_yuv_float's values, lutr_dither.hip): whole frames, chroma planes in the output layout
__global__ __launch_bounds__(256) void k_yuv_float_xsub(LutConsts L, YuvConsts K, PlaneSet P, FrameGeom G, FloatPlanes F, int win,
                                                        int icsx, int icsy, int ocsx, int ocsy, int mode)
{
    const GFetch f(L);
    FloatSink sink(K, F, G, ocsx, ocsy);
    for_each_block(G, cmax(icsx, ocsx), cmax(icsy, ocsy), true, [&](long long fr, int ux, int uy) {
        xsub_union_block(K, P, G, fr, ux, uy, win, icsx, icsy, ocsx, ocsy, sink, [&](long long, int, int, const Rgb &q) {
            return lut3d_px_rt(mode, L, f, q.r, q.g, q.b);
        });
    });
}

void launch_yuv_float_xsub(hipStream_t st, const LutConsts &L, const YuvConsts &K, const PlaneSet &P, const FrameGeom &G,
                           const FloatPlanes &F, int win, int icsx, int icsy, int ocsx, int ocsy, int mode)
{
    hipLaunchKernelGGL(k_yuv_float_xsub, dim3(block_grid("k_yuv_float_xsub", G.w, G.h, G.nframes, cmax(icsx, ocsx), cmax(icsy, ocsy))), dim3(256),
                       0, st,
                       L, K, P, G, F, win, icsx, icsy, ocsx, ocsy, mode);
}

// ================================================================= launcher
const char *launch_yuv_xsub(hipStream_t st, int variant, const LutConsts &L, const YuvConsts &K, const PlaneSet &P,
                            const FrameGeom &G, int din, int dout, int icsx, int icsy, int ocsx, int ocsy, int mode)
{
    const UnionLaunch U(G, din, dout, icsx, icsy, ocsx, ocsy);
    auto vec = [&](const PlaneSet &Q, const FrameGeom &H) -> const char * {
        if (U.win && U.wout) return launch_yuv_xsub_vec_w11(st, L, K, Q, H, icsx, icsy, ocsx, ocsy, mode);
        if (U.win) return launch_yuv_xsub_vec_w10(st, L, K, Q, H, icsx, icsy, ocsx, ocsy, mode);
        return launch_yuv_xsub_vec_w00(st, L, K, Q, H, icsx, icsy, ocsx, ocsy, mode);
    };
    auto generic = [&](const PlaneSet &Q, const FrameGeom &H, int) {
        hipLaunchKernelGGL(k_yuv_xsub_generic, dim3(U.generic_grid("k_yuv_xsub_generic", H)), dim3(256), 0, st, L, K, Q, H, U.win, U.wout,
                           icsx, icsy, ocsx, ocsy, mode);
        return "k_yuv_xsub_generic";
    };
    // (no LDS-window kernel for a subsampling change; the unit is 4, 8 or 16 luma samples wide, whole union blocks)
    return launch_union(variant, P, G, U, vec_mode(mode), vec, generic);
}
#endif  // LUTR_XS_WI

}  // namespace lutr
