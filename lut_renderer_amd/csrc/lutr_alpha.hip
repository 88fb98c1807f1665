// lutr_alpha.hip -- gfx950 kernels for the alpha plane of yuva* / gbrap* frames.
//
// What they replace: what the reference's chain does to the fourth plane of an alpha-carrying frame:
//   lut3d=file=...:interp=...   copies the alpha plane through unchanged            (ffmpeg.py:246)
//   format=<pix_fmt>            alpha at the output depth, or opaque when the source has none   (ffmpeg.py:304-310)
// Alpha never meets the colour arithmetic: one plane of h x w samples in, one out, on the stream of the colour pass.
//   same depth           the words are copied as they are
//   integer din -> dout  a = min(word, Mi); a' = floor((2 a Mo + Mi) / (2 Mi)), the nearest code (Mi is odd: no ties).  Evaluated
//                        as (a * K + 2^39) >> 40 with K = ceil(Mo 2^40 / Mi): K is at most 2^-40 too large, a < 2^16, and the exact
//                        value keeps 1 / (2 Mi) > 2^-17 away from the next integer, so the floor is the same; the launcher's
//                        host checks every code of a pair against the integer formula before the pair's first launch
//   float -> integer     q = clip(rintf(a * (float)Mo), 0, Mo), NaN -> 0 decided on the bits (the library is built with
//                        -fno-honor-nans)
//   no source            every sample is Mo
// Memory-bound: no LDS, whole-dword accesses (16 bytes a lane on the wider side), a capped grid with a grid-stride loop.
#include <mutex>

#include "lutr_device.h"
#include "lutr_launch.h"

namespace lutr {

// ================================================================= the sample
__device__ __forceinline__ uint32_t alpha_int(const AlphaArgs &A, uint32_t word)
{
    const uint32_t a = word < A.mi ? word : A.mi;
    return (uint32_t)(((unsigned long long)a * A.k + (1ull << 39)) >> 40);
}

__device__ __forceinline__ uint32_t alpha_float(const AlphaArgs &A, float v)
{
    const uint32_t u = __float_as_uint(v);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0;              // NaN
    return (uint32_t)med3(__builtin_rintf(v * A.mof), 0.0f, A.mof);
}

// ================================================================= vector kernel
// SRC: 0 = 8-bit, 1 = 16-bit, 2 = float32 source words; WOUT: 16-bit destination words.  A thread owns PXT samples of one row:
// 16 for 8 -> 8 bit, else 8 -- 16 bytes on the wider integer side (a float source: two loads of 16 bytes).
template <int SRC, int WOUT>
__global__ __launch_bounds__(256) void k_alpha_vec(AlphaArgs A, FrameGeom G)
{
    constexpr int PXT = (SRC == 0 && !WOUT) ? 16 : 8;
    constexpr int NWI = SRC == 2 ? 8 : PXT * (SRC ? 2 : 1) / 4;   // words in
    constexpr int NWO = PXT * (WOUT ? 2 : 1) / 4;                 // words out
    const unsigned uw = (unsigned)G.w / PXT;
    const unsigned total = uw * (unsigned)G.rows * (unsigned)G.nframes;
    for (unsigned u = blockIdx.x * 256u + threadIdx.x; u < total; u += gridDim.x * 256u) {
        const unsigned xu = u % uw, t = u / uw;
        const long long y = G.row0 + (int)(t % (unsigned)G.rows), fr = t / (unsigned)G.rows;
        const uint8_t *sp = A.s + fr * A.sfs + y * A.ss + (long long)xu * (NWI * 4);
        uint8_t *dp = A.d + fr * A.dfs + y * A.ds + (long long)xu * (NWO * 4);
        uint32_t in[NWI], out[NWO];
        if constexpr (NWI == 8) { ld_words<4>(in, sp); ld_words<4>(in + 4, sp + 16); }
        else ld_words<NWI>(in, sp);
        if constexpr (SRC == WOUT) {                              // same depth: word for word (uniform)
            if (A.copy) { st_words<NWO>(dp, in); continue; }
        }
#pragma unroll
        for (int k = 0; k < NWO; k++) out[k] = 0;
#pragma unroll
        for (int i = 0; i < PXT; i++) {
            uint32_t q;
            if constexpr (SRC == 2) q = alpha_float(A, __uint_as_float(in[i]));
            else if constexpr (SRC == 1) q = alpha_int(A, (in[i >> 1] >> ((i & 1) * 16)) & 0xffffu);
            else q = alpha_int(A, (in[i >> 2] >> ((i & 3) * 8)) & 0xffu);
            if constexpr (WOUT) out[i >> 1] |= q << ((i & 1) * 16);
            else out[i >> 2] |= q << ((i & 3) * 8);
        }
        st_words<NWO>(dp, out);
    }
}

// ================================================================= generic kernel
// One sample per thread: any stride (negative included), any alignment the C-ABI admits, odd sizes; the source sample of pixel x
// is element x * step + off of its row (the A of a packed RGB image).
__global__ __launch_bounds__(256) void k_alpha_generic(AlphaArgs A, FrameGeom G)
{
    const long long total = (long long)G.w * G.rows * G.nframes;
    for (long long u = blockIdx.x * 256ll + threadIdx.x; u < total; u += gridDim.x * 256ll) {
        const int x = (int)(u % G.w);
        const long long t = u / G.w;
        const long long y = G.row0 + (int)(t % G.rows), fr = t / G.rows;
        const uint8_t *row = A.s + fr * A.sfs + y * A.ss;
        const long long e = (long long)x * A.step + A.off;
        uint32_t q;
        if (A.kind == 2) q = alpha_float(A, ((const float *)row)[e]);
        else {
            const uint32_t word = A.swide ? ((const uint16_t *)row)[e] : row[e];
            q = A.copy ? word : alpha_int(A, word);
        }
        uint8_t *drow = A.d + fr * A.dfs + y * A.ds;
        if (A.wout) ((uint16_t *)drow)[x] = (uint16_t)q;
        else drow[x] = (uint8_t)q;
    }
}

// ================================================================= fill
// No alpha on the source: every sample is Mo (opaque).  VEC: a thread stores 16 bytes of whole samples.
template <bool VEC>
__global__ __launch_bounds__(256) void k_alpha_fill(AlphaArgs A, FrameGeom G)
{
    if constexpr (VEC) {
        const unsigned pxt = A.wout ? 8 : 16;
        const unsigned uw = (unsigned)G.w / pxt;
        const unsigned total = uw * (unsigned)G.rows * (unsigned)G.nframes;
        const uint32_t v = A.wout ? A.mo * 0x10001u : A.mo * 0x01010101u;
        const uint32_t out[4] = {v, v, v, v};
        for (unsigned u = blockIdx.x * 256u + threadIdx.x; u < total; u += gridDim.x * 256u) {
            const unsigned xu = u % uw, t = u / uw;
            const long long y = G.row0 + (int)(t % (unsigned)G.rows), fr = t / (unsigned)G.rows;
            st_words<4>(A.d + fr * A.dfs + y * A.ds + (long long)xu * 16, out);
        }
    } else {
        const long long total = (long long)G.w * G.rows * G.nframes;
        for (long long u = blockIdx.x * 256ll + threadIdx.x; u < total; u += gridDim.x * 256ll) {
            const int x = (int)(u % G.w);
            const long long t = u / G.w;
            const long long y = G.row0 + (int)(t % G.rows), fr = t / G.rows;
            uint8_t *drow = A.d + fr * A.dfs + y * A.ds;
            if (A.wout) ((uint16_t *)drow)[x] = (uint16_t)A.mo;
            else drow[x] = (uint8_t)A.mo;
        }
    }
}

// ================================================================= host
// K of a depth pair, checked once against the integer formula over every code; 0 = the check failed (it cannot: see the top)
static unsigned long long alpha_multiplier(int din, int dout)
{
    static unsigned long long memo[17][17];
    static bool known[17][17];
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    if (!known[din][dout]) {
        const unsigned long long mi = (1ull << din) - 1, mo = (1ull << dout) - 1;
        unsigned long long k = ((mo << 40) + mi - 1) / mi;
        for (unsigned long long a = 0; a <= mi; a++)
            if ((a * k + (1ull << 39)) >> 40 != (2 * a * mo + mi) / (2 * mi)) { k = 0; break; }
        memo[din][dout] = k;
        known[din][dout] = true;
    }
    return memo[din][dout];
}

bool alpha_consts(AlphaArgs *A, int kind, int din, int dout)
{
    A->kind = kind;
    A->swide = din > 8;
    A->wout = dout > 8;
    A->mi = kind == 1 ? (1u << din) - 1 : 0;
    A->mo = (1u << dout) - 1;
    A->mof = (float)A->mo;
    A->copy = kind == 1 && din == dout;
    A->k = 0;
    if (kind == 1 && !A->copy && !(A->k = alpha_multiplier(din, dout))) return false;
    return true;
}

// blocks of a grid-stride kernel of this family: enough to fill 256 CUs x 8
constexpr unsigned kAlphaGridCap = 2048;

const char *launch_alpha(hipStream_t st, int variant, const AlphaArgs &A, const FrameGeom &G)
{
    const bool batch = G.nframes > 1;
    const int src = A.kind == 2 ? 2 : A.swide;
    const int pxt = (A.kind == 0 ? !A.wout : (src == 0 && !A.wout)) ? 16 : 8;     // samples a thread of the vector kernel takes
    const long long sb = src == 2 ? 4 : src ? 2 : 1, db = A.wout ? 2 : 1;          // bytes per sample
    const long long sa = src == 2 ? 16 : pxt * sb, da = pxt * db;                  // bytes per access
    auto vec_fits = [&](const AlphaArgs &S, const FrameGeom &H) {
        if (H.w % pxt || !units_fit((long long)(H.w / pxt) * H.rows * H.nframes)) return false;
        if (S.kind != 0 && (S.step != 1 || S.off != 0 || !plane_ok(S.s, S.ss, S.sfs, sa, batch, kStrideAny, false))) return false;
        return plane_ok(S.d, S.ds, S.dfs, da, batch, kStrideAny, false);
    };
    auto vec = [&](const AlphaArgs &S, const FrameGeom &H) -> const char * {
        const dim3 grid(stride_grid(S.kind == 0 ? "k_alpha_fill" : "k_alpha_vec", (long long)(H.w / pxt) * H.rows * H.nframes, kAlphaGridCap)),
                        block(256);
        if (S.kind == 0) { hipLaunchKernelGGL(k_alpha_fill<true>, grid, block, 0, st, S, H); return "k_alpha_fill"; }
        switch (src * 2 + S.wout) {
        case 0:  hipLaunchKernelGGL((k_alpha_vec<0, 0>), grid, block, 0, st, S, H); return "k_alpha_vec<0,0>";
        case 1:  hipLaunchKernelGGL((k_alpha_vec<0, 1>), grid, block, 0, st, S, H); return "k_alpha_vec<0,1>";
        case 2:  hipLaunchKernelGGL((k_alpha_vec<1, 0>), grid, block, 0, st, S, H); return "k_alpha_vec<1,0>";
        case 3:  hipLaunchKernelGGL((k_alpha_vec<1, 1>), grid, block, 0, st, S, H); return "k_alpha_vec<1,1>";
        case 4:  hipLaunchKernelGGL((k_alpha_vec<2, 0>), grid, block, 0, st, S, H); return "k_alpha_vec<2,0>";
        default: hipLaunchKernelGGL((k_alpha_vec<2, 1>), grid, block, 0, st, S, H); return "k_alpha_vec<2,1>";
        }
    };
    auto generic = [&](const AlphaArgs &S, const FrameGeom &H) {
        const dim3 grid(stride_grid(S.kind == 0 ? "k_alpha_fill" : "k_alpha_generic", (long long)H.w * H.rows * H.nframes, kAlphaGridCap)),
                        block(256);
        if (S.kind == 0) { hipLaunchKernelGGL(k_alpha_fill<false>, grid, block, 0, st, S, H); return "k_alpha_fill"; }
        hipLaunchKernelGGL(k_alpha_generic, grid, block, 0, st, S, H);
        return "k_alpha_generic";
    };
    // (no LDS kernel for this path; a ragged right edge is only split off a plane, never off a packed image: step 1)
    return launch_vec_or_generic(variant, A, G, pxt, vec_fits, vec, generic, [&](int wv) {
        AlphaArgs T = A;
        if (T.s) T.s += wv * sb;
        T.d += wv * db;
        return T;
    });
}

}  // namespace lutr
