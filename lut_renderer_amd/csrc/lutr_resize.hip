// lutr_resize.hip -- gfx950 kernel of the output resize: a separable bicubic (B = 0, C = 0.6) from one
// plane size to another, in integer arithmetic, on the planes the LUT path has already written.  It stands in for the `-s WxH`
// the reference appends after its `-vf` chain (ffmpeg.py:312-313), which libswscale runs on the CPU.
//
// Work split.  One workgroup (4 waves) per output tile of kRzTileW columns x A.th rows (64, 32 or 16) of one plane of one frame; the grid
// is every tile of the three planes of every frame, flattened (RzArgs::tile0 gives each plane's first tile inside a frame).
//   1. The tile's per-column start and horizontal weights (transposed, [tap][column]) and its per-row start and vertical
//      weights go to LDS.
//   2. Horizontal pass, A.rows source rows per wave and step: the wave copies the rows' footprint (the source columns its 64
//      output columns read, clamped to the plane) into wave-private LDS rows with consecutive lanes on consecutive samples --
//      all of a lane's loads of the step in flight at once (a register batch of kRzRows x kRzU samples) -- then lane c
//      filters column c out of LDS into the int32 tile T[source row][c].
//   3. Vertical pass out of T: lane c, one output row per wave and step; the row's weights are uniform across the wave (LDS
//      broadcast).  Stores are non-temporal.
// T is 64 int32 wide and every wave reads or writes one whole T row per instruction (lane c -> dword c), so the 32 lanes of
// a ds_read_b32 / ds_write_b32 group hit 32 distinct banks without padding (MI355X_MICROARCH.md LDS table).
//
// Every index clamps to its plane (edge replicate); the table start of an output sample is unclamped.
#include "lutr_internal.h"

namespace lutr {

namespace {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <int W>
__global__ __launch_bounds__(256) void k_resize(RzArgs A)
{
    extern __shared__ int lds[];
    int *T = lds;                                   // [spy][64]
    int *WX = T + A.spy * kRzTileW;                 // [nx][64]
    int *XS = WX + A.nx_max * kRzTileW;             // [64]
    int *WY = XS + kRzTileW;                        // [A.th][ny]
    int *YS = WY + A.th * A.ny_max;             // [A.th]
    uint16_t *RB = (uint16_t *)(YS + A.th);     // [4][rows][spx]

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int f = (int)(blockIdx.x / (unsigned)A.tiles_per_frame);
    int t = (int)(blockIdx.x - (unsigned)f * (unsigned)A.tiles_per_frame);
    const int pi = t >= A.p[2].tile0 ? 2 : (t >= A.p[1].tile0 ? 1 : 0);
    const RzPlane &P = A.p[pi];
    t -= P.tile0;
    const int ty = t / P.tiles_x, tx = t - ty * P.tiles_x;
    const int ox0 = tx * kRzTileW, oy0 = ty * A.th;
    const int ncol = min(kRzTileW, P.dw - ox0), nrow = min(A.th, P.dh - oy0);
    const int nx = P.nx, ny = P.ny;

    if (tid < kRzTileW) XS[tid] = P.xs[min(ox0 + tid, P.dw - 1)];
    for (int e = tid; e < nx * kRzTileW; e += 256) {
        const int k = e >> 6, c = e & 63;
        WX[e] = P.xw[(long long)min(ox0 + c, P.dw - 1) * nx + k];
    }
    for (int e = tid; e < nrow * ny; e += 256) WY[e] = P.yw[(long long)oy0 * ny + e];
    if (tid < nrow) YS[tid] = P.ys[oy0 + tid];
    __syncthreads();

    const int xlo = XS[0], xspan = XS[ncol - 1] + nx - xlo;
    const int ylo = YS[0], yspan = YS[nrow - 1] + ny - ylo;
    const int d = A.depth;
    const int hround = 1 << (d - 3), hshift = d - 2;
    const uint8_t *sbase = P.s + (long long)f * P.sfs;
    uint16_t *rows = RB + wv * A.rows * A.spx;
    const int xoff = XS[lane < ncol ? lane : 0] - xlo;

    // rows r0 + 4 g + wv (g < A.rows) per wave and step; every lane's loads of a step are issued before the first is used
    const int rstep = 4 * A.rows;
    for (int r0 = 0; r0 < yspan; r0 += rstep) {
        for (int i0 = 0; i0 < xspan; i0 += 64 * kRzU) {
            uint16_t v[kRzRows][kRzU];
#pragma unroll
            for (int g = 0; g < kRzRows; g++) {
                const int r = r0 + 4 * g + wv;
                const uint8_t *src = sbase + (long long)clampi(ylo + r, 0, P.sh - 1) * P.ss;
#pragma unroll
                for (int u = 0; u < kRzU; u++) {
                    const int i = i0 + 64 * u + lane;
                    const int sx = clampi(xlo + i, 0, P.sw - 1);
                    v[g][u] = 0;
                    if (g < A.rows && r < yspan && i < xspan) v[g][u] = W ? ((const uint16_t *)src)[sx] : (uint16_t)src[sx];
                }
            }
#pragma unroll
            for (int g = 0; g < kRzRows; g++)
#pragma unroll
                for (int u = 0; u < kRzU; u++) {
                    const int i = i0 + 64 * u + lane;
                    if (g < A.rows && r0 + 4 * g + wv < yspan && i < xspan) rows[g * A.spx + i] = v[g][u];
                }
        }
        __syncthreads();
        if (lane < ncol)
            for (int g = 0; g < A.rows; g++) {
                const int r = r0 + 4 * g + wv;
                if (r >= yspan) break;
                const uint16_t *row = rows + g * A.spx;
                int acc = 0;
                for (int k = 0; k < nx; k++) acc += WX[k * kRzTileW + lane] * (int)row[xoff + k];
                T[r * kRzTileW + lane] = (acc + hround) >> hshift;
            }
        __syncthreads();
    }

    const int vround = 1 << (29 - d), vshift = 30 - d, maxv = (1 << d) - 1;
    uint8_t *dbase = P.d + (long long)f * P.dfs;
    for (int rr = wv; rr < nrow; rr += 4) {
        if (lane >= ncol) continue;
        const int off = YS[rr] - ylo;
        const int *wy = WY + rr * ny;
        int acc = 0;
        for (int k = 0; k < ny; k++) acc += wy[k] * T[(off + k) * kRzTileW + lane];
        const int o = clampi((acc + vround) >> vshift, 0, maxv);
        uint8_t *out = dbase + (long long)(oy0 + rr) * P.ds;
        if (W)
            __builtin_nontemporal_store((uint16_t)o, (uint16_t *)out + ox0 + lane);
        else
            __builtin_nontemporal_store((uint8_t)o, out + ox0 + lane);
    }
}

}  // namespace

size_t resize_lds_bytes(const RzArgs &A)
{
    return ((size_t)A.spy * kRzTileW + (size_t)A.nx_max * kRzTileW + kRzTileW + (size_t)A.th * A.ny_max + A.th) * 4 +
           (size_t)4 * A.rows * A.spx * 2;
}

const char *launch_resize(hipStream_t st, RzArgs A, int nframes)
{
    // th, rows and the footprints come from the host's plan (resize_plan, lutr_api.cpp); the kernel's register batch holds kRzRows rows
    const long long blocks = (long long)A.tiles_per_frame * nframes;
    const size_t lds = resize_lds_bytes(A);
    if (blocks <= 0 || blocks > 0x7fffffffll || lds > 65536 || A.rows < 1 || A.rows > kRzRows) return nullptr;
    const dim3 grid((unsigned)blocks), block(256);
    if (A.depth > 8) {
        hipLaunchKernelGGL(k_resize<1>, grid, block, lds, st, A);
        return "k_resize<16>";
    }
    hipLaunchKernelGGL(k_resize<0>, grid, block, lds, st, A);
    return "k_resize<8>";
}

}  // namespace lutr
