// lutr_tube.h -- what the LDS tile kernels share: small machine helpers, the per-code coordinate pair, the two-level chunk queue
// of the tube kernels (lutr_tile2.hip, lutr_rgb2.hip) and the host-side LDS layouts padded against bank conflicts.  lutr_tile.hip
// takes the helpers and chunk_at; its one-level queue is a different protocol and lives there.
#pragma once
#include <cstdlib>

#include "lutr_internal.h"

namespace lutr {
namespace tube {

#define DEV __device__ __forceinline__

// ---------------------------------------------------------------- small machine helpers
DEV float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
DEV float med3(float a, float lo, float hi) { return __builtin_amdgcn_fmed3f(a, lo, hi); }
DEV int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
DEV float unif(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
// v_min3 / v_max3 fold two values per instruction; written as asm because hipcc only forms them from some fminf / fmaxf chains
DEV float vmin3(float a, float b, float c) { float o; asm("v_min3_f32 %0, %1, %2, %3" : "=v"(o) : "v"(a), "v"(b), "v"(c)); return o; }
DEV float vmax3(float a, float b, float c) { float o; asm("v_max3_f32 %0, %1, %2, %3" : "=v"(o) : "v"(a), "v"(b), "v"(c)); return o; }
DEV float wave_min(float v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fminf(v, __shfl_xor(v, m, 64));
    return v;
}
DEV float wave_max(float v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}
// FFmpeg's lerp: each of the three ops rounds on its own (-ffp-contract=off)
DEV float tlerp(float v0, float v1, float f) { return v0 + (v1 - v0) * f; }

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f2v __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------- samples in word vectors
// sample i of a vector of 16-bit (WIDE) or 8-bit samples, as a float
template <int WIDE> DEV float wsample(const uint32_t *w, int i)
{
    if constexpr (WIDE) return (float)((w[i >> 1] >> ((i & 1) * 16)) & 0xffffu);
    else return (float)((w[i >> 2] >> ((i & 3) * 8)) & 0xffu);
}
// NW words (1, 2 or a multiple of 4) to memory, non-temporal: every output byte is written once
// (The loads and the SDWA sample insert stay in each file: lutr_tile2.hip loads non-temporally, the others do not, and its wput and
// lutr_rgb2.hip's put, the same idea, compile to differently scheduled code when they share one body.)
template <int NW> DEV void stw(uint8_t *p, const uint32_t *w)
{
    typedef unsigned nt4 __attribute__((ext_vector_type(4)));
    typedef unsigned nt2 __attribute__((ext_vector_type(2)));
    if constexpr (NW == 1) __builtin_nontemporal_store(w[0], (uint32_t *)p);
    else if constexpr (NW == 2) __builtin_nontemporal_store(nt2{w[0], w[1]}, (nt2 *)p);
    else {
#pragma unroll
        for (int j = 0; j < NW / 4; j++) __builtin_nontemporal_store(nt4{w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3]}, (nt4 *)(p + 16 * j));
    }
}

// ---------------------------------------------------------------- coordinates
// (prev, frac) of one channel
struct Crd { float p, d; };

// lattice coordinate -> cell and fraction; nearest rounds to a node: NEAR(x) = (int)(x + .5) with a double .5 (lutr_device.h near_f)
template <int INTERP> DEV Crd crd_split(float s)
{
    Crd c;
    if constexpr (INTERP == LUTR_INTERP_NEAREST) {
        const float fl = floorf(s);
        c.p = (s - fl >= .5f) ? fl + 1.0f : fl;
        c.d = 0.0f;
    } else { c.p = floorf(s); c.d = s - c.p; }
    return c;
}

// The per-code {prev, frac} table sits at LDS address 0 (the kernels have no static LDS, the dynamic block starts at 0), so a
// byte offset IS the address: no v_add of the block's base.
typedef __attribute__((address_space(3))) const f2v *lds_f2p;
DEV Crd crd_table8(unsigned off)
{
    const f2v e = *(lds_f2p)(uintptr_t)off;
    return Crd{e.x, e.y};
}
// The YUV tile kernels (lutr_tile2.hip) keep the cell as an INTEGER, in the table ({int32 prev, float frac}) and from there on: the tap
// address is then three fma on the cells' bits, with no conversion (struct Win there), and nothing downstream converts.  The RGB tube kernels
// (lutr_rgb2.hip) keep the float pair above: their bodies subtract cells per pixel pair (the tube test), in fp32 as ever.
struct CrdI { int p; float d; };
typedef unsigned u2v_ __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) const u2v_ *lds_u2p;
DEV CrdI crd_table8i(unsigned off)
{
    const u2v_ e = *(lds_u2p)(uintptr_t)off;
    return CrdI{(int)e.x, __uint_as_float(e.y)};
}

// ---------------------------------------------------------------- work distribution
// Work is handed out in chunks of `ch` consecutive tile rows of one strip; chunk id = (frame * nrc + row chunk) * nsx + strip, so
// chunks claimed at about the same time are neighbouring strips of the same rows.  Position of chunk c; false when c is past the end.
// G: the kernel's geometry struct (nchunks, nsx, nrc, ch, nry; the queue below also reads queue and qbase).
template <class G> DEV bool chunk_at(const G &TG, unsigned c, int &fr, int &sx, int &ry, int &rem)
{
    if (c >= (unsigned)TG.nchunks) return false;
    const int per_frame = TG.nrc * TG.nsx;
    fr = (int)c / per_frame;
    const int r = (int)c - fr * per_frame;
    const int rc = r / TG.nsx;
    sx = r - rc * TG.nsx;
    ry = rc * TG.ch;
    rem = min(TG.ch, TG.nry - ry);
    return true;
}

// THE TWO-LEVEL CHUNK QUEUE.  Every wave takes its first chunk by its id (a burst of atomics on one address at kernel start
// serialises in the L2).  After that a wave draws a ticket from its workgroup's LDS counter (a ds_add_rtn, ~100 cycles on the lgkm
// counter, the vector-memory pipeline keeps running); ticket 16 j + slot means chunk base[j] + slot, and the wave that draws slot 0
// fetches base[j] = atomicAdd(queue, 16) for the block and publishes it in LDS (the others of that block, if they arrive before it has
// landed, spin on the ready tag -- all waves of a workgroup are resident, the publisher cannot be descheduled).  One claim in sixteen
// pays the L2 round trip that a single counter paid on every claim (its phase timers: 9 % of a wave's time, with the memory pipeline
// drained behind it), and the global counter sees a sixteenth of the traffic, so short launches can use smaller chunks
// (profiles/r03_exp18_two_level_queue.txt, r03_exp20_rgb_tube_two_level_queue.txt; the one-level queue this replaced can be recovered
// from git history).
// TG.queue: device words {claims, waves done}, both 0 between launches -- the last wave to leave resets them (queue_leave), so a launch
// needs no memset node in front of it (profiles/r03_exp33_self_resetting_queue.txt).  TG.qbase: waves in the grid = the first chunk the
// counter hands out (the waves' ids come before it).
// LDS: kQueueLds bytes per workgroup, as words -- ticket at 0, base[8] at 8, ready[8] at 16, waves that have left at 24.  The functions
// take the LDS address of the kernel's dynamic block (`lds0`: the file's own lds_base(), each kernel file names its block itself) and
// the byte offset of the queue's words in it.
constexpr int kQueueLds = 128;
typedef __attribute__((address_space(3))) volatile unsigned *lds_vup;

// The kernel zeroes words 0 and 8..30 before its first barrier (`if (threadIdx.x < 24) words[threadIdx.x + (threadIdx.x ? 7 : 0)] = 0`,
// written out in each kernel: as a function here it compiled to different code).
// WPB: waves per workgroup
template <int WPB, class G> DEV bool claim_chunk(const G &TG, int lane, int lds0, int wgq_off, int &fr, int &sx, int &ry, int &rem, bool &first)
{
    unsigned c = 0;
    if (first) {
        // (a wave whose id is not a chunk has no work at all: the counter starts behind the ids.  It must not touch the
        // allocator's LDS words either -- this call runs before they are initialised.)
        first = false;
        c = (unsigned)((int)(blockIdx.x * WPB) + uni((int)(threadIdx.x >> 6)));
        return chunk_at(TG, c, fr, sx, ry, rem);
    }
    const lds_vup q = (lds_vup)(uintptr_t)(unsigned)(lds0 + wgq_off);
    unsigned t = 0;
    if (lane == 0) t = __hip_atomic_fetch_add((__attribute__((address_space(3))) unsigned *)q, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    t = (unsigned)uni((int)t);
    const unsigned j = t >> 4, slot = t & 15u, r = j & 7u;
    if (slot == 0) {
        if (lane == 0) {
            c = atomicAdd(TG.queue, 16u) + TG.qbase;
            q[8 + r] = c;                                  // base[r]
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            q[16 + r] = j + 1u;                            // ready[r]
        }
        c = (unsigned)uni((int)c);
    } else {
        while ((unsigned)uni((int)q[16 + r]) != j + 1u) __builtin_amdgcn_s_sleep(2);
        c = (unsigned)uni((int)q[8 + r]) + slot;
    }
    return chunk_at(TG, c, fr, sx, ry, rem);
}

// Every wave calls this once, when it will claim no more: the last one puts the two words back to zero for the next launch.  (A wave's
// claims have returned before it gets here -- it needed their values -- so the plain stores cannot overtake anybody's atomic.)
template <int WPB, class G> DEV void queue_leave(const G &TG, int lane, int lds0, int wgq_off)
{
    // two levels, like the claims: the waves of a workgroup count themselves out in LDS, the last one reports the workgroup -- 4096
    // atomics on one address at the end of a short launch cost it 15 us
    if (lane == 0) {
        const lds_vup q = (lds_vup)(uintptr_t)(unsigned)(lds0 + wgq_off);
        const unsigned left = __hip_atomic_fetch_add((__attribute__((address_space(3))) unsigned *)(q + 24), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (left == (unsigned)WPB - 1u) {
            const unsigned done = atomicAdd(TG.queue + 1, 1u);
            if (done == gridDim.x - 1u) {
                __hip_atomic_store(TG.queue, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(TG.queue + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

// ---------------------------------------------------------------- LDS layouts (host)
// The tube holds every cell with |pg - pr| <= H and |pb - pg| <= H, all of r; node index = pr * A + (pg - pr) * nb + (pb - pg) + const
// = pr * (plane - nb) + pg * (nb - 1) + pb + const.  The second difference axis is (b - g), not (b - r): with BT.709 / 601 / 2020
// g - r is almost -Cr and b - g almost +Cb (dG = -0.21 cb - 2.33 cr, dBG = 2.33 cb + 0.53 cr at 10 bit), so the tube's cross-section is
// a near-square in the chroma plane; b - r = 2.12 cb - 1.80 cr makes it a parallelogram stretched along the magenta-green diagonal and
// thin along orange-blue, where video lives (profiles/r03_exp3_tube_axis_and_padding.txt).
//
// Nodes between two r planes of the tube.  The lanes of a wave read cells that are mostly one step apart (neighbouring pixels):
// with node index = pr * A + pg * B + pb two of them collide in the LDS banks when dr * A + dg * B + db is a multiple of 32 (a tap
// read is 32 lanes per pass, the bank is the dword address mod 32 or 64, node strides of 2 or 3 dwords are invertible mod 32).
// The unpadded 15 x 15 and 17 x 17 planes of the strict kernels' tubes have exactly that for (dr, dg) = +-(1, 1): every luma step
// that moves r and g but not b costs a second LDS pass.  A few nodes of padding per plane remove it for steps of +-1 (+-2 if possible).
// 16-byte nodes are read with ds_read_b128: 16 lanes per pass, bank = dword address mod 64, a node is four dwords -- two lanes
// collide when their node indices agree mod 16 (not 32).
inline int lds_collisions(int A, int B, int mod)
{
    int bad = 0;
    for (int dr = -2; dr <= 2; dr++)
        for (int dg = -2; dg <= 2; dg++)
            for (int db = -2; db <= 2; db++) {
                if (!dr && !dg && !db) continue;
                if (((dr * A + dg * B + db) % mod + mod) % mod == 0) bad += (abs(dr) <= 1 && abs(dg) <= 1 && abs(db) <= 1) ? 100 : 1;
            }
    return bad;
}
inline int tube_plane_stride(int nb, int node)
{
    const int mod = node == 16 ? 16 : 32;
    int best = nb * nb, best_bad = 1 << 30;
    for (int pad = 0; pad < 12; pad++) {
        const int plane = nb * nb + pad;
        const int bad = lds_collisions(plane - nb, nb - 1, mod);
        if (bad < best_bad) { best_bad = bad; best = plane; }
        if (!bad) break;
    }
    return best;
}

// Whole-lattice mode: node (r, g, b) sits at index r * A + g * B + b.  With A = n1^2, B = n1 neighbouring cells collide in the LDS
// banks for unlucky sizes (n1 = 20: A = 400 = 0 mod 16 -- every step along r lands in the same bank group of a ds_read_b128).  A few
// nodes of padding per row and per plane remove that, as tube_plane_stride does for the tube.  Returns the bytes, or 0 if no layout
// fits `room`.
inline long long whole_strides(int n1, int node, long long room, int *A, int *B)
{
    const int mod = node == 16 ? 16 : 32;
    long long best_bytes = 0;
    int best_bad = 1 << 30;
    for (int pb = 0; pb < 4; pb++)
        for (int pa = 0; pa < 16; pa++) {
            const int b = n1 + pb, a = n1 * b + pa;
            const long long bytes = (long long)n1 * a * node;
            if (bytes > room) continue;
            const int bad = lds_collisions(a, b, mod);
            if (bad < best_bad || (bad == best_bad && bytes < best_bytes)) { best_bad = bad; best_bytes = bytes; *A = a; *B = b; }
        }
    return best_bytes;
}

}  // namespace tube
}  // namespace lutr
