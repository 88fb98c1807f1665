// lutr_api.cpp -- C-ABI layer of liblutr.so: contexts, lattice upload, argument
// checking, and the YUV constant block.  Kernels live in lutr_kernels.hip.
//
// Boundary being replaced: the reference spawns `ffmpeg ... -vf ...lut3d=...` per task
// (/root/reference/src/lut_renderer/task_manager.py:145-151 with the argv from
// ffmpeg.py:179-414); include/lutr.h lists which filter-string fragment each entry
// point stands in for.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <atomic>
#include <cstring>
#include <string>
#include <vector>

#include "lutr_internal.h"
#include "lutr_launch.h"
#include "lutr_bn_mask.h"

namespace lutr {

static thread_local std::string g_last_error;

void set_error(const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
}

static int hip_fail(hipError_t e, const char *what)
{
    set_error("%s: %s", what, hipGetErrorString(e));
    return LUTR_EIO;
}

#define HIP_TRY(call) \
    do { \
        hipError_t e_ = (call); \
        if (e_ != hipSuccess) return hip_fail(e_, #call); \
    } while (0)

// ---------------------------------------------------------------- YUV constants
static bool matrix_k(int m, double *kr, double *kb)
{
    switch (m) {
    case LUTR_MATRIX_BT709:  *kr = 0.2126; *kb = 0.0722; return true;
    case LUTR_MATRIX_BT601:  *kr = 0.299;  *kb = 0.114;  return true;
    case LUTR_MATRIX_BT2020: *kr = 0.2627; *kb = 0.0593; return true;
    }
    return false;
}

// DESIGN.md "YUV contract".  All coefficients are formed in double and rounded to
// float once; the kernels then use exactly these floats.  chroma_n: samples of one OUTPUT chroma block (the block mean's n,
// folded into cbr..crb).
static int yuv_consts_n(const lutr_yuv_params &p, int chroma_n, YuvConsts *o)
{
    const int din = LUTR_FMT_DEPTH(p.fmt_in), dout = LUTR_FMT_DEPTH(p.fmt_out), dl = p.lut_depth;
    if (din < 8 || din > 16 || dout < 8 || dout > 16 || dl < 8 || dl > 16) {
        set_error("unsupported bit depth (in %d, lut %d, out %d)", din, dl, dout);
        return LUTR_EINVAL;
    }
    if ((LUTR_FMT_CSX(p.fmt_in) == 0 && LUTR_FMT_CSY(p.fmt_in) == 1) ||
        (LUTR_FMT_CSX(p.fmt_out) == 0 && LUTR_FMT_CSY(p.fmt_out) == 1)) {
        set_error("4:4:0 chroma layout is not supported");
        return LUTR_EINVAL;
    }
    auto range_ok = [](int r) { return r == LUTR_RANGE_TV || r == LUTR_RANGE_PC; };
    if (!range_ok(p.range_src) || !range_ok(p.range_in) || !range_ok(p.range_out)) {
        set_error("bad range value");
        return LUTR_EINVAL;
    }
    const bool prologue = (p.range_src != p.range_in) || (din != dl);
    if (prologue && p.range_src != LUTR_RANGE_PC) {
        // the reference only emits the prologue for full-range sources (ffmpeg.py:129-134, :212)
        set_error("a range/depth prologue is only defined for full-range (pc) sources");
        return LUTR_EINVAL;
    }
    double kr, kb;
    if (!matrix_k(p.matrix_in, &kr, &kb)) {
        set_error("bad matrix_in %d", p.matrix_in);
        return LUTR_EINVAL;
    }
    std::memset(o, 0, sizeof(*o));

    if (prologue) {
        const double mi = (double)((1 << din) - 1);
        const double sl = (double)(1 << (dl - 8));
        const double ml = (double)((1 << dl) - 1);
        const double half_in = (double)(1 << (din - 1));
        double py, pyo, pc, pco;
        if (p.range_in == LUTR_RANGE_TV) {
            py = 219.0 * sl / mi;  pyo = 16.0 * sl;
            pc = 224.0 * sl / mi;  pco = 128.0 * sl - half_in * pc;
        } else {
            py = ml / mi;          pyo = 0.0;
            pc = ml / mi;          pco = 128.0 * sl - half_in * pc;
        }
        o->pre = 1.0f;
        o->py = (float)py;  o->pyb = (float)(pyo + 0.5);
        o->pc = (float)pc;  o->pcb = (float)(pco + 0.5);
        o->pre_max = (float)ml;
    }
    {
        const double kg = 1.0 - kr - kb;
        const double s = (double)(1 << (dl - 8));
        const double m = (double)((1 << dl) - 1);
        double ky, yoff, kc;
        if (p.range_in == LUTR_RANGE_TV) { ky = m / (219.0 * s); yoff = 16.0 * s; kc = m / (224.0 * s); }
        else { ky = 1.0; yoff = 0.0; kc = 1.0; }
        o->ky = (float)ky;
        o->yb = (float)(-ky * yoff + 0.5);
        o->coff = (float)(128.0 * s);
        o->krv = (float)(2.0 * (1.0 - kr) * kc);
        o->kbu = (float)(2.0 * (1.0 - kb) * kc);
        o->kgu = (float)(-2.0 * kb * (1.0 - kb) / kg * kc);
        o->kgv = (float)(-2.0 * kr * (1.0 - kr) / kg * kc);
        o->max_l = (float)m;
    }
    if (!matrix_k(p.matrix_out, &kr, &kb)) {
        set_error("bad matrix_out %d", p.matrix_out);
        return LUTR_EINVAL;
    }
    {
        const double kg = 1.0 - kr - kb;
        const double so = (double)(1 << (dout - 8));
        const double mo = (double)((1 << dout) - 1);
        const double ml = (double)((1 << dl) - 1);
        const double n = (double)chroma_n;
        double ys, yoff, cs;
        if (p.range_out == LUTR_RANGE_TV) { ys = 219.0 * so; yoff = 16.0 * so; cs = 224.0 * so; }
        else { ys = mo; yoff = 0.0; cs = mo; }
        o->cyr = (float)(ys * kr / ml);
        o->cyg = (float)(ys * kg / ml);
        o->cyb = (float)(ys * kb / ml);
        o->yob = (float)(yoff + 0.5);
        o->cbr = (float)(cs * (-kr / (2.0 * (1.0 - kb))) / ml / n);
        o->cbg = (float)(cs * (-kg / (2.0 * (1.0 - kb))) / ml / n);
        o->cbb = (float)(cs * 0.5 / ml / n);
        o->crr = (float)(cs * 0.5 / ml / n);
        o->crg = (float)(cs * (-kg / (2.0 * (1.0 - kr))) / ml / n);
        o->crb = (float)(cs * (-kb / (2.0 * (1.0 - kr))) / ml / n);
        o->cob = (float)(128.0 * so + 0.5);
        o->max_o = (float)mo;
    }
    return LUTR_OK;
}

// lutr_apply_yuv's constants: input and output share the chroma layout
int make_yuv_consts(const lutr_yuv_params &p, YuvConsts *o)
{
    if (LUTR_FMT_CSX(p.fmt_in) != LUTR_FMT_CSX(p.fmt_out) || LUTR_FMT_CSY(p.fmt_in) != LUTR_FMT_CSY(p.fmt_out)) {
        set_error("fmt_in and fmt_out must share chroma subsampling");
        return LUTR_EINVAL;
    }
    return yuv_consts_n(p, 1 << (LUTR_FMT_CSX(p.fmt_in) + LUTR_FMT_CSY(p.fmt_in)), o);
}

// any pair of 4:2:0 / 4:2:2 / 4:4:4 layouts; the block mean is over the OUTPUT block, n = 2^(ocsx + ocsy)
int make_yuv_consts_xsub(const lutr_yuv_params &p, YuvConsts *o)
{
    return yuv_consts_n(p, 1 << (LUTR_FMT_CSX(p.fmt_out) + LUTR_FMT_CSY(p.fmt_out)), o);
}

// down-sampling taps sum to 4 on a co-sited axis, 2 on an interstitial one, 1 on an axis that is not
// subsampled; n is their product.  1/n is folded into cbr..crb like the block mean's 1/4 (formed in double, rounded once).
int make_yuv_consts_sited(const lutr_yuv_params &p, int loc, YuvConsts *o)
{
    if (loc < LUTR_CHROMA_REPLICATE || loc > LUTR_CHROMA_TOPLEFT) {
        set_error("unknown chroma location %d", loc);
        return LUTR_EINVAL;
    }
    const int csx = LUTR_FMT_CSX(p.fmt_in), csy = LUTR_FMT_CSY(p.fmt_in);
    const int rc = make_yuv_consts(p, o);
    if (rc || loc == LUTR_CHROMA_REPLICATE || (csx == 0 && csy == 0)) return rc;
    const int nx = csx ? (loc == LUTR_CHROMA_CENTER ? 2 : 4) : 1;
    const int ny = csy ? (loc == LUTR_CHROMA_TOPLEFT ? 4 : 2) : 1;
    lutr_yuv_params q = p;
    q.fmt_in = LUTR_FMT(LUTR_FMT_DEPTH(p.fmt_in), 0, 0);
    q.fmt_out = LUTR_FMT(LUTR_FMT_DEPTH(p.fmt_out), 0, 0);
    YuvConsts k1;
    if (const int rc1 = make_yuv_consts(q, &k1)) return rc1;
    // n is a power of two: double(c) / n rounds to the same float as the 4:4:4 float times 1/n
    const float inv = 1.0f / (float)(nx * ny);
    o->cbr = k1.cbr * inv; o->cbg = k1.cbg * inv; o->cbb = k1.cbb * inv;
    o->crr = k1.crr * inv; o->crg = k1.crg * inv; o->crb = k1.crb * inv;
    return LUTR_OK;
}

// an RGB source at depth lut_depth.  Only the output side enters the kernels; matrix_in, range_src, range_in and
// the depth of fmt_in are ignored (the block's input-stage entries are filled from the output side's matrix and range so that
// the call cannot fail on them).  The output-stage entries are yuv_consts_n's for a 4:4:4 source at that depth.
int make_yuv_consts_rgb2yuv(const lutr_yuv_params &p, YuvConsts *o)
{
    lutr_yuv_params q = p;
    q.fmt_in = LUTR_FMT(p.lut_depth & 0xff, 0, 0);
    q.matrix_in = p.matrix_out;
    q.range_src = q.range_in = p.range_out;
    return yuv_consts_n(q, 1 << (LUTR_FMT_CSX(p.fmt_out) + LUTR_FMT_CSY(p.fmt_out)), o);
}

// a YUV source converted to integer RGB at lut_depth, the depth of the RGB destination.  Only the input side
// enters the kernels; fmt_out, matrix_out and range_out are ignored (the block's output-stage entries are those of a 4:4:4 output
// at lut_depth with the input side's matrix and range, so that the call cannot fail on them).  With range_src != range_in the
// block is yuv_consts_n's: the prologue of a full-range source lands at (lut_depth, range_in).  Otherwise a depth change is no
// prologue here (yuv_consts_n refuses one for a tv source): it is folded into the input-stage entries, each formed in double and
// rounded once.  For din == lut_depth these are yuv_consts_n's entries bit for bit (pc: Ml / Mi is exactly 1).
int make_yuv_consts_yuv2rgb(const lutr_yuv_params &p, YuvConsts *o)
{
    const int din = LUTR_FMT_DEPTH(p.fmt_in), dl = p.lut_depth;
    lutr_yuv_params q = p;
    q.fmt_out = LUTR_FMT(dl & 0xff, 0, 0);
    q.matrix_out = p.matrix_in;
    q.range_out = p.range_in;
    if (p.range_src != p.range_in) return yuv_consts_n(q, 1, o);
    if (din < 8 || din > 16) {
        set_error("unsupported bit depth (in %d, lut %d)", din, dl);
        return LUTR_EINVAL;
    }
    q.fmt_in = LUTR_FMT(dl & 0xff, LUTR_FMT_CSX(p.fmt_in), LUTR_FMT_CSY(p.fmt_in));
    if (const int rc = yuv_consts_n(q, 1, o)) return rc;
    double kr, kb;
    matrix_k(p.matrix_in, &kr, &kb);                      // (checked by yuv_consts_n)
    const double kg = 1.0 - kr - kb;
    const double s = (double)(1 << (din - 8));
    const double mi = (double)((1 << din) - 1), ml = (double)((1 << dl) - 1);
    double ky, yoff, kc;
    if (p.range_in == LUTR_RANGE_TV) { ky = ml / (219.0 * s); yoff = 16.0 * s; kc = ml / (224.0 * s); }
    else { ky = ml / mi; yoff = 0.0; kc = ml / mi; }
    o->ky = (float)ky;
    o->yb = (float)(-ky * yoff + 0.5);
    o->coff = (float)(128.0 * s);
    o->krv = (float)(2.0 * (1.0 - kr) * kc);
    o->kbu = (float)(2.0 * (1.0 - kb) * kc);
    o->kgu = (float)(-2.0 * kb * (1.0 - kb) / kg * kc);
    o->kgv = (float)(-2.0 * kr * (1.0 - kr) / kg * kc);
    o->max_l = (float)ml;
    return LUTR_OK;
}


// ---------------------------------------------------------------- output resize tables
// The bicubic of libswscale's SWS_BICUBIC defaults (B = 0, C = 0.6).  Evaluated in this exact order: tests/_resize_twin.py
// repeats it operation for operation in double.
static double bicubic_k(double t)
{
    const double a = std::fabs(t);
    if (a < 1.0) return 1.4 * a * a * a - 2.4 * a * a + 1.0;
    if (a < 2.0) return -0.6 * a * a * a + 3.0 * a * a - 4.8 * a + 2.4;
    return 0.0;
}

// Taps per output sample for a luma ratio src -> dst (no checks): 2 * ceil(2 * max(1, src / dst)).
static int resize_taps(int src, int dst)
{
    const double f = (double)src / (double)dst, stretch = f > 1.0 ? f : 1.0;
    return 2 * (int)std::ceil(2.0 * stretch);
}

// One axis of one plane: src / dst are LUMA sizes, cs = log2 subsampling of this plane's axis, cosited = chroma sample j sits on
// luma 2^cs j (else halfway across its block).  start[dst_plane], w[dst_plane * taps].  LUTR_EINVAL when the limits fail.
static int resize_table(int src, int dst, int cs, int cosited, std::vector<int> *start, std::vector<int> *w, int *taps)
{
    if (src < 1 || dst < 1 || cs < 0 || cs > 1 || (long long)dst * 8 < src || dst > 16LL * src) {
        set_error("resize %d -> %d (subsampling %d) outside the limits 1/8 <= dst/src <= 16", src, dst, cs);
        return LUTR_EINVAL;
    }
    const int n = resize_taps(src, dst);
    const int dplane = (dst + (1 << cs) - 1) >> cs;
    const double f = (double)src / (double)dst, stretch = f > 1.0 ? f : 1.0;
    const double step = (double)(1 << cs), o = cosited ? 0.0 : (step - 1.0) / 2.0;
    start->assign(dplane, 0);
    w->assign((size_t)dplane * n, 0);
    std::vector<double> wd(n);
    for (int j = 0; j < dplane; j++) {
        const double X = (step * j + o + 0.5) * f - 0.5;
        const double x = (X - o) / step;
        const int first = (int)std::floor(x) - n / 2 + 1;
        double sum = 0.0;
        for (int k = 0; k < n; k++) {
            wd[k] = bicubic_k(((double)(first + k) - x) / stretch);
            sum += wd[k];
        }
        int *q = w->data() + (size_t)j * n;
        int total = 0, big = 0, mag = 0;
        for (int k = 0; k < n; k++) {
            q[k] = (int)std::floor(wd[k] / sum * 16384.0 + 0.5);
            total += q[k];
            if (q[k] > q[big]) big = k;
        }
        q[big] += 16384 - total;
        for (int k = 0; k < n; k++) mag += q[k] < 0 ? -q[k] : q[k];
        // |v| < 2^31 in the vertical pass needs sum |w| <= 1.35 * 2^14
        if (mag > 22118) {
            set_error("resize %d -> %d: weight magnitude %d exceeds 1.35 * 2^14", src, dst, mag);
            return LUTR_EINVAL;
        }
        (*start)[j] = first;
    }
    *taps = n;
    return LUTR_OK;
}

// What the launch plan needs of one axis table: its taps, and the most source samples an aligned run of 64 (32, 16) outputs reads.
// start is non-decreasing: the first and the last sample of a run decide its footprint.
struct RzAxis {
    int taps;
    int span[3];
};

static RzAxis resize_axis(const std::vector<int> &start, int taps)
{
    RzAxis a{taps, {0, 0, 0}};
    const int m = (int)start.size();
    for (int e = 0; e < 3; e++)
        for (int u0 = 0, len = 64 >> e; u0 < m; u0 += len)
            a.span[e] = std::max(a.span[e], start[std::min(u0 + len, m) - 1] + taps - start[u0]);
    return a;
}

// The launch plan of a resize, from the axis tables of the three planes (x, y) and the planes' output sizes: the
// one place that chooses the footprints, the tile height, the staged rows and the tile counts.  Fills every RzArgs field that is
// not a pointer, a stride or a plane size.
static void resize_plan(const RzAxis ax[3], const RzAxis ay[3], const int pdw[3], const int pdh[3], RzArgs *A)
{
    A->spx = A->nx_max = A->ny_max = 0;
    for (int i = 0; i < 3; i++) {
        A->spx = std::max(A->spx, ax[i].span[0]);
        A->nx_max = std::max(A->nx_max, ax[i].taps);
        A->ny_max = std::max(A->ny_max, ay[i].taps);
    }
    A->spx = (A->spx + 1) & ~1;
    A->rows = 1;
    // the tallest tile whose LDS stays within 40 KiB, so that several workgroups share a CU (64 rows on upscales, 32 for 2:1 and
    // 3:1, 16 for stronger vertical reductions)
    for (A->th = kRzTileHMax; ; A->th /= 2) {
        A->spy = 0;
        for (int i = 0; i < 3; i++) A->spy = std::max(A->spy, ay[i].span[A->th == 64 ? 0 : A->th == 32 ? 1 : 2]);
        if (A->th == 16 || resize_lds_bytes(*A) <= 40960) break;
    }
    // as many staged rows per wave as fit beside the rest of the LDS (the tables and T), at most kRzRows
    A->rows = kRzRows;
    while (A->rows > 1 && resize_lds_bytes(*A) > 65536) A->rows--;
    int tile0 = 0;
    for (int i = 0; i < 3; i++) {
        RzPlane &P = A->p[i];
        P.nx = ax[i].taps; P.ny = ay[i].taps;
        P.tiles_x = (pdw[i] + kRzTileW - 1) / kRzTileW;
        P.tile0 = tile0;
        tile0 += P.tiles_x * ((pdh[i] + A->th - 1) / A->th);
    }
    A->tiles_per_frame = tile0;
}

}  // namespace lutr

using namespace lutr;

struct lutr_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    float4 *lat = nullptr;
    size_t lat_bytes = 0;
    int n = 0;
    float scale[3] = {1.f, 1.f, 1.f};
    int variant = VAR_AUTO;
    std::string last_kernel;
    bool unit = false;               // every lattice node known to lie in [0, 1]
    unsigned *queue = nullptr;       // work-queue words of the tile kernels (device, 4 words: see lutr_ctx_create)
    float *fscratch = nullptr;       // float planes of the dither path
    float *bn_tab = nullptr;         // blue-noise dither: the 64 x 64 offsets d, uploaded on first use and kept
    size_t fscratch_floats = 0;
    unsigned *stats = nullptr;       // 8 device counters (4 reported + clock stamps), see lutr_ctx_tile_stats
    // The queue counter, the dither scratch and the stats block are per context, not per stream: launches of one
    // context must not overlap.  Every launch records `done` on the stream it ran on; binding another stream makes
    // that stream wait for it (lutr_ctx_set_stream), so applies issued from different streams serialise on the GPU.
    hipEvent_t done = nullptr;
    bool pending = false;            // `done` was recorded on `stream` and nothing has waited for it yet
    // fast variant (lutr_ctx_set_precision): fp16 copies of the lattice pre-multiplied by 2^depth - 1, built on first
    // use per depth (index 0: 8 bit, 1: 10 bit) and dropped whenever the lattice changes
    int precision = LUTR_PRECISION_STRICT;
    uint2 *lat16[2] = {nullptr, nullptr};
    // fma32 variant: fp32 copies of the lattice pre-multiplied by 2^depth - 1, per LUT depth (index depth - 8), same life cycle
    float4 *latm[9] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    // lut3d's prelut (lutr_ctx_set_prelut): the host copy, and per LUT depth a device table of the lattice coordinate of every
    // integer code -- the shaper, the scale and the clip folded into one lookup (pre_tab[depth - 8])
    std::vector<float> prelut;
    int pre_size = 0;
    float pre_min[3] = {0, 0, 0}, pre_scale[3] = {0, 0, 0};
    struct PreTable {
        float *dev = nullptr;            // 3 x entries floats, or nullptr: not built yet (everything below is then stale)
        int entries = 0;                 // 256 for 8-bit containers, else 65536
        int shared = 0;                  // the three tables agree and never fall (LutConsts::pre_shared)
        float kappa = 0.0f;              // ... and their largest step between neighbouring codes
        std::vector<float> host;         // ... and the shared table itself, codes 0 .. 2^depth - 1 (LutConsts::pre_host)
        unsigned long long gen = 0;      // the table's number (LutConsts::pre_gen, g_prelut_gen)
    };
    PreTable pre_tab[9];
    // the float path interpolates the prelut per pixel: a device copy of `prelut` as it was given (3 x pre_size
    // floats), uploaded on first use and dropped with the per-depth tables
    float *pre_raw = nullptr;
    // lutr_lut_broadcast: copies other contexts are still reading out of THIS context's lattice (one event per receiver,
    // recorded on the receiver's stream behind its copy).  The lattice must not be overwritten or freed before they finish.
    std::vector<std::pair<int, hipEvent_t>> readers;      // (receiver's device, event)
    // output resize (lutr_resize_planes): Q14 tables per axis geometry, uploaded once and kept
    struct RzTable {
        int src, dst, cs, cosited;
        RzAxis axis;                 // taps, and the most source samples an output tile of 64 (32, 16) samples reads
        int *dev;                    // dst start words, then dst * taps weights (int32)
    };
    std::vector<RzTable> rz_tables;
    // the second lattice of lutr_apply_yuv_chain (lutr_ctx_set_lut2): a buffer of its own in `lat`'s layout; no
    // prelut, no derived copies.  Nothing but that entry point reads it
    float4 *lat2 = nullptr;
    size_t lat2_bytes = 0;
    int n2 = 0;
    float scale2[3] = {1.f, 1.f, 1.f};
    // the ASC CDL's per-code table (lutr_apply_yuv_cdl): 3 x 2^cdl_depth floats on the device, built for the slope,
    // offset and power in cdl_key; cdl_depth 0: nothing valid is there.  Per-clip use replaces it while the previous call's kernel
    // may still read it: see cdl_device_table
    float *cdl_tab = nullptr;
    size_t cdl_cap = 0;              // floats allocated
    int cdl_depth = 0;
    float cdl_key[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    // the 1D LUT of lutr_apply_yuv_lut1d / lutr_apply_planar_rgb_lut1d (lutr_ctx_set_lut1d): the host copy as it
    // was given (3 x l1d_size floats; size 0: none set), and per depth a device table of 3 x 2^depth codes (l1d_tab[depth - 8]),
    // built at first use.  l1d_gen counts the calls of lutr_ctx_set_lut1d; a device table is current when it carries that number
    std::vector<float> l1d;
    int l1d_size = 0;
    float l1d_scale[3] = {1.f, 1.f, 1.f};
    int l1d_interp = LUTR_INTERP1D_LINEAR;
    unsigned long long l1d_gen = 0;
    struct L1dTable {
        uint16_t *dev = nullptr;         // 3 x 2^depth entries, allocated once per depth and kept
        unsigned long long gen = 0;      // the l1d_gen its contents were built from (0: never)
    };
    L1dTable l1d_tab[9];
};

// Wait for every peer copy that reads this context's lattice, then forget the events.
static void wait_readers(lutr_ctx *c)
{
    for (auto &r : c->readers) {
        (void)hipEventSynchronize(r.second);
        (void)hipSetDevice(r.first);
        (void)hipEventDestroy(r.second);
    }
    if (!c->readers.empty()) (void)hipSetDevice(c->device);
    c->readers.clear();
}

// (the fma32 copies too: every caller drops whatever was derived from the lattice)
static void drop_lat16(lutr_ctx *c)
{
    for (auto &p : c->lat16)
        if (p) { (void)hipStreamSynchronize(c->stream); (void)hipFree(p); p = nullptr; }
    for (auto &p : c->latm)
        if (p) { (void)hipStreamSynchronize(c->stream); (void)hipFree(p); p = nullptr; }
}

static void drop_prelut_tables(lutr_ctx *c)
{
    for (auto &t : c->pre_tab)
        if (t.dev) { (void)hipStreamSynchronize(c->stream); (void)hipFree(t.dev); t.dev = nullptr; }
    if (c->pre_raw) { (void)hipStreamSynchronize(c->stream); (void)hipFree(c->pre_raw); c->pre_raw = nullptr; }
}

// The body of the four lutr_yuv_constants* exports; make(YuvConsts *) is only called with p checked.
template <class Make>
static int export_consts(const char *entry, const lutr_yuv_params *p, float *out, Make make)
{
    if (!p || !out) {
        set_error("%s: null argument", entry);
        return LUTR_EINVAL;
    }
    YuvConsts k;
    const int rc = make(&k);
    if (rc) return rc;
    std::memcpy(out, &k, sizeof(k));
    return LUTR_OK;
}

// A copy of the lattice pre-multiplied by 2^depth - 1 in *slot, built on first use by `build` (nullptr: out of memory).
template <class T>
static const T *derived_lattice(lutr_ctx *c, T **slot, int depth,
                                void (*build)(hipStream_t, const float4 *, T *, size_t, float))
{
    if (!*slot) {
        const size_t nodes = c->lat_bytes / sizeof(float4);
        void *p = nullptr;
        if (hipMalloc(&p, nodes * sizeof(T)) != hipSuccess) return nullptr;
        *slot = (T *)p;
        build(c->stream, c->lat, *slot, nodes, (float)((1 << depth) - 1));   // same stream as the apply that follows
    }
    return *slot;
}

extern "C" {

const char *lutr_version(void) { return LUTR_VERSION_STRING; }
const char *lutr_last_error(void) { return g_last_error.c_str(); }

size_t lutr_lattice_bytes(int n)
{
    if (n < 2 || n > 256) return 0;
    const size_t n1 = (size_t)n + 1;
    return n1 * n1 * n1 * sizeof(float4);
}

int lutr_max_waves_knob(const char *text, int waves_per_block, int uncapped)
{
    return capped_waves(text, waves_per_block, uncapped);
}

int lutr_max_blocks_knob(const char *text, int cap)
{
    return cap < 1 ? cap : (int)capped_blocks(text, (unsigned)cap);
}

int lutr_yuv_constants(const lutr_yuv_params *p, float out[32])
{
    return export_consts("lutr_yuv_constants", p, out, [&](YuvConsts *k) { return make_yuv_consts(*p, k); });
}

int lutr_yuv_constants_sited(const lutr_yuv_params *p, int chroma_loc, float out[32])
{
    return export_consts("lutr_yuv_constants_sited", p, out, [&](YuvConsts *k) { return make_yuv_consts_sited(*p, chroma_loc, k); });
}

int lutr_yuv_constants_xsub(const lutr_yuv_params *p, float out[32])
{
    return export_consts("lutr_yuv_constants_xsub", p, out, [&](YuvConsts *k) { return make_yuv_consts_xsub(*p, k); });
}

int lutr_yuv_constants_rgb2yuv(const lutr_yuv_params *p, float out[32])
{
    return export_consts("lutr_yuv_constants_rgb2yuv", p, out, [&](YuvConsts *k) { return make_yuv_consts_rgb2yuv(*p, k); });
}

int lutr_yuv_constants_yuv2rgb(const lutr_yuv_params *p, float out[32])
{
    return export_consts("lutr_yuv_constants_yuv2rgb", p, out, [&](YuvConsts *k) { return make_yuv_consts_yuv2rgb(*p, k); });
}

int lutr_ctx_create(int device, lutr_ctx **out)
{
    if (!out) {
        set_error("lutr_ctx_create: null out pointer");
        return LUTR_EINVAL;
    }
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        set_error("no HIP device available (%s); liblutr has no CPU fallback",
                  e == hipSuccess ? "device count 0" : hipGetErrorString(e));
        return LUTR_EIO;
    }
    if (device < 0 || device >= count) {
        set_error("device %d out of range (have %d)", device, count);
        return LUTR_EINVAL;
    }
    HIP_TRY(hipSetDevice(device));
    lutr_ctx *c = new lutr_ctx();
    c->device = device;
    const char *what = "hipStreamCreateWithFlags";
    e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
    c->stream = c->own_stream;
    // four words: {claims, waves done} of the round-3 tile kernels, which return them to zero themselves at the end of every launch
    // (no memset node per launch), word 2 for round 1's RGB kernel (set by its launcher), one spare
    if (e == hipSuccess) { what = "hipMalloc(queue)"; e = hipMalloc((void **)&c->queue, 4 * sizeof(unsigned)); }
    if (e == hipSuccess) e = hipMemset(c->queue, 0, 4 * sizeof(unsigned));
    if (e == hipSuccess) { what = "hipEventCreateWithFlags"; e = hipEventCreateWithFlags(&c->done, hipEventDisableTiming); }
    if (e != hipSuccess) {
        lutr_ctx_destroy(c);             // it tolerates the members that were never made
        return hip_fail(e, what);
    }
    *out = c;
    return LUTR_OK;
}

void lutr_ctx_destroy(lutr_ctx *c)
{
    if (!c) return;
    wait_readers(c);
    (void)hipSetDevice(c->device);
    drop_lat16(c);
    drop_prelut_tables(c);
    if (c->lat) (void)hipFree(c->lat);
    if (c->lat2) (void)hipFree(c->lat2);
    if (c->stats) (void)hipFree(c->stats);
    if (c->fscratch) (void)hipFree(c->fscratch);
    if (c->bn_tab) (void)hipFree(c->bn_tab);
    if (c->cdl_tab) (void)hipFree(c->cdl_tab);
    for (auto &t : c->l1d_tab)
        if (t.dev) (void)hipFree(t.dev);
    for (auto &t : c->rz_tables) (void)hipFree(t.dev);
    if (c->queue) (void)hipFree(c->queue);
    if (c->done) (void)hipEventDestroy(c->done);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

int lutr_ctx_set_stream(lutr_ctx *c, void *hip_stream)
{
    if (!c) { set_error("null context"); return LUTR_EINVAL; }
    hipStream_t next = (hipStream_t)hip_stream;   // NULL is HIP's default (null) stream, e.g. torch's default
    if (next != c->stream && c->pending) {
        // work of this context may still be running on the old stream, and it owns the context's queue counter and
        // scratch: the new stream starts behind it
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipStreamWaitEvent(next, c->done, 0));
    }
    c->stream = next;
    return LUTR_OK;
}

int lutr_ctx_sync(lutr_ctx *c)
{
    if (!c) { set_error("null context"); return LUTR_EINVAL; }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return LUTR_OK;
}

int lutr_ctx_set_precision(lutr_ctx *c, int precision)
{
    if (!c || (precision != LUTR_PRECISION_STRICT && precision != LUTR_PRECISION_FAST && precision != LUTR_PRECISION_FMA32)) {
        set_error("bad precision %d", precision);
        return LUTR_EINVAL;
    }
    c->precision = precision;
    return LUTR_OK;
}

int lutr_ctx_set_variant(lutr_ctx *c, int variant)
{
    if (!c || variant < VAR_AUTO || variant > VAR_VEC_LDS) {
        set_error("bad variant %d", variant);
        return LUTR_EINVAL;
    }
    c->variant = variant;
    return LUTR_OK;
}

const char *lutr_ctx_last_kernel(lutr_ctx *c) { return c ? c->last_kernel.c_str() : ""; }

int lutr_ctx_tile_stats(lutr_ctx *c, int enable, uint64_t out[8])
{
    if (!c) { set_error("null context"); return LUTR_EINVAL; }
    HIP_TRY(hipSetDevice(c->device));
    if (out) {
        for (int i = 0; i < 8; i++) out[i] = 0;
        if (c->stats) {
            unsigned h[32];
            HIP_TRY(hipStreamSynchronize(c->stream));
            HIP_TRY(hipMemcpy(h, c->stats, sizeof(h), hipMemcpyDeviceToHost));
            for (int i = 0; i < 4; i++) out[i] = h[i];
            out[4] = h[30];                                         // mixed tiles: tube body + gather body for the few lanes outside the tube
            out[5] = 0;
            out[6] = h[12];                                         // tiles served by the workgroup's grey tube
            out[7] = h[6];                                          // tiles that needed the second-level (exact) window test
            if (getenv("LUTR_DEBUG"))
            {
                fprintf(stderr, "[lutr stats raw] %u %u %u %u | %u %u %u | %u %u %u | %u %u |", h[0], h[1], h[2], h[3], h[4], h[5], h[6],
                        h[7], h[8], h[9], h[10], h[11]);
                for (int i = 12; i < 32; i++) fprintf(stderr, " %u", h[i]);
                fprintf(stderr, "\n");
            }
        }
    }
    if (enable && !c->stats) {
        HIP_TRY(hipMalloc((void **)&c->stats, 32 * sizeof(unsigned)));
    } else if (!enable && c->stats) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        (void)hipFree(c->stats);
        c->stats = nullptr;
    }
    if (c->stats) HIP_TRY(hipMemset(c->stats, 0, 32 * sizeof(unsigned)));
    return LUTR_OK;
}

static int alloc_lattice(lutr_ctx *c, int n, const float scale[3])
{
    if (!c || !scale) { set_error("null argument"); return LUTR_EINVAL; }
    if (n < 2 || n > 256) {
        set_error("too large or invalid 3D LUT size %d", n);
        return LUTR_EINVAL;
    }
    for (int i = 0; i < 3; i++)
        if (!(scale[i] >= 0.f && scale[i] <= 1.f)) {
            set_error("scale[%d] = %g outside [0,1]", i, (double)scale[i]);
            return LUTR_EINVAL;
        }
    HIP_TRY(hipSetDevice(c->device));
    wait_readers(c);                 // peers of an earlier lutr_lut_broadcast may still be copying out of the buffer
    drop_lat16(c);                   // they describe the previous lattice
    drop_prelut_tables(c);           // and so does a prelut: it belongs to the LUT file (set it again after the lattice)
    c->prelut.clear(); c->pre_size = 0;
    const size_t bytes = lutr_lattice_bytes(n);
    if (bytes != c->lat_bytes) {
        if (c->lat) { HIP_TRY(hipStreamSynchronize(c->stream)); (void)hipFree(c->lat); c->lat = nullptr; c->lat_bytes = 0; }
        void *p = nullptr;
        hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) { set_error("hipMalloc(%zu): %s", bytes, hipGetErrorString(e)); return LUTR_ENOMEM; }
        c->lat = (float4 *)p;
        c->lat_bytes = bytes;
    }
    c->n = n;
    c->unit = false;                 // unknown until the nodes are seen (lutr_ctx_set_lut / lutr_ctx_lut_seal)
    std::memcpy(c->scale, scale, sizeof(c->scale));
    return LUTR_OK;
}

int lutr_ctx_lut_alloc(lutr_ctx *c, int n, const float scale[3]) { return alloc_lattice(c, n, scale); }

// the nodes of a host lattice are finite (*unit: and all inside [0, 1]); nothing is looked at for a size alloc_lattice refuses
static int scan_lattice(const float *rgb, int n, bool *unit)
{
    const size_t count = (size_t)(n > 0 ? n : 0) * n * n * 3;
    *unit = true;
    for (size_t i = 0; i < count && n >= 2 && n <= 256; i++) {
        if (!std::isfinite(rgb[i])) {
            set_error("non-finite lattice value at float %zu", i);
            return LUTR_EINVAL;
        }
        *unit = *unit && rgb[i] >= 0.0f && rgb[i] <= 1.0f;
    }
    return LUTR_OK;
}

// pack [r][g][b][3] -> (n+1)^3 float4 with the last node replicated on each axis
static std::vector<float4> pack_lattice(const float *rgb, int n)
{
    const int n1 = n + 1;
    std::vector<float4> host((size_t)n1 * n1 * n1);
    for (int r = 0; r < n1; r++) {
        const int rr = r < n ? r : n - 1;
        for (int g = 0; g < n1; g++) {
            const int gg = g < n ? g : n - 1;
            for (int b = 0; b < n1; b++) {
                const int bb = b < n ? b : n - 1;
                const float *s = &rgb[(((size_t)rr * n + gg) * n + bb) * 3];
                host[((size_t)r * n1 + g) * n1 + b] = make_float4(s[0], s[1], s[2], 0.f);
            }
        }
    }
    return host;
}

int lutr_ctx_set_lut(lutr_ctx *c, const float *rgb, int n, const float scale[3])
{
    if (!rgb) { set_error("null lattice"); return LUTR_EINVAL; }
    bool unit;
    if (const int rc = scan_lattice(rgb, n, &unit)) return rc;
    const int rc = alloc_lattice(c, n, scale);
    if (rc) return rc;
    const std::vector<float4> host = pack_lattice(rgb, n);
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(c->lat, host.data(), c->lat_bytes, hipMemcpyHostToDevice));
    c->unit = unit;
    return LUTR_OK;
}

int lutr_ctx_set_lut2(lutr_ctx *c, const float *rgb, int n, const float scale[3])
{
    if (!c) { set_error("null context"); return LUTR_EINVAL; }
    if (!rgb || n == 0) {                // remove the second lattice
        HIP_TRY(hipSetDevice(c->device));
        if (c->lat2) { HIP_TRY(hipStreamSynchronize(c->stream)); (void)hipFree(c->lat2); }
        c->lat2 = nullptr; c->lat2_bytes = 0; c->n2 = 0;
        return LUTR_OK;
    }
    if (!scale) { set_error("null argument"); return LUTR_EINVAL; }
    if (n < 2 || n > 256) {
        set_error("too large or invalid 3D LUT size %d", n);
        return LUTR_EINVAL;
    }
    for (int i = 0; i < 3; i++)
        if (!(scale[i] >= 0.f && scale[i] <= 1.f)) {
            set_error("scale[%d] = %g outside [0,1]", i, (double)scale[i]);
            return LUTR_EINVAL;
        }
    bool unit;
    if (const int rc = scan_lattice(rgb, n, &unit)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const size_t bytes = lutr_lattice_bytes(n);
    HIP_TRY(hipStreamSynchronize(c->stream));        // a chain launch may still be reading the old nodes
    if (bytes != c->lat2_bytes) {
        if (c->lat2) { (void)hipFree(c->lat2); c->lat2 = nullptr; c->lat2_bytes = 0; c->n2 = 0; }
        void *p = nullptr;
        hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) { set_error("hipMalloc(%zu): %s", bytes, hipGetErrorString(e)); return LUTR_ENOMEM; }
        c->lat2 = (float4 *)p;
        c->lat2_bytes = bytes;
    }
    const std::vector<float4> host = pack_lattice(rgb, n);
    HIP_TRY(hipMemcpy(c->lat2, host.data(), bytes, hipMemcpyHostToDevice));
    c->n2 = n;
    std::memcpy(c->scale2, scale, sizeof(c->scale2));
    return LUTR_OK;
}

int lutr_ctx_set_prelut(lutr_ctx *c, const float *prelut, int size, const float vmin[3], const float vscale[3])
{
    if (!c) { set_error("null context"); return LUTR_EINVAL; }
    HIP_TRY(hipSetDevice(c->device));
    drop_prelut_tables(c);
    c->prelut.clear(); c->pre_size = 0;
    if (!prelut || size == 0) return LUTR_OK;
    if (size < 2 || size > 65536 || !vmin || !vscale) { set_error("prelut size %d outside [2, 65536] or null ranges", size); return LUTR_EINVAL; }
    for (size_t i = 0; i < (size_t)3 * size; i++)
        if (!std::isfinite(prelut[i])) { set_error("non-finite prelut value at float %zu", i); return LUTR_EINVAL; }
    for (int i = 0; i < 3; i++)
        if (!std::isfinite(vmin[i]) || !std::isfinite(vscale[i])) { set_error("non-finite prelut range"); return LUTR_EINVAL; }
    c->prelut.assign(prelut, prelut + (size_t)3 * size);
    c->pre_size = size;
    std::memcpy(c->pre_min, vmin, sizeof(c->pre_min));
    std::memcpy(c->pre_scale, vscale, sizeof(c->pre_scale));
    return LUTR_OK;
}

// The lattice coordinate of every integer code at this LUT depth with the prelut in front: FFmpeg's
// prelut_interp_1d_linear on code * (1 / M), then * scale * (n - 1), clipped to [0, n - 1] -- per pixel in FFmpeg, per code here,
// float for float the same operations (this file is compiled without contraction).  256 entries for 8-bit containers, else 65536.
// Every table prelut_table builds gets a number of its own from this counter (never 0).  The tile launcher memoises the tube bound
// it reads off a shared table under that number: a rebuilt table reuses the vector of the old one, and a new context may be handed
// a freed one's memory, so the address says nothing about the contents.
static std::atomic<unsigned long long> g_prelut_gen{0};

// *out: the table of `depth`, built on first use; an empty one (dev == nullptr) when the context has no prelut.
static int prelut_table(lutr_ctx *c, int depth, const lutr_ctx::PreTable **out)
{
    static const lutr_ctx::PreTable none;
    *out = &none;
    if (!c->pre_size) return LUTR_OK;
    const int slot = depth - 8;
    if (slot < 0 || slot > 8) { set_error("prelut: LUT depth %d outside 8..16", depth); return LUTR_EINVAL; }
    lutr_ctx::PreTable &t = c->pre_tab[slot];
    *out = &t;
    if (t.dev) return LUTR_OK;
    const int ne = depth <= 8 ? 256 : 65536;
    const int maxi = (1 << depth) - 1, pmax = c->pre_size - 1;
    const float scale_f = 1.0f / (float)maxi, lut_max = (float)(c->n - 1);
    std::vector<float> host((size_t)3 * ne);
    for (int ch = 0; ch < 3; ch++) {
        const float sc = c->scale[ch] * lut_max;
        const float *tab = &c->prelut[(size_t)ch * c->pre_size];
        for (int code = 0; code < ne; code++) {
            const float s = (float)code * scale_f;
            const float scaled = (s - c->pre_min[ch]) * c->pre_scale[ch];
            const float x = scaled < 0.0f ? 0.0f : (scaled > (float)pmax ? (float)pmax : scaled);
            const int prev = (int)x, next = (prev + 1) < pmax ? prev + 1 : pmax;
            const float p = tab[prev], nn = tab[next], d = x - (float)prev;
            const float v = p + (nn - p) * d;
            const float t = v * sc;
            host[(size_t)ch * ne + code] = t < 0.0f ? 0.0f : (t > lut_max ? lut_max : t);
        }
    }
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, host.size() * sizeof(float));
    if (e != hipSuccess) { set_error("hipMalloc(prelut table): %s", hipGetErrorString(e)); return LUTR_ENOMEM; }
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(p, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
    t.dev = (float *)p;
    t.entries = ne;
    // one table for the three channels?  (what the fused YUV tile kernels can take: their coordinate table is indexed by code alone,
    // and their validity bounds want a monotone map with a known largest slope)
    bool same = true;
    float step = 0.0f;
    for (int code = 0; code <= maxi && same; code++) {
        const float v = host[code];
        same = host[(size_t)ne + code] == v && host[(size_t)2 * ne + code] == v;
        if (code) { const float d = v - host[code - 1]; if (d < 0.0f) same = false; else if (d > step) step = d; }
    }
    t.shared = same ? 1 : 0;
    t.kappa = same ? step : 0.0f;
    t.host.clear();
    if (same) t.host.assign(host.begin(), host.begin() + maxi + 1);
    t.gen = ++g_prelut_gen;
    return LUTR_OK;
}

int lutr_ctx_lut_seal(lutr_ctx *c)
{
    if (!c) { set_error("null argument"); return LUTR_EINVAL; }
    if (!c->lat) { set_error("no lattice set on this context"); return LUTR_EINVAL; }
    HIP_TRY(hipSetDevice(c->device));
    std::vector<float4> host(c->lat_bytes / sizeof(float4));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(host.data(), c->lat, c->lat_bytes, hipMemcpyDeviceToHost));
    bool unit = true;
    for (size_t i = 0; i < host.size(); i++) {
        const float v[3] = {host[i].x, host[i].y, host[i].z};
        for (int k = 0; k < 3; k++) {
            if (!std::isfinite(v[k])) {
                c->unit = false;
                set_error("non-finite lattice value at node %zu", i);
                return LUTR_EINVAL;
            }
            unit = unit && v[k] >= 0.0f && v[k] <= 1.0f;
        }
    }
    drop_lat16(c);
    c->unit = unit;
    return LUTR_OK;
}

int lutr_lut_broadcast(lutr_ctx **ctxs, int nctx, int root) { return lutr_lut_broadcast_ex(ctxs, nctx, root, 0); }

int lutr_lut_broadcast_ex(lutr_ctx **ctxs, int nctx, int root, unsigned flags)
{
    if (!ctxs || nctx < 1 || root < 0 || root >= nctx || (flags & ~(unsigned)LUTR_BCAST_FORCE_PEER_COPY)) {
        set_error("lutr_lut_broadcast: bad arguments");
        return LUTR_EINVAL;
    }
    for (int i = 0; i < nctx; i++)
        if (!ctxs[i]) { set_error("lutr_lut_broadcast: null context %d", i); return LUTR_EINVAL; }
    lutr_ctx *r = ctxs[root];
    if (!r->lat) { set_error("the root context holds no lattice"); return LUTR_EINVAL; }
    // the root's upload (a blocking copy) has landed; order the peers' copies behind whatever the root's stream still runs
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(hipEventRecord(r->done, r->stream));
    r->pending = true;
    for (int i = 0; i < nctx; i++) {
        lutr_ctx *c = ctxs[i];
        if (c == r) continue;
        int rc = alloc_lattice(c, r->n, r->scale);        // selects c's device
        if (rc) return rc;
        HIP_TRY(hipStreamWaitEvent(c->stream, r->done, 0));
        // (LUTR_BCAST_FORCE_PEER_COPY: the cross-device call on a same-device pair -- a self-peer copy is legal -- so that a
        // one-GPU box executes the branch an 8-GPU node takes)
        if (c->device == r->device && !(flags & LUTR_BCAST_FORCE_PEER_COPY))
            HIP_TRY(hipMemcpyAsync(c->lat, r->lat, r->lat_bytes, hipMemcpyDeviceToDevice, c->stream));
        else
            HIP_TRY(hipMemcpyPeerAsync(c->lat, c->device, r->lat, r->device, r->lat_bytes, c->stream));   // xGMI, GPU to GPU
        c->unit = r->unit;           // same nodes: the root's scan of the value range holds for the copy
        // later applies of the receiver are ordered behind its copy even if it is rebound to another stream first
        HIP_TRY(hipEventRecord(c->done, c->stream));
        c->pending = true;
        // ... and the root must not overwrite or free the buffer while this copy reads it
        hipEvent_t ev = nullptr;
        HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(ev, c->stream));
        r->readers.emplace_back(c->device, ev);
    }
    HIP_TRY(hipSetDevice(r->device));
    return LUTR_OK;
}

int lutr_ctx_lut_device(lutr_ctx *c, void **dptr, size_t *bytes)
{
    if (!c || !dptr || !bytes) { set_error("null argument"); return LUTR_EINVAL; }
    if (!c->lat) { set_error("no lattice set on this context"); return LUTR_EINVAL; }
    *dptr = c->lat;
    *bytes = c->lat_bytes;
    return LUTR_OK;
}

static int check_geometry(int w, int h, int nframes, int row0, int rows)
{
    if (w < 0 || h < 0 || nframes < 0 || row0 < 0 || rows < 0 || row0 + rows > h) {
        set_error("bad geometry w=%d h=%d nframes=%d row0=%d rows=%d", w, h, nframes, row0, rows);
        return LUTR_EINVAL;
    }
    return LUTR_OK;
}

// min_interp: the lowest legal mode -- LUTR_INTERP_NEAREST, or LUTR_INTERP_NONE where the entry point can leave lut3d out
// (no lattice is needed for that mode then)
static int check_common(lutr_ctx *c, int interp, int min_interp, int w, int h, int nframes, const void *src, const void *dst,
                        int row0, int rows)
{
    if (!c || !src || !dst) { set_error("null argument"); return LUTR_EINVAL; }
    if (!c->lat && (interp != LUTR_INTERP_NONE || min_interp > LUTR_INTERP_NONE)) {
        set_error("no lattice set on this context (call lutr_ctx_set_lut first)");
        return LUTR_EINVAL;
    }
    if (interp < min_interp || interp > LUTR_INTERP_PRISM) {
        set_error("unknown interpolation mode %d", interp);
        return LUTR_EINVAL;
    }
    return check_geometry(w, h, nframes, row0, rows);
}

// every plane of a (and of b, when given) has a base pointer
static int check_planes_set(const lutr_planes *a, const lutr_planes *b)
{
    for (int i = 0; i < 3; i++)
        if (!a->data[i] || (b && !b->data[i])) { set_error("null plane %d", i); return LUTR_EINVAL; }
    return LUTR_OK;
}

// a row range made of whole chroma blocks of height bh (the frame's last block may be cut); `noun` names the block in the message
static int check_row_blocks(int row0, int rows, int h, int bh, const char *noun)
{
    if (row0 % bh || (rows % bh && row0 + rows != h)) {
        set_error("row0/rows must be multiples of the %s %d", noun, bh);
        return LUTR_EINVAL;
    }
    return LUTR_OK;
}

static int check_dither(int dither)
{
    if (dither != LUTR_DITHER_NONE && dither != LUTR_DITHER_ERROR_DIFFUSION && dither != LUTR_DITHER_BLUE_NOISE) {
        set_error("unknown dither mode %d", dither);
        return LUTR_EINVAL;
    }
    return LUTR_OK;
}

static int check_dither_rows(int dither, int row0, int rows, int h)
{
    if (dither == LUTR_DITHER_ERROR_DIFFUSION && (row0 != 0 || rows != h)) {
        set_error("error-diffusion dither couples the rows of a frame: whole frames only (row0 = 0, rows = h)");
        return LUTR_EINVAL;
    }
    return LUTR_OK;
}

struct PackedFmt { int bits, nc, ro, go, bo; };

static int decode_packed(int pfmt, PackedFmt *f)
{
    *f = PackedFmt{LUTR_PACKED_BITS(pfmt), LUTR_PACKED_NCOMP(pfmt), LUTR_PACKED_RO(pfmt), LUTR_PACKED_GO(pfmt), LUTR_PACKED_BO(pfmt)};
    if ((f->bits != 8 && f->bits != 16) || (f->nc != 3 && f->nc != 4) || (pfmt >> 24) || f->ro >= f->nc || f->go >= f->nc ||
        f->bo >= f->nc || f->ro == f->go || f->go == f->bo || f->ro == f->bo) {
        set_error("unsupported packed format 0x%x", pfmt);
        return LUTR_EINVAL;
    }
    return LUTR_OK;
}

// Samples of a chroma plane along an axis of n luma samples at log2 subsampling cs.
static int chroma_dim(int n, int cs) { return (n + (1 << cs) - 1) >> cs; }

// True when a base pointer, its row stride and (batches) its frame stride have none of `mask`'s bits set.
static bool check_aligned(const void *ptr, long long stride, long long frame_stride, int nframes, unsigned mask)
{
    return !(((uintptr_t)ptr | (uintptr_t)stride | (nframes > 1 ? (uintptr_t)frame_stride : 0)) & mask);
}

// The source (src = true) or destination side of P has planes [0, k) only: slots [k, 3) are cleared.
static void clear_planes(PlaneSet *P, bool src, int k)
{
    for (int i = k; i < 3; i++) {
        if (src) { P->s[i] = nullptr; P->ss[i] = 0; P->sfs[i] = 0; }
        else { P->d[i] = nullptr; P->ds[i] = 0; P->dfs[i] = 0; }
    }
}

static void fill_planes(PlaneSet *P, const lutr_planes *src, const lutr_planes *dst)
{
    for (int i = 0; i < 3; i++) {
        P->s[i] = (const uint8_t *)src->data[i];
        P->d[i] = (uint8_t *)dst->data[i];
        P->ss[i] = src->stride[i];
        P->ds[i] = dst->stride[i];
        P->sfs[i] = src->frame_stride[i];
        P->dfs[i] = dst->frame_stride[i];
    }
}

// The fast variant's lattice for `depth`, or nullptr when fast does not apply: strict precision selected, a depth
// other than 8 / 10 (the tolerance is only defined there), or a lattice outside [0, 1] (the fast kernels are clip-free).
static const uint2 *fast_lattice(lutr_ctx *c, int depth)
{
    if (c->precision != LUTR_PRECISION_FAST || !c->unit || (depth != 8 && depth != 10)) return nullptr;
    return derived_lattice(c, &c->lat16[depth == 8 ? 0 : 1], depth, launch_make_lat16);
}

// The fma32 variant's lattice for `depth`, or nullptr when fma32 does not apply: another precision selected, or a lattice
// outside [0, 1] (the fma32 kernels are clip-free).  No depth limit of its own -- the <= 1 code bound holds at every depth
// (DESIGN.md 3.5); the tile kernels take it at the depths their coordinate table serves (8 to 10).
static const float4 *fma32_lattice(lutr_ctx *c, int depth)
{
    if (c->precision != LUTR_PRECISION_FMA32 || !c->unit || depth < 8 || depth > 16) return nullptr;
    return derived_lattice(c, &c->latm[depth - 8], depth, launch_make_latm);
}

// the lattice side of LutConsts (everything but the prelut's per-code table).  Every entry but lutr_apply_yuv is always strict:
// the fast / fma32 lattices are left unset here and in fill_lut, and no kernel of the other paths reads them
static void fill_lattice(LutConsts *L, lutr_ctx *c, int depth)
{
    const int maxi = (1 << depth) - 1;
    L->lat = c->lat;
    L->lat16 = nullptr;
    L->latm = nullptr;
    L->n1 = c->n + 1;
    L->maxf = (float)maxi;
    L->unit = c->unit ? 1 : 0;
    L->scale_f = 1.0f / (float)maxi;
    L->lut_max = (float)(c->n - 1);
    for (int i = 0; i < 3; i++) L->sc[i] = c->scale[i] * L->lut_max;
}

static int fill_lut(LutConsts *L, lutr_ctx *c, int depth)
{
    const lutr_ctx::PreTable *t;
    if (const int rc = prelut_table(c, depth, &t)) return rc;
    L->pre = t->dev;
    L->pre_stride = t->entries;
    L->pre_shared = t->shared;
    L->pre_kappa = t->kappa;
    L->pre_host = t->shared ? t->host.data() : nullptr;
    L->pre_gen = t->gen;
    fill_lattice(L, c, depth);
    return LUTR_OK;
}

// The second lattice (lutr_ctx_set_lut2) at `depth`: its own size and scale, no prelut (pre stays null), never the clip-free path
static LutConsts second_lattice(const lutr_ctx *c, int depth)
{
    LutConsts L{};
    const int maxi = (1 << depth) - 1;
    L.lat = c->lat2;
    L.n1 = c->n2 + 1;
    L.maxf = (float)maxi;
    L.scale_f = 1.0f / (float)maxi;
    L.lut_max = (float)(c->n2 - 1);
    for (int i = 0; i < 3; i++) L.sc[i] = c->scale2[i] * L.lut_max;
    return L;
}

// The float path's constants: the lattice (at depth 16, which only sets fields these kernels do not read) and the prelut as the
// raw table, uploaded on first use.  lut = false (LUTR_INTERP_NONE): neither is read.
static int fill_lut_float(LutConsts *L, FloatPre *Q, lutr_ctx *c, bool lut)
{
    *L = LutConsts{};
    *Q = FloatPre{};
    if (!lut) return LUTR_OK;
    fill_lattice(L, c, 16);
    if (!c->pre_size) return LUTR_OK;
    if (!c->pre_raw) {
        void *p = nullptr;
        hipError_t e = hipMalloc(&p, c->prelut.size() * sizeof(float));
        if (e != hipSuccess) { set_error("hipMalloc(prelut): %s", hipGetErrorString(e)); return LUTR_ENOMEM; }
        e = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) e = hipMemcpy(p, c->prelut.data(), c->prelut.size() * sizeof(float), hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(p); return hip_fail(e, "prelut upload"); }
        c->pre_raw = (float *)p;
    }
    Q->tab = c->pre_raw;
    Q->size = c->pre_size;
    for (int i = 0; i < 3; i++) { Q->min[i] = c->pre_min[i]; Q->scale[i] = c->pre_scale[i]; }
    return LUTR_OK;
}

static int finish_launch(lutr_ctx *c, const char *name)
{
    if (!name) {
        set_error("the requested kernel variant cannot take this layout (alignment, width multiple, depth mix or mode)");
        return LUTR_EINVAL;
    }
    c->last_kernel = name;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, name);
    HIP_TRY(hipEventRecord(c->done, c->stream));
    c->pending = true;
    return LUTR_OK;
}

int lutr_apply_planar_rgb(lutr_ctx *c, int depth, int interp, int w, int h, int nframes,
                          const lutr_planes *src, const lutr_planes *dst, int row0, int rows)
{
    int rc = check_common(c, interp, LUTR_INTERP_NEAREST, w, h, nframes, src, dst, row0, rows);
    if (rc) return rc;
    if (depth < 8 || depth > 16) { set_error("unsupported depth %d", depth); return LUTR_EINVAL; }
    if (w == 0 || rows == 0 || nframes == 0) return LUTR_OK;
    if (const int rc = check_planes_set(src, dst)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    LutConsts L; PlaneSet P; FrameGeom G{w, h, row0, rows, nframes};
    if (const int rc = fill_lut(&L, c, depth)) return rc;
    fill_planes(&P, src, dst);
    return finish_launch(c, launch_rgb(c->stream, c->variant, L, P, G, depth, interp, c->stats, c->queue));
}

int lutr_apply_packed_rgb(lutr_ctx *c, int pfmt, int interp, int w, int h, int nframes,
                          const lutr_packed *src, const lutr_packed *dst, int row0, int rows)
{
    int rc = check_common(c, interp, LUTR_INTERP_NEAREST, w, h, nframes, src, dst, row0, rows);
    if (rc) return rc;
    PackedFmt f;
    if (const int rc = decode_packed(pfmt, &f)) return rc;
    if (w == 0 || rows == 0 || nframes == 0) return LUTR_OK;
    if (!src->data || !dst->data) { set_error("null image"); return LUTR_EINVAL; }
    const int wide = f.bits == 16;
    if (wide && !(check_aligned(src->data, src->stride, src->frame_stride, nframes, 1) &&
                  check_aligned(dst->data, dst->stride, dst->frame_stride, nframes, 1))) {
        set_error("16-bit packed formats need 2-byte aligned rows");
        return LUTR_EINVAL;
    }
    HIP_TRY(hipSetDevice(c->device));
    LutConsts L; FrameGeom G{w, h, row0, rows, nframes};
    if (const int rc = fill_lut(&L, c, f.bits)) return rc;
    PackedSet P;
    P.s = (const uint8_t *)src->data; P.d = (uint8_t *)dst->data;
    P.ss = src->stride; P.ds = dst->stride;
    P.sfs = src->frame_stride; P.dfs = dst->frame_stride;
    P.ro = f.ro; P.go = f.go; P.bo = f.bo; P.ao = f.nc == 4 ? 6 - f.ro - f.go - f.bo : 3;
    return finish_launch(c, launch_packed(c->stream, c->variant, L, P, G, wide, f.nc, interp, c->stats, c->queue));
}

int lutr_apply_yuv(lutr_ctx *c, const lutr_yuv_params *p, int interp, int w, int h, int nframes,
                   const lutr_planes *src, const lutr_planes *dst, int row0, int rows)
{
    int rc = check_common(c, interp, LUTR_INTERP_NEAREST, w, h, nframes, src, dst, row0, rows);
    if (rc) return rc;
    if (!p) { set_error("null yuv params"); return LUTR_EINVAL; }
    YuvConsts K;
    rc = make_yuv_consts(*p, &K);
    if (rc) return rc;
    const int csx = LUTR_FMT_CSX(p->fmt_in), csy = LUTR_FMT_CSY(p->fmt_in);
    const int bh = 1 << csy;
    if (const int rc = check_row_blocks(row0, rows, h, bh, "chroma block height")) return rc;
    if (w == 0 || rows == 0 || nframes == 0) return LUTR_OK;
    if (const int rc = check_planes_set(src, dst)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    LutConsts L; PlaneSet P; FrameGeom G{w, h, row0, rows, nframes};
    if (const int rc = fill_lut(&L, c, p->lut_depth)) return rc;
    L.lat16 = fast_lattice(c, p->lut_depth);
    L.latm = fma32_lattice(c, p->lut_depth);
    fill_planes(&P, src, dst);
    return finish_launch(c, launch_yuv(c->stream, c->variant, L, K, P, G, LUTR_FMT_DEPTH(p->fmt_in),
                                       LUTR_FMT_DEPTH(p->fmt_out), p->lut_depth, csx, csy, interp, L.lat16 != nullptr,
                                       c->stats, c->queue));
}

// Byte range [lo, hi) that `rows` rows of `row_bytes` bytes span in each of `nframes` frames.
struct Span { uintptr_t lo, hi; };

static Span plane_span(const void *p, long long stride, long long fstride, int rows, long long row_bytes, int nframes)
{
    const long long r = (long long)(rows - 1) * stride, f = nframes > 1 ? (long long)(nframes - 1) * fstride : 0;
    const long long a = (r < 0 ? r : 0) + (f < 0 ? f : 0), b = (r > 0 ? r : 0) + (f > 0 ? f : 0) + row_bytes;
    return Span{(uintptr_t)p + (intptr_t)a, (uintptr_t)p + (intptr_t)b};
}

// The three spans of a planar side: w x h samples of luma, chroma planes subsampled by 2^csx x 2^csy.
static void planar_spans(const lutr_planes *pl, int csx, int csy, int w, int h, int bytes_per_sample, int nframes, Span out[3])
{
    for (int i = 0; i < 3; i++)
        out[i] = plane_span(pl->data[i], pl->stride[i], pl->frame_stride[i], i ? chroma_dim(h, csy) : h,
                            (long long)(i ? chroma_dim(w, csx) : w) * bytes_per_sample, nframes);
}

// No source span may overlap a destination span: `what` cannot run in place.  name_src: the message names the source plane.
static int check_disjoint(const char *what, bool name_src, const Span *s, int ns, const Span *d, int nd)
{
    for (int i = 0; i < ns; i++)
        for (int j = 0; j < nd; j++)
            if (s[i].lo < d[j].hi && d[j].lo < s[i].hi) {
                char src[32] = "the source";
                if (name_src) std::snprintf(src, sizeof(src), "source plane %d", i);
                set_error("%s cannot run in place: the byte range of %s overlaps that of destination plane %d (bounding ranges over all rows and frames must be disjoint)", what, src, j);
                return LUTR_EINVAL;
            }
    return LUTR_OK;
}

// One side of a call: the name the messages give it, its planes, and the depth and chroma layout of its format code (depth 32:
// the float samples of gbrpf32).
// packed: the side is one plane (a packed 4:2:2 or v210 container) of packed_row bytes a row, not three planes.
// semi: the side is two planes, luma and one plane of chroma pairs (2 * ceil(w / 2) samples a row); plane 2 is absent.
struct Side { const char *name; const lutr_planes *pl; int depth, csx, csy; bool packed; long long packed_row; bool semi = false; };

static Side planar_side(const char *name, const lutr_planes *pl, int fmt)
{
    return Side{name, pl, LUTR_FMT_DEPTH(fmt), LUTR_FMT_CSX(fmt), LUTR_FMT_CSY(fmt), false, 0};
}

// Samples above 8 bit are 16-bit words: the base pointer, row stride and frame stride of plane i are even.  `held` is what holds
// them in the entry's message ("planes" | "containers"); this is the only place that message is formatted.
static int check_plane_aligned(const Side &s, int i, int nframes, const char *held)
{
    if (s.depth > 8 && !check_aligned(s.pl->data[i], s.pl->stride[i], s.pl->frame_stride[i], nframes, 1)) {
        set_error("%s plane %d: 16-bit %s need 2-byte aligned rows", s.name, i, held);
        return LUTR_EINVAL;
    }
    return LUTR_OK;
}

// ... for the three planes of each of n sides, in the order given
static int check_sides_aligned(const Side *sides, int n, int nframes)
{
    for (int k = 0; k < n; k++)
        for (int i = 0; i < 3; i++)
            if (const int rc = check_plane_aligned(sides[k], i, nframes, "planes")) return rc;
    return LUTR_OK;
}

// the byte ranges of a side's planes over all rows and frames, and their number
static int side_spans(const Side &s, const FrameGeom &G, Span out[3])
{
    if (s.packed) {
        out[0] = plane_span(s.pl->data[0], s.pl->stride[0], s.pl->frame_stride[0], G.h, s.packed_row, G.nframes);
        return 1;
    }
    planar_spans(s.pl, s.csx, s.csy, G.w, G.h, s.depth > 16 ? 4 : s.depth > 8 ? 2 : 1, G.nframes, out);
    if (s.semi) {
        out[1] = plane_span(s.pl->data[1], s.pl->stride[1], s.pl->frame_stride[1], chroma_dim(G.h, s.csy),
                            2ll * chroma_dim(G.w, 1) * (s.depth > 8 ? 2 : 1), G.nframes);
        return 2;
    }
    return 3;
}

// check_disjoint between the planes of two sides
static int check_sides_disjoint(const char *what, bool name_src, const Side &a, const Side &b, const FrameGeom &G)
{
    Span as[3], bs[3];
    const int na = side_spans(a, G, as), nb = side_spans(b, G, bs);
    return check_disjoint(what, name_src, as, na, bs, nb);
}

// In place means the same container on both sides (`same`: the entry's word on that) and the same bytes; anything else must not
// overlap at all.
static int check_in_place(const char *what, bool same, const Side &s, const Side &d, const FrameGeom &G)
{
    if (same && s.pl->data[0] == d.pl->data[0] && s.pl->stride[0] == d.pl->stride[0] &&
        (G.nframes <= 1 || s.pl->frame_stride[0] == d.pl->frame_stride[0])) return LUTR_OK;
    return check_sides_disjoint(what, true, s, d, G);
}

// ---- what the host entries of the union-block kernels share (lutr_apply_yuv_xsub's pass with something added to it: DESIGN.md
// 3.13, 3.17 - 3.23).  An entry runs its own refusals, then union_open, then whatever its family refuses on the formats, then
// union_rules, the empty call, union_planes_ready and the overlap check under its own noun.
struct UnionCall {
    YuvConsts K;           // make_yuv_consts_xsub's block for side[1]
    Side side[3];          // source, destination, and lutr_apply_yuv_dual's second destination
    int nsides;
    int lut_depth;
};

// First half: the constants, then the layouts and depths of the two sides.
static int union_open(const lutr_yuv_params &p, const lutr_planes *src, const lutr_planes *dst, UnionCall *u)
{
    if (const int rc = make_yuv_consts_xsub(p, &u->K)) return rc;
    u->side[0] = planar_side("source", src, p.fmt_in);
    u->side[1] = planar_side("destination", dst, p.fmt_out);
    u->nsides = 2;
    u->lut_depth = p.lut_depth;
    return LUTR_OK;
}

// Second half, ahead of the empty call: lut_depth in range under the family's `tag` (nullptr: the family has no such check, the
// constants have refused a depth outside 8..16), whole union blocks of every side, and no LDS-window kernel (`lds_noun`: for what).
static int union_rules(const lutr_ctx *c, const UnionCall &u, const FrameGeom &G, const char *tag, const char *lds_noun)
{
    if (tag && (u.lut_depth < 8 || u.lut_depth > 16)) { set_error("%s: LUT depth %d outside 8..16", tag, u.lut_depth); return LUTR_EINVAL; }
    int csy = 0;
    for (int k = 0; k < u.nsides; k++) csy = std::max(csy, u.side[k].csy);
    if (const int rc = check_row_blocks(G.row0, G.rows, G.h, 1 << csy, "union chroma block height")) return rc;
    if (c->variant == VAR_VEC_LDS) { set_error("variant vec_lds: there is no LDS-window kernel for %s", lds_noun); return LUTR_EINVAL; }
    return LUTR_OK;
}

// ... and behind it: every plane has a base pointer, and the 16-bit planes are aligned.
static int union_planes_ready(const UnionCall &u, const FrameGeom &G)
{
    if (const int rc = check_planes_set(u.side[0].pl, u.side[1].pl)) return rc;
    if (u.nsides > 2)
        if (const int rc = check_planes_set(u.side[2].pl, nullptr)) return rc;
    return check_sides_aligned(u.side, u.nsides, G.nframes);
}

// The dither path's float planes for the whole frames of G with output chroma subsampled by 2^csx x 2^csy, out of the context's
// scratch (grown when too small).
static int dither_scratch(lutr_ctx *c, const FrameGeom &G, int csx, int csy, FloatPlanes *F)
{
    const size_t ny = (size_t)G.w * G.h * G.nframes, nc = (size_t)chroma_dim(G.w, csx) * chroma_dim(G.h, csy) * G.nframes;
    if (ny + 2 * nc > c->fscratch_floats) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (c->fscratch) (void)hipFree(c->fscratch);
        c->fscratch = nullptr;
        c->fscratch_floats = 0;
        void *q = nullptr;
        hipError_t e = hipMalloc(&q, (ny + 2 * nc) * sizeof(float));
        if (e != hipSuccess) { set_error("hipMalloc(%zu): %s", (ny + 2 * nc) * sizeof(float), hipGetErrorString(e)); return LUTR_ENOMEM; }
        c->fscratch = (float *)q;
        c->fscratch_floats = ny + 2 * nc;
    }
    *F = FloatPlanes{c->fscratch, c->fscratch + ny, c->fscratch + ny + nc};
    return LUTR_OK;
}

// The blue-noise table of the context's device: d = (2 rank - 4095) / 8192 per mask cell, exact in fp32.
static int bn_table(lutr_ctx *c, const float **out)
{
    if (!c->bn_tab) {
        std::vector<float> d(64 * 64);
        for (int i = 0; i < 64 * 64; i++) d[i] = (float)(2 * (int)kLutrBnMask[i] - 4095) / 8192.0f;
        void *p = nullptr;
        hipError_t e = hipMalloc(&p, d.size() * sizeof(float));
        if (e != hipSuccess) { set_error("hipMalloc(dither table): %s", hipGetErrorString(e)); return LUTR_ENOMEM; }
        e = hipMemcpy(p, d.data(), d.size() * sizeof(float), hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(p); return hip_fail(e, "dither table upload"); }
        c->bn_tab = (float *)p;
    }
    *out = c->bn_tab;
    return LUTR_OK;
}

int lutr_apply_yuv_sited(lutr_ctx *c, const lutr_yuv_params *p, int interp, int chroma_loc, int w, int h, int nframes,
                         const lutr_planes *src, lutr_planes *dst, int row0, int rows)
{
    if (chroma_loc < LUTR_CHROMA_REPLICATE || chroma_loc > LUTR_CHROMA_TOPLEFT) {
        set_error("unknown chroma location %d", chroma_loc);
        return LUTR_EINVAL;
    }
    int rc = check_common(c, interp, LUTR_INTERP_NEAREST, w, h, nframes, src, dst, row0, rows);
    if (rc) return rc;
    if (!p) { set_error("null yuv params"); return LUTR_EINVAL; }
    const int csx = LUTR_FMT_CSX(p->fmt_in), csy = LUTR_FMT_CSY(p->fmt_in);
    if (chroma_loc == LUTR_CHROMA_REPLICATE || (csx == 0 && csy == 0))
        return lutr_apply_yuv(c, p, interp, w, h, nframes, src, dst, row0, rows);
    YuvConsts K;
    rc = make_yuv_consts_sited(*p, chroma_loc, &K);
    if (rc) return rc;
    const int bh = 1 << csy;
    if (const int rc = check_row_blocks(row0, rows, h, bh, "chroma block height")) return rc;
    if (w == 0 || rows == 0 || nframes == 0) return LUTR_OK;
    if (const int rc = check_planes_set(src, dst)) return rc;
    // the resampling reads around every output sample: a destination that overlaps a source would be read after being written
    const int din = LUTR_FMT_DEPTH(p->fmt_in), dout = LUTR_FMT_DEPTH(p->fmt_out);
    const FrameGeom G{w, h, row0, rows, nframes};
    if (const int rc = check_sides_disjoint("sited chroma resampling", true, planar_side("source", src, p->fmt_in),
                                            planar_side("destination", dst, p->fmt_out), G)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    LutConsts L; PlaneSet P;
    if (const int rc = fill_lut(&L, c, p->lut_depth)) return rc;
    fill_planes(&P, src, dst);
    const char *name = launch_yuv_sited(c->stream, L, K, P, G, din, dout, csy, chroma_loc, interp);
    if (!name) { set_error("launch too large for the sited kernels (split the batch)"); return LUTR_EINVAL; }
    return finish_launch(c, name);
}

int lutr_apply_yuv_dither(lutr_ctx *c, const lutr_yuv_params *p, int interp, int dither, int w, int h, int nframes,
                          const lutr_planes *src, const lutr_planes *dst)
{
    if (dither == LUTR_DITHER_NONE) return lutr_apply_yuv(c, p, interp, w, h, nframes, src, dst, 0, h);
    if (dither == LUTR_DITHER_BLUE_NOISE) return lutr_apply_yuv_xsub(c, p, interp, dither, w, h, nframes, src, dst, 0, h);
    if (dither != LUTR_DITHER_ERROR_DIFFUSION) { set_error("unknown dither mode %d", dither); return LUTR_EINVAL; }
    int rc = check_common(c, interp, LUTR_INTERP_NEAREST, w, h, nframes, src, dst, 0, h);
    if (rc) return rc;
    if (!p) { set_error("null yuv params"); return LUTR_EINVAL; }
    YuvConsts K;
    rc = make_yuv_consts(*p, &K);
    if (rc) return rc;
    if (w == 0 || h == 0 || nframes == 0) return LUTR_OK;
    if (const int rc = check_planes_set(src, dst)) return rc;
    const int csx = LUTR_FMT_CSX(p->fmt_in), csy = LUTR_FMT_CSY(p->fmt_in);
    HIP_TRY(hipSetDevice(c->device));
    FloatPlanes F; FrameGeom G{w, h, 0, h, nframes};
    if (const int rc = dither_scratch(c, G, csx, csy, &F)) return rc;
    LutConsts L; PlaneSet P;
    if (const int rc = fill_lut(&L, c, p->lut_depth)) return rc;
    fill_planes(&P, src, dst);
    return finish_launch(c, launch_yuv_dither(c->stream, L, K, P, G, F, LUTR_FMT_DEPTH(p->fmt_in),
                                              LUTR_FMT_DEPTH(p->fmt_out), csx, csy, interp, csx, csy));
}

int lutr_apply_yuv_xsub(lutr_ctx *c, const lutr_yuv_params *p, int interp, int dither, int w, int h, int nframes,
                        const lutr_planes *src, const lutr_planes *dst, int row0, int rows)
{
    if (const int rc = check_dither(dither)) return rc;
    int rc = check_common(c, interp, LUTR_INTERP_NEAREST, w, h, nframes, src, dst, row0, rows);
    if (rc) return rc;
    if (!p) { set_error("null yuv params"); return LUTR_EINVAL; }
    YuvConsts K;
    rc = make_yuv_consts_xsub(*p, &K);
    if (rc) return rc;
    if (const int rc = check_dither_rows(dither, row0, rows, h)) return rc;
    const int icsx = LUTR_FMT_CSX(p->fmt_in), icsy = LUTR_FMT_CSY(p->fmt_in);
    const int ocsx = LUTR_FMT_CSX(p->fmt_out), ocsy = LUTR_FMT_CSY(p->fmt_out);
    if (icsx == ocsx && icsy == ocsy && dither != LUTR_DITHER_BLUE_NOISE)        // one layout: lutr_apply_yuv's contract, kernels and bits
        return dither == LUTR_DITHER_NONE ? lutr_apply_yuv(c, p, interp, w, h, nframes, src, dst, row0, rows)
                                          : lutr_apply_yuv_dither(c, p, interp, dither, w, h, nframes, src, dst);
    const int bh = 1 << (icsy > ocsy ? icsy : ocsy);
    if (const int rc = check_row_blocks(row0, rows, h, bh, "union chroma block height")) return rc;
    if (w == 0 || rows == 0 || nframes == 0) return LUTR_OK;
    if (const int rc = check_planes_set(src, dst)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    LutConsts L; PlaneSet P; FrameGeom G{w, h, row0, rows, nframes};
    if (const int rc = fill_lut(&L, c, p->lut_depth)) return rc;
    fill_planes(&P, src, dst);
    const int din = LUTR_FMT_DEPTH(p->fmt_in), dout = LUTR_FMT_DEPTH(p->fmt_out);
    if (dither == LUTR_DITHER_NONE)
        return finish_launch(c, launch_yuv_xsub(c->stream, c->variant, L, K, P, G, din, dout, icsx, icsy, ocsx, ocsy, interp));
    if (dither == LUTR_DITHER_BLUE_NOISE) {
        const float *bn;
        if (const int rc = bn_table(c, &bn)) return rc;
        return finish_launch(c, launch_yuv_bn(c->stream, c->variant, L, K, P, G, bn, din, dout, icsx, icsy, ocsx, ocsy, interp));
    }
    FloatPlanes F;
    if (const int rc = dither_scratch(c, G, ocsx, ocsy, &F)) return rc;
    return finish_launch(c, launch_yuv_dither(c->stream, L, K, P, G, F, din, dout, icsx, icsy, interp, ocsx, ocsy));
}

// lutr_apply_yuv_xsub's pass with a second destination.  Each output's constants are the block
// make_yuv_consts_xsub forms for it (the input-stage entries of the two agree: they do not depend on fmt_out).
int lutr_apply_yuv_dual(lutr_ctx *c, const lutr_yuv_params *p, int fmt_out2, int interp, int w, int h, int nframes,
                        const lutr_planes *src, const lutr_planes *dst, const lutr_planes *dst2, int row0, int rows)
{
    int rc = check_common(c, interp, LUTR_INTERP_NEAREST, w, h, nframes, src, dst, row0, rows);
    if (rc) return rc;
    if (!dst2) { set_error("null argument"); return LUTR_EINVAL; }
    if (!p) { set_error("null yuv params"); return LUTR_EINVAL; }
    UnionCall U; YuvConsts K2; const FrameGeom G{w, h, row0, rows, nframes};
    if (const int rc = union_open(*p, src, dst, &U)) return rc;
    lutr_yuv_params p2 = *p;
    p2.fmt_out = fmt_out2;
    if ((fmt_out2 >> 10) || make_yuv_consts_xsub(p2, &K2)) {
        set_error("bad fmt_out2 0x%x: the second output is planar 4:2:0 / 4:2:2 / 4:4:4 at a depth of 8 to 16 bit", fmt_out2);
        return LUTR_EINVAL;
    }
    U.side[U.nsides++] = planar_side("second destination", dst2, fmt_out2);
    const Side &S = U.side[0], &D1 = U.side[1], &D2 = U.side[2];
    if (const int rc = union_rules(c, U, G, nullptr, "two outputs")) return rc;
    if (w == 0 || rows == 0 || nframes == 0) return LUTR_OK;
    if (const int rc = union_planes_ready(U, G)) return rc;
    // one pass writes both outputs while it still reads the source: nothing may overlap anything
    if (const int rc = check_sides_disjoint("the two-output pass", true, S, D1, G)) return rc;
    if (check_sides_disjoint("the two-output pass", true, S, D2, G)) {
        const std::string m = g_last_error;
        set_error("%s (the second destination)", m.c_str());
        return LUTR_EINVAL;
    }
    if (check_sides_disjoint("", false, D1, D2, G)) {
        set_error("the two destinations overlap: their byte ranges over all rows and frames must be disjoint");
        return LUTR_EINVAL;
    }
    HIP_TRY(hipSetDevice(c->device));
    LutConsts L; PlaneSet P; DstPlanes P2;
    if (const int rc = fill_lut(&L, c, p->lut_depth)) return rc;
    fill_planes(&P, src, dst);
    for (int i = 0; i < 3; i++) {
        P2.d[i] = (uint8_t *)dst2->data[i];
        P2.ds[i] = dst2->stride[i];
        P2.dfs[i] = dst2->frame_stride[i];
    }
    return finish_launch(c, launch_yuv_dual(c->stream, c->variant, L, U.K, K2, P, P2, G, S.depth, D1.depth, D1.csx, D1.csy, D2.depth,
                                            D2.csx, D2.csy, S.csx, S.csy, interp));
}

// lutr_apply_yuv_xsub's pass for any pair of layouts with the second lattice behind the first.
int lutr_apply_yuv_chain(lutr_ctx *c, const lutr_yuv_params *p, int interp, int interp2, int w, int h, int nframes,
                         const lutr_planes *src, const lutr_planes *dst, int row0, int rows)
{
    int rc = check_common(c, interp, LUTR_INTERP_NEAREST, w, h, nframes, src, dst, row0, rows);
    if (rc) return rc;
    if (!c->lat2) { set_error("no second lattice set on this context (call lutr_ctx_set_lut2 first)"); return LUTR_EINVAL; }
    if (interp2 < LUTR_INTERP_NEAREST || interp2 > LUTR_INTERP_PRISM) {
        set_error("unknown interpolation mode %d for the second LUT", interp2);
        return LUTR_EINVAL;
    }
    if (!p) { set_error("null yuv params"); return LUTR_EINVAL; }
    UnionCall U; const FrameGeom G{w, h, row0, rows, nframes};
    if (const int rc = union_open(*p, src, dst, &U)) return rc;
    const Side &S = U.side[0], &D = U.side[1];
    if (const int rc = union_rules(c, U, G, nullptr, "two LUTs in one pass")) return rc;
    if (w == 0 || rows == 0 || nframes == 0) return LUTR_OK;
    if (const int rc = union_planes_ready(U, G)) return rc;
    if (const int rc = check_sides_disjoint("the two-LUT pass", true, S, D, G)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    LutConsts L; PlaneSet P;
    if (const int rc = fill_lut(&L, c, p->lut_depth)) return rc;
    fill_planes(&P, src, dst);
    return finish_launch(c, launch_yuv_chain(c->stream, c->variant, L, second_lattice(c, p->lut_depth), U.K, P, G, S.depth, D.depth,
                                             S.csx, S.csy, D.csx, D.csy, interp, interp2));
}

// ---- ASC CDL in front of lut3d
// what both entry points refuse in a CDL: a number that is not finite, a negative slope or saturation, a power that is not above 0
static int check_cdl(const lutr_cdl *d)
{
    static const char *const ch[3] = {"R", "G", "B"};
    for (int i = 0; i < 3; i++) {
        if (!std::isfinite(d->slope[i]) || !std::isfinite(d->offset[i]) || !std::isfinite(d->power[i])) {
            set_error("CDL: slope, offset or power of %s is not finite (%g, %g, %g)", ch[i], (double)d->slope[i], (double)d->offset[i],
                      (double)d->power[i]);
            return LUTR_EINVAL;
        }
        if (d->slope[i] < 0.0f) { set_error("CDL: slope of %s is negative (%g)", ch[i], (double)d->slope[i]); return LUTR_EINVAL; }
        if (!(d->power[i] > 0.0f)) { set_error("CDL: power of %s must be above 0 (%g)", ch[i], (double)d->power[i]); return LUTR_EINVAL; }
    }
    if (!std::isfinite(d->saturation)) { set_error("CDL: saturation is not finite (%g)", (double)d->saturation); return LUTR_EINVAL; }
    if (d->saturation < 0.0f) { set_error("CDL: saturation is negative (%g)", (double)d->saturation); return LUTR_EINVAL; }
    return LUTR_OK;
}

// Stage A for one channel, codes 0 .. 2^depth - 1 (the entry past M of a depth below 16 does not exist: 2^depth - 1 = M).  In
// double: the product of two floats is exact there, the sum is rounded once.
static void cdl_channel_table(const lutr_cdl &d, int depth, int ch, float *out)
{
    const int maxi = (1 << depth) - 1;
    const float scale_f = 1.0f / (float)maxi;
    const double slope = d.slope[ch], offset = d.offset[ch], power = d.power[ch];
    for (int k = 0; k <= maxi; k++) {
        const double x = (double)((float)k * scale_f);
        const double v = x * slope + offset;
        const double t = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
        out[k] = (float)(power == 1.0 ? t : std::pow(t, power));
    }
}

// The device table of (slope, offset, power) at `depth`, rebuilt when that key changes.  The kernel of the previous call may
// still be reading the old contents, so the copy goes on the context's stream, behind it; hipMemcpyWithStream returns when the
// copy is done, so the host table (a local) is never rewritten or freed under a pending copy.
static int cdl_device_table(lutr_ctx *c, const lutr_cdl &d, int depth, CdlConsts *C)
{
    const size_t ne = (size_t)1 << depth, n = 3 * ne;
    float key[9];
    std::memcpy(key, d.slope, sizeof(key));          // slope, offset, power: the first nine floats of lutr_cdl
    if (!c->cdl_tab || c->cdl_depth != depth || std::memcmp(key, c->cdl_key, sizeof(key)) != 0) {
        c->cdl_depth = 0;
        if (c->cdl_cap < n) {
            void *p = nullptr;
            const hipError_t e = hipMalloc(&p, n * sizeof(float));
            if (e != hipSuccess) { set_error("hipMalloc(CDL table): %s", hipGetErrorString(e)); return LUTR_ENOMEM; }
            if (c->cdl_tab) {
                HIP_TRY(hipStreamSynchronize(c->stream));    // a launch may still be reading the smaller table
                (void)hipFree(c->cdl_tab);
            }
            c->cdl_tab = (float *)p;
            c->cdl_cap = n;
        }
        std::vector<float> host(n);
        for (int ch = 0; ch < 3; ch++) cdl_channel_table(d, depth, ch, &host[(size_t)ch * ne]);
        HIP_TRY(hipMemcpyWithStream(c->cdl_tab, host.data(), n * sizeof(float), hipMemcpyHostToDevice, c->stream));
        std::memcpy(c->cdl_key, key, sizeof(key));
        c->cdl_depth = depth;
    }
    C->tab = c->cdl_tab;
    C->stride = (int)ne;
    C->sat = d.saturation;
    return LUTR_OK;
}

int lutr_cdl_table(const lutr_cdl *cdl, int depth, int channel, float *out)
{
    if (!cdl || !out) { set_error("lutr_cdl_table: null argument"); return LUTR_EINVAL; }
    if (depth < 8 || depth > 16) { set_error("lutr_cdl_table: depth %d outside 8..16", depth); return LUTR_EINVAL; }
    if (channel < 0 || channel > 2) { set_error("lutr_cdl_table: channel %d outside 0..2", channel); return LUTR_EINVAL; }
    if (const int rc = check_cdl(cdl)) return rc;
    cdl_channel_table(*cdl, depth, channel, out);
    return LUTR_OK;
}

// lutr_apply_yuv_xsub's pass for any pair of layouts with the CDL between its first stage and the lattice.
int lutr_apply_yuv_cdl(lutr_ctx *c, const lutr_yuv_params *p, int interp, const lutr_cdl *cdl, int w, int h, int nframes,
                       const lutr_planes *src, const lutr_planes *dst, int row0, int rows)
{
    int rc = check_common(c, interp, LUTR_INTERP_NEAREST, w, h, nframes, src, dst, row0, rows);
    if (rc) return rc;
    if (!cdl) { set_error("null CDL"); return LUTR_EINVAL; }
    if (const int rc = check_cdl(cdl)) return rc;
    if (c->pre_size) {
        set_error("CDL: the LUT has a .csp prelut; its table is indexed by integer codes, and the CDL's output is not a code");
        return LUTR_EINVAL;
    }
    if (!p) { set_error("null yuv params"); return LUTR_EINVAL; }
    UnionCall U; const FrameGeom G{w, h, row0, rows, nframes};
    if (const int rc = union_open(*p, src, dst, &U)) return rc;
    const Side &S = U.side[0], &D = U.side[1];
    if (const int rc = union_rules(c, U, G, "CDL", "the CDL pass")) return rc;
    if (w == 0 || rows == 0 || nframes == 0) return LUTR_OK;
    if (const int rc = union_planes_ready(U, G)) return rc;
    if (const int rc = check_sides_disjoint("the CDL pass", true, S, D, G)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    LutConsts L; CdlConsts C; PlaneSet P;
    if (const int rc = fill_lut(&L, c, p->lut_depth)) return rc;
    if (const int rc = cdl_device_table(c, *cdl, p->lut_depth, &C)) return rc;
    fill_planes(&P, src, dst);
    return finish_launch(c, launch_yuv_cdl(c->stream, c->variant, L, C, U.K, P, G, S.depth, D.depth, S.csx, S.csy, D.csx, D.csy, interp));
}

// ---- 1D LUT alone or in front of lut3d
int lutr_ctx_set_lut1d(lutr_ctx *c, const float *lut, int size, const float scale[3], int interp1d)
{
    if (!c) { set_error("null context"); return LUTR_EINVAL; }
    if (!lut || size == 0) {             // remove it; the device tables stay allocated and go stale with the generation
        c->l1d.clear();
        c->l1d_size = 0;
        c->l1d_gen++;
        return LUTR_OK;
    }
    if (!scale) { set_error("null argument"); return LUTR_EINVAL; }
    // the table builder's own checks (size, mode, scale, finite nodes), on a depth-8 table of every channel
    uint16_t probe[256];
    for (int ch = 0; ch < 3; ch++)
        if (const int rc = lutr_lut1d_table(lut, size, scale, interp1d, 8, ch, probe)) return rc;
    c->l1d.assign(lut, lut + (size_t)3 * size);
    c->l1d_size = size;
    std::memcpy(c->l1d_scale, scale, sizeof(c->l1d_scale));
    c->l1d_interp = interp1d;
    c->l1d_gen++;
    return LUTR_OK;
}

// The device table of the context's 1D LUT at `depth`, rebuilt when lutr_ctx_set_lut1d has run since it was built.  The kernel of
// the previous call may still be reading the old contents, so the copy goes on the context's stream, behind it;
// hipMemcpyWithStream returns when the copy is done, so the host table (a local) is never freed under a pending copy.
static int l1d_device_table(lutr_ctx *c, int depth, L1dConsts *C)
{
    if (!c->l1d_size) { set_error("no 1D LUT set on this context (call lutr_ctx_set_lut1d first)"); return LUTR_EINVAL; }
    const size_t ne = (size_t)1 << depth, n = 3 * ne;
    lutr_ctx::L1dTable &t = c->l1d_tab[depth - 8];
    if (!t.dev) {
        void *p = nullptr;
        const hipError_t e = hipMalloc(&p, n * sizeof(uint16_t));
        if (e != hipSuccess) { set_error("hipMalloc(1D LUT table): %s", hipGetErrorString(e)); return LUTR_ENOMEM; }
        t.dev = (uint16_t *)p;
        t.gen = 0;
    }
    if (t.gen != c->l1d_gen) {
        std::vector<uint16_t> host(n);
        for (int ch = 0; ch < 3; ch++)
            if (const int rc = lutr_lut1d_table(c->l1d.data(), c->l1d_size, c->l1d_scale, c->l1d_interp, depth, ch, &host[(size_t)ch * ne]))
                return rc;
        t.gen = 0;
        HIP_TRY(hipMemcpyWithStream(t.dev, host.data(), n * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
        t.gen = c->l1d_gen;
    }
    C->tab = t.dev;
    C->stride = (int)ne;
    return LUTR_OK;
}

// lutr_apply_yuv_cdl's pass with the 1D table in the CDL's place; interp LUTR_INTERP_NONE leaves lut3d out.
int lutr_apply_yuv_lut1d(lutr_ctx *c, const lutr_yuv_params *p, int interp, int w, int h, int nframes, const lutr_planes *src,
                         const lutr_planes *dst, int row0, int rows)
{
    int rc = check_common(c, interp, LUTR_INTERP_NONE, w, h, nframes, src, dst, row0, rows);
    if (rc) return rc;
    if (!c->l1d_size) { set_error("no 1D LUT set on this context (call lutr_ctx_set_lut1d first)"); return LUTR_EINVAL; }
    if (!p) { set_error("null yuv params"); return LUTR_EINVAL; }
    UnionCall U; const FrameGeom G{w, h, row0, rows, nframes};
    if (const int rc = union_open(*p, src, dst, &U)) return rc;
    const Side &S = U.side[0], &D = U.side[1];
    if (const int rc = union_rules(c, U, G, "lut1d", "the lut1d pass")) return rc;
    if (w == 0 || rows == 0 || nframes == 0) return LUTR_OK;
    if (const int rc = union_planes_ready(U, G)) return rc;
    if (const int rc = check_sides_disjoint("the lut1d pass", true, S, D, G)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    LutConsts L{}; L1dConsts C; PlaneSet P;
    if (interp != LUTR_INTERP_NONE)
        if (const int rc = fill_lut(&L, c, p->lut_depth)) return rc;
    if (const int rc = l1d_device_table(c, p->lut_depth, &C)) return rc;
    fill_planes(&P, src, dst);
    return finish_launch(c, launch_yuv_l1d(c->stream, c->variant, L, C, U.K, P, G, S.depth, D.depth, S.csx, S.csy, D.csx, D.csy, interp));
}

// The matrix of lutr_apply_yuv_stack_matrix: every entry finite and at most 65536 in magnitude, so that every sum of the stage is
// finite.  The test is on the bits (this file is built without honouring NaNs): 65536.0f is 0x47800000.
static int check_rgb_matrix(const lutr_rgb_matrix *mtx)
{
    for (int i = 0; i < 12; i++) {
        const float v = i < 9 ? mtx->m[i] : mtx->offset[i - 9];
        uint32_t bits;
        memcpy(&bits, &v, sizeof bits);
        if ((bits & 0x7fffffffu) > 0x47800000u) {
            if (i < 9) set_error("stack: matrix entry m[%d] = %g is not finite or above 65536 in magnitude", i, (double)v);
            else set_error("stack: matrix entry offset[%d] = %g is not finite or above 65536 in magnitude", i - 9, (double)v);
            return LUTR_EINVAL;
        }
    }
    return LUTR_OK;
}

// ---- the stage list of the stack entries, the one copy of its checks, its compilation into steps
// and its device resources.  What a list gives: which kinds it names, its text for lutr_ctx_last_kernel, its step word.
struct StackList {
    bool seen[6] = {false, false, false, false, false, false};
    std::string list;
    unsigned long long ops = 0;
};

// `with_mtx`: the entry takes a matrix stage (lutr_apply_yuv_stack_matrix, lutr_apply_rgb_stack); `mtx` is its matrix, or nullptr
static int stack_check_list(const lutr_ctx *c, const lutr_stage *stages, int nstages, const lutr_cdl *cdl, bool with_mtx,
                            const lutr_rgb_matrix *mtx, StackList *T)
{
    if (nstages < 1 || nstages > 4) { set_error("stack: %d stages; a stack has 1 to 4", nstages); return LUTR_EINVAL; }
    if (!stages) { set_error("stack: null stage list"); return LUTR_EINVAL; }
    static const char *const kind_name[6] = {"", "lut3d", "lut3d2", "lut1d", "cdl", "matrix"};
    for (int i = 0; i < nstages; i++) {
        const int k = stages[i].kind;
        if (k < LUTR_STAGE_LUT3D || k > LUTR_STAGE_MATRIX) { set_error("stack: stage %d has unknown kind %d", i, k); return LUTR_EINVAL; }
        if (k == LUTR_STAGE_MATRIX && !with_mtx) {
            set_error("stack: stage %d is a matrix stage; a matrix is lutr_apply_yuv_stack_matrix's, and a strength or a matte "
                      "together with a matrix is not supported", i);
            return LUTR_EINVAL;
        }
        if (T->seen[k]) { set_error("stack: stage kind %s is listed twice; each kind may appear once", kind_name[k]); return LUTR_EINVAL; }
        T->seen[k] = true;
        if (i) T->list += ",";
        T->list += kind_name[k];
        if (k == LUTR_STAGE_LUT3D || k == LUTR_STAGE_LUT3D_2) {
            if (stages[i].interp < LUTR_INTERP_NEAREST || stages[i].interp > LUTR_INTERP_PRISM) {
                set_error("stack: unknown interpolation mode %d on stage %d (%s)", stages[i].interp, i, kind_name[k]);
                return LUTR_EINVAL;
            }
            T->list += ":" + std::to_string(stages[i].interp);
        }
    }
    if (T->seen[LUTR_STAGE_LUT3D] && !c->lat) { set_error("stack: no lattice set on this context (call lutr_ctx_set_lut first)"); return LUTR_EINVAL; }
    if (T->seen[LUTR_STAGE_LUT3D_2] && !c->lat2) {
        set_error("stack: no second lattice set on this context (call lutr_ctx_set_lut2 first)");
        return LUTR_EINVAL;
    }
    if (T->seen[LUTR_STAGE_LUT1D] && !c->l1d_size) {
        set_error("stack: no 1D LUT set on this context (call lutr_ctx_set_lut1d first)");
        return LUTR_EINVAL;
    }
    if (T->seen[LUTR_STAGE_CDL] && !cdl) { set_error("stack: a cdl stage is listed and the CDL is null"); return LUTR_EINVAL; }
    if (!T->seen[LUTR_STAGE_CDL] && cdl) { set_error("stack: a CDL is given and no cdl stage is listed"); return LUTR_EINVAL; }
    if (cdl)
        if (const int rc = check_cdl(cdl)) return rc;
    if (T->seen[LUTR_STAGE_MATRIX] && !mtx) { set_error("stack: a matrix stage is listed and the matrix is null"); return LUTR_EINVAL; }
    if (!T->seen[LUTR_STAGE_MATRIX] && mtx) { set_error("stack: a matrix is given and no matrix stage is listed"); return LUTR_EINVAL; }
    if (mtx)
        if (const int rc = check_rgb_matrix(mtx)) return rc;
    return LUTR_OK;
}

// The pixel's state (codes or unit) is followed here, so the kernels are told which form of a lattice stage to run and where the
// rounding goes.
static int stack_compile_steps(const lutr_ctx *c, const lutr_stage *stages, int nstages, StackList *T)
{
    // the steps: a unit pixel is rounded to codes ahead of lut1d, ahead of the CDL (behind a matrix) and at the end of the list
    unsigned long long ops = 0;
    int nops = 0;
    bool unit = false;
    auto push = [&](int op, int mode) { ops |= (unsigned long long)(op | (mode << 4)) << (8 * nops++); };
    for (int i = 0; i < nstages; i++) {
        switch (stages[i].kind) {
        case LUTR_STAGE_LUT1D:
            if (unit) push(STACK_OP_ROUND, 0);
            push(STACK_OP_L1D, 0);
            unit = false;
            break;
        case LUTR_STAGE_CDL:
            if (unit) push(STACK_OP_ROUND, 0);   // behind a matrix only: the CDL's table is per code
            push(STACK_OP_CDL, 0);
            unit = true;
            break;
        case LUTR_STAGE_MATRIX:
            push(unit ? STACK_OP_MTX_UNIT : STACK_OP_MTX_CODES, 0);
            unit = true;
            break;
        case LUTR_STAGE_LUT3D:
            if (unit && c->pre_size) {
                if (stages[i - 1].kind == LUTR_STAGE_MATRIX)
                    set_error("stack: lut3d directly behind matrix, and the LUT has a .csp prelut; its table is indexed by integer "
                              "codes, and the matrix's output is not a code");
                else
                    set_error("stack: lut3d directly behind cdl, and the LUT has a .csp prelut; its table is indexed by integer codes, and "
                              "the CDL's output is not a code");
                return LUTR_EINVAL;
            }
            push(unit ? STACK_OP_LAT_UNIT : STACK_OP_LAT_CODES, stages[i].interp);
            unit = false;
            break;
        default:
            push(unit ? STACK_OP_LAT2_UNIT : STACK_OP_LAT2_CODES, stages[i].interp);
            unit = false;
            break;
        }
    }
    if (unit) push(STACK_OP_ROUND, 0);
    T->ops = ops;
    return LUTR_OK;
}

// the lattices, the step word and the tables of the listed stages at `depth`, behind hipSetDevice
static int stack_device_consts(lutr_ctx *c, const StackList &T, const lutr_cdl *cdl, const lutr_rgb_matrix *mtx, int depth, LutConsts *L,
                               LutConsts *L2, StackConsts *S, MtxConsts *X)
{
    if (T.seen[LUTR_STAGE_LUT3D])
        if (const int rc = fill_lut(L, c, depth)) return rc;
    if (T.seen[LUTR_STAGE_LUT3D_2]) *L2 = second_lattice(c, depth);
    S->ops = T.ops;
    S->stride = 1 << depth;
    S->sat = 1.0f;
    S->maxf = (float)((1 << depth) - 1);
    if (cdl) {
        CdlConsts C;
        if (const int rc = cdl_device_table(c, *cdl, depth, &C)) return rc;
        S->cdl_tab = C.tab;
        S->sat = C.sat;
        S->lds_cdl_words = 3 * S->stride;
    }
    if (T.seen[LUTR_STAGE_LUT1D]) {
        L1dConsts C1;
        if (const int rc = l1d_device_table(c, depth, &C1)) return rc;
        S->l1d_tab = C1.tab;
        S->lds_l1d_words = 3 * (S->stride >> 1);
    }
    if (mtx) {
        for (int i = 0; i < 9; i++) X->m[i] = mtx->m[i];
        for (int i = 0; i < 3; i++) X->off[i] = mtx->offset[i];
        X->rcp = 1.0f / S->maxf;
    }
    return LUTR_OK;
}

// ---- an ordered stack of lut1d / CDL / lut3d stages
// lutr_apply_yuv_cdl's pass with the stage list compiled into steps (stack_compile_steps).
// `mix`: nullptr for lutr_apply_yuv_stack, the strength for lutr_apply_yuv_stack_mix.
// `matte` (with `mix`): the matte of lutr_apply_yuv_stack_matte, its pointer, depth and invert already checked.
// `with_mtx` (without `mix`): the call is lutr_apply_yuv_stack_matrix's, the one entry that takes a matrix stage;
// `mtx` is its matrix, or nullptr.
// `iy`, `oy` (without `mix` and `with_mtx`): the containers of the two sides of lutr_apply_yuv_stack_semi, both
// or neither; with them a side may be two planes, and the kernels are the semi forms.
static int check_semi_side(const Side &s, const lutr_yuv_layout *y, int nframes);
static int apply_yuv_stack(lutr_ctx *c, const lutr_yuv_params *p, const lutr_stage *stages, int nstages, const lutr_cdl *cdl,
                           const MixConsts *mix, const lutr_matte *matte, bool with_mtx, const lutr_rgb_matrix *mtx, int w, int h,
                           int nframes, const lutr_planes *src, const lutr_planes *dst, int row0, int rows,
                           const lutr_yuv_layout *iy = nullptr, const lutr_yuv_layout *oy = nullptr)
{
    if (!c || !src || !dst) { set_error("null argument"); return LUTR_EINVAL; }
    StackList T;
    if (const int rc = stack_check_list(c, stages, nstages, cdl, with_mtx, mtx, &T)) return rc;
    if (const int rc = check_geometry(w, h, nframes, row0, rows)) return rc;
    if (const int rc = stack_compile_steps(c, stages, nstages, &T)) return rc;
    if (!p) { set_error("null yuv params"); return LUTR_EINVAL; }
    UnionCall U; const FrameGeom G{w, h, row0, rows, nframes};
    if (const int rc = union_open(*p, src, dst, &U)) return rc;
    const Side &Si = U.side[0], &Di = U.side[1];
    if (iy) {
        // each side's layout against its format, the planes it has and their alignment (union_planes_ready's part, per container)
        if (const int rc = check_semi_side(Si, iy, nframes)) return rc;
        if (const int rc = check_semi_side(Di, oy, nframes)) return rc;
        U.side[0].semi = iy->semi != 0;
        U.side[1].semi = oy->semi != 0;
    }
    if (const int rc = union_rules(c, U, G, "stack", "the stack pass")) return rc;
    if (w == 0 || rows == 0 || nframes == 0) return LUTR_OK;
    if (!iy)
        if (const int rc = union_planes_ready(U, G)) return rc;
    if (const int rc = check_sides_disjoint("the stack pass", true, Si, Di, G)) return rc;
    MatteConsts A{};
    if (matte) {
        Span ds[3];
        side_spans(Di, G, ds);
        const int mb = matte->depth > 8 ? 2 : 1;
        if ((long long)matte->stride < (long long)w * mb) {
            set_error("stack: matte stride %lld is shorter than a row of %d samples of %d byte(s)", (long long)matte->stride, w, mb);
            return LUTR_EINVAL;
        }
        if (mb == 2 && (((uintptr_t)matte->data | (uintptr_t)matte->stride | (uintptr_t)matte->frame_stride) & 1)) {
            set_error("stack: a matte of %d bits is held in 16-bit words: base, stride and frame stride must be even", matte->depth);
            return LUTR_EINVAL;
        }
        const Span ms = plane_span(matte->data, matte->stride, matte->frame_stride, h, (long long)w * mb, nframes);
        for (int j = 0; j < 3; j++)
            if (ms.lo < ds[j].hi && ds[j].lo < ms.hi) {
                set_error("stack: the byte range of the matte overlaps that of destination plane %d", j);
                return LUTR_EINVAL;
            }
        const float maxm = (float)((1 << matte->depth) - 1);
        A = MatteConsts{(const uint8_t *)matte->data, (long long)matte->stride, nframes > 1 ? (long long)matte->frame_stride : 0, maxm,
                        1.0f / maxm, matte->invert, mb == 2};
    }
    HIP_TRY(hipSetDevice(c->device));
    LutConsts L{}, L2{}; StackConsts S{}; MtxConsts X{}; PlaneSet P;
    if (const int rc = stack_device_consts(c, T, cdl, mtx, p->lut_depth, &L, &L2, &S, &X)) return rc;
    fill_planes(&P, src, dst);
    const char *name;
    if (iy) {
        if (iy->semi) clear_planes(&P, true, 2);
        if (oy->semi) clear_planes(&P, false, 2);
        const SemiArgs Y{iy->semi, iy->swap, iy->shift, oy->semi, oy->swap, oy->shift};
        name = launch_yuv_stack_semi(c->stream, c->variant, L, L2, S, U.K, P, G, Y, Si.depth, Di.depth, Si.csx, Si.csy, Di.csx, Di.csy);
    } else {
        name = launch_yuv_stack(c->stream, c->variant, L, L2, S, U.K, P, G, Si.depth, Di.depth, Si.csx, Si.csy, Di.csx, Di.csy, mix,
                                matte ? &A : nullptr, with_mtx ? &X : nullptr);
    }
    if (!name) return finish_launch(c, nullptr);
    const std::string full = std::string(name) + "[" + T.list + "]";
    return finish_launch(c, full.c_str());
}

int lutr_apply_yuv_stack(lutr_ctx *c, const lutr_yuv_params *p, const lutr_stage *stages, int nstages, const lutr_cdl *cdl, int w,
                         int h, int nframes, const lutr_planes *src, const lutr_planes *dst, int row0, int rows)
{
    return apply_yuv_stack(c, p, stages, nstages, cdl, nullptr, nullptr, false, nullptr, w, h, nframes, src, dst, row0, rows);
}

// ---- the stack with an RGB matrix stage: the same pass, the matrix kernels whatever the list
int lutr_apply_yuv_stack_matrix(lutr_ctx *c, const lutr_yuv_params *p, const lutr_stage *stages, int nstages, const lutr_cdl *cdl,
                                const lutr_rgb_matrix *mtx, int w, int h, int nframes, const lutr_planes *src,
                                const lutr_planes *dst, int row0, int rows)
{
    return apply_yuv_stack(c, p, stages, nstages, cdl, nullptr, nullptr, true, mtx, w, h, nframes, src, dst, row0, rows);
}

// The strength of the mix and matte entries: the scalar is read only without the array; a NaN is found by its bits (this file is
// built without honouring NaNs)
static int check_strength(float strength, const float *frame_strength)
{
    uint32_t bits;
    memcpy(&bits, &strength, sizeof bits);
    if (!frame_strength && ((bits & 0x7fffffffu) > 0x7f800000u || strength < 0.0f || strength > 1.0f)) {
        set_error("stack: strength %g outside [0, 1]", (double)strength);
        return LUTR_EINVAL;
    }
    return LUTR_OK;
}

// ---- the stack with a strength behind it: the same pass, the mix kernels whatever the strength
int lutr_apply_yuv_stack_mix(lutr_ctx *c, const lutr_yuv_params *p, const lutr_stage *stages, int nstages, const lutr_cdl *cdl,
                             float strength, const float *frame_strength, int w, int h, int nframes, const lutr_planes *src,
                             const lutr_planes *dst, int row0, int rows)
{
    if (const int rc = check_strength(strength, frame_strength)) return rc;
    const MixConsts M{frame_strength, frame_strength ? 1.0f : strength};
    return apply_yuv_stack(c, p, stages, nstages, cdl, &M, nullptr, false, nullptr, w, h, nframes, src, dst, row0, rows);
}

// ---- the stack with a matte scaling the strength per pixel: the same pass, the matte kernels whatever the matte
int lutr_apply_yuv_stack_matte(lutr_ctx *c, const lutr_yuv_params *p, const lutr_stage *stages, int nstages, const lutr_cdl *cdl,
                               float strength, const float *frame_strength, const lutr_matte *matte, int w, int h, int nframes,
                               const lutr_planes *src, const lutr_planes *dst, int row0, int rows)
{
    if (const int rc = check_strength(strength, frame_strength)) return rc;
    if (!matte || !matte->data) { set_error("stack: null matte"); return LUTR_EINVAL; }
    if (matte->depth < 8 || matte->depth > 16) { set_error("stack: matte depth %d outside 8..16", matte->depth); return LUTR_EINVAL; }
    if (matte->invert != 0 && matte->invert != 1) { set_error("stack: matte invert %d is neither 0 nor 1", matte->invert); return LUTR_EINVAL; }
    if (matte->frame_stride < 0) {
        set_error("stack: matte frame stride %lld is negative", (long long)matte->frame_stride);
        return LUTR_EINVAL;
    }
    const MixConsts M{frame_strength, frame_strength ? 1.0f : strength};
    return apply_yuv_stack(c, p, stages, nstages, cdl, &M, matte, false, nullptr, w, h, nframes, src, dst, row0, rows);
}

// ---- the stack on semi-planar sides: the same pass, each side in its own container, the semi kernels
int lutr_apply_yuv_stack_semi(lutr_ctx *c, const lutr_yuv_params *p, const lutr_stage *stages, int nstages, const lutr_cdl *cdl,
                              const lutr_yuv_layout *in_layout, const lutr_yuv_layout *out_layout, int w, int h, int nframes,
                              const lutr_planes *src, const lutr_planes *dst, int row0, int rows)
{
    if (!in_layout || !out_layout) { set_error("stack: null layout"); return LUTR_EINVAL; }
    if (!in_layout->semi && !out_layout->semi && !in_layout->swap && !out_layout->swap && !in_layout->shift && !out_layout->shift)
        return lutr_apply_yuv_stack(c, p, stages, nstages, cdl, w, h, nframes, src, dst, row0, rows);   // planar both ways: that call itself
    return apply_yuv_stack(c, p, stages, nstages, cdl, nullptr, nullptr, false, nullptr, w, h, nframes, src, dst, row0, rows, in_layout,
                           out_layout);
}

int lutr_apply_planar_rgb_lut1d(lutr_ctx *c, int depth, int w, int h, int nframes, const lutr_planes *src, const lutr_planes *dst,
                                int row0, int rows)
{
    int rc = check_common(c, LUTR_INTERP_NONE, LUTR_INTERP_NONE, w, h, nframes, src, dst, row0, rows);
    if (rc) return rc;
    if (!c->l1d_size) { set_error("no 1D LUT set on this context (call lutr_ctx_set_lut1d first)"); return LUTR_EINVAL; }
    if (depth < 8 || depth > 16) { set_error("unsupported depth %d", depth); return LUTR_EINVAL; }
    if (c->variant == VAR_VEC_LDS) { set_error("variant vec_lds: there is no LDS-window kernel for the lut1d pass"); return LUTR_EINVAL; }
    if (w == 0 || rows == 0 || nframes == 0) return LUTR_OK;
    if (const int rc = check_planes_set(src, dst)) return rc;
    if (depth > 8)
        for (int i = 0; i < 3; i++)
            if (!check_aligned(src->data[i], src->stride[i], src->frame_stride[i], nframes, 1) ||
                !check_aligned(dst->data[i], dst->stride[i], dst->frame_stride[i], nframes, 1)) {
                set_error("plane %d: 16-bit planes need 2-byte aligned rows", i);
                return LUTR_EINVAL;
            }
    HIP_TRY(hipSetDevice(c->device));
    L1dConsts C; PlaneSet P; FrameGeom G{w, h, row0, rows, nframes};
    if (const int rc = l1d_device_table(c, depth, &C)) return rc;
    fill_planes(&P, src, dst);
    return finish_launch(c, launch_rgb_l1d(c->stream, c->variant, C, P, G, depth));
}

// the first `nplanes` planes of a container's side, plane by plane: a base pointer, then the 16-bit alignment
static int check_container_planes(const Side &s, int nplanes, int nframes)
{
    for (int i = 0; i < nplanes; i++) {
        if (!s.pl->data[i]) { set_error("null %s plane %d", s.name, i); return LUTR_EINVAL; }
        if (const int rc = check_plane_aligned(s, i, nframes, "containers")) return rc;
    }
    return LUTR_OK;
}

// What a semi-planar and a packed side share: `noun` ("layout" | "packing") names the struct in the messages; the shift against
// the format's depth, then `bad_shape` (the side's own refusal of the format's subsampling, or nullptr -- it has always come
// between the two), then the `nplanes` planes the side has and their alignment.
static int check_container_side(const Side &s, const char *noun, int shift, int nplanes, int nframes, const char *bad_shape)
{
    if (s.depth <= 8 ? shift != 0 : (shift != 0 && shift != 16 - s.depth)) {
        if (s.depth <= 8) set_error("%s %s: an 8-bit container takes shift 0, not %d", s.name, noun, shift);
        else set_error("%s %s: shift is %d (16 - depth) or 0 at %d bit, not %d", s.name, noun, 16 - s.depth, s.depth, shift);
        return LUTR_EINVAL;
    }
    if (bad_shape) { set_error("%s %s: %s", s.name, noun, bad_shape); return LUTR_EINVAL; }
    return check_container_planes(s, nplanes, nframes);
}

// one side of lutr_apply_yuv_semi: the layout against the format, the planes it needs and their alignment
static int check_semi_side(const Side &s, const lutr_yuv_layout *y, int nframes)
{
    if ((y->semi != 0 && y->semi != 1) || (y->swap != 0 && y->swap != 1)) {
        set_error("%s layout: semi and swap are 0 or 1 (got %d, %d)", s.name, y->semi, y->swap);
        return LUTR_EINVAL;
    }
    if (y->swap && !y->semi) { set_error("%s layout: swap needs a semi-planar side", s.name); return LUTR_EINVAL; }
    return check_container_side(s, "layout", y->shift, y->semi ? 2 : 3, nframes,
                                y->semi && s.csx != 1 ? "semi-planar frames are 4:2:0 or 4:2:2" : nullptr);
}

int lutr_apply_yuv_semi(lutr_ctx *c, const lutr_yuv_params *p, int interp, const lutr_yuv_layout *in_layout,
                        const lutr_yuv_layout *out_layout, int w, int h, int nframes, const lutr_planes *src,
                        const lutr_planes *dst, int row0, int rows)
{
    int rc = check_common(c, interp, LUTR_INTERP_NEAREST, w, h, nframes, src, dst, row0, rows);
    if (rc) return rc;
    if (!p || !in_layout || !out_layout) { set_error("null yuv params or layout"); return LUTR_EINVAL; }
    if (!in_layout->semi && !out_layout->semi && !in_layout->swap && !out_layout->swap && !in_layout->shift && !out_layout->shift)
        return lutr_apply_yuv(c, p, interp, w, h, nframes, src, dst, row0, rows);      // planar both ways: that call itself
    YuvConsts K;
    rc = make_yuv_consts(*p, &K);
    if (rc) return rc;
    if (const int rc = check_semi_side(planar_side("source", src, p->fmt_in), in_layout, nframes)) return rc;
    if (const int rc = check_semi_side(planar_side("destination", dst, p->fmt_out), out_layout, nframes)) return rc;
    const int csx = LUTR_FMT_CSX(p->fmt_in), csy = LUTR_FMT_CSY(p->fmt_in);
    if (csx != 1) { set_error("a shifted planar container is taken at 4:2:0 / 4:2:2 only"); return LUTR_EINVAL; }
    if (const int rc = check_row_blocks(row0, rows, h, 1 << csy, "chroma block height")) return rc;
    if (w == 0 || rows == 0 || nframes == 0) return LUTR_OK;
    HIP_TRY(hipSetDevice(c->device));
    LutConsts L; PlaneSet P; FrameGeom G{w, h, row0, rows, nframes};
    if (const int rc = fill_lut(&L, c, p->lut_depth)) return rc;
    fill_planes(&P, src, dst);
    if (in_layout->semi) clear_planes(&P, true, 2);
    if (out_layout->semi) clear_planes(&P, false, 2);
    const SemiArgs A{in_layout->semi, in_layout->swap, in_layout->shift, out_layout->semi, out_layout->swap, out_layout->shift};
    return finish_launch(c, launch_yuv_semi(c->stream, c->variant, L, K, P, G, A, LUTR_FMT_DEPTH(p->fmt_in),
                                            LUTR_FMT_DEPTH(p->fmt_out), csy, interp));
}


// one side of lutr_apply_yuv_packed: the packing against the format, the planes it needs and their alignment
static int check_packed_side(const Side &s, const lutr_yuv_packing *y, int nframes)
{
    if (y->packed != 0 && y->packed != 1) { set_error("%s packing: packed is 0 or 1 (got %d)", s.name, y->packed); return LUTR_EINVAL; }
    if (y->order < LUTR_PK_YUYV || y->order > LUTR_PK_YVYU) {
        set_error("%s packing: order is 0 (yuyv), 1 (uyvy) or 2 (yvyu), not %d", s.name, y->order);
        return LUTR_EINVAL;
    }
    if (!y->packed && (y->order || y->shift)) { set_error("%s packing: a planar side takes order 0 and shift 0", s.name); return LUTR_EINVAL; }
    return check_container_side(s, "packing", y->shift, y->packed ? 1 : 3, nframes,
                                y->packed && !(s.csx == 1 && s.csy == 0) ? "packed frames are 4:2:2" : nullptr);
}

// one side of lutr_apply_yuv_packed as a value: a packed side is one plane of whole groups of two pixels, four samples each
static Side packed_side(const char *name, const lutr_planes *pl, int fmt, const lutr_yuv_packing *y, int w)
{
    Side s = planar_side(name, pl, fmt);
    s.packed = y->packed != 0;
    s.packed_row = 4ll * ((w + 1) >> 1) * (s.depth > 8 ? 2 : 1);
    return s;
}

int lutr_apply_yuv_packed(lutr_ctx *c, const lutr_yuv_params *p, int interp, const lutr_yuv_packing *in,
                          const lutr_yuv_packing *out, int w, int h, int nframes, const lutr_planes *src,
                          const lutr_planes *dst, int row0, int rows)
{
    int rc = check_common(c, interp, LUTR_INTERP_NEAREST, w, h, nframes, src, dst, row0, rows);
    if (rc) return rc;
    if (!p || !in || !out) { set_error("null yuv params or packing"); return LUTR_EINVAL; }
    if (!in->packed && !out->packed && !in->order && !out->order && !in->shift && !out->shift)
        return lutr_apply_yuv_xsub(c, p, interp, LUTR_DITHER_NONE, w, h, nframes, src, dst, row0, rows);   // planar both ways: that call itself
    YuvConsts K;
    rc = make_yuv_consts_xsub(*p, &K);           // (one layout on both sides: lutr_apply_yuv's own constants)
    if (rc) return rc;
    const int ocsx = LUTR_FMT_CSX(p->fmt_out), ocsy = LUTR_FMT_CSY(p->fmt_out);
    if (!(LUTR_FMT_CSX(p->fmt_in) == 1 && LUTR_FMT_CSY(p->fmt_in) == 0)) {
        set_error(out->packed ? "a packed destination takes a 4:2:2 source (no subsampling change into a packed frame)"
                              : "the source of a packed call is 4:2:2");
        return LUTR_EINVAL;
    }
    if (!((ocsx == 1 && ocsy <= 1) || (ocsx == 0 && ocsy == 0))) { set_error("the destination is 4:2:2, 4:2:0 or 4:4:4"); return LUTR_EINVAL; }
    const Side S = packed_side("source", src, p->fmt_in, in, w), D = packed_side("destination", dst, p->fmt_out, out, w);
    const FrameGeom G{w, h, row0, rows, nframes};
    if (const int rc = check_packed_side(S, in, nframes)) return rc;
    if (const int rc = check_packed_side(D, out, nframes)) return rc;
    if (const int rc = check_row_blocks(row0, rows, h, 1 << ocsy, "chroma block height")) return rc;
    if (w == 0 || rows == 0 || nframes == 0) return LUTR_OK;
    const bool same = in->packed && out->packed && in->order == out->order && in->shift == out->shift && S.depth == D.depth;
    if (const int rc = check_in_place("a packed 4:2:2 call between different buffers or containers", same, S, D, G)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    LutConsts L; PlaneSet P;
    if (const int rc = fill_lut(&L, c, p->lut_depth)) return rc;
    fill_planes(&P, src, dst);
    if (in->packed) clear_planes(&P, true, 1);
    if (out->packed) clear_planes(&P, false, 1);
    const PkArgs A{in->packed, in->order == LUTR_PK_UYVY, in->order == LUTR_PK_YVYU, in->shift,
                   out->packed, out->order == LUTR_PK_UYVY, out->order == LUTR_PK_YVYU, out->shift};
    return finish_launch(c, launch_yuv_packed(c->stream, c->variant, L, K, P, G, A, LUTR_FMT_DEPTH(p->fmt_in),
                                              LUTR_FMT_DEPTH(p->fmt_out), ocsx, ocsy, interp));
}

// bytes of a v210 row that hold groups: 16 for every six luma samples, the last group whole
static long long v210_row_bytes(int w) { return 16ll * ((w + 5) / 6); }

// one side of lutr_apply_yuv_v210: a v210 side's format, plane, alignment and stride; a planar side's three planes
// (`fmt`: the side's whole format code, as the message prints it)
static int check_v210_side(const Side &s, int fmt, int w, int nframes)
{
    if (!s.packed) return check_container_planes(s, 3, nframes);
    const lutr_planes *pl = s.pl;
    if (fmt != LUTR_FMT(10, 1, 0)) { set_error("%s: a v210 frame is 10-bit 4:2:2 (format 0x%x)", s.name, fmt); return LUTR_EINVAL; }
    if (!pl->data[0]) { set_error("null %s plane 0", s.name); return LUTR_EINVAL; }
    if (!check_aligned(pl->data[0], pl->stride[0], pl->frame_stride[0], nframes, 3)) {
        set_error("%s: v210 rows are 32-bit words: base, stride and frame stride must be 4-byte aligned", s.name);
        return LUTR_EINVAL;
    }
    const long long st = pl->stride[0] < 0 ? -(long long)pl->stride[0] : (long long)pl->stride[0];
    if (st < s.packed_row) {
        set_error("%s: a v210 row of %d samples takes %lld bytes, the stride is %lld", s.name, w, s.packed_row, (long long)pl->stride[0]);
        return LUTR_EINVAL;
    }
    return LUTR_OK;
}

// one side of lutr_apply_yuv_v210 as a value
static Side v210_side(const char *name, const lutr_planes *pl, int fmt, int v210, int w)
{
    Side s = planar_side(name, pl, fmt);
    s.packed = v210 != 0;
    s.packed_row = v210_row_bytes(w);
    return s;
}

int lutr_apply_yuv_v210(lutr_ctx *c, const lutr_yuv_params *p, int interp, int in_v210, int out_v210, int w, int h, int nframes,
                        const lutr_planes *src, const lutr_planes *dst, int row0, int rows)
{
    int rc = check_common(c, interp, LUTR_INTERP_NEAREST, w, h, nframes, src, dst, row0, rows);
    if (rc) return rc;
    if (!p) { set_error("null yuv params"); return LUTR_EINVAL; }
    if ((in_v210 != 0 && in_v210 != 1) || (out_v210 != 0 && out_v210 != 1)) {
        set_error("in_v210 and out_v210 are 0 or 1 (got %d, %d)", in_v210, out_v210);
        return LUTR_EINVAL;
    }
    if (!in_v210 && !out_v210) {
        set_error("neither side is v210: planar frames on both sides are lutr_apply_yuv / lutr_apply_yuv_xsub");
        return LUTR_EINVAL;
    }
    // (the container's own refusals first: they name the side; then the constants, which check depths, matrices and ranges)
    const Side S = v210_side("source", src, p->fmt_in, in_v210, w), D = v210_side("destination", dst, p->fmt_out, out_v210, w);
    const FrameGeom G{w, h, row0, rows, nframes};
    if (const int rc = check_v210_side(S, p->fmt_in, w, nframes)) return rc;
    if (!(S.csx == 1 && S.csy == 0)) {
        set_error("a v210 destination takes a 4:2:2 source (no subsampling change into a v210 frame)");
        return LUTR_EINVAL;
    }
    if (const int rc = check_v210_side(D, p->fmt_out, w, nframes)) return rc;
    YuvConsts K;
    rc = make_yuv_consts_xsub(*p, &K);           // (one layout on both sides: lutr_apply_yuv's own constants)
    if (rc) return rc;
    const int ocsx = LUTR_FMT_CSX(p->fmt_out), ocsy = LUTR_FMT_CSY(p->fmt_out);
    if (!((ocsx == 1 && ocsy <= 1) || (ocsx == 0 && ocsy == 0))) { set_error("the destination is 4:2:2, 4:2:0 or 4:4:4"); return LUTR_EINVAL; }
    if (const int rc = check_row_blocks(row0, rows, h, 1 << ocsy, "chroma block height")) return rc;
    if (w == 0 || rows == 0 || nframes == 0) return LUTR_OK;
    if (const int rc = check_in_place("a v210 call between different buffers or containers", in_v210 && out_v210, S, D, G)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    LutConsts L; PlaneSet P;
    if (const int rc = fill_lut(&L, c, p->lut_depth)) return rc;
    fill_planes(&P, src, dst);
    if (in_v210) clear_planes(&P, true, 1);
    if (out_v210) clear_planes(&P, false, 1);
    const V210Args A{in_v210, out_v210};
    return finish_launch(c, launch_yuv_v210(c->stream, c->variant, L, K, P, G, A, LUTR_FMT_DEPTH(p->fmt_in),
                                            LUTR_FMT_DEPTH(p->fmt_out), ocsx, ocsy, interp));
}

// ---- the stage stack on packed 4:2:2 and v210 frames: lutr_apply_yuv_stack's list, constants and resources between
// the container checks of lutr_apply_yuv_packed / lutr_apply_yuv_v210 and the kernels of lutr_pkstack.hip.
// `in` / `out`: the packings of lutr_apply_yuv_stack_packed; null for lutr_apply_yuv_stack_v210, whose sides are in_v210 / out_v210.
static int apply_yuv_stack_capture(lutr_ctx *c, const lutr_yuv_params *p, const lutr_stage *stages, int nstages, const lutr_cdl *cdl,
                                   const lutr_yuv_packing *in, const lutr_yuv_packing *out, int in_v210, int out_v210, int w, int h,
                                   int nframes, const lutr_planes *src, const lutr_planes *dst, int row0, int rows)
{
    if (!c || !src || !dst) { set_error("null argument"); return LUTR_EINVAL; }
    StackList T;
    if (const int rc = stack_check_list(c, stages, nstages, cdl, false, nullptr, &T)) return rc;
    if (const int rc = check_geometry(w, h, nframes, row0, rows)) return rc;
    if (const int rc = stack_compile_steps(c, stages, nstages, &T)) return rc;
    if (!p) { set_error("null yuv params"); return LUTR_EINVAL; }
    UnionCall U; const FrameGeom G{w, h, row0, rows, nframes};
    U.nsides = 2;
    U.lut_depth = p->lut_depth;
    const int ocsx = LUTR_FMT_CSX(p->fmt_out), ocsy = LUTR_FMT_CSY(p->fmt_out);
    const bool src_422 = LUTR_FMT_CSX(p->fmt_in) == 1 && LUTR_FMT_CSY(p->fmt_in) == 0;
    if (in) {
        // lutr_apply_yuv_packed's order: the constants, the layouts, then each side's packing
        if (const int rc = make_yuv_consts_xsub(*p, &U.K)) return rc;
        if (!src_422) {
            set_error(out->packed ? "a packed destination takes a 4:2:2 source (no subsampling change into a packed frame)"
                                  : "the source of a packed call is 4:2:2");
            return LUTR_EINVAL;
        }
        if (!((ocsx == 1 && ocsy <= 1) || (ocsx == 0 && ocsy == 0))) { set_error("the destination is 4:2:2, 4:2:0 or 4:4:4"); return LUTR_EINVAL; }
        U.side[0] = packed_side("source", src, p->fmt_in, in, w);
        U.side[1] = packed_side("destination", dst, p->fmt_out, out, w);
        if (const int rc = check_packed_side(U.side[0], in, nframes)) return rc;
        if (const int rc = check_packed_side(U.side[1], out, nframes)) return rc;
    } else {
        // lutr_apply_yuv_v210's order: the container's own refusals first, then the constants
        U.side[0] = v210_side("source", src, p->fmt_in, in_v210, w);
        U.side[1] = v210_side("destination", dst, p->fmt_out, out_v210, w);
        if (const int rc = check_v210_side(U.side[0], p->fmt_in, w, nframes)) return rc;
        if (!src_422) {
            set_error("a v210 destination takes a 4:2:2 source (no subsampling change into a v210 frame)");
            return LUTR_EINVAL;
        }
        if (const int rc = check_v210_side(U.side[1], p->fmt_out, w, nframes)) return rc;
        if (const int rc = make_yuv_consts_xsub(*p, &U.K)) return rc;
        if (!((ocsx == 1 && ocsy <= 1) || (ocsx == 0 && ocsy == 0))) { set_error("the destination is 4:2:2, 4:2:0 or 4:4:4"); return LUTR_EINVAL; }
    }
    const Side &Si = U.side[0], &Di = U.side[1];
    if (const int rc = union_rules(c, U, G, "stack", "the stack pass")) return rc;
    if (w == 0 || rows == 0 || nframes == 0) return LUTR_OK;
    if (const int rc = check_sides_disjoint("the stack pass", true, Si, Di, G)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    LutConsts L{}, L2{}; StackConsts S{}; MtxConsts X{}; PlaneSet P;
    if (const int rc = stack_device_consts(c, T, cdl, nullptr, p->lut_depth, &L, &L2, &S, &X)) return rc;
    fill_planes(&P, src, dst);
    if (Si.packed) clear_planes(&P, true, 1);
    if (Di.packed) clear_planes(&P, false, 1);
    const char *name;
    if (in) {
        const PkArgs A{in->packed, in->order == LUTR_PK_UYVY, in->order == LUTR_PK_YVYU, in->shift,
                       out->packed, out->order == LUTR_PK_UYVY, out->order == LUTR_PK_YVYU, out->shift};
        name = launch_yuv_stack_packed(c->stream, c->variant, L, L2, S, U.K, P, G, A, Si.depth, Di.depth, ocsx, ocsy);
    } else {
        const V210Args A{in_v210, out_v210};
        name = launch_yuv_stack_v210(c->stream, c->variant, L, L2, S, U.K, P, G, A, Si.depth, Di.depth, ocsx, ocsy);
    }
    if (!name) return finish_launch(c, nullptr);
    const std::string full = std::string(name) + "[" + T.list + "]";
    return finish_launch(c, full.c_str());
}

int lutr_apply_yuv_stack_packed(lutr_ctx *c, const lutr_yuv_params *p, const lutr_stage *stages, int nstages, const lutr_cdl *cdl,
                                const lutr_yuv_packing *in, const lutr_yuv_packing *out, int w, int h, int nframes,
                                const lutr_planes *src, const lutr_planes *dst, int row0, int rows)
{
    if (!in || !out) { set_error("stack: null packing"); return LUTR_EINVAL; }
    if (!in->packed && !out->packed && !in->order && !out->order && !in->shift && !out->shift)
        return lutr_apply_yuv_stack(c, p, stages, nstages, cdl, w, h, nframes, src, dst, row0, rows);   // planar both ways: that call itself
    return apply_yuv_stack_capture(c, p, stages, nstages, cdl, in, out, 0, 0, w, h, nframes, src, dst, row0, rows);
}

int lutr_apply_yuv_stack_v210(lutr_ctx *c, const lutr_yuv_params *p, const lutr_stage *stages, int nstages, const lutr_cdl *cdl,
                              int in_v210, int out_v210, int w, int h, int nframes, const lutr_planes *src, const lutr_planes *dst,
                              int row0, int rows)
{
    if ((in_v210 != 0 && in_v210 != 1) || (out_v210 != 0 && out_v210 != 1)) {
        set_error("in_v210 and out_v210 are 0 or 1 (got %d, %d)", in_v210, out_v210);
        return LUTR_EINVAL;
    }
    if (!in_v210 && !out_v210)
        return lutr_apply_yuv_stack(c, p, stages, nstages, cdl, w, h, nframes, src, dst, row0, rows);   // planar both ways: that call itself
    return apply_yuv_stack_capture(c, p, stages, nstages, cdl, nullptr, nullptr, in_v210, out_v210, w, h, nframes, src, dst, row0, rows);
}

// ---- the RGB side of lutr_apply_rgb_to_yuv / lutr_apply_yuv_to_rgb (`side`: "source" | "destination"): gbrp planes at lut_depth
// (kind 0), or the packed format `kind`, whose depth lut_depth must be
static int rgb_side_layout(int kind, int lut_depth, const char *side, RgbLayout *Y)
{
    *Y = RgbLayout{1, lut_depth > 8, 0, 0, 0};
    if (!kind) return LUTR_OK;
    PackedFmt f;
    if (const int rc = decode_packed(kind, &f)) return rc;
    if (lut_depth != f.bits) { set_error("lut_depth %d must be the packed %s's depth %d", lut_depth, side, f.bits); return LUTR_EINVAL; }
    *Y = RgbLayout{f.nc, f.bits == 16, f.ro, f.go, f.bo};
    return LUTR_OK;
}

// ... and behind the empty call: the image, or the three planes, must be there (a packed image aligned to its samples).  Its streams
// go into the source (src = true) or destination half of P in R, G, B order -- gbrp planes are G, B, R, and a null one is reported
// under its own number -- and their byte ranges into sp; returns how many ranges differ (1 for an image) through *n.
static int rgb_side_streams(const RgbLayout &Y, const lutr_planes *planar, const lutr_packed *packed, const FrameGeom &G, bool src,
                            PlaneSet *P, Span sp[3], int *n)
{
    const bool image = Y.step > 1;
    if (image) {
        if (!packed->data) { set_error("null image"); return LUTR_EINVAL; }
        if (Y.wide && !check_aligned(packed->data, packed->stride, packed->frame_stride, G.nframes, 1)) {
            set_error("16-bit packed formats need 2-byte aligned rows");
            return LUTR_EINVAL;
        }
    }
    for (int k = 0; k < 3; k++) {
        const int f = kGbrpToRgb[k];
        const void *data = image ? packed->data : planar->data[f];
        const long long stride = image ? packed->stride : planar->stride[f];
        const long long fstride = image ? packed->frame_stride : planar->frame_stride[f];
        if (!data) { set_error("null plane %d", f); return LUTR_EINVAL; }
        if (src) { P->s[k] = (const uint8_t *)data; P->ss[k] = stride; P->sfs[k] = fstride; }
        else { P->d[k] = (uint8_t *)data; P->ds[k] = stride; P->dfs[k] = fstride; }
        sp[k] = plane_span(data, stride, fstride, G.h, (long long)G.w * Y.step * (Y.wide ? 2 : 1), G.nframes);
    }
    *n = image ? 1 : 3;
    return LUTR_OK;
}

int lutr_apply_rgb_to_yuv(lutr_ctx *c, const lutr_yuv_params *p, int interp, int dither, int src_kind, int w, int h, int nframes,
                          const lutr_planes *src_planar, const lutr_packed *src_packed, const lutr_planes *dst, int row0, int rows)
{
    if (const int rc = check_dither(dither)) return rc;
    const void *src = src_kind ? (const void *)src_packed : (const void *)src_planar;
    int rc = check_common(c, interp, LUTR_INTERP_NONE, w, h, nframes, src, dst, row0, rows);
    if (rc) return rc;
    if (!p) { set_error("null yuv params"); return LUTR_EINVAL; }
    YuvConsts K;
    rc = make_yuv_consts_rgb2yuv(*p, &K);
    if (rc) return rc;
    const int dl = p->lut_depth;
    const Side D = planar_side("destination", dst, p->fmt_out);
    RgbLayout Y;
    if (const int rc = rgb_side_layout(src_kind, dl, "source", &Y)) return rc;
    if (const int rc = check_dither_rows(dither, row0, rows, h)) return rc;
    if (const int rc = check_row_blocks(row0, rows, h, 1 << D.csy, "output chroma block height")) return rc;
    if (w == 0 || rows == 0 || nframes == 0) return LUTR_OK;
    PlaneSet P{}; Span ss[3], ds[3]; int ns; const FrameGeom G{w, h, row0, rows, nframes};
    if (const int rc = rgb_side_streams(Y, src_planar, src_packed, G, true, &P, ss, &ns)) return rc;
    if (const int rc = check_planes_set(dst, nullptr)) return rc;
    for (int i = 0; i < 3; i++) { P.d[i] = (uint8_t *)dst->data[i]; P.ds[i] = dst->stride[i]; P.dfs[i] = dst->frame_stride[i]; }
    // a chroma sample is written by one thread while another may still read the pixels of its block: no in-place operation
    side_spans(D, G, ds);
    if (const int rc = check_disjoint("RGB -> YUV", false, ss, ns, ds, 3)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    LutConsts L{};
    if (interp != LUTR_INTERP_NONE)
        if (const int rc = fill_lut(&L, c, dl)) return rc;
    if (dither == LUTR_DITHER_NONE)
        return finish_launch(c, launch_rgb2yuv(c->stream, c->variant, L, K, P, Y, G, D.depth, D.csx, D.csy, interp));
    if (dither == LUTR_DITHER_BLUE_NOISE) {
        const float *bn;
        if (const int rc = bn_table(c, &bn)) return rc;
        return finish_launch(c, launch_rgb2yuv_bn(c->stream, c->variant, L, K, P, Y, G, bn, D.depth, D.csx, D.csy, interp));
    }
    FloatPlanes F;
    if (const int rc = dither_scratch(c, G, D.csx, D.csy, &F)) return rc;
    return finish_launch(c, launch_rgb2yuv_dither(c->stream, L, K, P, Y, G, F, D.depth, D.csx, D.csy, interp));
}

// ---- the stage stack on an RGB source: lutr_apply_rgb_to_yuv's source through the list of
// lutr_apply_yuv_stack_matrix into planar YUV (dst_kind 0) or three gbrp planes at the source's depth (dst_kind = that depth)
int lutr_apply_rgb_stack(lutr_ctx *c, const lutr_yuv_params *p, const lutr_stage *stages, int nstages, const lutr_cdl *cdl,
                         const lutr_rgb_matrix *mtx, int src_kind, int w, int h, int nframes, const lutr_planes *src_planar,
                         const lutr_packed *src_packed, int dst_kind, const lutr_planes *dst, int row0, int rows)
{
    const void *src = src_kind ? (const void *)src_packed : (const void *)src_planar;
    if (!c || !src || !dst) { set_error("null argument"); return LUTR_EINVAL; }
    StackList T;
    if (const int rc = stack_check_list(c, stages, nstages, cdl, true, mtx, &T)) return rc;
    if (const int rc = check_geometry(w, h, nframes, row0, rows)) return rc;
    if (const int rc = stack_compile_steps(c, stages, nstages, &T)) return rc;
    const bool yuv = dst_kind == LUTR_RGB_STACK_YUV;
    if (!yuv && (dst_kind < 8 || dst_kind > 16)) {
        set_error("rgb stack: destination kind %d is neither LUTR_RGB_STACK_YUV nor a gbrp depth in 8..16", dst_kind);
        return LUTR_EINVAL;
    }
    if (yuv && !p) { set_error("null yuv params"); return LUTR_EINVAL; }
    YuvConsts K{};
    if (yuv)
        if (const int rc = make_yuv_consts_rgb2yuv(*p, &K)) return rc;
    // the depth of the list: the YUV call's lut_depth, which a packed source must have; else the gbrp destination's, likewise
    const int dl = yuv ? p->lut_depth : dst_kind;
    RgbLayout Y;
    if (!yuv && src_kind) {
        PackedFmt f;
        if (const int rc = decode_packed(src_kind, &f)) return rc;
        if (f.bits != dl) {
            set_error("rgb stack: a gbrp destination of %d bits from a source of %d bits: the planar RGB destination has the source's depth",
                      dl, f.bits);
            return LUTR_EINVAL;
        }
    }
    if (const int rc = rgb_side_layout(src_kind, dl, "source", &Y)) return rc;
    const Side D = yuv ? planar_side("destination", dst, p->fmt_out) : Side{};
    const int ocsx = yuv ? D.csx : 0, ocsy = yuv ? D.csy : 0;
    if (c->variant == VAR_VEC_LDS) {
        set_error("variant vec_lds: there is no LDS-window kernel for the RGB stack pass");
        return LUTR_EINVAL;
    }
    if (const int rc = check_row_blocks(row0, rows, h, 1 << ocsy, "output chroma block height")) return rc;
    if (w == 0 || rows == 0 || nframes == 0) return LUTR_OK;
    PlaneSet P{}; Span ss[3], ds[3]; int ns; const FrameGeom G{w, h, row0, rows, nframes};
    if (const int rc = rgb_side_streams(Y, src_planar, src_packed, G, true, &P, ss, &ns)) return rc;
    if (const int rc = check_planes_set(dst, nullptr)) return rc;
    if (yuv) {
        for (int i = 0; i < 3; i++) { P.d[i] = (uint8_t *)dst->data[i]; P.ds[i] = dst->stride[i]; P.dfs[i] = dst->frame_stride[i]; }
        // a chroma sample is written by one thread while another may still read the pixels of its block: no in-place operation
        side_spans(D, G, ds);
        if (const int rc = check_disjoint("the RGB stack pass", false, ss, ns, ds, 3)) return rc;
    } else {
        const RgbLayout Yd{1, dl > 8, 0, 0, 0};
        int nd;
        if (const int rc = rgb_side_streams(Yd, dst, nullptr, G, false, &P, ds, &nd)) return rc;
        if (Yd.wide)
            for (int i = 0; i < 3; i++)
                if (!check_aligned(dst->data[i], dst->stride[i], dst->frame_stride[i], nframes, 1)) {
                    set_error("plane %d: 16-bit planes need 2-byte aligned rows", i);
                    return LUTR_EINVAL;
                }
        // A sample is read and written by the same lane: plane k of the destination may be plane k of a planar source, row for
        // row.  Any other overlap would let a thread's stores land on samples another thread has yet to read.
        bool same = !src_kind;
        for (int k = 0; k < 3 && same; k++) same = P.s[k] == P.d[k] && P.ss[k] == P.ds[k] && (nframes == 1 || P.sfs[k] == P.dfs[k]);
        if (!same)
            if (const int rc = check_disjoint("an RGB stack call between different buffers", false, ss, ns, ds, 3)) return rc;
    }
    if (Y.step == 1 && Y.wide)
        for (int i = 0; i < 3; i++)
            if (!check_aligned(src_planar->data[i], src_planar->stride[i], src_planar->frame_stride[i], nframes, 1)) {
                set_error("plane %d: 16-bit planes need 2-byte aligned rows", i);
                return LUTR_EINVAL;
            }
    HIP_TRY(hipSetDevice(c->device));
    LutConsts L{}, L2{}; StackConsts S{}; MtxConsts X{};
    if (const int rc = stack_device_consts(c, T, cdl, mtx, dl, &L, &L2, &S, &X)) return rc;
    const char *name = launch_rgb_stack(c->stream, c->variant, L, L2, S, X, K, P, Y, G, yuv ? SINK_YUV : SINK_RGB, yuv ? D.depth : dl,
                                        ocsx, ocsy);
    if (!name) return finish_launch(c, nullptr);
    const std::string full = std::string(name) + "[" + T.list + "]";
    return finish_launch(c, full.c_str());
}

// lutr_apply_yuv_to_rgb and lutr_apply_yuv_stack_to_rgb behind their own first checks: the constants, the
// two sides, the row rule, the plane and overlap checks.  `what`: the pass as the overlap message names it.  *empty: nothing to do.
struct Yuv2RgbCall { YuvConsts K; Side S; RgbLayout Y; PlaneSet P; FrameGeom G; bool empty; };

static int yuv2rgb_open(const lutr_yuv_params *p, int dst_kind, int w, int h, int nframes, const lutr_planes *src,
                        const lutr_planes *dst_planar, const lutr_packed *dst_packed, int row0, int rows, const char *what,
                        Yuv2RgbCall *u)
{
    if (!p) { set_error("null yuv params"); return LUTR_EINVAL; }
    if (const int rc = make_yuv_consts_yuv2rgb(*p, &u->K)) return rc;
    u->S = planar_side("source", src, p->fmt_in);
    if (const int rc = rgb_side_layout(dst_kind, p->lut_depth, "destination", &u->Y)) return rc;
    if (const int rc = check_row_blocks(row0, rows, h, 1 << u->S.csy, "chroma block height")) return rc;
    u->G = FrameGeom{w, h, row0, rows, nframes};
    u->P = PlaneSet{};
    u->empty = w == 0 || rows == 0 || nframes == 0;
    if (u->empty) return LUTR_OK;
    if (const int rc = check_planes_set(src, nullptr)) return rc;
    Span ss[3], ds[3]; int nd;
    for (int i = 0; i < 3; i++) { u->P.s[i] = (const uint8_t *)src->data[i]; u->P.ss[i] = src->stride[i]; u->P.sfs[i] = src->frame_stride[i]; }
    if (const int rc = rgb_side_streams(u->Y, dst_planar, dst_packed, u->G, false, &u->P, ds, &nd)) return rc;
    // the two sides differ in size and layout: a thread's stores would land on samples another thread has yet to read
    side_spans(u->S, u->G, ss);
    return check_disjoint(what, true, ss, 3, ds, nd);
}

int lutr_apply_yuv_to_rgb(lutr_ctx *c, const lutr_yuv_params *p, int interp, int dst_kind, int w, int h, int nframes,
                          const lutr_planes *src, const lutr_planes *dst_planar, const lutr_packed *dst_packed, int row0, int rows)
{
    const void *dst = dst_kind ? (const void *)dst_packed : (const void *)dst_planar;
    if (const int rc = check_common(c, interp, LUTR_INTERP_NONE, w, h, nframes, src, dst, row0, rows)) return rc;
    Yuv2RgbCall U;
    if (const int rc = yuv2rgb_open(p, dst_kind, w, h, nframes, src, dst_planar, dst_packed, row0, rows, "YUV -> RGB", &U)) return rc;
    if (U.empty) return LUTR_OK;
    HIP_TRY(hipSetDevice(c->device));
    LutConsts L{};
    if (interp != LUTR_INTERP_NONE)
        if (const int rc = fill_lut(&L, c, p->lut_depth)) return rc;
    return finish_launch(c, launch_yuv2rgb(c->stream, c->variant, L, U.K, U.P, U.Y, U.G, U.S.depth, U.S.csx, U.S.csy, interp));
}

// ---- the stage stack from a YUV source into an RGB frame: lutr_apply_yuv_to_rgb's two sides with the list of
// lutr_apply_rgb_stack between the conversion and the stores
int lutr_apply_yuv_stack_to_rgb(lutr_ctx *c, const lutr_yuv_params *p, const lutr_stage *stages, int nstages, const lutr_cdl *cdl,
                                const lutr_rgb_matrix *mtx, int dst_kind, int w, int h, int nframes, const lutr_planes *src,
                                const lutr_planes *dst_planar, const lutr_packed *dst_packed, int row0, int rows)
{
    const void *dst = dst_kind ? (const void *)dst_packed : (const void *)dst_planar;
    if (!c || !src || !dst) { set_error("null argument"); return LUTR_EINVAL; }
    StackList T;
    if (const int rc = stack_check_list(c, stages, nstages, cdl, true, mtx, &T)) return rc;
    if (const int rc = check_geometry(w, h, nframes, row0, rows)) return rc;
    if (const int rc = stack_compile_steps(c, stages, nstages, &T)) return rc;
    if (c->variant == VAR_VEC_LDS) {
        set_error("variant vec_lds: there is no LDS-window kernel for the YUV -> RGB stack pass");
        return LUTR_EINVAL;
    }
    Yuv2RgbCall U;
    if (const int rc = yuv2rgb_open(p, dst_kind, w, h, nframes, src, dst_planar, dst_packed, row0, rows, "the YUV -> RGB stack pass", &U))
        return rc;
    if (U.empty) return LUTR_OK;
    HIP_TRY(hipSetDevice(c->device));
    LutConsts L{}, L2{}; StackConsts S{}; MtxConsts X{};
    if (const int rc = stack_device_consts(c, T, cdl, mtx, p->lut_depth, &L, &L2, &S, &X)) return rc;
    const char *name = launch_yuv2rgb_stack(c->stream, c->variant, L, L2, S, X, U.K, U.P, U.Y, U.G, U.S.depth, U.S.csx, U.S.csy);
    if (!name) return finish_launch(c, nullptr);
    const std::string full = std::string(name) + "[" + T.list + "]";
    return finish_launch(c, full.c_str());
}

// gbrpf32 planes hold 4-byte samples: base pointers, row strides and (batches) frame strides must be multiples of 4
static int check_float_planes(const lutr_planes *a, int nframes, const char *what)
{
    for (int i = 0; i < 3; i++)
        if (!check_aligned(a->data[i], a->stride[i], a->frame_stride[i], nframes, 3)) {
            set_error("float planes need 4-byte aligned rows: %s plane %d (pointer, stride and frame stride must be multiples of 4)", what, i);
            return LUTR_EINVAL;
        }
    return LUTR_OK;
}

int lutr_apply_planar_rgb_f32(lutr_ctx *c, int interp, int w, int h, int nframes, const lutr_planes *src, const lutr_planes *dst,
                              int row0, int rows)
{
    int rc = check_common(c, interp, LUTR_INTERP_NEAREST, w, h, nframes, src, dst, row0, rows);
    if (rc) return rc;
    if (w == 0 || rows == 0 || nframes == 0) return LUTR_OK;
    if (const int rc = check_planes_set(src, dst)) return rc;
    if (const int rc = check_float_planes(src, nframes, "source")) return rc;
    if (const int rc = check_float_planes(dst, nframes, "destination")) return rc;
    HIP_TRY(hipSetDevice(c->device));
    LutConsts L; FloatPre Q; PlaneSet P; FrameGeom G{w, h, row0, rows, nframes};
    if (const int rc = fill_lut_float(&L, &Q, c, true)) return rc;
    fill_planes(&P, src, dst);
    return finish_launch(c, launch_rgbf(c->stream, c->variant, L, Q, gbrp_to_rgb(P), G, interp));
}

int lutr_apply_rgbf_to_yuv(lutr_ctx *c, const lutr_yuv_params *p, int interp, int dither, int w, int h, int nframes,
                           const lutr_planes *src, const lutr_planes *dst, int row0, int rows)
{
    if (const int rc = check_dither(dither)) return rc;
    int rc = check_common(c, interp, LUTR_INTERP_NONE, w, h, nframes, src, dst, row0, rows);
    if (rc) return rc;
    if (!p) { set_error("null yuv params"); return LUTR_EINVAL; }
    if (p->lut_depth != 16) { set_error("lut_depth %d: a float source is quantised to 16-bit codes, lut_depth must be 16", p->lut_depth); return LUTR_EINVAL; }
    YuvConsts K;
    rc = make_yuv_consts_rgb2yuv(*p, &K);
    if (rc) return rc;
    const int dout = LUTR_FMT_DEPTH(p->fmt_out), ocsx = LUTR_FMT_CSX(p->fmt_out), ocsy = LUTR_FMT_CSY(p->fmt_out);
    if (const int rc = check_dither_rows(dither, row0, rows, h)) return rc;
    const int bh = 1 << ocsy;
    if (const int rc = check_row_blocks(row0, rows, h, bh, "output chroma block height")) return rc;
    if (w == 0 || rows == 0 || nframes == 0) return LUTR_OK;
    if (const int rc = check_planes_set(src, dst)) return rc;
    if (const int rc = check_float_planes(src, nframes, "source")) return rc;
    PlaneSet P;
    fill_planes(&P, src, dst);
    // a chroma sample is written by one thread while another may still read the pixels of its block: no in-place operation
    const FrameGeom G{w, h, row0, rows, nframes};
    if (const int rc = check_sides_disjoint("float RGB -> YUV", true, planar_side("source", src, LUTR_FMT(32, 0, 0)),
                                            planar_side("destination", dst, p->fmt_out), G)) return rc;
    // source planes in R, G, B order (gbrp planes are G, B, R); the destination stays Y, Cb, Cr
    const PlaneSet S = gbrp_to_rgb(P);
    for (int k = 0; k < 3; k++) { P.s[k] = S.s[k]; P.ss[k] = S.ss[k]; P.sfs[k] = S.sfs[k]; }
    HIP_TRY(hipSetDevice(c->device));
    LutConsts L; FloatPre Q;
    if (const int rc = fill_lut_float(&L, &Q, c, interp != LUTR_INTERP_NONE)) return rc;
    if (dither == LUTR_DITHER_NONE)
        return finish_launch(c, launch_rgbf2yuv(c->stream, c->variant, L, Q, K, P, G, dout, ocsx, ocsy, interp));
    if (dither == LUTR_DITHER_BLUE_NOISE) {
        const float *bn;
        if (const int rc = bn_table(c, &bn)) return rc;
        return finish_launch(c, launch_rgbf2yuv_bn(c->stream, c->variant, L, Q, K, P, G, bn, dout, ocsx, ocsy, interp));
    }
    FloatPlanes F;
    if (const int rc = dither_scratch(c, G, ocsx, ocsy, &F)) return rc;
    return finish_launch(c, launch_rgbf2yuv_dither(c->stream, L, Q, K, P, G, F, dout, ocsx, ocsy, interp));
}

int lutr_alpha_plane(lutr_ctx *c, const lutr_alpha_src *src, int dout, void *dst, ptrdiff_t dst_stride, int64_t dst_frame_stride,
                     int w, int h, int nframes, int row0, int rows)
{
    if (!c || !src || !dst) { set_error("null argument"); return LUTR_EINVAL; }
    const int kind = src->kind;
    if (kind != LUTR_ALPHA_NONE && kind != LUTR_ALPHA_INT && kind != LUTR_ALPHA_FLOAT) {
        set_error("unknown alpha source kind %d", kind);
        return LUTR_EINVAL;
    }
    if (dout < 8 || dout > 16) { set_error("unsupported alpha depth %d on the destination", dout); return LUTR_EINVAL; }
    if (kind == LUTR_ALPHA_INT && (src->depth < 8 || src->depth > 16)) {
        set_error("unsupported alpha depth %d on the source", (int)src->depth);
        return LUTR_EINVAL;
    }
    if (const int rc = check_geometry(w, h, nframes, row0, rows)) return rc;
    const int din = kind == LUTR_ALPHA_INT ? src->depth : 0;
    const long long sb = kind == LUTR_ALPHA_FLOAT ? 4 : din > 8 ? 2 : 1, db = dout > 8 ? 2 : 1;
    if (kind != LUTR_ALPHA_NONE) {
        if (!src->data) { set_error("null alpha source plane"); return LUTR_EINVAL; }
        if (src->step < 1 || src->offset < 0 || src->offset >= src->step) {
            set_error("bad alpha source step %d / offset %d", (int)src->step, (int)src->offset);
            return LUTR_EINVAL;
        }
        if (!check_aligned(src->data, src->stride, src->frame_stride, nframes, (unsigned)sb - 1)) {
            set_error(kind == LUTR_ALPHA_FLOAT ? "float alpha planes need 4-byte aligned base pointers and strides"
                                               : "16-bit alpha planes need 2-byte aligned base pointers and strides");
            return LUTR_EINVAL;
        }
    }
    if (!check_aligned(dst, dst_stride, dst_frame_stride, nframes, (unsigned)db - 1)) {
        set_error("16-bit alpha planes need 2-byte aligned base pointers and strides");
        return LUTR_EINVAL;
    }
    if (w == 0 || rows == 0 || nframes == 0) return LUTR_OK;
    if (kind != LUTR_ALPHA_NONE) {
        const bool same = kind == LUTR_ALPHA_INT && din == dout && src->step == 1 && src->data == dst && src->stride == dst_stride &&
                          (nframes == 1 || src->frame_stride == dst_frame_stride);
        if (same) { c->last_kernel = "k_alpha_nop"; return LUTR_OK; }
        const Span s = plane_span(src->data, src->stride, src->frame_stride, h, (long long)w * src->step * sb, nframes);
        const Span d = plane_span(dst, dst_stride, dst_frame_stride, h, (long long)w * db, nframes);
        if (s.lo < d.hi && d.lo < s.hi) {
            set_error("the alpha source overlaps the alpha destination other than as the same plane at the same depth (bounding "
                      "byte ranges over all rows and frames must be disjoint)");
            return LUTR_EINVAL;
        }
    }
    AlphaArgs A{};
    if (!alpha_consts(&A, kind, din, dout)) { set_error("no alpha multiplier for %d -> %d bit", din, dout); return LUTR_EINVAL; }
    A.s = kind == LUTR_ALPHA_NONE ? nullptr : (const uint8_t *)src->data;
    A.d = (uint8_t *)dst;
    A.ss = kind == LUTR_ALPHA_NONE ? 0 : src->stride; A.ds = dst_stride;
    A.sfs = kind == LUTR_ALPHA_NONE ? 0 : src->frame_stride; A.dfs = dst_frame_stride;
    A.step = kind == LUTR_ALPHA_NONE ? 1 : src->step;
    A.off = kind == LUTR_ALPHA_NONE ? 0 : src->offset;
    HIP_TRY(hipSetDevice(c->device));
    return finish_launch(c, launch_alpha(c->stream, c->variant, A, FrameGeom{w, h, row0, rows, nframes}));
}

// the alpha plane a premultiplied call reads beside the colour planes -- a plane (step 1, offset 0) of `kind`,
// aligned to its samples; an integer one at the source's depth `din`.  `entry` opens the messages.
static int check_premul_alpha(const char *entry, const lutr_alpha_src *a, int kind, int din, int nframes)
{
    if (a->kind != kind) {
        set_error("%s: the alpha source must be %s (kind %d), got kind %d -- premultiplied alpha is defined only for a source that "
                  "carries alpha", entry, kind == LUTR_ALPHA_INT ? "an integer plane" : "a float plane", kind, (int)a->kind);
        return LUTR_EINVAL;
    }
    if (kind == LUTR_ALPHA_INT && a->depth != din) {
        set_error("%s: the alpha plane has the source's depth %d, not %d", entry, din, (int)a->depth);
        return LUTR_EINVAL;
    }
    if (a->step != 1 || a->offset != 0) {
        set_error("%s: the alpha source must be a plane (step 1, offset 0), got step %d / offset %d", entry, (int)a->step, (int)a->offset);
        return LUTR_EINVAL;
    }
    if (!a->data) { set_error("%s: null alpha source plane", entry); return LUTR_EINVAL; }
    const unsigned sb = kind == LUTR_ALPHA_FLOAT ? 4 : din > 8 ? 2 : 1;
    if (!check_aligned(a->data, a->stride, a->frame_stride, nframes, sb - 1)) {
        set_error(kind == LUTR_ALPHA_FLOAT ? "%s: float alpha planes need 4-byte aligned base pointers and strides"
                                           : "%s: 16-bit alpha planes need 2-byte aligned base pointers and strides", entry);
        return LUTR_EINVAL;
    }
    return LUTR_OK;
}

// lutr_apply_yuv_xsub's pass for any pair of layouts with unpremultiply / premultiply around lut3d.
int lutr_apply_yuv_premul(lutr_ctx *c, const lutr_yuv_params *p, int interp, int w, int h, int nframes, const lutr_planes *src,
                          const lutr_alpha_src *alpha, const lutr_planes *dst, int row0, int rows)
{
    int rc = check_common(c, interp, LUTR_INTERP_NEAREST, w, h, nframes, src, dst, row0, rows);
    if (rc) return rc;
    if (!p) { set_error("null yuv params"); return LUTR_EINVAL; }
    if (!alpha) { set_error("null alpha source"); return LUTR_EINVAL; }
    UnionCall U; const FrameGeom G{w, h, row0, rows, nframes};
    if (const int rc = union_open(*p, src, dst, &U)) return rc;
    const Side &S = U.side[0], &D = U.side[1];
    if (p->range_src != p->range_in || p->lut_depth != S.depth) {
        set_error("premultiplied alpha: a call with a prologue (range_src != range_in, or lut_depth %d other than the source's depth "
                  "%d) has no alpha to carry", p->lut_depth, S.depth);
        return LUTR_EINVAL;
    }
    if (const int rc = check_premul_alpha("premultiplied alpha", alpha, LUTR_ALPHA_INT, S.depth, nframes)) return rc;
    if (const int rc = union_rules(c, U, G, nullptr, "premultiplied alpha")) return rc;
    if (w == 0 || rows == 0 || nframes == 0) return LUTR_OK;
    if (const int rc = union_planes_ready(U, G)) return rc;
    // not in place: the three colour planes and the alpha plane (source plane 3 in the message) against every colour destination
    Span ss[4], ds[3];
    side_spans(S, G, ss);
    ss[3] = plane_span(alpha->data, alpha->stride, alpha->frame_stride, h, (long long)w * (S.depth > 8 ? 2 : 1), nframes);
    side_spans(D, G, ds);
    if (const int rc = check_disjoint("the premultiplied-alpha pass", true, ss, 4, ds, 3)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    LutConsts L; PremulPlanes P;
    if (const int rc = fill_lut(&L, c, p->lut_depth)) return rc;
    fill_planes(&P.p, src, dst);
    P.a = AlphaIn{(const uint8_t *)alpha->data, (long long)alpha->stride, (long long)alpha->frame_stride};
    return finish_launch(c, launch_yuva_premul(c->stream, c->variant, L, U.K, P, G, S.depth, D.depth, p->lut_depth, S.csx, S.csy, D.csx,
                                               D.csy, interp));
}

// lutr_apply_planar_rgb_f32's pass with the division by alpha in front of lut3d and the multiplication behind it.
int lutr_apply_planar_rgb_f32_premul(lutr_ctx *c, int interp, int w, int h, int nframes, const lutr_planes *src,
                                     const lutr_alpha_src *alpha, const lutr_planes *dst, int row0, int rows)
{
    int rc = check_common(c, interp, LUTR_INTERP_NEAREST, w, h, nframes, src, dst, row0, rows);
    if (rc) return rc;
    if (!alpha) { set_error("null alpha source"); return LUTR_EINVAL; }
    if (const int rc = check_premul_alpha("premultiplied alpha", alpha, LUTR_ALPHA_FLOAT, 0, nframes)) return rc;
    if (c->variant == VAR_VEC_LDS) { set_error("variant vec_lds: there is no LDS-window kernel for premultiplied alpha"); return LUTR_EINVAL; }
    if (w == 0 || rows == 0 || nframes == 0) return LUTR_OK;
    if (const int rc = check_planes_set(src, dst)) return rc;
    if (const int rc = check_float_planes(src, nframes, "source")) return rc;
    if (const int rc = check_float_planes(dst, nframes, "destination")) return rc;
    // dst == src is pixelwise and fine; the alpha plane is read by every colour plane's pixel and must not be written
    Span as = plane_span(alpha->data, alpha->stride, alpha->frame_stride, h, (long long)w * 4, nframes), ds[3];
    planar_spans(dst, 0, 0, w, h, 4, nframes, ds);
    for (int j = 0; j < 3; j++)
        if (as.lo < ds[j].hi && ds[j].lo < as.hi) {
            set_error("premultiplied alpha: the byte range of the alpha source overlaps that of destination plane %d (bounding ranges "
                      "over all rows and frames must be disjoint)", j);
            return LUTR_EINVAL;
        }
    HIP_TRY(hipSetDevice(c->device));
    LutConsts L; FloatPre Q; PremulPlanes P; FrameGeom G{w, h, row0, rows, nframes};
    if (const int rc = fill_lut_float(&L, &Q, c, true)) return rc;
    fill_planes(&P.p, src, dst);
    P.p = gbrp_to_rgb(P.p);
    P.a = AlphaIn{(const uint8_t *)alpha->data, (long long)alpha->stride, (long long)alpha->frame_stride};
    return finish_launch(c, launch_rgbaf_premul(c->stream, c->variant, L, Q, P, G, interp));
}

int lutr_dither_mask(uint16_t out[4096])
{
    if (!out) { set_error("lutr_dither_mask: null out pointer"); return LUTR_EINVAL; }
    std::memcpy(out, kLutrBnMask, sizeof(kLutrBnMask));
    return LUTR_OK;
}

int lutr_resize_filter(int src, int dst, int cs, int cosited, int *start, int16_t *weights, int *ntaps)
{
    if (!ntaps) { set_error("lutr_resize_filter: null ntaps"); return LUTR_EINVAL; }
    std::vector<int> st, w;
    int n = 0;
    const int rc = resize_table(src, dst, cs, cosited, &st, &w, &n);
    if (rc) return rc;
    *ntaps = n;
    if (start) std::memcpy(start, st.data(), st.size() * sizeof(int));
    if (weights)
        for (size_t i = 0; i < w.size(); i++) weights[i] = (int16_t)w[i];
    return LUTR_OK;
}

// The device table of one axis geometry, built and uploaded on first use (asynchronously, on the context's stream; the host
// copy is freed only after the upload has finished).
static int rz_table(lutr_ctx *c, int src, int dst, int cs, int cosited, lutr_ctx::RzTable *out)
{
    for (auto &t : c->rz_tables)
        if (t.src == src && t.dst == dst && t.cs == cs && t.cosited == cosited) { *out = t; return LUTR_OK; }
    std::vector<int> st, w;
    int n = 0;
    if (const int rc = resize_table(src, dst, cs, cosited, &st, &w, &n)) return rc;
    std::vector<int> host(st);
    host.insert(host.end(), w.begin(), w.end());
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, host.size() * sizeof(int));
    if (e != hipSuccess) { set_error("hipMalloc(resize table): %s", hipGetErrorString(e)); return LUTR_ENOMEM; }
    e = hipMemcpy(p, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(p); return hip_fail(e, "hipMemcpy(resize table)"); }
    c->rz_tables.push_back({src, dst, cs, cosited, resize_axis(st, n), (int *)p});
    *out = c->rz_tables.back();
    return LUTR_OK;
}

// The geometry checks lutr_resize_planes and lutr_resize_plan share.
static int check_resize_geometry(int family, int depth, int csx, int csy, int chroma_loc, int sw, int sh, int dw, int dh, int nframes)
{
    if (family != LUTR_RESIZE_YUV && family != LUTR_RESIZE_GBR) { set_error("unknown plane family %d", family); return LUTR_EINVAL; }
    if (depth < 8 || depth > 16) { set_error("unsupported depth %d", depth); return LUTR_EINVAL; }
    if (csx < 0 || csx > 1 || csy < 0 || csy > 1 || (family == LUTR_RESIZE_GBR && (csx || csy))) {
        set_error("unsupported chroma subsampling %d x %d", csx, csy);
        return LUTR_EINVAL;
    }
    if (chroma_loc < LUTR_CHROMA_REPLICATE || chroma_loc > LUTR_CHROMA_TOPLEFT) {
        set_error("unknown chroma location %d", chroma_loc);
        return LUTR_EINVAL;
    }
    if (sw < 1 || sh < 1 || dw < 1 || dh < 1 || nframes < 0) {
        set_error("bad geometry %dx%d -> %dx%d, nframes %d", sw, sh, dw, dh, nframes);
        return LUTR_EINVAL;
    }
    if ((long long)dw * 8 < sw || dw > 16LL * sw || (long long)dh * 8 < sh || dh > 16LL * sh) {
        set_error("resize %dx%d -> %dx%d outside the limits 1/8 <= dst/src <= 16 per axis", sw, sh, dw, dh);
        return LUTR_EINVAL;
    }
    return LUTR_OK;
}

// The three planes' sizes (luma, chroma, chroma) of a w x h frame subsampled by 2^csx x 2^csy.
static void plane_dims(int w, int h, int csx, int csy, int pw[3], int ph[3])
{
    for (int i = 0; i < 3; i++) { pw[i] = chroma_dim(w, i ? csx : 0); ph[i] = chroma_dim(h, i ? csy : 0); }
}

int lutr_resize_plan(int family, int depth, int csx, int csy, int chroma_loc, int sw, int sh, int dw, int dh, int *out)
{
    if (!out) { set_error("lutr_resize_plan: null out pointer"); return LUTR_EINVAL; }
    if (const int rc = check_resize_geometry(family, depth, csx, csy, chroma_loc, sw, sh, dw, dh, 1)) return rc;
    const int cox = chroma_loc == LUTR_CHROMA_LEFT || chroma_loc == LUTR_CHROMA_TOPLEFT;
    const int coy = chroma_loc == LUTR_CHROMA_TOPLEFT;
    int pdw[3], pdh[3];
    plane_dims(dw, dh, csx, csy, pdw, pdh);
    RzAxis ax[3], ay[3];
    std::vector<int> st, w;
    for (int i = 0; i < 3; i++) {
        const int cx = i ? csx : 0, cy = i ? csy : 0;
        int n = 0;
        if (const int rc = resize_table(sw, dw, cx, cx ? cox : 0, &st, &w, &n)) return rc;
        ax[i] = resize_axis(st, n);
        if (const int rc = resize_table(sh, dh, cy, cy ? coy : 0, &st, &w, &n)) return rc;
        ay[i] = resize_axis(st, n);
    }
    RzArgs A{};
    resize_plan(ax, ay, pdw, pdh, &A);
    const int lds = (int)resize_lds_bytes(A);
    const int plan[8] = {A.th, A.rows, lds, A.spx, A.spy, A.nx_max, A.ny_max, A.tiles_per_frame};
    std::memcpy(out, plan, sizeof(plan));
    if (lds > 65536) { set_error("resize footprint needs %d bytes of LDS (at most 65536)", lds); return LUTR_EINVAL; }
    return LUTR_OK;
}

int lutr_resize_planes(lutr_ctx *c, int family, int depth, int csx, int csy, int chroma_loc, int sw, int sh, int dw, int dh,
                       int nframes, const lutr_planes *src, lutr_planes *dst)
{
    if (!c || !src || !dst) { set_error("null argument"); return LUTR_EINVAL; }
    if (const int rc = check_resize_geometry(family, depth, csx, csy, chroma_loc, sw, sh, dw, dh, nframes)) return rc;
    if (nframes == 0) return LUTR_OK;
    if (const int rc = check_planes_set(src, dst)) return rc;
    const int es = depth > 8 ? 2 : 1;
    int psw[3], psh[3], pdw[3], pdh[3];
    plane_dims(sw, sh, csx, csy, psw, psh);
    plane_dims(dw, dh, csx, csy, pdw, pdh);
    // every destination sample reads a neighbourhood of source samples: no destination may overlap a source
    Span ss[3], ds[3];
    side_spans(planar_side("source", src, LUTR_FMT(depth, csx, csy)), FrameGeom{sw, sh, 0, sh, nframes}, ss);
    side_spans(planar_side("destination", dst, LUTR_FMT(depth, csx, csy)), FrameGeom{dw, dh, 0, dh, nframes}, ds);
    if (const int rc = check_disjoint("resize", true, ss, 3, ds, 3)) return rc;
    if (es == 2)
        for (int i = 0; i < 3; i++)
            if (!(check_aligned(src->data[i], src->stride[i], src->frame_stride[i], nframes, 1) &&
                  check_aligned(dst->data[i], dst->stride[i], dst->frame_stride[i], nframes, 1))) {
                set_error("16-bit planes need 2-byte aligned rows");
                return LUTR_EINVAL;
            }
    const int cox = chroma_loc == LUTR_CHROMA_LEFT || chroma_loc == LUTR_CHROMA_TOPLEFT;
    const int coy = chroma_loc == LUTR_CHROMA_TOPLEFT;
    HIP_TRY(hipSetDevice(c->device));
    if (c->rz_tables.size() > 58) {              // many geometries in one context: start over (a call adds at most 6 tables)
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (auto &t : c->rz_tables) (void)hipFree(t.dev);
        c->rz_tables.clear();
    }
    RzArgs A{};
    A.depth = depth;
    lutr_ctx::RzTable tx[3], ty[3];
    RzAxis ax[3], ay[3];
    for (int i = 0; i < 3; i++) {
        const int cx = i ? csx : 0, cy = i ? csy : 0;
        if (const int rc = rz_table(c, sw, dw, cx, cx ? cox : 0, &tx[i])) return rc;
        if (const int rc = rz_table(c, sh, dh, cy, cy ? coy : 0, &ty[i])) return rc;
        ax[i] = tx[i].axis; ay[i] = ty[i].axis;
    }
    resize_plan(ax, ay, pdw, pdh, &A);
    for (int i = 0; i < 3; i++) {
        RzPlane &P = A.p[i];
        P.s = (const uint8_t *)src->data[i]; P.d = (uint8_t *)dst->data[i];
        P.ss = src->stride[i]; P.ds = dst->stride[i]; P.sfs = src->frame_stride[i]; P.dfs = dst->frame_stride[i];
        P.sw = psw[i]; P.sh = psh[i]; P.dw = pdw[i]; P.dh = pdh[i];
        P.xs = tx[i].dev; P.xw = tx[i].dev + pdw[i];
        P.ys = ty[i].dev; P.yw = ty[i].dev + pdh[i];
    }
    const char *name = launch_resize(c->stream, A, nframes);
    if (!name) { set_error("resize launch too large (split the batch)"); return LUTR_EINVAL; }
    return finish_launch(c, name);
}

}  // extern "C"
