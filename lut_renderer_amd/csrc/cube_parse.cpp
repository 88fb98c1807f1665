// cube_parse.cpp -- the product's .cube reader (host side of lutr_cube_parse).
//
// Replaces what FFmpeg's lut3d does with the file= option the reference passes at
// /root/reference/src/lut_renderer/ffmpeg.py:246 (the GUI only admits *.cube files:
// lut_manager.py:121).  Semantics follow FFmpeg's parse_cube as distilled in
// SURVEY.md Appendix A.2; the implementation is a small line-driven state machine,
// independent of the oracle's restatement (oracle/lut3d_oracle.c) so that the parity
// tests compare two separately written readers.
//
// Deliberate deviation: a lattice entry that is not finite (nan/inf are accepted by
// sscanf("%f")) is rejected as invalid data, because the kernels' tie handling in the
// tetrahedral blend relies on 0 * c == 0 (DESIGN.md "Kernels").
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "lutr_internal.h"

namespace {

constexpr int kMaxLine = 512;    // fgets buffer FFmpeg uses: longer lines arrive in pieces
constexpr int kMaxLevel = 256;

bool ends_with_cube(const char *path)
{
    const char *dot = std::strrchr(path, '.');
    if (!dot) return false;
    std::string ext(dot + 1);
    for (auto &ch : ext) ch = (char)std::tolower((unsigned char)ch);
    return ext == "cube";
}

bool blank_or_comment(const char *s)
{
    while (*s && std::isspace((unsigned char)*s)) s++;
    return *s == 0 || *s == '#';
}

struct Reader {
    FILE *f = nullptr;
    char buf[kMaxLine];
    ~Reader() { if (f) std::fclose(f); }
    bool next() { return std::fgets(buf, sizeof(buf), f) != nullptr; }
    bool starts(const char *prefix) const { return std::strncmp(buf, prefix, std::strlen(prefix)) == 0; }
};

// vf_lut3d.c: av_clipf(1. / (max[c] - min[c]), 0.f, 1.f): float subtraction, double division, float clip
void domain_scale(const float dmin[3], const float dmax[3], float scale[3])
{
    for (int c = 0; c < 3; c++) {
        const float span = dmax[c] - dmin[c];
        float s = (float)(1.0 / (double)span);
        if (!(s == s)) s = 0.f;
        s = s < 0.f ? 0.f : s;
        s = s > 1.f ? 1.f : s;
        scale[c] = s;
    }
}

}  // namespace

extern "C" int lutr_cube_parse(const char *path, float **rgb, int *n, float scale[3])
{
    if (!path || !rgb || !n || !scale) {
        lutr::set_error("lutr_cube_parse: null argument");
        return LUTR_EINVAL;
    }
    *rgb = nullptr;
    *n = 0;
    if (!ends_with_cube(path)) {
        lutr::set_error("'%s': unrecognised LUT extension (only .cube is supported)", path);
        return LUTR_EINVAL;
    }
    Reader rd;
    rd.f = std::fopen(path, "r");
    if (!rd.f) {
        lutr::set_error("'%s': cannot open", path);
        return LUTR_ENOENT;
    }

    // phase 1: everything up to the LUT_3D_SIZE line is ignored (DOMAIN_/TITLE included)
    int size = 0;
    while (rd.next()) {
        if (rd.starts("LUT_3D_SIZE")) {
            size = (int)std::strtol(rd.buf + 12, nullptr, 0);
            if (size < 2 || size > kMaxLevel) {
                lutr::set_error("'%s': too large or invalid 3D LUT size %d", path, size);
                return LUTR_EINVAL;
            }
            break;
        }
    }
    if (size == 0) {
        lutr::set_error("'%s': 3D LUT is empty (no LUT_3D_SIZE)", path);
        return LUTR_EILSEQ;
    }

    // phase 2: size^3 triplets in file order (red fastest), stored blue fastest
    float dmin[3] = {0.f, 0.f, 0.f}, dmax[3] = {1.f, 1.f, 1.f};
    const size_t count = (size_t)size * size * size;
    std::vector<float> table(count * 3);
    size_t filled = 0;
    while (filled < count) {
        if (!rd.next()) {
            lutr::set_error("'%s': unexpected EOF after %zu of %zu entries", path, filled, count);
            return LUTR_EILSEQ;
        }
        if (rd.starts("DOMAIN_")) {
            float *dst = rd.starts("DOMAIN_MIN ") ? dmin : rd.starts("DOMAIN_MAX ") ? dmax : nullptr;
            if (!dst) {
                lutr::set_error("'%s': malformed DOMAIN_ line", path);
                return LUTR_EILSEQ;
            }
            std::sscanf(rd.buf + 11, "%f %f %f", dst, dst + 1, dst + 2);
            continue;
        }
        if (rd.starts("TITLE") || blank_or_comment(rd.buf))
            continue;
        float v[3];
        if (std::sscanf(rd.buf, "%f %f %f", &v[0], &v[1], &v[2]) != 3) {
            lutr::set_error("'%s': invalid data at entry %zu", path, filled);
            return LUTR_EILSEQ;
        }
        if (!std::isfinite(v[0]) || !std::isfinite(v[1]) || !std::isfinite(v[2])) {
            lutr::set_error("'%s': non-finite lattice value at entry %zu", path, filled);
            return LUTR_EILSEQ;
        }
        // entry index = r + size*(g + size*b)
        const size_t r = filled % size, g = (filled / size) % size, b = filled / ((size_t)size * size);
        float *dst = &table[((r * size + g) * size + b) * 3];
        dst[0] = v[0]; dst[1] = v[1]; dst[2] = v[2];
        filled++;
    }

    domain_scale(dmin, dmax, scale);
    float *out = (float *)std::malloc(table.size() * sizeof(float));
    if (!out) {
        lutr::set_error("out of memory");
        return LUTR_ENOMEM;
    }
    std::memcpy(out, table.data(), table.size() * sizeof(float));
    *rgb = out;
    *n = size;
    return LUTR_OK;
}

extern "C" void lutr_cube_free(float *rgb) { std::free(rgb); }

// ---------------------------------------------------------------- 1D .cube files
// FFmpeg's lut1d reads them with parse_cube_1d in the same source file as lut3d's reader; lines are handled as above, plus the
// LUT_1D_INPUT_RANGE keyword.  Result: 3 x size floats, channel c at [c * size].
constexpr int kMax1dLevel = 65536;

extern "C" int lutr_lut1d_parse(const char *path, float **lut, int *size_out, float scale[3])
{
    if (!path || !lut || !size_out || !scale) {
        lutr::set_error("lutr_lut1d_parse: null argument");
        return LUTR_EINVAL;
    }
    *lut = nullptr;
    *size_out = 0;
    if (!ends_with_cube(path)) {
        lutr::set_error("'%s': unrecognised 1D LUT extension (only .cube is supported)", path);
        return LUTR_EINVAL;
    }
    Reader rd;
    rd.f = std::fopen(path, "r");
    if (!rd.f) {
        lutr::set_error("'%s': cannot open", path);
        return LUTR_ENOENT;
    }
    const char *both = "'%s': the file carries LUT_1D_SIZE and LUT_3D_SIZE (a shaper ahead of a cube); that pair is not supported";

    // phase 1: everything up to the LUT_1D_SIZE line is ignored, but a 3D size ahead of it names a shaper + cube file
    int size = 0;
    bool has3d = false;
    while (rd.next()) {
        if (rd.starts("LUT_3D_SIZE")) has3d = true;
        if (rd.starts("LUT_1D_SIZE")) {
            size = (int)std::strtol(rd.buf + 12, nullptr, 0);
            if (size < 2 || size > kMax1dLevel) {
                lutr::set_error("'%s': too large or invalid 1D LUT size %d", path, size);
                return LUTR_EINVAL;
            }
            break;
        }
    }
    if (size == 0) {
        lutr::set_error(has3d ? "'%s': a 3D LUT file (LUT_3D_SIZE), not a 1D one" : "'%s': 1D LUT is empty (no LUT_1D_SIZE)", path);
        return has3d ? LUTR_EINVAL : LUTR_EILSEQ;
    }
    if (has3d) {
        lutr::set_error(both, path);
        return LUTR_EINVAL;
    }

    // phase 2: size rows of three floats
    float dmin[3] = {0.f, 0.f, 0.f}, dmax[3] = {1.f, 1.f, 1.f};
    std::vector<float> table((size_t)size * 3);
    int filled = 0;
    while (filled < size) {
        if (!rd.next()) {
            lutr::set_error("'%s': unexpected EOF after %d of %d rows", path, filled, size);
            return LUTR_EILSEQ;
        }
        if (rd.starts("LUT_3D_SIZE")) {
            lutr::set_error(both, path);
            return LUTR_EINVAL;
        }
        if (rd.starts("DOMAIN_")) {
            float *dst = rd.starts("DOMAIN_MIN ") ? dmin : rd.starts("DOMAIN_MAX ") ? dmax : nullptr;
            if (!dst) {
                lutr::set_error("'%s': malformed DOMAIN_ line", path);
                return LUTR_EILSEQ;
            }
            std::sscanf(rd.buf + 11, "%f %f %f", dst, dst + 1, dst + 2);
            continue;
        }
        if (rd.starts("LUT_1D_INPUT_RANGE ")) {
            std::sscanf(rd.buf + 19, "%f %f", dmin, dmax);
            dmin[1] = dmin[2] = dmin[0];
            dmax[1] = dmax[2] = dmax[0];
            continue;
        }
        if (rd.starts("TITLE") || blank_or_comment(rd.buf))
            continue;
        float v[3];
        if (std::sscanf(rd.buf, "%f %f %f", &v[0], &v[1], &v[2]) != 3) {
            lutr::set_error("'%s': invalid data at row %d (a row is three numbers)", path, filled);
            return LUTR_EILSEQ;
        }
        if (!std::isfinite(v[0]) || !std::isfinite(v[1]) || !std::isfinite(v[2])) {
            lutr::set_error("'%s': non-finite value at row %d", path, filled);
            return LUTR_EILSEQ;
        }
        for (int c = 0; c < 3; c++) table[(size_t)c * size + filled] = v[c];
        filled++;
    }
    // a 3D size behind the rows: the same pair
    while (rd.next())
        if (rd.starts("LUT_3D_SIZE")) {
            lutr::set_error(both, path);
            return LUTR_EINVAL;
        }

    domain_scale(dmin, dmax, scale);
    float *out = (float *)std::malloc(table.size() * sizeof(float));
    if (!out) {
        lutr::set_error("out of memory");
        return LUTR_ENOMEM;
    }
    std::memcpy(out, table.data(), table.size() * sizeof(float));
    *lut = out;
    *size_out = size;
    return LUTR_OK;
}

// The per-code table of one channel: FFmpeg's interp_1d_* on every integer code, every operation rounded to
// fp32 (this file is compiled without contraction), then truncated to a code.  Host only.
extern "C" int lutr_lut1d_table(const float *lut, int size, const float scale[3], int interp1d, int depth, int channel, uint16_t *out)
{
    if (!lut || !scale || !out) { lutr::set_error("lutr_lut1d_table: null argument"); return LUTR_EINVAL; }
    if (size < 2 || size > kMax1dLevel) { lutr::set_error("lutr_lut1d_table: 1D LUT size %d outside 2..65536", size); return LUTR_EINVAL; }
    if (interp1d < LUTR_INTERP1D_NEAREST || interp1d > LUTR_INTERP1D_SPLINE) {
        lutr::set_error("lutr_lut1d_table: unknown 1D interpolation mode %d", interp1d);
        return LUTR_EINVAL;
    }
    if (depth < 8 || depth > 16) { lutr::set_error("lutr_lut1d_table: depth %d outside 8..16", depth); return LUTR_EINVAL; }
    if (channel < 0 || channel > 2) { lutr::set_error("lutr_lut1d_table: channel %d outside 0..2", channel); return LUTR_EINVAL; }
    if (!(scale[channel] >= 0.f && scale[channel] <= 1.f)) {
        lutr::set_error("lutr_lut1d_table: scale[%d] = %g outside [0,1]", channel, (double)scale[channel]);
        return LUTR_EINVAL;
    }
    const float *l = lut + (size_t)channel * size;
    for (int i = 0; i < size; i++)
        if (!std::isfinite(l[i])) { lutr::set_error("lutr_lut1d_table: node %d of channel %d is not finite", i, channel); return LUTR_EINVAL; }
    const int maxi = (1 << depth) - 1, last = size - 1;
    const float factor = (float)maxi;
    const float sc = (scale[channel] / factor) * (float)last;
    // (the min() on the indices never binds for scale <= 1: s stays below size - 1/2; it keeps a rounding surprise inside the table)
    auto at = [&](int i) { return l[i < 0 ? 0 : (i > last ? last : i)]; };
    for (int k = 0; k <= maxi; k++) {
        const float s = (float)k * sc;
        const int prev = (int)s, next = prev + 1 < last ? prev + 1 : last;
        const float mu = s - (float)prev;
        const float p = at(prev), q = at(next);
        float v;
        switch (interp1d) {
        case LUTR_INTERP1D_NEAREST:
            v = at((int)((double)s + .5));
            break;
        case LUTR_INTERP1D_LINEAR:
            v = p + (q - p) * mu;
            break;
        case LUTR_INTERP1D_COSINE: {
            const float m = (1.f - cosf((float)((double)mu * M_PI))) * .5f;
            v = p + (q - p) * m;
            break;
        }
        case LUTR_INTERP1D_CUBIC: {
            const float y0 = at(prev - 1), y1 = p, y2 = q, y3 = at(next + 1);
            const float mu2 = mu * mu;
            const float a0 = y3 - y2 - y0 + y1, a1 = y0 - y1 - a0, a2 = y2 - y0, a3 = y1;
            v = a0 * mu * mu2 + a1 * mu2 + a2 * mu + a3;
            break;
        }
        default: {
            const float y0 = at(prev - 1), y1 = p, y2 = q, y3 = at(next + 1);
            const float c0 = y1, c1 = .5f * (y2 - y0);
            const float c2 = y0 - 2.5f * y1 + 2.f * y2 - .5f * y3;
            const float c3 = .5f * (y3 - y0) + 1.5f * (y1 - y2);
            v = ((c3 * mu + c2) * mu + c1) * mu + c0;
            break;
        }
        }
        // clamp in float ahead of the conversion (a huge node is not undefined behaviour; a NaN of inf - inf gives 0), then truncate
        const float x = v * factor;
        out[k] = (uint16_t)(int)(!(x > 0.f) ? 0.f : (x > factor ? factor : x));
    }
    return LUTR_OK;
}
