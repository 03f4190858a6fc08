// ply_reader.cpp — host reader of standard 3DGS scene files (include/lsr_ply.h, "import").  Plain C++ with no HIP in
// it, so that it can be built and run under the host sanitizers on its own (tools/ply_reader_fuzz.cpp).  The input
// is untrusted: every line is bounded, every count is checked before it is used as a size, and the caller's
// structures are written only after all checks have passed.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "lsr_ply.h"

namespace {

constexpr int kMaxLine = 255;           // bytes of one header line, newline excluded
constexpr int kMaxTokens = 8;
constexpr long kMaxHeaderBytes = 1 << 20;

// One header line into buf (NUL-terminated, '\n' and a trailing '\r' dropped).  1: a line, 0: end of file before a
// newline, -1: longer than kMaxLine or holds a NUL byte.
int read_line(FILE *f, char *buf, long *consumed) {
    int len = 0;
    for (;;) {
        const int c = fgetc(f);
        if (c == EOF) return 0;
        ++*consumed;
        if (c == '\n') break;
        if (c == 0 || len == kMaxLine) return -1;
        buf[len++] = (char)c;
    }
    if (len > 0 && buf[len - 1] == '\r') --len;
    buf[len] = 0;
    return 1;
}

// Splits at blanks in place; returns the token count, kMaxTokens + 1 if there are more.
int tokenize(char *s, char *tok[kMaxTokens]) {
    int n = 0;
    while (*s) {
        while (*s == ' ' || *s == '\t') ++s;
        if (!*s) break;
        if (n == kMaxTokens) return kMaxTokens + 1;
        tok[n++] = s;
        while (*s && *s != ' ' && *s != '\t') ++s;
        if (*s) *s++ = 0;
    }
    return n;
}

// Decimal int64 with an optional sign.  0: ok, 1: not a number, 2: out of range.
int parse_i64(const char *s, int64_t *out) {
    bool neg = false;
    if (*s == '-' || *s == '+') neg = *s++ == '-';
    if (!*s) return 1;
    uint64_t v = 0;
    bool over = false;
    for (; *s; ++s) {
        if (*s < '0' || *s > '9') return 1;
        const uint64_t d = (uint64_t)(*s - '0');
        if (v > (UINT64_MAX - d) / 10) over = true;
        if (!over) v = v * 10 + d;
    }
    if (over || v > (uint64_t)INT64_MAX) return 2;
    *out = neg ? -(int64_t)v : (int64_t)v;
    return 0;
}

// "<prefix><index>" with a plain decimal index (no sign, no leading zeros beyond "0"): the index, else -1.
int indexed_name(const char *name, const char *prefix) {
    const size_t pl = strlen(prefix);
    if (strncmp(name, prefix, pl) != 0) return -1;
    const char *d = name + pl;
    if (!*d || (d[0] == '0' && d[1])) return -1;
    int v = 0;
    for (; *d; ++d) {
        if (*d < '0' || *d > '9') return -1;
        v = v * 10 + (*d - '0');
        if (v > 1 << 20) return -1;
    }
    return v;
}

struct Parsed {
    lsr_ply_layout layout;
    int64_t row_floats;    // n * stride
};

// Header, then the size check.  A file with several problems reports the one met first, line by line; what can only
// be judged at end_header (missing properties, the f_rest count, the file's size) comes after every line's own.
int parse(FILE *f, Parsed *p) {
    lsr_ply_layout L;
    memset(&L, 0, sizeof(L));
    int32_t *const single[] = {&L.xyz[0], &L.xyz[1], &L.xyz[2], &L.opacity};
    static const char *const single_names[] = {"x", "y", "z", "opacity"};
    bool seen_single[4] = {}, seen_dc[3] = {}, seen_scale[3] = {}, seen_rot[4] = {}, seen_rest[LSR_PLY_MAX_REST] = {};
    int rest_count = 0, rest_beyond = 0;
    bool have_format = false, have_element = false, ended = false;
    char line[kMaxLine + 1];
    char *tok[kMaxTokens];
    long consumed = 0;

    if (read_line(f, line, &consumed) != 1 || strcmp(line, "ply") != 0) return LSR_EINVAL;
    while (!ended) {
        if (consumed > kMaxHeaderBytes) return LSR_EINVAL;
        if (read_line(f, line, &consumed) != 1) return LSR_EINVAL;          // over-long line, or no end_header
        if (!strncmp(line, "comment", 7) && (line[7] == 0 || line[7] == ' ' || line[7] == '\t')) continue;
        if (!strncmp(line, "obj_info", 8) && (line[8] == 0 || line[8] == ' ' || line[8] == '\t')) continue;
        const int nt = tokenize(line, tok);
        if (nt == 0 || nt > kMaxTokens) return LSR_EINVAL;
        if (!strcmp(tok[0], "end_header")) {
            if (nt != 1) return LSR_EINVAL;
            ended = true;
        } else if (!strcmp(tok[0], "format")) {
            if (nt != 3 || have_format || have_element) return LSR_EINVAL;
            if (strcmp(tok[1], "binary_little_endian") != 0 || strcmp(tok[2], "1.0") != 0) return LSR_EUNSUPPORTED;
            have_format = true;
        } else if (!strcmp(tok[0], "element")) {
            if (nt != 3 || !have_format) return LSR_EINVAL;
            if (have_element || strcmp(tok[1], "vertex") != 0) return LSR_EUNSUPPORTED;
            if (parse_i64(tok[2], &L.n) != 0 || L.n < 0) return LSR_EINVAL;
            have_element = true;
        } else if (!strcmp(tok[0], "property")) {
            if (!have_element || nt < 3) return LSR_EINVAL;
            if (!strcmp(tok[1], "list")) return LSR_EUNSUPPORTED;
            if (nt != 3) return LSR_EINVAL;
            if (strcmp(tok[1], "float") != 0 && strcmp(tok[1], "float32") != 0) return LSR_EUNSUPPORTED;
            if (L.stride == LSR_PLY_MAX_STRIDE) return LSR_EUNSUPPORTED;
            const int32_t at = L.stride++;
            const char *name = tok[2];
            bool *seen = nullptr;
            int32_t *slot = nullptr;
            int k;
            for (int s = 0; s < 4; ++s)
                if (!strcmp(name, single_names[s])) { seen = &seen_single[s]; slot = single[s]; }
            if (!seen && (k = indexed_name(name, "f_dc_")) >= 0 && k < 3) { seen = &seen_dc[k]; slot = &L.f_dc[k]; }
            if (!seen && (k = indexed_name(name, "scale_")) >= 0 && k < 3) { seen = &seen_scale[k]; slot = &L.scale[k]; }
            if (!seen && (k = indexed_name(name, "rot_")) >= 0 && k < 4) { seen = &seen_rot[k]; slot = &L.rot[k]; }
            if (!seen && (k = indexed_name(name, "f_rest_")) >= 0) {
                if (k >= LSR_PLY_MAX_REST) { ++rest_beyond; continue; }
                seen = &seen_rest[k];
                slot = &L.f_rest[k];
                if (!*seen) ++rest_count;
            }
            if (!seen) continue;                                            // some other float property: skipped
            if (*seen) return LSR_EINVAL;                                   // given twice
            *seen = true;
            *slot = at;
        } else {
            return LSR_EINVAL;
        }
    }
    if (!have_format || !have_element) return LSR_EINVAL;
    for (int s = 0; s < 4; ++s)
        if (!seen_single[s]) return LSR_EINVAL;
    for (int s = 0; s < 3; ++s)
        if (!seen_dc[s] || !seen_scale[s]) return LSR_EINVAL;
    for (int s = 0; s < 4; ++s)
        if (!seen_rot[s]) return LSR_EINVAL;
    if (rest_beyond) return LSR_EUNSUPPORTED;                               // more coefficients than degree 4 has
    int K = 0;
    for (int deg = 0; deg <= LSR_MAX_SH_DEGREE; ++deg)
        if (rest_count == 3 * ((deg + 1) * (deg + 1) - 1)) K = (deg + 1) * (deg + 1);
    if (!K) return LSR_EUNSUPPORTED;
    for (int k = 0; k < rest_count; ++k)
        if (!seen_rest[k]) return LSR_EINVAL;                               // the right count but not f_rest_0..count-1
    L.sh_coeffs = K;
    L.data_offset = consumed;

    // size: header + n * stride * 4 bytes must be there (stride >= 14 here, so the division is safe)
    if (L.n > INT64_MAX / 4 / L.stride) return LSR_EINVAL;
    const int64_t row_floats = L.n * L.stride;
    if (fseeko(f, 0, SEEK_END) != 0) return LSR_EINVAL;
    const int64_t size = (int64_t)ftello(f);
    if (size < L.data_offset || size - L.data_offset < row_floats * 4) return LSR_EINVAL;
    p->layout = L;
    p->row_floats = row_floats;
    return LSR_OK;
}

// ---- point clouds: the files the published trainer's storePly writes and COLMAP conversions produce ----

constexpr int kMaxPointProps = 1024;      // scalar properties per vertex
constexpr int kRowBatchBytes = 1 << 16;   // rows are read through a buffer of this size (>= one row: 1024 x 8 bytes)

// Size in bytes of a PLY scalar type under either of its spellings, 0 for anything else.  *is_float: float / double.
int scalar_size(const char *t, bool *is_float) {
    static const struct { const char *a, *b; int size; bool flt; } types[] = {
        {"char", "int8", 1, false}, {"uchar", "uint8", 1, false}, {"short", "int16", 2, false}, {"ushort", "uint16", 2, false},
        {"int", "int32", 4, false}, {"uint", "uint32", 4, false}, {"float", "float32", 4, true}, {"double", "float64", 8, true}};
    for (const auto &e : types)
        if (!strcmp(t, e.a) || !strcmp(t, e.b)) { *is_float = e.flt; return e.size; }
    return 0;
}

struct PointsParsed {
    int64_t n, data_offset, stride;       // stride in bytes
    int32_t xyz[3], xyz_size[3];          // byte offsets inside a row; 4 (float) or 8 (double)
    int32_t rgb[3];                       // byte offsets of the uchar colours; has_colors says whether they are there
    bool has_colors;
};

int parse_points(FILE *f, PointsParsed *out) {
    PointsParsed P;
    memset(&P, 0, sizeof(P));
    static const char *const xyz_names[] = {"x", "y", "z"}, *const rgb_names[] = {"red", "green", "blue"};
    bool seen_xyz[3] = {}, seen_rgb[3] = {};
    bool have_format = false, have_element = false, ended = false;
    int props = 0;
    char line[kMaxLine + 1];
    char *tok[kMaxTokens];
    long consumed = 0;

    if (read_line(f, line, &consumed) != 1 || strcmp(line, "ply") != 0) return LSR_EINVAL;
    while (!ended) {
        if (consumed > kMaxHeaderBytes) return LSR_EINVAL;
        if (read_line(f, line, &consumed) != 1) return LSR_EINVAL;
        if (!strncmp(line, "comment", 7) && (line[7] == 0 || line[7] == ' ' || line[7] == '\t')) continue;
        if (!strncmp(line, "obj_info", 8) && (line[8] == 0 || line[8] == ' ' || line[8] == '\t')) continue;
        const int nt = tokenize(line, tok);
        if (nt == 0 || nt > kMaxTokens) return LSR_EINVAL;
        if (!strcmp(tok[0], "end_header")) {
            if (nt != 1) return LSR_EINVAL;
            ended = true;
        } else if (!strcmp(tok[0], "format")) {
            if (nt != 3 || have_format || have_element) return LSR_EINVAL;
            if (strcmp(tok[1], "binary_little_endian") != 0 || strcmp(tok[2], "1.0") != 0) return LSR_EUNSUPPORTED;
            have_format = true;
        } else if (!strcmp(tok[0], "element")) {
            if (nt != 3 || !have_format) return LSR_EINVAL;
            if (have_element || strcmp(tok[1], "vertex") != 0) return LSR_EUNSUPPORTED;
            if (parse_i64(tok[2], &P.n) != 0 || P.n < 0) return LSR_EINVAL;
            have_element = true;
        } else if (!strcmp(tok[0], "property")) {
            if (!have_element || nt < 3) return LSR_EINVAL;
            if (!strcmp(tok[1], "list")) return LSR_EUNSUPPORTED;
            if (nt != 3) return LSR_EINVAL;
            bool is_float = false;
            const int size = scalar_size(tok[1], &is_float);
            if (!size) return LSR_EINVAL;                                   // not a PLY scalar type
            if (props == kMaxPointProps) return LSR_EUNSUPPORTED;
            ++props;
            const int32_t at = (int32_t)P.stride;                           // <= 1024 x 8
            P.stride += size;
            for (int k = 0; k < 3; ++k) {
                if (!strcmp(tok[2], xyz_names[k])) {
                    if (seen_xyz[k]) return LSR_EINVAL;                     // given twice
                    if (!is_float) return LSR_EUNSUPPORTED;
                    seen_xyz[k] = true; P.xyz[k] = at; P.xyz_size[k] = size;
                }
                if (!strcmp(tok[2], rgb_names[k])) {
                    if (seen_rgb[k]) return LSR_EINVAL;
                    if (size != 1 || (strcmp(tok[1], "uchar") != 0 && strcmp(tok[1], "uint8") != 0)) return LSR_EUNSUPPORTED;
                    seen_rgb[k] = true; P.rgb[k] = at;
                }
            }
        } else {
            return LSR_EINVAL;
        }
    }
    if (!have_format || !have_element) return LSR_EINVAL;
    if (!seen_xyz[0] || !seen_xyz[1] || !seen_xyz[2]) return LSR_EINVAL;
    const int colours = (int)seen_rgb[0] + (int)seen_rgb[1] + (int)seen_rgb[2];
    if (colours != 0 && colours != 3) return LSR_EUNSUPPORTED;              // only some of the three
    P.has_colors = colours == 3;
    P.data_offset = consumed;
    // size: header + n * stride bytes must be there (stride >= 12 here); n * 3 floats must be a size the caller can hold
    if (P.n > INT64_MAX / 16 / P.stride) return LSR_EINVAL;
    if (fseeko(f, 0, SEEK_END) != 0) return LSR_EINVAL;
    const int64_t size = (int64_t)ftello(f);
    if (size < P.data_offset || size - P.data_offset < P.n * P.stride) return LSR_EINVAL;
    *out = P;
    return LSR_OK;
}

}  // namespace

extern "C" {

int lsr_ply_read_header(const char *path, lsr_ply_layout *layout) {
    if (!path || !layout) return LSR_ENULL;
    FILE *f = fopen(path, "rb");
    if (!f) return LSR_EINVAL;
    Parsed p;
    const int rc = parse(f, &p);
    fclose(f);
    if (rc == LSR_OK) *layout = p.layout;
    return rc;
}

int lsr_ply_read_rows(const char *path, float *rows_host, int64_t capacity_floats) {
    if (!path) return LSR_ENULL;
    FILE *f = fopen(path, "rb");
    if (!f) return LSR_EINVAL;
    Parsed p;
    int rc = parse(f, &p);
    if (rc == LSR_OK && capacity_floats < p.row_floats) rc = LSR_EINVAL;
    if (rc == LSR_OK && p.row_floats > 0 && !rows_host) rc = LSR_ENULL;
    if (rc == LSR_OK && p.row_floats > 0) {
        // (a file that shrinks between the size check and here gives a short read: reported, and the buffer then
        // holds a prefix of the rows)
        if (fseeko(f, (off_t)p.layout.data_offset, SEEK_SET) != 0 ||
            fread(rows_host, sizeof(float), (size_t)p.row_floats, f) != (size_t)p.row_floats)
            rc = LSR_EINVAL;
    }
    fclose(f);
    return rc;
}

int lsr_ply_read_points_header(const char *path, int64_t *n, int32_t *has_colors) {
    if (!path || !n || !has_colors) return LSR_ENULL;
    FILE *f = fopen(path, "rb");
    if (!f) return LSR_EINVAL;
    PointsParsed p;
    const int rc = parse_points(f, &p);
    fclose(f);
    if (rc == LSR_OK) { *n = p.n; *has_colors = p.has_colors ? 1 : 0; }
    return rc;
}

int lsr_ply_read_points(const char *path, float *xyz_host, float *rgb_host, int64_t capacity_points) {
    if (!path) return LSR_ENULL;
    FILE *f = fopen(path, "rb");
    if (!f) return LSR_EINVAL;
    PointsParsed p;
    int rc = parse_points(f, &p);
    if (rc == LSR_OK && capacity_points < p.n) rc = LSR_EINVAL;
    if (rc == LSR_OK && p.n > 0 && !xyz_host) rc = LSR_ENULL;
    if (rc == LSR_OK && p.n > 0) {
        // (a file that shrinks between the size check and here gives a short read: reported, and the buffers then hold
        // a prefix of the points)
        static_assert(kMaxPointProps * 8 <= kRowBatchBytes, "one row fits the batch buffer");
        unsigned char buf[kRowBatchBytes];
        const int64_t per_batch = kRowBatchBytes / p.stride;
        const bool colours = p.has_colors && rgb_host;
        if (fseeko(f, (off_t)p.data_offset, SEEK_SET) != 0) rc = LSR_EINVAL;
        for (int64_t done = 0; rc == LSR_OK && done < p.n; ) {
            const int64_t rows = p.n - done < per_batch ? p.n - done : per_batch;
            if (fread(buf, (size_t)p.stride, (size_t)rows, f) != (size_t)rows) { rc = LSR_EINVAL; break; }
            for (int64_t r = 0; r < rows; ++r) {
                const unsigned char *row = buf + r * p.stride;
                for (int k = 0; k < 3; ++k) {
                    float v;
                    if (p.xyz_size[k] == 4) memcpy(&v, row + p.xyz[k], 4);
                    else { double d; memcpy(&d, row + p.xyz[k], 8); v = (float)d; }
                    xyz_host[3 * (done + r) + k] = v;
                    if (colours) rgb_host[3 * (done + r) + k] = (float)row[p.rgb[k]] / 255.0f;
                }
            }
            done += rows;
        }
    }
    fclose(f);
    return rc;
}

}  // extern "C"
