// colmap_reader.cpp — host reader of COLMAP sparse models (include/lsr_colmap.h).  Plain C++ with no HIP in it, so that
// it can be built and run under the host sanitizers on its own (colmap_check.cpp, `make colmap-check`).  The input is
// untrusted: every read and every skip goes through File, which knows the file's size and refuses to pass it; every
// count is checked against the smallest payload it implies before anything is sized by it.
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "lsr_colmap.h"

static_assert(__BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__, "the binary layouts are read with memcpy on a little-endian host");

namespace {

thread_local char g_detail[320];

int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_detail, sizeof(g_detail), fmt, ap);
    va_end(ap);
    return code;
}

struct Model { const char *name; int params; };
// COLMAP's model ids in its own order; the first five are read, the others only named
constexpr Model kModels[] = {{"SIMPLE_PINHOLE", 3}, {"PINHOLE", 4}, {"SIMPLE_RADIAL", 4}, {"RADIAL", 5}, {"OPENCV", 8},
                             {"OPENCV_FISHEYE", -1}, {"FULL_OPENCV", -1}, {"FOV", -1}, {"SIMPLE_RADIAL_FISHEYE", -1},
                             {"RADIAL_FISHEYE", -1}, {"THIN_PRISM_FISHEYE", -1}};
constexpr int kNumModels = (int)(sizeof(kModels) / sizeof(kModels[0]));
constexpr int kSupportedModels = 5;

constexpr int64_t kMinCameraBytes = 4 + 4 + 8 + 8 + 3 * 8;        // SIMPLE_PINHOLE
constexpr int64_t kMinImageBytes = 4 + 7 * 8 + 4 + 1 + 8;         // an empty name, no observations
constexpr int64_t kMinPointBytes = 8 + 3 * 8 + 3 + 8 + 8;         // an empty track
constexpr int kToken = LSR_COLMAP_MAX_NAME + 1;                   // bytes of one kept text token, terminator included
constexpr int kMaxKept = 12;                                      // tokens kept per line: a camera line has 4 + 8

// A file that knows its size: nothing is read or skipped beyond it.
struct File {
    FILE *f = nullptr;
    int64_t size = 0, pos = 0;
    ~File() { if (f) fclose(f); }
    bool open(const std::string &path) {
        f = fopen(path.c_str(), "rb");
        if (!f) return false;
        if (fseeko(f, 0, SEEK_END) != 0) return false;
        size = (int64_t)ftello(f);
        return size >= 0 && fseeko(f, 0, SEEK_SET) == 0;
    }
    int64_t left() const { return size - pos; }
    bool get(void *dst, int64_t n) {
        if (n > left() || fread(dst, 1, (size_t)n, f) != (size_t)n) return false;
        pos += n;
        return true;
    }
    template <typename T> bool value(T *v) { return get(v, (int64_t)sizeof(T)); }
    // count records of `each` bytes: the product is formed only after the count is known to fit
    bool skip(uint64_t count, int64_t each) {
        if (count > (uint64_t)(left() / each)) return false;
        const int64_t n = (int64_t)count * each;
        if (n > 0 && fseeko(f, (off_t)n, SEEK_CUR) != 0) return false;
        pos += n;
        return true;
    }
    int byte() {
        if (pos >= size) return EOF;
        const int c = fgetc(f);
        if (c != EOF) ++pos;
        return c;
    }
};

bool exists(const std::string &path) {
    FILE *f = fopen(path.c_str(), "rb");
    if (f) fclose(f);
    return f != nullptr;
}

bool all_finite(const double *v, int n) {
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

template <typename T> bool has_duplicates(std::vector<T> v) {
    std::sort(v.begin(), v.end());
    return std::adjacent_find(v.begin(), v.end()) != v.end();
}

// ---- text: a line as blank-separated tokens ----

// One line: the first kMaxKept tokens into tok, all of them counted.  -1: a kept token longer than kToken - 1 bytes, or a
// NUL byte.  *eof: the file ended on this line (which may still hold tokens).
int read_tokens(File &f, char (*tok)[kToken], bool *eof) {
    int count = 0, len = 0;
    bool in_token = false;
    *eof = false;
    for (;;) {
        const int c = f.byte();
        if (c == EOF) *eof = true;
        if (c == 0) return -1;
        const bool blank = c == ' ' || c == '\t' || c == '\r';
        if (c == EOF || c == '\n' || blank) {
            if (in_token) {
                if (count < kMaxKept) tok[count][len] = 0;
                ++count;
                in_token = false;
            }
            if (!blank) return count;
            continue;
        }
        if (!in_token) { in_token = true; len = 0; }
        if (count < kMaxKept) {
            if (len == kToken - 1) return -1;
            tok[count][len++] = (char)c;
        }
    }
}

void skip_line(File &f) {
    for (int c = f.byte(); c != EOF && c != '\n'; c = f.byte()) {}
}

// The next token of the current line into tok (kToken bytes).  1: a token; 0: the line (or the file) ended first, and the
// line break is consumed; -1: an over-long token or a NUL byte.  After a token that the line break ended, *eol is set and
// the next call must not be made for this line.
int next_token(File &f, char *tok, bool *eol) {
    int len = 0;
    *eol = false;
    for (;;) {
        const int c = f.byte();
        if (c == 0) return -1;
        const bool blank = c == ' ' || c == '\t' || c == '\r';
        if (c == EOF || c == '\n' || blank) {
            if (c == EOF || c == '\n') *eol = true;
            if (len > 0) { tok[len] = 0; return 1; }
            if (*eol) return 0;
            continue;
        }
        if (len == kToken - 1) return -1;
        tok[len++] = (char)c;
    }
}

bool parse_u64(const char *s, uint64_t *out) {
    if (!*s) return false;
    uint64_t v = 0;
    for (; *s; ++s) {
        if (*s < '0' || *s > '9') return false;
        const uint64_t d = (uint64_t)(*s - '0');
        if (v > (UINT64_MAX - d) / 10) return false;
        v = v * 10 + d;
    }
    *out = v;
    return true;
}

bool parse_u32(const char *s, uint32_t *out) {
    uint64_t v;
    if (!parse_u64(s, &v) || v > UINT32_MAX) return false;
    *out = (uint32_t)v;
    return true;
}

// (strtod rounds correctly: a double written with 17 significant digits comes back in the same bits; "nan" and "inf"
// parse and are refused by the caller's finiteness check)
bool parse_f64(const char *s, double *out) {
    if (!*s) return false;
    char *end = nullptr;
    *out = strtod(s, &end);
    return end && *end == 0;
}

// ---- cameras ----

struct CameraOut { uint32_t *ids; int32_t *models; int64_t *sizes; double *params; int64_t capacity; };

int check_camera(const char *file, int64_t at, uint32_t id, int64_t model, uint64_t w, uint64_t h, const double *params, int P) {
    if (w < 1 || w > LSR_COLMAP_MAX_EXTENT || h < 1 || h > LSR_COLMAP_MAX_EXTENT)
        return fail(LSR_EINVAL, "%s: camera %u (record %lld) has size %llu x %llu, outside [1, %d]", file, id, (long long)at,
                    (unsigned long long)w, (unsigned long long)h, LSR_COLMAP_MAX_EXTENT);
    if (!all_finite(params, P))
        return fail(LSR_EINVAL, "%s: camera %u (record %lld) has a non-finite parameter", file, id, (long long)at);
    (void)model;
    return LSR_OK;
}

int store_camera(const CameraOut *out, int64_t at, uint32_t id, int32_t model, uint64_t w, uint64_t h, const double *params, int P) {
    if (!out) return LSR_OK;
    if (at >= out->capacity) return fail(LSR_EINVAL, "more cameras than the capacity %lld", (long long)out->capacity);
    out->ids[at] = id;
    out->models[at] = model;
    out->sizes[2 * at] = (int64_t)w;
    out->sizes[2 * at + 1] = (int64_t)h;
    for (int k = 0; k < LSR_COLMAP_MAX_PARAMS; ++k) out->params[LSR_COLMAP_MAX_PARAMS * at + k] = k < P ? params[k] : 0.0;
    return LSR_OK;
}

int unsupported_model(const char *file, uint32_t id, int64_t model) {
    if (model >= 0 && model < kNumModels)
        return fail(LSR_EUNSUPPORTED, "%s: camera %u has model %lld (%s); only SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL, RADIAL and "
                    "OPENCV are read", file, id, (long long)model, kModels[model].name);
    return fail(LSR_EUNSUPPORTED, "%s: camera %u has the unknown model id %lld", file, id, (long long)model);
}

int cameras_bin(const std::string &dir, const CameraOut *out, std::vector<uint32_t> *ids) {
    const char *file = "cameras.bin";
    File f;
    if (!f.open(dir + "/" + file)) return fail(LSR_EINVAL, "%s: cannot be opened", file);
    uint64_t n;
    if (!f.value(&n)) return fail(LSR_EINVAL, "%s: truncated before the count", file);
    if (n > (uint64_t)(f.left() / kMinCameraBytes))
        return fail(LSR_EINVAL, "%s: %llu cameras do not fit %lld bytes", file, (unsigned long long)n, (long long)f.left());
    ids->clear();
    ids->reserve((size_t)n);
    for (int64_t at = 0; at < (int64_t)n; ++at) {
        uint32_t id;
        int32_t model;
        uint64_t w, h;
        double params[LSR_COLMAP_MAX_PARAMS];
        if (!f.value(&id) || !f.value(&model) || !f.value(&w) || !f.value(&h))
            return fail(LSR_EINVAL, "%s: truncated in camera record %lld", file, (long long)at);
        if (model < 0 || model >= kSupportedModels) return unsupported_model(file, id, model);
        const int P = kModels[model].params;
        if (!f.get(params, 8 * P)) return fail(LSR_EINVAL, "%s: truncated in camera record %lld", file, (long long)at);
        int rc = check_camera(file, at, id, model, w, h, params, P);
        if (rc == LSR_OK) rc = store_camera(out, at, id, model, w, h, params, P);
        if (rc != LSR_OK) return rc;
        ids->push_back(id);
    }
    if (f.left() != 0) return fail(LSR_EINVAL, "%s: %lld trailing bytes", file, (long long)f.left());
    if (has_duplicates(*ids)) return fail(LSR_EINVAL, "%s: a camera id is given twice", file);
    return LSR_OK;
}

int cameras_txt(const std::string &dir, const CameraOut *out, std::vector<uint32_t> *ids) {
    const char *file = "cameras.txt";
    File f;
    if (!f.open(dir + "/" + file)) return fail(LSR_EINVAL, "%s: cannot be opened", file);
    std::vector<char> store((size_t)kMaxKept * kToken);
    char (*tok)[kToken] = (char (*)[kToken])store.data();
    ids->clear();
    bool eof = false;
    for (int64_t at = 0; !eof; ) {
        const int nt = read_tokens(f, tok, &eof);
        if (nt < 0) return fail(LSR_EINVAL, "%s: an over-long token or a NUL byte", file);
        if (nt == 0 || tok[0][0] == '#') continue;
        uint32_t id;
        uint64_t w, h;
        int model = -1;
        if (nt < 4 || !parse_u32(tok[0], &id) || !parse_u64(tok[2], &w) || !parse_u64(tok[3], &h))
            return fail(LSR_EINVAL, "%s: malformed camera record %lld", file, (long long)at);
        for (int m = 0; m < kNumModels; ++m)
            if (!strcmp(tok[1], kModels[m].name)) model = m;
        if (model < 0) return fail(LSR_EUNSUPPORTED, "%s: camera %u has the unknown model %.64s", file, id, tok[1]);
        if (model >= kSupportedModels) return unsupported_model(file, id, model);
        const int P = kModels[model].params;
        double params[LSR_COLMAP_MAX_PARAMS];
        if (nt != 4 + P) return fail(LSR_EINVAL, "%s: camera %u has %d parameters, %s takes %d", file, id, nt - 4, kModels[model].name, P);
        for (int k = 0; k < P; ++k)
            if (!parse_f64(tok[4 + k], &params[k])) return fail(LSR_EINVAL, "%s: malformed camera record %lld", file, (long long)at);
        int rc = check_camera(file, at, id, model, w, h, params, P);
        if (rc == LSR_OK) rc = store_camera(out, at, id, model, w, h, params, P);
        if (rc != LSR_OK) return rc;
        ids->push_back(id);
        ++at;
    }
    if (has_duplicates(*ids)) return fail(LSR_EINVAL, "%s: a camera id is given twice", file);
    return LSR_OK;
}

// ---- images ----

struct ImageOut {
    uint32_t *ids; double *qvec; double *tvec; uint32_t *camera_ids; char *names; int64_t *name_offsets;
    int64_t capacity, name_capacity;
};

// offsets[image_capacity + 1], xy[capacity][2], point_ids[capacity]
struct ObsOut { int64_t *offsets; double *xy; uint64_t *point_ids; int64_t image_capacity, capacity; };

struct ImageWalk {
    const std::vector<uint32_t> *cameras;   // sorted
    const ImageOut *out;
    std::vector<uint32_t> ids;
    int64_t name_bytes = 0;
    bool observations = false;              // parse the 2D observations instead of skipping them
    const ObsOut *obs = nullptr;            // ... and store those that carry a point
    int64_t obs_total = 0;                  // observations with a point so far
};

constexpr uint64_t kNoPoint = UINT64_MAX;   // images.bin: an observation without a 3D point (images.txt writes -1)

// The observations of image record `at` begin: its offset.
int begin_observations(ImageWalk *w, int64_t at) {
    if (const ObsOut *o = w->obs) {
        if (at >= o->image_capacity) return fail(LSR_EINVAL, "more images than the capacity %lld", (long long)o->image_capacity);
        o->offsets[at] = w->obs_total;
        o->offsets[at + 1] = w->obs_total;
    }
    return LSR_OK;
}

// Observation `k` of image record `at`; has_point: it carries the 3D point `point`.
int take_observation(const char *file, ImageWalk *w, int64_t at, int64_t k, double x, double y, bool has_point, uint64_t point) {
    if (!std::isfinite(x) || !std::isfinite(y))
        return fail(LSR_EINVAL, "%s: observation %lld of image record %lld has a non-finite position", file, (long long)k, (long long)at);
    if (!has_point) return LSR_OK;
    if (const ObsOut *o = w->obs) {
        if (w->obs_total >= o->capacity)
            return fail(LSR_EINVAL, "%s: more observations with a point than the capacity %lld (image record %lld)", file,
                        (long long)o->capacity, (long long)at);
        o->xy[2 * w->obs_total] = x;
        o->xy[2 * w->obs_total + 1] = y;
        o->point_ids[w->obs_total] = point;
        o->offsets[at + 1] = w->obs_total + 1;
    }
    ++w->obs_total;
    return LSR_OK;
}

// name: NUL-terminated, len bytes without the terminator
int take_image(const char *file, ImageWalk *w, uint32_t id, const double *q, const double *t, uint32_t camera, const char *name, int len) {
    const int64_t at = (int64_t)w->ids.size();
    if (!all_finite(q, 4) || !all_finite(t, 3))
        return fail(LSR_EINVAL, "%s: image %u (record %lld) has a non-finite pose", file, id, (long long)at);
    if (q[0] == 0.0 && q[1] == 0.0 && q[2] == 0.0 && q[3] == 0.0)
        return fail(LSR_EINVAL, "%s: image %u (record %lld) has a zero quaternion", file, id, (long long)at);
    if (!std::binary_search(w->cameras->begin(), w->cameras->end(), camera))
        return fail(LSR_EINVAL, "%s: image %u (record %lld) names camera %u, which the model does not have", file, id, (long long)at, camera);
    if (const ImageOut *o = w->out) {
        if (at >= o->capacity) return fail(LSR_EINVAL, "more images than the capacity %lld", (long long)o->capacity);
        if (len + 1 > o->name_capacity - w->name_bytes)
            return fail(LSR_EINVAL, "more name bytes than the capacity %lld", (long long)o->name_capacity);
        o->ids[at] = id;
        memcpy(o->qvec + 4 * at, q, 4 * sizeof(double));
        memcpy(o->tvec + 3 * at, t, 3 * sizeof(double));
        o->camera_ids[at] = camera;
        o->name_offsets[at] = w->name_bytes;
        memcpy(o->names + w->name_bytes, name, (size_t)len + 1);
        o->name_offsets[at + 1] = w->name_bytes + len + 1;
    }
    w->name_bytes += len + 1;
    w->ids.push_back(id);
    return LSR_OK;
}

int images_bin(const std::string &dir, ImageWalk *w) {
    const char *file = "images.bin";
    File f;
    if (!f.open(dir + "/" + file)) return fail(LSR_EINVAL, "%s: cannot be opened", file);
    uint64_t n;
    if (!f.value(&n)) return fail(LSR_EINVAL, "%s: truncated before the count", file);
    if (n > (uint64_t)(f.left() / kMinImageBytes))
        return fail(LSR_EINVAL, "%s: %llu images do not fit %lld bytes", file, (unsigned long long)n, (long long)f.left());
    w->ids.reserve((size_t)n);
    if (w->out) w->out->name_offsets[0] = 0;
    char name[LSR_COLMAP_MAX_NAME + 1];
    for (int64_t at = 0; at < (int64_t)n; ++at) {
        uint32_t id, camera;
        double q[4], t[3];
        uint64_t m;
        if (!f.value(&id) || !f.get(q, sizeof(q)) || !f.get(t, sizeof(t)) || !f.value(&camera))
            return fail(LSR_EINVAL, "%s: truncated in image record %lld", file, (long long)at);
        int len = 0;
        for (;;) {
            const int c = f.byte();
            if (c == EOF) return fail(LSR_EINVAL, "%s: the name of image %u (record %lld) has no terminator", file, id, (long long)at);
            if (c == 0) break;
            if (len == LSR_COLMAP_MAX_NAME)
                return fail(LSR_EINVAL, "%s: the name of image %u (record %lld) is longer than %d bytes", file, id, (long long)at, LSR_COLMAP_MAX_NAME);
            name[len++] = (char)c;
        }
        name[len] = 0;
        if (!f.value(&m)) return fail(LSR_EINVAL, "%s: truncated in the observations of image record %lld", file, (long long)at);
        if (!w->observations) {
            if (!f.skip(m, 24)) return fail(LSR_EINVAL, "%s: truncated in the observations of image record %lld", file, (long long)at);
        } else {
            // the count against what is left of the file before the loop is sized by it
            if (m > (uint64_t)(f.left() / 24))
                return fail(LSR_EINVAL, "%s: truncated in the observations of image record %lld", file, (long long)at);
            int rc = begin_observations(w, at);
            for (int64_t k = 0; rc == LSR_OK && k < (int64_t)m; ++k) {
                double xy[2];
                uint64_t point;
                if (!f.get(xy, sizeof(xy)) || !f.value(&point))
                    return fail(LSR_EINVAL, "%s: truncated in the observations of image record %lld", file, (long long)at);
                rc = take_observation(file, w, at, k, xy[0], xy[1], point != kNoPoint, point);
            }
            if (rc != LSR_OK) return rc;
        }
        const int rc = take_image(file, w, id, q, t, camera, name, len);
        if (rc != LSR_OK) return rc;
    }
    if (f.left() != 0) return fail(LSR_EINVAL, "%s: %lld trailing bytes", file, (long long)f.left());
    if (has_duplicates(w->ids)) return fail(LSR_EINVAL, "%s: an image id is given twice", file);
    return LSR_OK;
}

int images_txt(const std::string &dir, ImageWalk *w) {
    const char *file = "images.txt";
    File f;
    if (!f.open(dir + "/" + file)) return fail(LSR_EINVAL, "%s: cannot be opened", file);
    std::vector<char> store((size_t)kMaxKept * kToken);
    char (*tok)[kToken] = (char (*)[kToken])store.data();
    if (w->out) w->out->name_offsets[0] = 0;
    bool eof = false;
    while (!eof) {
        const int nt = read_tokens(f, tok, &eof);
        if (nt < 0) return fail(LSR_EINVAL, "%s: an over-long token or a NUL byte", file);
        if (nt == 0 || tok[0][0] == '#') continue;
        const long long at = (long long)w->ids.size();
        uint32_t id, camera;
        double qt[7];
        if (nt != 10 || !parse_u32(tok[0], &id) || !parse_u32(tok[8], &camera)) return fail(LSR_EINVAL, "%s: malformed image record %lld", file, at);
        for (int k = 0; k < 7; ++k)
            if (!parse_f64(tok[1 + k], &qt[k])) return fail(LSR_EINVAL, "%s: malformed image record %lld", file, at);
        int rc = take_image(file, w, id, qt, qt + 4, camera, tok[9], (int)strlen(tok[9]));
        if (rc != LSR_OK) return rc;
        if (!w->observations) {
            if (!eof) skip_line(f);           // the 2D observations: possibly empty, not parsed by this walk
            continue;
        }
        rc = begin_observations(w, at);
        if (rc != LSR_OK) return rc;
        // the next line, whatever it holds, is this image's: X Y POINT3D_ID triples, -1 for an observation without a point
        bool eol = eof;
        for (int64_t k = 0; !eol; ++k) {
            double xy[2] = {0.0, 0.0};
            uint64_t point = 0;
            bool has_point = true;
            int field = 0;
            for (; field < 3 && !eol; ++field) {
                const int got = next_token(f, tok[0], &eol);
                if (got < 0) return fail(LSR_EINVAL, "%s: an over-long token or a NUL byte", file);
                if (got == 0) break;
                bool ok;
                if (field < 2) ok = parse_f64(tok[0], &xy[field]);
                else if (!strcmp(tok[0], "-1")) { has_point = false; ok = true; }
                else ok = parse_u64(tok[0], &point);
                if (!ok) return fail(LSR_EINVAL, "%s: malformed observation %lld of image record %lld", file, (long long)k, at);
            }
            if (field == 0) break;            // the line ended after a whole triple (or held none)
            if (field != 3) return fail(LSR_EINVAL, "%s: observation %lld of image record %lld is incomplete", file, (long long)k, at);
            rc = take_observation(file, w, at, k, xy[0], xy[1], has_point, point);
            if (rc != LSR_OK) return rc;
        }
        if (f.left() == 0) eof = true;
    }
    if (has_duplicates(w->ids)) return fail(LSR_EINVAL, "%s: an image id is given twice", file);
    return LSR_OK;
}

// ---- points ----

struct PointOut { uint64_t *ids; double *xyz; uint8_t *rgb; double *errors; int64_t capacity; };

int take_point(const char *file, const PointOut *out, std::vector<uint64_t> *ids, uint64_t id, const double *xyz, const uint8_t *rgb, double error) {
    const int64_t at = (int64_t)ids->size();
    if (!all_finite(xyz, 3) || !std::isfinite(error))
        return fail(LSR_EINVAL, "%s: point %llu (record %lld) has a non-finite number", file, (unsigned long long)id, (long long)at);
    if (out) {
        if (at >= out->capacity) return fail(LSR_EINVAL, "more points than the capacity %lld", (long long)out->capacity);
        out->ids[at] = id;
        memcpy(out->xyz + 3 * at, xyz, 3 * sizeof(double));
        memcpy(out->rgb + 3 * at, rgb, 3);
        out->errors[at] = error;
    }
    ids->push_back(id);
    return LSR_OK;
}

int points_bin(const std::string &dir, const PointOut *out, std::vector<uint64_t> *ids) {
    const char *file = "points3D.bin";
    File f;
    if (!f.open(dir + "/" + file)) return fail(LSR_EINVAL, "%s: cannot be opened", file);
    uint64_t n;
    if (!f.value(&n)) return fail(LSR_EINVAL, "%s: truncated before the count", file);
    if (n > (uint64_t)(f.left() / kMinPointBytes))
        return fail(LSR_EINVAL, "%s: %llu points do not fit %lld bytes", file, (unsigned long long)n, (long long)f.left());
    ids->reserve((size_t)n);
    for (int64_t at = 0; at < (int64_t)n; ++at) {
        uint64_t id, L;
        double xyz[3], error;
        uint8_t rgb[3];
        if (!f.value(&id) || !f.get(xyz, sizeof(xyz)) || !f.get(rgb, 3) || !f.value(&error) || !f.value(&L) || !f.skip(L, 8))
            return fail(LSR_EINVAL, "%s: truncated in point record %lld", file, (long long)at);
        const int rc = take_point(file, out, ids, id, xyz, rgb, error);
        if (rc != LSR_OK) return rc;
    }
    if (f.left() != 0) return fail(LSR_EINVAL, "%s: %lld trailing bytes", file, (long long)f.left());
    if (has_duplicates(*ids)) return fail(LSR_EINVAL, "%s: a point id is given twice", file);
    return LSR_OK;
}

int points_txt(const std::string &dir, const PointOut *out, std::vector<uint64_t> *ids) {
    const char *file = "points3D.txt";
    File f;
    if (!f.open(dir + "/" + file)) return fail(LSR_EINVAL, "%s: cannot be opened", file);
    std::vector<char> store((size_t)kMaxKept * kToken);
    char (*tok)[kToken] = (char (*)[kToken])store.data();
    bool eof = false;
    while (!eof) {
        const int nt = read_tokens(f, tok, &eof);          // the track's tokens beyond the twelfth are counted, not kept
        if (nt < 0) return fail(LSR_EINVAL, "%s: an over-long token or a NUL byte", file);
        if (nt == 0 || tok[0][0] == '#') continue;
        const long long at = (long long)ids->size();
        uint64_t id;
        double xyz[3], error;
        uint8_t rgb[3];
        bool ok = nt >= 8 && (nt - 8) % 2 == 0 && parse_u64(tok[0], &id) && parse_f64(tok[7], &error);
        for (int k = 0; ok && k < 3; ++k) {
            uint64_t c = 0;
            ok = parse_f64(tok[1 + k], &xyz[k]) && parse_u64(tok[4 + k], &c) && c <= 255;
            rgb[k] = (uint8_t)c;
        }
        if (!ok) return fail(LSR_EINVAL, "%s: malformed point record %lld", file, at);
        const int rc = take_point(file, out, ids, id, xyz, rgb, error);
        if (rc != LSR_OK) return rc;
    }
    if (has_duplicates(*ids)) return fail(LSR_EINVAL, "%s: a point id is given twice", file);
    return LSR_OK;
}

// ---- the three files of a directory ----

int find_format(const std::string &dir, int *format) {
    if (exists(dir + "/cameras.bin")) { *format = LSR_COLMAP_BINARY; return LSR_OK; }
    if (exists(dir + "/cameras.txt")) { *format = LSR_COLMAP_TEXT; return LSR_OK; }
    return fail(LSR_EINVAL, "neither cameras.bin nor cameras.txt can be opened in the model directory");
}

int read_cameras(const std::string &dir, int format, const CameraOut *out, std::vector<uint32_t> *ids) {
    return format == LSR_COLMAP_BINARY ? cameras_bin(dir, out, ids) : cameras_txt(dir, out, ids);
}

int read_images(const std::string &dir, int format, const ImageOut *out, int64_t *count, int64_t *name_bytes,
                bool observations = false, const ObsOut *obs = nullptr, int64_t *obs_total = nullptr) {
    std::vector<uint32_t> cameras;
    int rc = read_cameras(dir, format, nullptr, &cameras);
    if (rc != LSR_OK) return rc;
    std::sort(cameras.begin(), cameras.end());
    ImageWalk w;
    w.cameras = &cameras;
    w.out = out;
    w.observations = observations;
    w.obs = obs;
    rc = format == LSR_COLMAP_BINARY ? images_bin(dir, &w) : images_txt(dir, &w);
    if (rc != LSR_OK) return rc;
    *count = (int64_t)w.ids.size();
    *name_bytes = w.name_bytes;
    if (obs_total) *obs_total = w.obs_total;
    return LSR_OK;
}

int read_points(const std::string &dir, int format, const PointOut *out, int64_t *count) {
    std::vector<uint64_t> ids;
    const int rc = format == LSR_COLMAP_BINARY ? points_bin(dir, out, &ids) : points_txt(dir, out, &ids);
    if (rc == LSR_OK) *count = (int64_t)ids.size();
    return rc;
}

// All three files walked and checked as lsr_colmap_count walks them, the observations parsed (and stored, with `obs`).
int walk_observations(const char *dir, const ObsOut *obs, int64_t *total) {
    int format = 0;
    int64_t images = 0, name_bytes = 0, points = 0;
    int rc = find_format(dir, &format);
    if (rc == LSR_OK) rc = read_images(dir, format, nullptr, &images, &name_bytes, true, obs, total);
    if (rc == LSR_OK) rc = read_points(dir, format, nullptr, &points);
    if (rc == LSR_OK && obs && images < obs->image_capacity)          // (fewer images than the caller sized for: the tail)
        for (int64_t k = images + 1; k <= obs->image_capacity; ++k) obs->offsets[k] = *total;
    return rc;
}

}  // namespace

extern "C" {

const char *lsr_colmap_last_error(void) { return g_detail; }

int lsr_colmap_count(const char *dir, lsr_colmap_counts *counts) {
    g_detail[0] = 0;
    if (!dir || !counts) return fail(LSR_ENULL, "a NULL argument");
    lsr_colmap_counts c;
    memset(&c, 0, sizeof(c));
    int format = 0;
    int rc = find_format(dir, &format);
    std::vector<uint32_t> cameras;
    if (rc == LSR_OK) rc = read_cameras(dir, format, nullptr, &cameras);
    if (rc == LSR_OK) rc = read_images(dir, format, nullptr, &c.images, &c.name_bytes);
    if (rc == LSR_OK) rc = read_points(dir, format, nullptr, &c.points);
    if (rc != LSR_OK) return rc;
    c.cameras = (int64_t)cameras.size();
    c.format = format;
    *counts = c;
    return LSR_OK;
}

int lsr_colmap_read_cameras(const char *dir, uint32_t *ids, int32_t *models, int64_t *sizes, double *params, int64_t capacity) {
    g_detail[0] = 0;
    if (!dir || (capacity > 0 && (!ids || !models || !sizes || !params))) return fail(LSR_ENULL, "a NULL argument");
    const CameraOut out = {ids, models, sizes, params, capacity < 0 ? 0 : capacity};
    int format = 0;
    std::vector<uint32_t> seen;
    const int rc = find_format(dir, &format);
    return rc != LSR_OK ? rc : read_cameras(dir, format, &out, &seen);
}

int lsr_colmap_read_images(const char *dir, uint32_t *ids, double *qvec, double *tvec, uint32_t *camera_ids, char *names,
                           int64_t *name_offsets, int64_t capacity, int64_t name_capacity) {
    g_detail[0] = 0;
    if (!dir || !name_offsets || (capacity > 0 && (!ids || !qvec || !tvec || !camera_ids || !names))) return fail(LSR_ENULL, "a NULL argument");
    const ImageOut out = {ids, qvec, tvec, camera_ids, names, name_offsets, capacity < 0 ? 0 : capacity, name_capacity < 0 ? 0 : name_capacity};
    int format = 0;
    int64_t count = 0, name_bytes = 0;
    const int rc = find_format(dir, &format);
    return rc != LSR_OK ? rc : read_images(dir, format, &out, &count, &name_bytes);
}

int lsr_colmap_read_points(const char *dir, uint64_t *ids, double *xyz, uint8_t *rgb, double *errors, int64_t capacity) {
    g_detail[0] = 0;
    if (!dir || (capacity > 0 && (!ids || !xyz || !rgb || !errors))) return fail(LSR_ENULL, "a NULL argument");
    const PointOut out = {ids, xyz, rgb, errors, capacity < 0 ? 0 : capacity};
    int format = 0;
    int64_t count = 0;
    const int rc = find_format(dir, &format);
    return rc != LSR_OK ? rc : read_points(dir, format, &out, &count);
}

int lsr_colmap_count_observations(const char *dir, int64_t *total) {
    g_detail[0] = 0;
    if (!dir || !total) return fail(LSR_ENULL, "a NULL argument");
    int64_t n = 0;
    const int rc = walk_observations(dir, nullptr, &n);
    if (rc == LSR_OK) *total = n;
    return rc;
}

int lsr_colmap_read_observations(const char *dir, int64_t *offsets, double *xy, uint64_t *point_ids, int64_t image_capacity,
                                 int64_t capacity) {
    g_detail[0] = 0;
    if (!dir || !offsets || (capacity > 0 && (!xy || !point_ids))) return fail(LSR_ENULL, "a NULL argument");
    const ObsOut out = {offsets, xy, point_ids, image_capacity < 0 ? 0 : image_capacity, capacity < 0 ? 0 : capacity};
    offsets[0] = 0;
    int64_t n = 0;
    return walk_observations(dir, &out, &n);
}

}  // extern "C"
