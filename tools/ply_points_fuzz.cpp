// ply_points_fuzz.cpp — feeds the point cloud reader (lsr_ply_read_points_header / lsr_ply_read_points of
// latentsplat_amd/csrc/ply_reader.cpp) valid and malformed files under the host sanitizers.  The sibling of
// tools/ply_reader_fuzz.cpp; stand-alone: no HIP, no GPU, no Python.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude
//       tools/ply_points_fuzz.cpp latentsplat_amd/csrc/ply_reader.cpp -o ply_points_fuzz   (one command), then run it
//
// Part 1: the valid layouts (with and without colours and normals, double coordinates, shuffled order, an extra alpha,
// every scalar type, n = 0, more rows than one read batch) with their values checked, and the documented rejections
// (include/lsr_ply.h), each checked for its return code.
// Part 2: `rounds` (default 600) files derived from valid ones by a fixed-seed generator — header truncated, bytes
// overwritten, lines duplicated / dropped / swapped, counts and types replaced, rows truncated — each parsed and read
// into buffers of exactly the size the header asks for, so that any write past them is caught.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <string>
#include <vector>

#include "lsr_ply.h"

struct Prop { const char *type, *name; int size; };

static const Prop kStore[] = {{"float", "x", 4}, {"float", "y", 4}, {"float", "z", 4}, {"float", "nx", 4}, {"float", "ny", 4},
                              {"float", "nz", 4}, {"uchar", "red", 1}, {"uchar", "green", 1}, {"uchar", "blue", 1}};

static std::string header(const std::vector<Prop> &props, const std::string &count, const char *fmt = "binary_little_endian") {
    std::string h = "ply\nformat " + std::string(fmt) + " 1.0\ncomment fuzz\nelement vertex " + count + "\n";
    for (const Prop &p : props) h += std::string("property ") + p.type + " " + p.name + "\n";
    return h + "end_header\n";
}

static int stride_of(const std::vector<Prop> &props) { int s = 0; for (const Prop &p : props) s += p.size; return s; }

// rows whose coordinates are 0.5 r + k and whose colours are (r + k) mod 256; other bytes 0x3f
static std::string body(const std::vector<Prop> &props, int n) {
    std::string b((size_t)n * (size_t)stride_of(props), '\x3f');
    for (int r = 0; r < n; ++r) {
        size_t at = (size_t)r * (size_t)stride_of(props);
        for (const Prop &p : props) {
            const char *names = "xyz";
            for (int k = 0; k < 3; ++k)
                if (p.name[0] == names[k] && !p.name[1]) {
                    const double v = 0.5 * r + k;
                    const float f = (float)v;
                    if (p.size == 8) memcpy(&b[at], &v, 8); else memcpy(&b[at], &f, 4);
                }
            const char *const rgb[] = {"red", "green", "blue"};
            for (int k = 0; k < 3; ++k)
                if (!strcmp(p.name, rgb[k])) b[at] = (char)(unsigned char)((r + k) & 255);
            at += (size_t)p.size;
        }
    }
    return b;
}

static std::string replaced(std::string s, const std::string &what, const std::string &with) {
    const size_t at = s.find(what);
    if (at == std::string::npos) { fprintf(stderr, "fuzz: '%s' not in the header\n", what.c_str()); exit(2); }
    return s.replace(at, what.size(), with);
}

static void write_file(const char *path, const std::string &bytes) {
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(bytes.data(), 1, bytes.size(), f) != bytes.size() || fclose(f) != 0) { perror(path); exit(2); }
}

static int failures = 0;

// Parses and, if accepted, reads the points into exactly sized heap buffers.  Returns the header's code.
static int run(const char *path, bool check_values = false) {
    int64_t n = -7;
    int32_t has = -7;
    const int rc = lsr_ply_read_points_header(path, &n, &has);
    if (rc != LSR_OK) {
        if (n != -7 || has != -7) { fprintf(stderr, "fuzz: outputs written on failure\n"); ++failures; }
        float guard[6] = {1, 1, 1, 1, 1, 1};
        if (lsr_ply_read_points(path, guard, guard + 3, 1 << 30) != rc) { fprintf(stderr, "fuzz: read_points disagrees with the header\n"); ++failures; }
        for (float v : guard) if (v != 1.0f) { fprintf(stderr, "fuzz: buffers written on failure\n"); ++failures; break; }
        return rc;
    }
    if (n < 0 || (has != 0 && has != 1)) { fprintf(stderr, "fuzz: accepted an inconsistent header\n"); ++failures; return rc; }
    if (n > (16 << 20)) { fprintf(stderr, "fuzz: accepted %lld points from a tiny file\n", (long long)n); ++failures; return rc; }
    std::vector<float> xyz((size_t)n * 3), rgb((size_t)n * 3);      // heap: the sanitizer sees one float too many
    if (lsr_ply_read_points(path, xyz.data(), has ? rgb.data() : nullptr, n) != LSR_OK) { fprintf(stderr, "fuzz: points of an accepted file not read\n"); ++failures; }
    if (has && lsr_ply_read_points(path, xyz.data(), nullptr, n) != LSR_OK) { fprintf(stderr, "fuzz: colours could not be left out\n"); ++failures; }
    if (n > 0) {
        std::vector<float> small((size_t)(n - 1) * 3, 7.0f);
        if (lsr_ply_read_points(path, small.data(), nullptr, n - 1) != LSR_EINVAL) { fprintf(stderr, "fuzz: short buffer accepted\n"); ++failures; }
        for (float v : small) if (v != 7.0f) { fprintf(stderr, "fuzz: short buffer written\n"); ++failures; break; }
        if (lsr_ply_read_points(path, nullptr, nullptr, n) != LSR_ENULL) { fprintf(stderr, "fuzz: NULL buffer accepted\n"); ++failures; }
    }
    if (check_values)
        for (int64_t r = 0; r < n; ++r)
            for (int k = 0; k < 3; ++k) {
                if (xyz[3 * r + k] != (float)(0.5 * r + k)) { fprintf(stderr, "fuzz: wrong coordinate at row %lld\n", (long long)r); ++failures; return rc; }
                if (has && rgb[3 * r + k] != (float)((r + k) & 255) / 255.0f) { fprintf(stderr, "fuzz: wrong colour at row %lld\n", (long long)r); ++failures; return rc; }
            }
    return rc;
}

static void expect(const char *what, const char *path, const std::string &bytes, int code, bool check_values = false) {
    write_file(path, bytes);
    const int rc = run(path, check_values);
    if (rc != code) { fprintf(stderr, "fuzz: %s: code %d, expected %d\n", what, rc, code); ++failures; }
}

int main(int argc, char **argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 600;
    char path[] = "/tmp/ply_points_fuzz_XXXXXX";
    const int fd = mkstemp(path);
    if (fd < 0) { perror("mkstemp"); return 2; }
    fclose(fdopen(fd, "wb"));
    const std::vector<Prop> store(kStore, kStore + 9);
    const std::vector<Prop> bare(kStore, kStore + 3), no_colours(kStore, kStore + 6);
    const std::vector<Prop> no_normals = {kStore[0], kStore[1], kStore[2], kStore[6], kStore[7], kStore[8]};
    const std::vector<Prop> doubles = {{"double", "x", 8}, {"float64", "y", 8}, {"double", "z", 8}, kStore[6], kStore[7], kStore[8]};
    const std::vector<Prop> shuffled = {kStore[8], kStore[2], kStore[3], kStore[6], kStore[0], kStore[4], kStore[7], kStore[1], kStore[5]};
    const std::vector<Prop> alpha = {{"float32", "x", 4}, {"float32", "y", 4}, {"float32", "z", 4}, {"uint8", "red", 1}, {"uint8", "green", 1},
                                     {"uint8", "blue", 1}, {"uint8", "alpha", 1}};
    const std::vector<Prop> every = {{"int", "id", 4}, {"float", "x", 4}, {"char", "a", 1}, {"int8", "b", 1}, {"float", "y", 4}, {"double", "err", 8},
                                     {"double", "z", 8}, {"ushort", "c", 2}, {"uint16", "d", 2}, {"short", "e", 2}, {"int16", "f", 2},
                                     {"uint", "g", 4}, {"uint32", "h", 4}, {"int32", "i", 4}, kStore[6], kStore[7], kStore[8]};

    // ---- part 1: the documented cases ----
    const struct { const char *what; const std::vector<Prop> *props; } valid[] = {
        {"storePly", &store}, {"bare", &bare}, {"no colours", &no_colours}, {"no normals", &no_normals}, {"double", &doubles},
        {"shuffled", &shuffled}, {"alpha", &alpha}, {"every scalar type", &every}};
    for (const auto &v : valid)
        for (int n : {0, 1, 3, 5000})                                     // 5000 rows: more than one read batch
            expect(v.what, path, header(*v.props, std::to_string(n)) + body(*v.props, n), LSR_OK, true);
    const std::string h = header(store, "3"), b = body(store, 3);
    expect("valid, trailing bytes", path, h + b + "xyz", LSR_OK, true);
    expect("ascii", path, header(store, "3", "ascii") + b, LSR_EUNSUPPORTED);
    expect("big endian", path, header(store, "3", "binary_big_endian") + b, LSR_EUNSUPPORTED);
    expect("list property", path, replaced(h, "property float nx", "property list uchar int nx") + b, LSR_EUNSUPPORTED);
    expect("second element", path, replaced(h, "end_header", "element face 0\nend_header") + b, LSR_EUNSUPPORTED);
    expect("element other than vertex", path, replaced(h, "element vertex", "element point") + b, LSR_EUNSUPPORTED);
    expect("float colours", path, replaced(h, "property uchar green", "property float green") + b, LSR_EUNSUPPORTED);
    expect("char colours", path, replaced(h, "property uchar blue", "property char blue") + b, LSR_EUNSUPPORTED);
    expect("only some colours", path, replaced(h, "property uchar green", "property uchar grey") + b, LSR_EUNSUPPORTED);
    expect("integer coordinate", path, replaced(h, "property float y", "property int y") + b, LSR_EUNSUPPORTED);
    expect("missing z", path, replaced(h, "property float z\n", "property float w\n") + b, LSR_EINVAL);
    expect("x twice", path, replaced(h, "property float nx", "property float x") + b, LSR_EINVAL);
    expect("red twice", path, replaced(h, "property float nx", "property uchar red") + b, LSR_EINVAL);
    expect("unknown type", path, replaced(h, "property float nx", "property half nx") + b, LSR_EINVAL);
    expect("no end_header", path, replaced(h, "end_header\n", "") + b, LSR_EINVAL);
    expect("count -1", path, header(store, "-1") + b, LSR_EINVAL);
    expect("count 2^62", path, header(store, "4611686018427387904") + b, LSR_EINVAL);
    expect("count 2^64", path, header(store, "18446744073709551616") + b, LSR_EINVAL);
    expect("count not a number", path, header(store, "3x") + b, LSR_EINVAL);
    expect("truncated by one byte", path, h + b.substr(1), LSR_EINVAL);
    expect("over-long line", path, replaced(h, "comment fuzz", "comment " + std::string(400, 'a')) + b, LSR_EINVAL);
    expect("NUL in a line", path, replaced(h, "comment fuzz", std::string("comment fu\0z", 12)) + b, LSR_EINVAL);
    expect("property without a name", path, replaced(h, "property float nx", "property float") + b, LSR_EINVAL);
    expect("property before element", path, replaced(h, "comment fuzz", "property float q") + b, LSR_EINVAL);
    expect("not a ply", path, replaced(h, "ply\n", "plx\n") + b, LSR_EINVAL);
    expect("empty file", path, "", LSR_EINVAL);
    {
        std::string many = replaced(h, "end_header\n", "");
        for (int i = 0; i < 1024; ++i) many += "property uchar e" + std::to_string(i) + "\n";
        expect("too many properties", path, many + "end_header\n" + b, LSR_EUNSUPPORTED);
    }
    const int part1 = failures;

    // ---- part 2: seeded corruption ----
    std::mt19937 rng(20241019u);
    const auto below = [&](size_t n) { return (size_t)(rng() % (n ? n : 1)); };
    int accepted = 0, rejected = 0;
    for (int r = 0; r < rounds; ++r) {
        const std::vector<Prop> &props = *valid[below(8)].props;
        std::string hh = header(props, "3"), bb = body(props, 3);
        const int edits = 1 + (int)below(3);
        for (int e = 0; e < edits; ++e) {
            std::vector<size_t> starts = {0};
            for (size_t i = 0; i + 1 < hh.size(); ++i) if (hh[i] == '\n') starts.push_back(i + 1);
            const size_t li = below(starts.size()), ls = starts[li], le = li + 1 < starts.size() ? starts[li + 1] : hh.size();
            switch (below(9)) {
                case 0: hh.resize(below(hh.size() + 1)); break;                                  // truncate the header
                case 1: if (!hh.empty()) hh[below(hh.size())] = (char)below(256); break;         // one byte
                case 2: hh.insert(ls, hh.substr(ls, le - ls)); break;                            // duplicate a line
                case 3: hh.erase(ls, le - ls); break;                                            // drop a line
                case 4: { const size_t lj = below(starts.size()), js = starts[lj], je = lj + 1 < starts.size() ? starts[lj + 1] : hh.size();
                          const std::string a = hh.substr(ls, le - ls), c = hh.substr(js, je - js);
                          if (li < lj) { hh.replace(js, je - js, a); hh.replace(ls, le - ls, c); }
                          else if (lj < li) { hh.replace(ls, le - ls, c); hh.replace(js, je - js, a); } } break;   // swap two lines
                case 5: { const char *counts[] = {"0", "1", "4", "-3", "99999999999", "9223372036854775807", "1e3", ""};
                          const size_t at = hh.find("vertex ");
                          if (at != std::string::npos) { const size_t nl = hh.find('\n', at); if (nl != std::string::npos) hh.replace(at + 7, nl - at - 7, counts[below(8)]); } } break;
                case 6: bb.resize(below(bb.size() + 1)); break;                                  // truncate the rows
                case 7: { const char *types[] = {"double", "uchar", "float", "int", "short", "list", "int8", "float64"};
                          const size_t at = hh.find("property ", ls);
                          if (at != std::string::npos) { const size_t sp = hh.find(' ', at + 9); if (sp != std::string::npos) hh.replace(at + 9, sp - at - 9, types[below(8)]); } } break;
                default: hh.insert(below(hh.size() + 1), std::string(1 + below(300), (char)(32 + below(90)))); break;  // junk run
            }
        }
        write_file(path, hh + bb);
        (run(path) == LSR_OK ? accepted : rejected) += 1;
    }
    remove(path);
    printf("ply_points_fuzz: %d documented-case failures, %d failures in all; %d corrupted files: %d rejected, %d accepted "
           "(still well-formed)\n", part1, failures, rounds, rejected, accepted);
    return failures ? 1 : 0;
}
