// ply_reader_fuzz.cpp — feeds the .ply scene reader (latentsplat_amd/csrc/ply_reader.cpp) malformed files under the
// host sanitizers.  Stand-alone: no HIP, no GPU, no Python.
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude
//       tools/ply_reader_fuzz.cpp latentsplat_amd/csrc/ply_reader.cpp -o ply_reader_fuzz   (one command), then run it
//
// Part 1: the malformed files of the documented rejections (include/lsr_ply.h), each checked for its return code.
// Part 2: `rounds` (default 600) headers derived from valid ones by a fixed-seed generator — truncated at a random
// byte, bytes overwritten, lines duplicated / dropped / swapped, counts replaced — each parsed and read into a buffer
// of exactly the size the header asks for, placed at the end of its allocation so that any write past it is caught.
// The layout of every accepted file is checked for consistency (offsets inside the row, data inside the file).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <string>
#include <vector>

#include "lsr_ply.h"

static std::string header(int K, const char *fmt = "binary_little_endian", const std::string &count = "3") {
    std::string h = "ply\nformat " + std::string(fmt) + " 1.0\ncomment fuzz\nelement vertex " + count + "\n";
    const char *head[] = {"x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"};
    for (const char *p : head) h += std::string("property float ") + p + "\n";
    for (int i = 0; i < 3 * (K - 1); ++i) h += "property float f_rest_" + std::to_string(i) + "\n";
    const char *tail[] = {"opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"};
    for (const char *p : tail) h += std::string("property float ") + p + "\n";
    return h + "end_header\n";
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

// Parses and, if accepted, reads the rows into an exactly sized heap buffer.  Returns the header's code.
static int run(const char *path, int64_t *floats_out = nullptr) {
    lsr_ply_layout canary, L;
    memset(&canary, 0x5a, sizeof(canary));
    L = canary;
    const int rc = lsr_ply_read_header(path, &L);
    if (rc != LSR_OK) {
        if (memcmp(&L, &canary, sizeof(L)) != 0) { fprintf(stderr, "fuzz: layout written on failure\n"); ++failures; }
        float guard = 1.0f;
        if (lsr_ply_read_rows(path, &guard, 1 << 30) != rc || guard != 1.0f) { fprintf(stderr, "fuzz: read_rows disagrees with read_header\n"); ++failures; }
        return rc;
    }
    bool ok = L.n >= 0 && L.stride >= 14 && L.stride <= LSR_PLY_MAX_STRIDE && L.data_offset > 0;
    const int K = L.sh_coeffs;
    ok = ok && (K == 1 || K == 4 || K == 9 || K == 16 || K == 25);
    const auto inside = [&](const int32_t *o, int n) { for (int i = 0; i < n; ++i) if (o[i] < 0 || o[i] >= L.stride) return false; return true; };
    ok = ok && inside(L.xyz, 3) && inside(L.f_dc, 3) && inside(&L.opacity, 1) && inside(L.scale, 3) && inside(L.rot, 4) && inside(L.f_rest, 3 * (K - 1));
    if (!ok) { fprintf(stderr, "fuzz: accepted an inconsistent layout\n"); ++failures; return rc; }
    const int64_t floats = L.n * L.stride;
    if (floats_out) *floats_out = floats;
    if (floats > (64 << 20)) { fprintf(stderr, "fuzz: accepted %lld floats from a tiny file\n", (long long)floats); ++failures; return rc; }
    std::vector<float> exact((size_t)floats);                        // heap: the sanitizer sees one float too many
    if (lsr_ply_read_rows(path, exact.data(), floats) != LSR_OK) { fprintf(stderr, "fuzz: rows of an accepted file not read\n"); ++failures; }
    if (floats > 0) {
        std::vector<float> small((size_t)floats - 1, 7.0f);
        if (lsr_ply_read_rows(path, small.data(), floats - 1) != LSR_EINVAL) { fprintf(stderr, "fuzz: short buffer accepted\n"); ++failures; }
        for (float v : small) if (v != 7.0f) { fprintf(stderr, "fuzz: short buffer written\n"); ++failures; break; }
    }
    return rc;
}

static void expect(const char *what, const char *path, const std::string &bytes, int code) {
    write_file(path, bytes);
    const int rc = run(path);
    if (rc != code) { fprintf(stderr, "fuzz: %s: code %d, expected %d\n", what, rc, code); ++failures; }
}

int main(int argc, char **argv) {
    const int rounds = argc > 1 ? atoi(argv[1]) : 600;
    char path[] = "/tmp/ply_reader_fuzz_XXXXXX";
    const int fd = mkstemp(path);
    if (fd < 0) { perror("mkstemp"); return 2; }
    fclose(fdopen(fd, "wb"));
    const auto body = [](int K, int n) { return std::string((size_t)n * (size_t)(14 + 3 * K) * 4, '\x3f'); };

    // ---- part 1: the documented cases ----
    const std::string h4 = header(4), b4 = body(4, 3);
    expect("valid K=4", path, h4 + b4, LSR_OK);
    for (int K : {1, 9, 16, 25}) expect("valid", path, header(K) + body(K, 3), LSR_OK);
    expect("valid, trailing bytes", path, h4 + b4 + "xyz", LSR_OK);
    expect("empty scene", path, header(4, "binary_little_endian", "0"), LSR_OK);
    expect("ascii", path, header(4, "ascii") + b4, LSR_EUNSUPPORTED);
    expect("big endian", path, header(4, "binary_big_endian") + b4, LSR_EUNSUPPORTED);
    expect("uchar property", path, replaced(h4, "property float nx", "property uchar nx") + b4, LSR_EUNSUPPORTED);
    expect("list property", path, replaced(h4, "property float nx", "property list uchar int nx") + b4, LSR_EUNSUPPORTED);
    expect("second element", path, replaced(h4, "end_header", "element face 0\nend_header") + b4, LSR_EUNSUPPORTED);
    expect("f_rest count 5", path, replaced(replaced(replaced(replaced(h4, "property float f_rest_5\n", ""), "property float f_rest_6\n", ""),
                                                              "property float f_rest_7\n", ""), "property float f_rest_8\n", "") + b4, LSR_EUNSUPPORTED);
    expect("f_rest beyond degree 4", path, replaced(h4, "f_rest_8", "f_rest_72") + b4, LSR_EUNSUPPORTED);
    expect("missing opacity", path, replaced(h4, "property float opacity\n", "") + b4, LSR_EINVAL);
    expect("duplicate x", path, replaced(h4, "property float nx", "property float x") + b4, LSR_EINVAL);
    expect("f_rest gap", path, replaced(h4, "f_rest_8", "f_rest_3") + b4, LSR_EINVAL);
    expect("no end_header", path, replaced(h4, "end_header\n", "") + b4, LSR_EINVAL);
    expect("count -1", path, header(4, "binary_little_endian", "-1") + b4, LSR_EINVAL);
    expect("count 2^62", path, header(4, "binary_little_endian", "4611686018427387904") + b4, LSR_EINVAL);
    expect("count 2^64", path, header(4, "binary_little_endian", "18446744073709551616") + b4, LSR_EINVAL);
    expect("count not a number", path, header(4, "binary_little_endian", "3x") + b4, LSR_EINVAL);
    expect("truncated by one byte", path, h4 + b4.substr(1), LSR_EINVAL);
    expect("over-long line", path, replaced(h4, "comment fuzz", "comment " + std::string(400, 'a')) + b4, LSR_EINVAL);
    expect("NUL in a line", path, replaced(h4, "comment fuzz", std::string("comment fu\0z", 12)) + b4, LSR_EINVAL);
    expect("property without a name", path, replaced(h4, "property float nx", "property float") + b4, LSR_EINVAL);
    expect("property before element", path, replaced(h4, "comment fuzz", "property float q") + b4, LSR_EINVAL);
    expect("not a ply", path, replaced(h4, "ply\n", "plx\n") + b4, LSR_EINVAL);
    expect("empty file", path, "", LSR_EINVAL);
    {
        std::string many = replaced(h4, "end_header\n", "");
        for (int i = 0; i < LSR_PLY_MAX_STRIDE; ++i) many += "property float e" + std::to_string(i) + "\n";
        expect("too many properties", path, many + "end_header\n" + b4, LSR_EUNSUPPORTED);
    }
    const int part1 = failures;

    // ---- part 2: seeded corruption ----
    std::mt19937 rng(20240917u);
    const auto below = [&](size_t n) { return (size_t)(rng() % (n ? n : 1)); };
    int accepted = 0, rejected = 0;
    for (int r = 0; r < rounds; ++r) {
        const int Ks[] = {1, 4, 9, 16, 25};
        const int K = Ks[below(5)];
        std::string h = header(K), b = body(K, 3);
        const int edits = 1 + (int)below(3);
        for (int e = 0; e < edits; ++e) {
            std::vector<size_t> starts = {0};
            for (size_t i = 0; i + 1 < h.size(); ++i) if (h[i] == '\n') starts.push_back(i + 1);
            const size_t li = below(starts.size()), ls = starts[li], le = li + 1 < starts.size() ? starts[li + 1] : h.size();
            switch (below(8)) {
                case 0: h.resize(below(h.size() + 1)); break;                                    // truncate the header
                case 1: if (!h.empty()) h[below(h.size())] = (char)below(256); break;            // one byte
                case 2: h.insert(ls, h.substr(ls, le - ls)); break;                              // duplicate a line
                case 3: h.erase(ls, le - ls); break;                                             // drop a line
                case 4: { const size_t lj = below(starts.size()), js = starts[lj], je = lj + 1 < starts.size() ? starts[lj + 1] : h.size();
                          const std::string a = h.substr(ls, le - ls), c = h.substr(js, je - js);
                          if (li < lj) { h.replace(js, je - js, a); h.replace(ls, le - ls, c); }
                          else if (lj < li) { h.replace(ls, le - ls, c); h.replace(js, je - js, a); } } break;   // swap two lines
                case 5: { const char *counts[] = {"0", "1", "4", "-3", "99999999999", "9223372036854775807", "1e3", ""};
                          const size_t at = h.find("vertex ");
                          if (at != std::string::npos) { const size_t nl = h.find('\n', at); if (nl != std::string::npos) h.replace(at + 7, nl - at - 7, counts[below(8)]); } } break;
                case 6: b.resize(below(b.size() + 1)); break;                                    // truncate the rows
                default: h.insert(below(h.size() + 1), std::string(1 + below(300), (char)(32 + below(90)))); break;  // junk run
            }
        }
        write_file(path, h + b);
        int64_t floats = 0;
        (run(path, &floats) == LSR_OK ? accepted : rejected) += 1;
    }
    remove(path);
    printf("ply_reader_fuzz: %d documented-case failures, %d failures in all; %d corrupted files: %d rejected, %d accepted "
           "(still well-formed)\n", part1, failures, rounds, rejected, accepted);
    return failures ? 1 : 0;
}
