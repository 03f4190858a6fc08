// colmap_check.cpp — the COLMAP reader over a directory of models, as a stand-alone program for the host sanitizers
// (`make colmap-check MODELS=dir`): every sub-directory of each argument (and the argument itself) that holds a
// cameras.bin or cameras.txt is counted and, where the count succeeds, read into arrays of exactly the counted sizes, so
// that a write past what phase one promised is a heap overflow the sanitizer sees; the 2D observations likewise, through
// lsr_colmap_count_observations / lsr_colmap_read_observations.  A model the first walk refuses is handed to the
// observation walk all the same (it must refuse it too).  Refusals are expected and printed;
// the exit status is 1 only when phase two contradicts phase one.
#include <dirent.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "lsr_colmap.h"

static bool is_model(const std::string &dir) {
    for (const char *name : {"/cameras.bin", "/cameras.txt"}) {
        FILE *f = fopen((dir + name).c_str(), "rb");
        if (f) { fclose(f); return true; }
    }
    return false;
}

// 0: refused or read in full; 1: counted, then not read
static int check(const std::string &dir, int *accepted) {
    lsr_colmap_counts c;
    int rc = lsr_colmap_count(dir.c_str(), &c);
    if (rc != LSR_OK) {
        printf("%s: refused (%d): %s\n", dir.c_str(), rc, lsr_colmap_last_error());
        int64_t total = -1;
        if (lsr_colmap_count_observations(dir.c_str(), &total) == LSR_OK) {
            printf("%s: refused, but its observations were counted (%lld)\n", dir.c_str(), (long long)total);
            return 1;
        }
        return 0;
    }
    std::vector<uint32_t> cam_ids((size_t)c.cameras), img_ids((size_t)c.images), img_cams((size_t)c.images);
    std::vector<int32_t> models((size_t)c.cameras);
    std::vector<int64_t> sizes((size_t)c.cameras * 2), offsets((size_t)c.images + 1);
    std::vector<double> params((size_t)c.cameras * LSR_COLMAP_MAX_PARAMS), q((size_t)c.images * 4), t((size_t)c.images * 3);
    std::vector<double> xyz((size_t)c.points * 3), errors((size_t)c.points);
    std::vector<char> names((size_t)c.name_bytes);
    std::vector<uint64_t> pt_ids((size_t)c.points);
    std::vector<uint8_t> rgb((size_t)c.points * 3);
    rc = lsr_colmap_read_cameras(dir.c_str(), cam_ids.data(), models.data(), sizes.data(), params.data(), c.cameras);
    if (rc == LSR_OK)
        rc = lsr_colmap_read_images(dir.c_str(), img_ids.data(), q.data(), t.data(), img_cams.data(), names.data(), offsets.data(),
                                    c.images, c.name_bytes);
    if (rc == LSR_OK) rc = lsr_colmap_read_points(dir.c_str(), pt_ids.data(), xyz.data(), rgb.data(), errors.data(), c.points);
    if (rc != LSR_OK) {
        printf("%s: counted, then refused (%d): %s\n", dir.c_str(), rc, lsr_colmap_last_error());
        return 1;
    }
    // the observations: counted, read into arrays of exactly the counted sizes, and the offsets must end at the count
    int64_t total = -1;
    rc = lsr_colmap_count_observations(dir.c_str(), &total);
    if (rc != LSR_OK) {
        printf("%s: observations refused (%d): %s\n", dir.c_str(), rc, lsr_colmap_last_error());
        return 0;
    }
    std::vector<int64_t> obs_offsets((size_t)c.images + 1);
    std::vector<double> obs_xy((size_t)total * 2);
    std::vector<uint64_t> obs_ids((size_t)total);
    rc = lsr_colmap_read_observations(dir.c_str(), obs_offsets.data(), obs_xy.data(), obs_ids.data(), c.images, total);
    if (rc != LSR_OK || obs_offsets[0] != 0 || obs_offsets[(size_t)c.images] != total) {
        printf("%s: %lld observations counted, then refused or miscounted (%d): %s\n", dir.c_str(), (long long)total, rc,
               lsr_colmap_last_error());
        return 1;
    }
    if (total > 0 && lsr_colmap_read_observations(dir.c_str(), obs_offsets.data(), obs_xy.data(), obs_ids.data(), c.images,
                                                  total - 1) == LSR_OK) {
        printf("%s: a capacity of %lld observations was accepted for %lld\n", dir.c_str(), (long long)(total - 1), (long long)total);
        return 1;
    }
    ++*accepted;
    printf("%s: %lld cameras, %lld images, %lld points, %lld observations (%s)\n", dir.c_str(), (long long)c.cameras,
           (long long)c.images, (long long)c.points, (long long)total, c.format == LSR_COLMAP_BINARY ? "binary" : "text");
    return 0;
}

int main(int argc, char **argv) {
    int models = 0, accepted = 0, bad = 0;
    for (int i = 1; i < argc; ++i) {
        std::vector<std::string> dirs = {argv[i]};
        if (DIR *d = opendir(argv[i])) {
            while (const dirent *e = readdir(d))
                if (strcmp(e->d_name, ".") != 0 && strcmp(e->d_name, "..") != 0) dirs.push_back(std::string(argv[i]) + "/" + e->d_name);
            closedir(d);
        }
        for (const std::string &dir : dirs)
            if (is_model(dir)) { ++models; bad += check(dir, &accepted); }
    }
    printf("colmap-check: %d models, %d read in full, %d refused, %d inconsistent\n", models, accepted, models - accepted - bad, bad);
    return bad || models == 0 ? 1 : 0;
}
