/*
 * lsr_colmap.h — C ABI of the host reader of COLMAP sparse models: the cameras, poses and points a photographed capture
 * comes with.  Same library (liblsr_hip.so) and error codes as lsr_rasterizer.h; host only, plain C++ with no HIP in it
 * (csrc/colmap_reader.cpp), so that it also builds and runs under the host sanitizers (`make colmap-check`).
 *
 * A model directory holds cameras / images / points3D, as `.bin` (preferred: taken when `cameras.bin` is there) or as
 * `.txt` (the fallback), all three in the same format.  The binary layouts are little-endian and packed:
 *   cameras.bin   uint64 n, then per camera  uint32 camera_id, int32 model_id, uint64 width, uint64 height, double params[P]
 *   images.bin    uint64 n, then per image   uint32 image_id, double q[4] (w x y z), double t[3], uint32 camera_id, the name
 *                 as a NUL-terminated string, uint64 m, then m x (double x, double y, uint64 point3D_id)
 *   points3D.bin  uint64 n, then per point   uint64 id, double xyz[3], uint8 rgb[3], double error, uint64 L, then
 *                 L x (uint32 image_id, uint32 point2D_idx)
 * The text files hold the same fields, blank separated, one record per line, `#` comments and empty lines between
 * records; an image is two lines, the second (its 2D observations) possibly empty.  lsr_colmap_count and the three
 * lsr_colmap_read_cameras / _images / _points skip the 2D observations and the tracks, each skip checked against the
 * file's size before seeking; the observations are read by lsr_colmap_count_observations / lsr_colmap_read_observations.
 *
 * Camera models (id, name, P, parameter order): 0 SIMPLE_PINHOLE 3 f cx cy; 1 PINHOLE 4 fx fy cx cy; 2 SIMPLE_RADIAL 4
 * f cx cy k; 3 RADIAL 5 f cx cy k1 k2; 4 OPENCV 8 fx fy cx cy k1 k2 p1 p2.  Any other model is LSR_EUNSUPPORTED, and
 * lsr_colmap_last_error names it.
 *
 * The input is untrusted and the reader is strict.  LSR_EINVAL: a missing or truncated file, a count whose smallest
 * possible payload exceeds the file's size (checked before any loop or allocation is sized by it), trailing bytes, an
 * image whose camera is absent, duplicate ids, a name without a terminator (or longer than LSR_COLMAP_MAX_NAME), a width
 * or height outside [1, 65536], a non-finite number, a zero quaternion, a malformed text record, or a capacity smaller
 * than the model.  Nothing outside the files is read.  On an error the caller's arrays hold unspecified values.
 */
#ifndef LSR_COLMAP_H
#define LSR_COLMAP_H

#include "lsr_rasterizer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LSR_COLMAP_MAX_PARAMS 8      /* doubles per camera in `params`; the unused tail is 0 */
#define LSR_COLMAP_MAX_EXTENT 65536  /* largest width / height accepted */
#define LSR_COLMAP_MAX_NAME 1023     /* bytes of an image name, terminator excluded */

enum { LSR_COLMAP_BINARY = 0, LSR_COLMAP_TEXT = 1 };

typedef struct lsr_colmap_counts {
    int64_t cameras, images, points;
    int64_t name_bytes;   /* of all image names, each with its terminator */
    int32_t format;       /* LSR_COLMAP_BINARY or LSR_COLMAP_TEXT */
    int32_t reserved;
} lsr_colmap_counts;

/* Phase one: walk and check all three files of `dir`; `*counts` is written only on LSR_OK. */
int lsr_colmap_count(const char *dir, lsr_colmap_counts *counts);

/* Phase two: fill the caller's HOST arrays, in file order.  Every file is checked again as it is read; a capacity
 * (records, or name bytes) smaller than what the file holds is LSR_EINVAL.
 *   cameras: ids[n], models[n], sizes[n][2] (width, height), params[n][LSR_COLMAP_MAX_PARAMS] in the model's own order
 *   images:  ids[n], qvec[n][4] (w x y z, as stored: world-to-camera, not normalised), tvec[n][3], camera_ids[n],
 *            names: the strings back to back with their terminators, name_offsets[n + 1] (where each starts; the last
 *            entry is the total)
 *   points:  ids[n], xyz[n][3], rgb[n][3], errors[n] */
int lsr_colmap_read_cameras(const char *dir, uint32_t *ids, int32_t *models, int64_t *sizes, double *params, int64_t capacity);
int lsr_colmap_read_images(const char *dir, uint32_t *ids, double *qvec, double *tvec, uint32_t *camera_ids, char *names,
                           int64_t *name_offsets, int64_t capacity, int64_t name_capacity);
int lsr_colmap_read_points(const char *dir, uint64_t *ids, double *xyz, uint8_t *rgb, double *errors, int64_t capacity);

/* The 2D observations of the images: which sparse point each image sees, and where.  Only observations that carry a point
 * are counted and returned (binary: point3D_id != 2^64 - 1; text: != -1); the others are parsed and checked all the same.
 * Both calls walk and check all three files as lsr_colmap_count does, so every refusal of that walk applies, and further
 * refuse (LSR_EINVAL) a non-finite x or y, an observation line in images.txt that is not whole X Y POINT3D_ID triples, a
 * binary observation count that the rest of the file cannot hold (checked before the loop is sized by it), and, in the
 * read, more images than `image_capacity` or more observations with a point than `capacity`.
 *   count: *total, written only on LSR_OK.
 *   read:  offsets[image_capacity + 1] (image k, in file order, owns [offsets[k], offsets[k + 1]); entries beyond the
 *          file's images repeat the total), xy[capacity][2] (COLMAP's measured position in source pixels, as stored),
 *          point_ids[capacity]; each image's observations in their own order.  A point id that points3D does not hold is
 *          NOT refused here (the files are walked one at a time): the caller that joins them checks it. */
int lsr_colmap_count_observations(const char *dir, int64_t *total);
int lsr_colmap_read_observations(const char *dir, int64_t *offsets, double *xy, uint64_t *point_ids, int64_t image_capacity,
                                 int64_t capacity);

/* What the calling thread's last lsr_colmap_* call refused, in words: the file, the record and the reason ("" after a call
 * that succeeded).  The pointer stays valid until the thread's next call into the reader. */
const char *lsr_colmap_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* LSR_COLMAP_H */
