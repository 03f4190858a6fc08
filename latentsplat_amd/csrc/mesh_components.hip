// mesh_components.hip — connected components of a triangle mesh over shared vertex indices (include/lsr_mesh.h, part C):
// what the cleanup after mesh extraction (keep the largest clusters, drop the floaters) labels its faces with.
//
// labels[v] ends as the lowest vertex index of v's component.  Rounds of two kernels over a label array that starts as
// labels[v] = v:
//   k_cc_hook      one thread per face: follow each corner's label chain to its root (labels[r] == r) and atomicMin the
//                  larger roots' labels with the smallest root; a device flag records that some face saw two roots;
//   k_cc_compress  one thread per vertex: labels[v] = root(v).
// The caller repeats the round until the flag stays 0 (it reads the flag between rounds and caps the rounds).
//
// Termination and result.  labels[x] <= x holds from the start and every write (an integer atomicMin with a smaller root,
// or a compression to the root) only lowers a label, so a chain x, labels[x], labels[labels[x]], ... is strictly
// decreasing until it reaches a root: every walk ends in at most x steps, whatever other threads write meanwhile (a stale
// read is an older, larger label of the same chain's component, still below x).  The walks carry that bound as an
// explicit step count all the same.  A label always names a vertex of the same component, so the component's minimum
// keeps itself as its label; a round whose flag stays 0 saw one root per face, hence one root per component, and that
// root is the minimum.  Integer atomicMin makes this fixed point independent of the order in which threads run: two
// calls give the same labels.  Root hooking with full compression merges every tree that has a smaller neighbour each
// round: O(log nv) rounds on meshes whose numbering is not adversarial.
#include <stdint.h>

#include <algorithm>

#include "lsr_internal.h"
#include "lsr_mesh.h"

namespace lsr {

constexpr int kCcThreads = 256;

// the root of x's chain; `steps` bounds the walk (nv: a chain is strictly decreasing)
__device__ __forceinline__ int32_t cc_root(const int32_t *labels, int32_t x, int32_t steps) {
    for (int32_t s = 0; s < steps; ++s) {
        const int32_t up = __atomic_load_n(labels + x, __ATOMIC_RELAXED);
        if (up >= x || up < 0) break;                      // a root (up == x); anything else cannot happen and ends the walk
        x = up;
    }
    return x;
}

__global__ __launch_bounds__(kCcThreads) void k_cc_init(int32_t nv, int32_t *__restrict__ labels) {
    const int64_t v = (int64_t)blockIdx.x * kCcThreads + threadIdx.x;
    if (v < nv) labels[v] = (int32_t)v;
}

__global__ __launch_bounds__(kCcThreads) void k_cc_hook(int32_t nv, int64_t nf, const int32_t *__restrict__ faces, int32_t *labels,
                                                       int32_t *changed) {
    const int64_t f = (int64_t)blockIdx.x * kCcThreads + threadIdx.x;
    if (f >= nf) return;
    const int32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (a < 0 || a >= nv || b < 0 || b >= nv || c < 0 || c >= nv) return;      // (the wrapper refuses such a mesh)
    const int32_t ra = cc_root(labels, a, nv), rb = cc_root(labels, b, nv), rc = cc_root(labels, c, nv);
    const int32_t r = min(ra, min(rb, rc));
    if (ra == r && rb == r && rc == r) return;
    if (ra != r) atomicMin(labels + ra, r);
    if (rb != r) atomicMin(labels + rb, r);
    if (rc != r) atomicMin(labels + rc, r);
    *changed = 1;                                          // (every writer stores the same value)
}

__global__ __launch_bounds__(kCcThreads) void k_cc_compress(int32_t nv, int32_t *labels) {
    const int64_t v = (int64_t)blockIdx.x * kCcThreads + threadIdx.x;
    if (v >= nv) return;
    const int32_t r = cc_root(labels, (int32_t)v, nv);
    if (r != labels[v]) __atomic_store_n(labels + v, r, __ATOMIC_RELAXED);
}

}  // namespace lsr

using namespace lsr;

extern "C" {

int lsr_mesh_components_init(int64_t num_vertices, int32_t *labels, lsr_stream_t stream) {
    note_hip_error(0);
    if (num_vertices < 0 || num_vertices > LSR_MESH_MAX_ELEMENTS) return LSR_EINVAL;
    if (num_vertices == 0) return LSR_OK;
    if (!labels) return LSR_ENULL;
    hipLaunchKernelGGL(k_cc_init, dim3((unsigned)((num_vertices + kCcThreads - 1) / kCcThreads)), dim3(kCcThreads), 0,
                       (hipStream_t)stream, (int32_t)num_vertices, labels);
    return launch_status();
}

int lsr_mesh_components_round(int64_t num_vertices, int64_t num_faces, const int32_t *faces, int32_t *labels, int32_t *changed,
                              lsr_stream_t stream) {
    note_hip_error(0);
    if (num_vertices < 0 || num_vertices > LSR_MESH_MAX_ELEMENTS || num_faces < 0 || num_faces > LSR_MESH_MAX_ELEMENTS) return LSR_EINVAL;
    if (!changed) return LSR_ENULL;
    if (num_vertices > 0 && num_faces > 0 && (!faces || !labels)) return LSR_ENULL;
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(changed, 0, sizeof(int32_t), s);
    if (e != hipSuccess) { note_hip_error((int)e); return LSR_ELAUNCH; }
    if (num_vertices == 0 || num_faces == 0) return LSR_OK;
    hipLaunchKernelGGL(k_cc_hook, dim3((unsigned)((num_faces + kCcThreads - 1) / kCcThreads)), dim3(kCcThreads), 0, s,
                       (int32_t)num_vertices, num_faces, faces, labels, changed);
    hipLaunchKernelGGL(k_cc_compress, dim3((unsigned)((num_vertices + kCcThreads - 1) / kCcThreads)), dim3(kCcThreads), 0, s,
                       (int32_t)num_vertices, labels);
    return launch_status();
}

}  // extern "C"
