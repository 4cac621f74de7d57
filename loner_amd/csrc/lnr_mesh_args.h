// What the entry points that take an indexed triangle mesh share (lnr_mesh_tools.hip, lnr_mesh_filters.hip, lnr_raycast.hip): the
// corner load with its range test and the count checks of the host prologue.  It holds no
// kernel, so a source that includes it gains no device code.  Everything is internal to its translation unit (the anonymous namespace).
#pragma once
#include "lnr_cloud_grid.h"

namespace {

// the three corners of triangle t; false when one lies outside [0, V)
__device__ inline bool load_corners(const int32_t* __restrict__ tri, uint32_t t, int64_t n_verts, int64_t* i) {
    i[0] = tri[3 * (size_t)t];
    i[1] = tri[3 * (size_t)t + 1];
    i[2] = tri[3 * (size_t)t + 2];
    return i[0] >= 0 && i[0] < n_verts && i[1] >= 0 && i[1] < n_verts && i[2] >= 0 && i[2] < n_verts;
}

// max_tris: CL_MAX_POINTS over the pairs a triangle gives the entry's sort
bool mesh_counts_ok(int64_t n_verts, int64_t n_tris, int64_t max_tris) {
    return n_verts >= 0 && n_verts <= INT32_MAX && n_tris >= 0 && n_tris <= max_tris;
}

#define MESH_REQUIRE_COUNTS(fn, v, f, max_tris)                                                                                   \
    LNR_REQUIRE(mesh_counts_ok(v, f, max_tris), fn ": %lld vertices, %lld triangles, the limits are %d and %lld", (long long)(v), \
                (long long)(f), INT32_MAX, (long long)(max_tris))

}  // namespace
