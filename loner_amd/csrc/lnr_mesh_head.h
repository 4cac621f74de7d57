// The call head of the mesh entries that sort (lnr_mesh_tools.hip, lnr_mesh_filters.hip): the words of one call on the device, the
// kernel that writes them before anything else runs and the kernel that reports them.  Everything is internal to its translation unit
// (the anonymous namespace), like the kernels that use it.
#pragma once
#include "lnr_mesh_args.h"
#include "lnr_radix_sort.h"

namespace {

struct MeshSortHead {
    uint32_t n;                     // pairs the sort works on
    int32_t npasses;                // digit passes of the (first) sort
    int32_t npasses2;               // digit passes of a second sort over the same pairs
    uint32_t status;                // the entry's status bits
    uint32_t n_a, n_b;              // the entry's two counts (a scan's total, a tally)
};

__global__ void mesh_head_init(MeshSortHead* h, uint32_t n, int32_t npasses, int32_t npasses2) {
    h->n = n;
    h->npasses = npasses;
    h->npasses2 = npasses2;
    h->status = 0;
    h->n_a = 0;
    h->n_b = 0;
}

// info[3] is the entry's: the mesh tools report their pass count there, the filters 0
__global__ void mesh_head_info(const MeshSortHead* __restrict__ h, int64_t* __restrict__ info, int64_t info3) {
    info[0] = h->status;
    info[1] = h->n_a;
    info[2] = h->n_b;
    info[3] = info3;
}

}  // namespace
