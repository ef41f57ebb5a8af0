// mesh_device.h -- what the operators over an indexed triangle mesh share and the point-cloud filters do not (kernels_mesh.hip,
// kernels_simplify.hip, kernels_smooth.hip, kernels_raster.hip).  Device half: the check of the triangles' indices.  Host half: the test
// every call makes of its mesh arguments and the prologue of a create.  What they share with the filters is voxel_device.h's (point
// sources, sort_rounds, gather_in_order, unit_of, the flag compaction), wave_device.h's (wave_add_to) and hip_host.h's (aligned4, stage_times).
// Everything has internal linkage: each including file compiles its own copy of the kernels it launches.
#pragma once
#include "voxel_device.h"

#include <new>

namespace rgbid {
namespace {

// counts the triangles with an index >= n_v into *bad; with PAIRS also the ordered corner pairs with equal ends (two per equal pair of
// corners) into *dropped.  One atomic per wave and count
template <bool PAIRS>
__global__ __launch_bounds__(VT) void k_mesh_check(const unsigned* __restrict__ tri, unsigned n_t, unsigned n_v, unsigned* __restrict__ bad,
                                                   unsigned* __restrict__ dropped) {
  unsigned n_bad = 0, n_dropped = 0;
  for (size_t t = (size_t)blockIdx.x * VT + threadIdx.x; t < n_t; t += (size_t)gridDim.x * VT) {
    const unsigned a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
    if (!(a < n_v && b < n_v && c < n_v)) ++n_bad;
    if (PAIRS) n_dropped += 2u * ((a == b) + (b == c) + (c == a));
  }
  wave_add_to(bad, n_bad);
  if (PAIRS) wave_add_to(dropped, n_dropped);
}

// n_t > 0 triangles checked on stream s
template <bool PAIRS = false>
void check_triangles(hipStream_t s, const unsigned* tri, unsigned n_t, unsigned n_v, unsigned* bad, unsigned* dropped = nullptr) {
  hipLaunchKernelGGL(k_mesh_check<PAIRS>, dim3(grid_of(((unsigned long long)n_t + VT - 1) / VT)), dim3(VT), 0, s, tri, n_t, n_v, bad, dropped);
}

// what every call checks about the mesh it is given: the counts against the handle's capacities, triangles that are there and 4-byte
// aligned, and none of them without a vertex
bool mesh_in_ok(unsigned long long n_v, unsigned long long n_t, const void* tri, unsigned long long cap_v, unsigned long long cap_t) {
  return n_v <= cap_v && n_t <= cap_t && (n_t == 0 || (tri && aligned4(tri) && n_v != 0));
}

// The create of a mesh operator's handle H (ctx, cap_v, cap_t, its Buffers and StageTimer): the capacities lie in 1 .. the header's limits,
// alloc(h) makes the operator's own allocations; a failed one destroys the handle
template <class H, class A>
int mesh_create(H** out, rgbid_ctx* ctx, unsigned long long max_v, unsigned long long max_t, unsigned long long limit_v, unsigned long long limit_t,
                A&& alloc) {
  if (!out) return RGBID_E_INVALID;
  *out = nullptr;
  if (!ctx || max_v < 1 || max_v > limit_v || max_t < 1 || max_t > limit_t) return RGBID_E_INVALID;
  (void)hipSetDevice(ctx->device);
  H* h = new (std::nothrow) H;
  if (!h) return RGBID_E_NOMEM;
  h->ctx = ctx;
  h->cap_v = max_v;
  h->cap_t = max_t;
  if (int r = alloc(h)) { destroy_handle(h); return r; }
  *out = h;
  return RGBID_OK;
}

}  // namespace
}  // namespace rgbid
