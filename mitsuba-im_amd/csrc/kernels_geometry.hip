// kernels_geometry.hip -- mi_scene_update_vertices, mi_scene_update_instances and mi_scene_update_geometry on the device: the per-triangle records, the instance
// records and the refit of the existing trees (DESIGN.md §3 "In-place edits").
//
// All kernels are thin: the arithmetic is geometry_records.h, shared with commitHost() and SceneHost::refreshHostGeometry(), so that an edited scene holds, bit for
// bit, the records a fresh commit of the new vertices would hold.  Compiled like every other unit: -ffp-contract=off, correctly rounded divide and square root.
//
//   k_tri_records   one thread per triangle: gathers its three vertices (12-B position records, indices from the triangle's own 128-B TriShade line), writes the
//                   48-B Wald record twice (leaf slot, packet-exact table), the geometric words of the TriShade line, the UV tangents and the 24-B padded leaf box.
//                   Memory bound: ~36 B gathered + 128 B read-modify-write + ~170 B written per triangle; no LDS, no cross-lane traffic.
//   k_instance_records   one thread per instance: reads its new to_world / to_object (96 B from the staging array), rewrites those 96 of the 128 B of its InstanceD
//                   and the 24-B padded box of its leaf record (the 8 transformed corners of the group box, which the record itself carries).  A geometry edit hands it
//                   the groups' new boxes (24 B per group, a handful of cache lines shared by all lanes): the record's glo / ghi are then rewritten from the box of its
//                   own `group` first.  No LDS, no cross-lane traffic, no atomics; k_refit follows on the same stream.
//   k_refit         one thread per node of ONE level (all of its inner children belong to lower levels, refitted by earlier launches on the same stream; a geometry
//                   edit puts the nodes of equal height of the scene-level tree and of every group tree into one level -- no tree reads another's nodes): unions
//                   the child boxes and rewrites the node's child boxes -- for a 4-wide node org, the three steps and the quantised bytes by the builder's rule.
//                   No atomics and no synchronisation between workgroups: the launch order is the only dependency, the result is deterministic.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "geometry_records.h"

#define GEO_WG 256

__global__ void __launch_bounds__(GEO_WG) k_tri_records(mi::GeoEditTables g) {
    const uint32_t t = blockIdx.x * GEO_WG + threadIdx.x;
    if (t >= g.nTris) return;
    mi::geoTriRecord(g, t);
}

__global__ void __launch_bounds__(GEO_WG) k_instance_records(mi::InstEditTables g) {
    const uint32_t i = blockIdx.x * GEO_WG + threadIdx.x;
    if (i >= g.n) return;
    mi::geoInstanceRecord(g, i);
}

// order[first .. first + count) = the node indices of this level
__global__ void __launch_bounds__(GEO_WG) k_refit(mi::GeoEditTables g, const uint32_t *order, uint32_t first, uint32_t count, uint32_t nNodes) {
    const uint32_t i = blockIdx.x * GEO_WG + threadIdx.x;
    if (i >= count) return;
    const uint32_t n = order[first + i];
    if (n >= nNodes) return;
    mi::geoRefitNode(g, n);
}

extern "C" {
void mi_launch_tri_records(const mi::GeoEditTables &g, hipStream_t st) {
    if (g.nTris) hipLaunchKernelGGL(k_tri_records, dim3((g.nTris + GEO_WG - 1) / GEO_WG), dim3(GEO_WG), 0, st, g);
}
void mi_launch_instance_records(const mi::InstEditTables &g, hipStream_t st) {
    if (g.n) hipLaunchKernelGGL(k_instance_records, dim3((g.n + GEO_WG - 1) / GEO_WG), dim3(GEO_WG), 0, st, g);
}
void mi_launch_refit_level(const mi::GeoEditTables &g, const uint32_t *order, uint32_t first, uint32_t count, uint32_t nNodes, hipStream_t st) {
    if (count) hipLaunchKernelGGL(k_refit, dim3((count + GEO_WG - 1) / GEO_WG), dim3(GEO_WG), 0, st, g, order, first, count, nNodes);
}
}
