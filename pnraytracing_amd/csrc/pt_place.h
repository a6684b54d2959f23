// pnraytracing_amd/csrc/pt_place.h -- models moved on the device by a matrix
// (pnrt_define_model, pnrt_place_models): the step the reference does once at load
// (main.cpp:207-237, ModelOutput model.hpp:101-135) -- a model's model-space vertices
// through M, its normals through N = transpose(inverse(M)) -- in front of pt_refit.h's
// regather and refit.
//
// The arithmetic is the host library's pnrt_scene_add_mesh, glm's operator*(mat4, vec4)
// with w = 1, every product and sum rounded on its own (-ffp-contract=off), for row r:
//   pos[r]    = (M[0][r] * p.x + M[1][r] * p.y) + (M[2][r] * p.z + M[3][r] * 1.0f)
//   normal[r] = (N[0][r] * n.x + N[1][r] * n.y) + (N[2][r] * n.z + N[3][r] * 1.0f)
// The normal is not normalised (ModelOutput does not); the texcoords are copied.
//
// One launch per call, one lane per vertex of the concatenated ranges of the call's
// placements: a lane finds its placement by a binary search over the exclusive prefix
// of the counts -- a wave inside one placement reads one table entry in every lane --,
// loads its model-space record (two float4) and stores the world-space record (two
// float4) into verts.  No LDS, nothing handed between lanes: the regather that reads
// verts is the next launch (the per-XCD L2s are not coherent inside one, pt_refit.h).
#pragma once
#include "pt_common.h"

#define PLACE_MAX 1024            // placements per call (pnrt.h)

// A model-space record is laid out as a vertex record of `verts`:
// (p.x, p.y, p.z, n.x), (n.y, n.z, u, v)
struct PlaceEntry {
    int prefix;                   // vertices of the placements before this one
    int first;                    // the model's first vertex in verts
    const float4* model;          // its model-space records, two float4 per vertex
    float4 M[3], N[3];            // row r of each: ([0][r], [1][r], [2][r], [3][r])
};

PN_DEV float place_row(const float4 m, float x, float y, float z) { return (m.x * x + m.y * y) + (m.z * z + m.w * 1.0f); }

__global__ void __launch_bounds__(256) pt_place_kernel(const PlaceEntry* __restrict__ table, int n, int total,
                                                       float4* __restrict__ verts, int n_verts) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    int lo = 0, hi = n;           // the last entry whose prefix is <= i
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (table[mid].prefix <= i) lo = mid;
        else hi = mid;
    }
    const PlaceEntry* e = table + lo;
    const int k = i - e->prefix, v = e->first + k;
    if (k < 0 || (unsigned)v >= (unsigned)n_verts) return;     // (the call validated every range)
    const float4 a = e->model[2 * (size_t)k], b = e->model[2 * (size_t)k + 1];
    const float4 M0 = e->M[0], M1 = e->M[1], M2 = e->M[2], N0 = e->N[0], N1 = e->N[1], N2 = e->N[2];
    verts[2 * (size_t)v] = make_float4(place_row(M0, a.x, a.y, a.z), place_row(M1, a.x, a.y, a.z), place_row(M2, a.x, a.y, a.z),
                                       place_row(N0, a.w, b.x, b.y));
    verts[2 * (size_t)v + 1] = make_float4(place_row(N1, a.w, b.x, b.y), place_row(N2, a.w, b.x, b.y), b.z, b.w);
}
