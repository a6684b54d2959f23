// pnraytracing_amd/csrc/pt_refit.h -- in-place geometry edits (pnrt_update_vertices):
// moved vertex records scattered into the vertex array, every per-triangle record
// regathered from them, and the BVH boxes refit bottom-up over the unchanged
// topology.  Not in the reference, which places every model once with a matrix
// (main.cpp:207-237) and has no edit of geometry.
//
// The refit rule is Bound::Union (bound.hpp:4-28) with the host library's min and
// max, (y < x) ? y : x and (x < y) ? y : x: on a tie the EARLIER operand stays, so
// -0 / +0 come out as BuildBVH has them, and a NaN coordinate never enters a box.
//   leaf      fold of its triangles in ascending order, vertices p0, p1, p2,
//             starting from (FLT_MAX, lowest); an empty leaf keeps its box
//   interior  fold(left child's box, right child's box)
// Folded this way the builder's own node array comes back bit for bit.
//
// A node record holds its two CHILDREN's boxes (pt_common.h), so a child's box is
// the fold of the two boxes in the child's record.  Levels hand their boxes on
// across kernel boundaries only: the per-XCD L2s are not coherent inside a launch.
// The breadth-first numbering puts each level in one contiguous index range.
//   1 pt_refit_scatter_kernel   staged 15-float records -> verts
//   2 pt_refit_gather_kernel    tris (positions), tri_attr, one lane per triangle
//   3 pt_refit_lights_kernel    light_rec's vertex records, n_lights + 1 entries
//   4 pt_refit_leaves_kernel    every (node, side) whose ref is a leaf
//   5 pt_refit_level_kernel     one launch per level with interior children,
//                               deepest first; level 0's lane also folds the root box
#pragma once
#include <float.h>
#include "pt_common.h"

struct RefitResult {
    float root[6];          // the root's box (min.xyz, max.xyz)
    uint32_t nonfinite;     // some box coordinate is not finite (z-slab culling is then off)
    uint32_t pad;
};

struct RBox { float lo[3], hi[3]; };

PN_DEV float rf_min(float x, float y) { return (y < x) ? y : x; }
PN_DEV float rf_max(float x, float y) { return (x < y) ? y : x; }
PN_DEV void rf_point(RBox& b, float x, float y, float z) {
    b.lo[0] = rf_min(b.lo[0], x); b.lo[1] = rf_min(b.lo[1], y); b.lo[2] = rf_min(b.lo[2], z);
    b.hi[0] = rf_max(b.hi[0], x); b.hi[1] = rf_max(b.hi[1], y); b.hi[2] = rf_max(b.hi[2], z);
}
PN_DEV RBox rf_union(const RBox& a, const RBox& b) {
    RBox r;
    for (int k = 0; k < 3; ++k) { r.lo[k] = rf_min(a.lo[k], b.lo[k]); r.hi[k] = rf_max(a.hi[k], b.hi[k]); }
    return r;
}
PN_DEV bool rf_finite(const RBox& b) {
    bool f = true;
    for (int k = 0; k < 3; ++k) f = f && fabsf(b.lo[k]) <= FLT_MAX && fabsf(b.hi[k]) <= FLT_MAX;
    return f;
}
// side 0 / 1 of a node record is floats 0-5 / 6-11 of its 16
PN_DEV RBox rf_load(const float* rec) {
    RBox b;
    for (int k = 0; k < 3; ++k) { b.lo[k] = rec[k]; b.hi[k] = rec[3 + k]; }
    return b;
}
PN_DEV void rf_store(float* rec, const RBox& b) {
    for (int k = 0; k < 3; ++k) { rec[k] = b.lo[k]; rec[3 + k] = b.hi[k]; }
}
// the triangle range of a leaf ref (pt_common.h); an empty leaf has count 0
PN_DEV void rf_leaf_range(uint32_t ref, int has_leaf_table, const int2* leaf_table, int n_leaf_table, int& first, int& count) {
    first = 0; count = 0;
    if (ref == REF_LEAF) return;
    if (!has_leaf_table) { count = (int)((ref >> 24) & 127u); first = (int)(ref & 0xFFFFFFu); return; }
    if (ref & REF_TABLE) {
        const uint32_t k = ref & ~(REF_LEAF | REF_TABLE);
        if (k < (uint32_t)n_leaf_table) { first = leaf_table[k].x; count = leaf_table[k].y; }
        return;
    }
    first = (int)((ref >> 7) & 0x7FFFFFu); count = (int)(ref & 127u);
}
PN_DEV RBox rf_fold_tris(const float4* tris, int n_tris, int first, int count) {
    RBox b;
    for (int k = 0; k < 3; ++k) { b.lo[k] = FLT_MAX; b.hi[k] = -FLT_MAX; }
    for (int t = first; t < first + count; ++t) {
        if (t < 0 || t >= n_tris) continue;       // (the upload validated every range)
        const float4 a = tris[3 * (size_t)t], c = tris[3 * (size_t)t + 1];
        const float z2 = tris[3 * (size_t)t + 2].x;
        rf_point(b, a.x, a.y, a.z);
        rf_point(b, a.w, c.x, c.y);
        rf_point(b, c.z, c.w, z2);
    }
    return b;
}

// src: count records of 15 floats (main.cpp:412-428), 4-byte aligned
__global__ void __launch_bounds__(256) pt_refit_scatter_kernel(const float* src, float4* verts, int first, int count, int n_verts) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count || first + i < 0 || first + i >= n_verts) return;
    const float* v = src + 15 * (size_t)i;
    verts[2 * (size_t)(first + i)] = make_float4(v[0], v[1], v[2], v[3]);
    verts[2 * (size_t)(first + i) + 1] = make_float4(v[4], v[5], v[12], v[13]);
}

__global__ void __launch_bounds__(256) pt_refit_gather_kernel(const int4* tri_idx, const float4* verts, float4* tris, float4* tri_attr,
                                                              int n_tris, int n_verts) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tris) return;
    const int4 id = tri_idx[t];
    if ((unsigned)id.x >= (unsigned)n_verts || (unsigned)id.y >= (unsigned)n_verts || (unsigned)id.z >= (unsigned)n_verts) return;
    const float4 a0 = verts[2 * (size_t)id.x], b0 = verts[2 * (size_t)id.x + 1];
    const float4 a1 = verts[2 * (size_t)id.y], b1 = verts[2 * (size_t)id.y + 1];
    const float4 a2 = verts[2 * (size_t)id.z], b2 = verts[2 * (size_t)id.z + 1];
    tris[3 * (size_t)t] = make_float4(a0.x, a0.y, a0.z, a1.x);
    tris[3 * (size_t)t + 1] = make_float4(a1.y, a1.z, a2.x, a2.y);
    tris[3 * (size_t)t + 2].x = a2.z;             // the material and texture words stay
    tri_attr[4 * (size_t)t + 0] = make_float4(a0.w, b0.x, b0.y, a1.w);
    tri_attr[4 * (size_t)t + 1] = make_float4(b1.x, b1.y, a2.w, b2.x);
    tri_attr[4 * (size_t)t + 2] = make_float4(b2.y, b0.z, b0.w, b1.z);
    tri_attr[4 * (size_t)t + 3] = make_float4(b1.w, b2.z, b2.w, 0.f);
}

// entry e < n_lights is the light list's triangle, entry n_lights triangle 0; the emission word stays
__global__ void __launch_bounds__(256) pt_refit_lights_kernel(const float2* lights, const int4* tri_idx, const float4* verts,
                                                              float4* light_rec, int n_lights, int n_tris, int n_verts) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e > n_lights) return;
    const int t = e < n_lights ? (int)lights[e].x : 0;
    if ((unsigned)t >= (unsigned)n_tris) return;
    const int4 id = tri_idx[t];
    const int vi[3] = {id.x, id.y, id.z};
    for (int k = 0; k < 3; ++k) {
        if ((unsigned)vi[k] >= (unsigned)n_verts) continue;
        light_rec[7 * (size_t)e + 2 * k] = verts[2 * (size_t)vi[k]];
        light_rec[7 * (size_t)e + 2 * k + 1] = verts[2 * (size_t)vi[k] + 1];
    }
}

// One lane per (node, side).  A tree whose root is a leaf (n_nodes == 0) has only
// the root box: lane 0 folds it from root_ref's triangles.
__global__ void __launch_bounds__(256) pt_refit_leaves_kernel(float4* nodes, int n_nodes, const float4* tris, int n_tris,
                                                              const int2* leaf_table, int n_leaf_table, int has_leaf_table,
                                                              uint32_t root_ref, RefitResult* res) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    int first, count;
    if (n_nodes == 0) {
        if (i != 0) return;
        rf_leaf_range(root_ref, has_leaf_table, leaf_table, n_leaf_table, first, count);
        if (count <= 0) return;
        const RBox b = rf_fold_tris(tris, n_tris, first, count);
        for (int k = 0; k < 3; ++k) { res->root[k] = b.lo[k]; res->root[3 + k] = b.hi[k]; }
        if (!rf_finite(b)) atomicOr(&res->nonfinite, 1u);
        return;
    }
    if (i >= 2 * n_nodes) return;
    const int node = i >> 1, side = i & 1;
    float* rec = reinterpret_cast<float*>(nodes + 4 * (size_t)node);
    const uint32_t ref = __float_as_uint(side ? rec[13] : rec[12]);
    if (!(ref & REF_LEAF)) return;
    rf_leaf_range(ref, has_leaf_table, leaf_table, n_leaf_table, first, count);
    RBox b;
    if (count <= 0) b = rf_load(rec + 6 * side);          // an empty leaf keeps its box
    else {
        b = rf_fold_tris(tris, n_tris, first, count);
        rf_store(rec + 6 * side, b);
    }
    if (!rf_finite(b)) atomicOr(&res->nonfinite, 1u);
}

// Nodes lo .. hi - 1 are one level: the box of every interior child is the fold of
// the two boxes in the child's record, which earlier launches completed.  With
// `root` (level 0: node 0 alone) one lane does both sides, then the root box.
__global__ void __launch_bounds__(256) pt_refit_level_kernel(float4* nodes, int n_nodes, int lo, int hi, int root, RefitResult* res) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (root) {
        if (i != 0 || n_nodes <= 0) return;
        float* rec = reinterpret_cast<float*>(nodes);
        RBox s[2];
        for (int side = 0; side < 2; ++side) {
            const uint32_t ref = __float_as_uint(rec[12 + side]);
            if (!(ref & REF_LEAF) && ref < (uint32_t)n_nodes) {
                const float* ch = reinterpret_cast<const float*>(nodes + 4 * (size_t)ref);
                s[side] = rf_union(rf_load(ch), rf_load(ch + 6));
                rf_store(rec + 6 * side, s[side]);
            } else s[side] = rf_load(rec + 6 * side);
        }
        const RBox b = rf_union(s[0], s[1]);
        for (int k = 0; k < 3; ++k) { res->root[k] = b.lo[k]; res->root[3 + k] = b.hi[k]; }
        if (!rf_finite(s[0]) || !rf_finite(s[1]) || !rf_finite(b)) atomicOr(&res->nonfinite, 1u);
        return;
    }
    if (lo < 0 || hi > n_nodes || i >= 2 * (hi - lo)) return;
    const int node = lo + (i >> 1), side = i & 1;
    float* rec = reinterpret_cast<float*>(nodes + 4 * (size_t)node);
    const uint32_t ref = __float_as_uint(rec[12 + side]);
    if ((ref & REF_LEAF) || ref >= (uint32_t)n_nodes) return;
    const float* ch = reinterpret_cast<const float*>(nodes + 4 * (size_t)ref);
    const RBox b = rf_union(rf_load(ch), rf_load(ch + 6));
    rf_store(rec + 6 * side, b);
    if (!rf_finite(b)) atomicOr(&res->nonfinite, 1u);
}
