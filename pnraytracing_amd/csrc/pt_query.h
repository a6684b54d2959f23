// pnraytracing_amd/csrc/pt_query.h -- ray queries (pnrt_query_rays): the closest hit
// (BVHIntersect, ray_tracing.comp:429-461) or any hit (BVHIntersectP, :464-494) of
// caller rays, through the trace kernel's unified step (pt_wf.h wf_step) -- the
// renderer's visit order, `>` tie rule and z-slab culling under the context's
// traversal mode, so a query answers exactly what the renderer's own rays would see.
//
// Modelled on pt_primary_wf: one ray per lane, grid-stride over block-sized chunks
// of the ray array (grid <= the trace grid: the spill area is sized for it), the LDS
// short stack with a global spill area of the queries' own.  Rays are traced in the
// caller's order: no lane is refilled from a queue while its wave still traces (the
// persistent trace kernel's machinery) and rays are not sorted for coherence -- a
// caller that wants coherent waves passes coherent rays.
//
// Input: n x 7 floats (origin, direction, tMax), 28 bytes apart -- not a vector
// load's alignment.  A wave's 64 rays are 448 contiguous dwords: the wave loads
// them as 7 coalesced dword loads (256 B each, all in flight together) and hands
// them out through the LDS stack, empty between chunks: dword m of ray r goes to
// lane r's own slot of stack depth m / 2, half m % 2, and every lane reads its
// slots back (three 8-byte reads and a 4-byte one at its stack base address).  Only
// the wave's own lanes' slots are touched, so the block's waves stay independent:
// no block barrier.  (The stores are 4-way bank-conflicted -- dwords m, m + 2, m + 4
// of a ray share a bank --: 7 stores per 64 rays, against hundreds of steps.)
//
// A ray with a non-finite float or a direction of three zeros is invalid: it is
// never traversed (its lane stays finished, like a lane beyond n) and its record
// says so.  Every other bit pattern is traversed, tMax <= 0 and unnormalised
// directions included.
//
// Output, 64 B per ray as four 16-byte stores (include/pnrt.h pnrt_hit): words 0-12
// are the oracle's record (oracle/pn_oracle.c put_isect) -- hit, position, normal,
// texcoord, textureId, materialId, time, tMax after --, 13 the accepted triangle
// (caller's order; -1: none), 14 flags (bit 0: invalid ray), 15 zero.  An any-hit
// query reports no interaction (words 1-11 zero) and names the triangle that ended it.
#pragma once
#include "pt_wf.h"

#define PT_QUERY_INVALID 1u        // record word 14, bit 0

// The thread index behind an opaque move: what is derived from it is computed where
// it is used, every chunk.  (Derived from threadIdx.x itself, the compiler hoists the
// staging addresses and the 64-bit ray index out of the chunk loop and keeps them in
// registers across the traversal: 14 VGPRs spilled to scratch at 7 waves per SIMD.)
PN_DEV uint32_t query_tid() {
    uint32_t t = threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
}

template <int STK, bool TBL>
__global__ void __launch_bounds__(WF_TRACE_BLOCK, PT_PRIM_WF_WAVES) pt_query_wf(DevScene s, WfBufs b, const float* rays,
                                                                             uint32_t n, int any_hit, int mode, uint4* out) {
    static_assert(STK + 1 >= 4, "the ray staging area takes four stack depths");
    __shared__ uint2 lds[(STK + 1) * WF_TRACE_BLOCK];     // STK depths + the spare one (wf_push)
    const __amdgpu_buffer_rsrc_t geo =
        __builtin_amdgcn_make_buffer_rsrc((void*)s.nodes, (short)0, (int)s.geo_bytes, 0x00020000);
    char* const stage = reinterpret_cast<char*>(lds);
    for (size_t base = (size_t)blockIdx.x * WF_TRACE_BLOCK; base < n; base += (size_t)gridDim.x * WF_TRACE_BLOCK) {
        // ---- the wave's rays: coalesced dword loads -> LDS -> 7 dwords per lane
        float q[7];
        {
            const uint32_t tid = query_tid(), lane = tid & 63u;
            const uint32_t w64 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid & ~63u));   // the wave's first ray of the chunk
            const size_t wray = base + w64;
            // dwords of the wave's rays that exist (0: the wave is beyond n)
            const uint32_t have = wray < n ? (uint32_t)min((size_t)n - wray, (size_t)64) * 7u : 0u;
            const float* src = rays + PT_CHECK(b.fault, have ? wray * 7u : 0, (size_t)n * 7u, PT_SITE_RAY);
            float v[7];
#pragma unroll
            for (uint32_t j = 0; j < 7; ++j) {       // (a dword beyond the array reads the wave's first instead, unused)
                const uint32_t k = lane + 64u * j;
                v[j] = have ? src[k < have ? k : 0u] : 0.f;
            }
#pragma unroll
            for (uint32_t j = 0; j < 7; ++j) {
                const uint32_t k = lane + 64u * j, r = k / 7u, m = k - 7u * r;
                *reinterpret_cast<float*>(stage + ((m >> 1) * WF_SPA_STRIDE + (w64 + r) * 8u + (m & 1u) * 4u)) = v[j];
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");     // the wave's stores before its lanes' reads
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (uint32_t m = 0; m < 7; ++m)
                q[m] = *reinterpret_cast<const float*>(stage + ((m >> 1) * WF_SPA_STRIDE + tid * 8u + (m & 1u) * 4u));
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");     // ... and the reads before the stack's pushes
            __builtin_amdgcn_wave_barrier();
        }
        bool valid = base + threadIdx.x < n;
#pragma unroll
        for (int m = 0; m < 7; ++m) valid = valid & ((__float_as_uint(q[m]) & 0x7f800000u) != 0x7f800000u);
        valid = valid & !((q[3] == 0.0f) & (q[4] == 0.0f) & (q[5] == 0.0f));
        TravState t;
        // (an invalid ray's lane holds a harmless ray: it is never stepped as a busy lane)
        t.r = valid ? make_ray(mk3(q[0], q[1], q[2]), mk3(q[3], q[4], q[5]), mode)
                    : make_ray(mk3(0.f, 0.f, 0.f), mk3(0.f, 0.f, 1.f), 0);
        t.tMax = valid ? q[6] : 0.f;
        t.hitTri = -1; t.lt = 0; t.lc = 0;
        t.spa = (uint32_t)threadIdx.x * 8u;
        t.cur = REF_NONE;
        t.rid = any_hit ? 0u : 2u << 30;       // a shadow kind (any hit) / closest hit
        t.nst = 0;
        float zlo;
        if (valid && box_fast(t.r, s.root_min[0], s.root_min[1], s.root_min[2], s.root_max[0], s.root_max[1],
                              s.root_max[2], zlo)) {
            t.cur = s.root_ref;
            if (t.cur & REF_LEAF) { if (TBL) decode_leaf(s, t.cur, t.lt, t.lc); else t.lt = (int)t.cur; t.cur = REF_NONE; }
        }
        int busy = valid && (t.cur != REF_NONE || wf_has_tri<TBL>(t));
        auto run = [&](auto ident_tag) {
            constexpr bool ID = decltype(ident_tag)::value;
            for (;;) {
                if (wf_step<STK, ID, TBL>(s, b, geo, lds, t) & (busy != 0)) {
                    // an any-hit ray may stop mid-tree: drop what it left, so that the lane's
                    // further steps are the no-ops a finished closest-hit lane's are
                    busy = 0;
                    t.lt = 0; t.lc = 0; t.cur = REF_NONE; t.spa &= WF_SPA_STRIDE - 1u;
                }
                if (__ballot(busy != 0) == 0) break;
            }
        };
        if (__ballot(busy != 0) != 0) {
            if (__ballot(busy != 0 && t.r.kz() != 2) == 0) run(std::true_type{});
            else run(std::false_type{});
        }
        const size_t i = base + query_tid();
        if (i >= n) continue;
        const int tri = wf_tri_index<TBL>(t.hitTri);
        uint4 r0 = make_uint4(0u, 0u, 0u, 0u), r1 = r0, r2 = r0;
        const uint4 r3 = make_uint4(__float_as_uint(t.tMax), (uint32_t)tri, valid ? 0u : PT_QUERY_INVALID, 0u);
        if (tri != -1) {
            r0.x = 1u;
            if (!any_hit) {
                const Hit h = make_hit(s, t.r, tri);
                r0 = make_uint4(1u, __float_as_uint(h.P.x), __float_as_uint(h.P.y), __float_as_uint(h.P.z));
                r1 = make_uint4(__float_as_uint(h.N.x), __float_as_uint(h.N.y), __float_as_uint(h.N.z), __float_as_uint(h.u));
                r2 = make_uint4(__float_as_uint(h.v), (uint32_t)h.tex, (uint32_t)h.mat, __float_as_uint(t.tMax));
            }
        }
        uint4* o = out + 4 * PT_CHECK(b.fault, i, (size_t)n, PT_SITE_RESULT);
        o[0] = r0; o[1] = r1; o[2] = r2; o[3] = r3;
    }
}
