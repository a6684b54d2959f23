// pnraytracing_amd/csrc/pt_cameras.h -- per-frame cameras (pnrt_render_cameras; DESIGN.md
// section 28): frame slot k of a batch is rendered with its own pinhole camera, the twelve
// floats at table[12 * k] (WfCams, pt_wf.h).  A sub-pixel shift of lower_left per frame is
// a box pixel filter, an eye moved over a lens disc with the image plane held at the focus
// distance a thin lens, an eye moved along a path camera motion blur; each frame stays the
// reference's shader for some camera uniforms (ray_tracing.comp:205-211, 980).
//
// The camera ray is therefore no longer one per pixel: pt_camera_rays_wf traces one per
// path slot and writes pt_primary_wf's record (q0, q1, q2) at rec[3 * slot]; the gen and
// shade kernels' WfCams instantiations (pt_wf.h) read it there.
#pragma once
#include "pt_wf.h"

// pt_primary_wf's loop over the batch's path slots: one camera ray per lane, grid-stride
// over block-sized chunks (grid <= the trace grid, so the trace's stack spill area serves
// it), the same step, visit order and culling.  wf_coords gives slot = (tile *
// chunk_frames + k) * 64 + p: the 64 slots of a wave are one 8x8 tile of ONE frame, so k
// is wave-uniform and the frame's camera is read with scalar loads (wf_camera_dir).
// b.n is a multiple of 64: a wave is inside the batch or outside it as a whole.
// Slots beyond the image's edge (x >= width, lr >= rows: partial tiles) trace nothing;
// their records are never read (gen starts no path there).
template <int STK, bool TBL>
__global__ void __launch_bounds__(WF_TRACE_BLOCK, PT_PRIM_WF_WAVES) pt_camera_rays_wf(DevScene s, FrameParams fp, WfBufs b,
                                                                                   WfCams cm, float4* rec) {
    __shared__ uint2 lds[(STK + 1) * WF_TRACE_BLOCK];     // STK depths + the spare one (wf_push)
    const __amdgpu_buffer_rsrc_t geo =
        __builtin_amdgcn_make_buffer_rsrc((void*)s.nodes, (short)0, (int)s.geo_bytes, 0x00020000);
    const size_t n = b.n;
    for (size_t base = (size_t)blockIdx.x * WF_TRACE_BLOCK; base < n; base += (size_t)gridDim.x * WF_TRACE_BLOCK) {
        const size_t i = base + threadIdx.x;
        // (wave-uniform: the loop's step and n are multiples of 64, so every lane reads a k of its own batch)
        if (i >= n) continue;
        int px, lr, k;
        wf_coords(b, (uint32_t)i, px, lr, k);
        const bool mine = px < fp.width && lr < fp.rows;
        const int py = shard_row(mine ? lr : 0, fp.band, fp.n_shards, fp.shard);
        f3 eye;
        const f3 dir = wf_camera_dir(fp, cm, k, mine ? px : 0, py, eye);
        TravState t;
        t.r = make_ray(eye, dir, fp.mode);
        t.tMax = PT_FLOAT_MAX;
        t.rid = 2u << 30;       // closest hit
        wf_trace_closest<STK, TBL>(s, b, geo, lds, t, mine);
        if (mine) wf_primary_record<TBL>(s, t, dir, rec + 3 * PT_CHECK(b.fault, i, n, PT_SITE_PRIMARY));
    }
}
