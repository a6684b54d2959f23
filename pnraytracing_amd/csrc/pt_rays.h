// pnraytracing_amd/csrc/pt_rays.h -- rendering from caller ray buffers (pnrt_render_rays,
// pnrt_render_guides_rays) and a device ray generator for four camera models
// (pnrt_make_rays); DESIGN.md section 29.
//
// A ray batch is a camera batch (pt_cameras.h) whose camera ray of pixel (x, y) of frame
// slot k is not made from the frame's twelve camera floats but read from memory: record
// k * frame_stride + y * width + x of the caller's buffer, 32 bytes (origin, -, direction,
// -) -- WfRays, pt_wf.h.  pt_rays_wf traces one ray per path slot and writes pt_primary_wf's
// record at rec[3 * slot]; the gen kernel's WfRays instantiation reads V = -direction from
// the buffer, the shade kernels' index the records by slot as a camera batch's do.
#pragma once
#include "pt_wf.h"

// pt_query.h's rule: a record with a non-finite float among its six, or a direction of
// three zeros, is no ray.
PN_DEV bool ray_record_valid(const float4& o, const float4& d) {
    bool v = true;
    const float q[6] = {o.x, o.y, o.z, d.x, d.y, d.z};
#pragma unroll
    for (int m = 0; m < 6; ++m) v = v & ((__float_as_uint(q[m]) & 0x7f800000u) != 0x7f800000u);
    return v & !((d.x == 0.0f) & (d.y == 0.0f) & (d.z == 0.0f));
}

// pt_camera_rays_wf's loop (the same step, visit order, culling, grid bound and spill area)
// with the lane's ray taken by two 16-byte loads.  wf_coords makes a wave one 8x8 tile of
// one frame: each of its eight rows reads one contiguous 256-byte run of the buffer.
// A record that is no ray is never traversed (its lane stays finished, like a lane beyond
// the image's edge) and its slot gets a miss record whose environment colour is 0: gen then
// writes the frame colour (0, 0, 0) and starts no path.
// PIX: the record of pixel (x, lr) goes to rec[3 * (lr * width + x)], the per-pixel order
// pt_guides reads (pnrt_render_guides_rays: one frame, the whole image), not to its slot.
// AD: empty, or WfAdapt -- the slots of an adaptive ray batch (pnrt_render_rays_adaptive; DESIGN.md
// section 30), through its list.  A wave is still one 8x8 tile of one frame; a lane whose mask bit
// is clear is a lane beyond the edge: never stepped as a busy lane, no record.
template <int STK, bool TBL, bool PIX = false, class... AD>
__global__ void __launch_bounds__(WF_TRACE_BLOCK, PT_PRIM_WF_WAVES) pt_rays_wf(DevScene s, FrameParams fp, WfBufs b, WfRays ry,
                                                                            float4* rec, AD... adv) {
    constexpr bool ADAPT = wf_pack_is<WfAdapt, AD...>;
    static_assert(!(ADAPT && PIX), "an adaptive batch's records go to their slots");
    [[maybe_unused]] const WfAdapt ad = wf_adapt(adv...);
    __shared__ uint2 lds[(STK + 1) * WF_TRACE_BLOCK];     // STK depths + the spare one (wf_push)
    const __amdgpu_buffer_rsrc_t geo =
        __builtin_amdgcn_make_buffer_rsrc((void*)s.nodes, (short)0, (int)s.geo_bytes, 0x00020000);
    const size_t n = b.n;
    for (size_t base = (size_t)blockIdx.x * WF_TRACE_BLOCK; base < n; base += (size_t)gridDim.x * WF_TRACE_BLOCK) {
        const size_t i = base + threadIdx.x;
        // (wave-uniform: the loop's step and n are multiples of 64)
        if (i >= n) continue;
        int px, lr, k;
        bool active = true;
        if constexpr (ADAPT) active = wf_coords_adaptive_wave(b, ad, (uint32_t)i, px, lr, k);
        else wf_coords(b, (uint32_t)i, px, lr, k);
        const bool mine = active && px < fp.width && lr < fp.rows;
        const int py = shard_row(mine ? lr : 0, fp.band, fp.n_shards, fp.shard);
        // (a lane beyond the edge reads the record of column 0 of its frame's first row, unused)
        const float4* r = wf_ray_record(b, fp, ry, k, mine ? px : 0, py);
        const float4 o = r[0], d = r[1];
        const bool go = mine & ray_record_valid(o, d);
        const f3 dir = mk3(d.x, d.y, d.z);
        TravState t;
        // (a lane without a ray holds a harmless one: it is never stepped as a busy lane)
        t.r = go ? make_ray(mk3(o.x, o.y, o.z), dir, fp.mode) : make_ray(mk3(0.f, 0.f, 0.f), mk3(0.f, 0.f, 1.f), 0);
        t.tMax = PT_FLOAT_MAX;
        t.rid = 2u << 30;       // closest hit
        wf_trace_closest<STK, TBL>(s, b, geo, lds, t, go);
        if (mine) {
            float4* out;
            if constexpr (PIX) out = rec + 3 * PT_CHECK(b.fault, (size_t)lr * fp.width + px, (size_t)fp.rows * fp.width, PT_SITE_PRIMARY);
            else out = rec + 3 * PT_CHECK(b.fault, i, n, PT_SITE_PRIMARY);
            if (go) {
                wf_primary_record<TBL>(s, t, dir, out);
            } else {
                out[0] = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
                out[1] = make_float4(0.f, 0.f, 0.f, 0.f);
                out[2] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    }
}

// ---- the ray generator (pnrt_make_rays) ------------------------------------------------------
#define PT_CAM_PINHOLE 0
#define PT_CAM_ORTHO 1
#define PT_CAM_EQUIRECT 2
#define PT_CAM_FISHEYE 3

struct MakeRays {
    float eye[3], llc[3], hor[3], ver[3];
    int model;
    float fov_deg, aa_width, lens_radius, focus_distance;
    int per_pixel;
    int width, height;
    uint32_t first_frame, n_sets;
    int64_t frame_stride;
};

// Sample i of frame `frame`: pnrt_camera_sequence's rank-1
// sequence, rotated per pixel by h (0: the per-frame samples of section 28.4).
PN_DEV float make_rays_u(uint32_t frame, int i, uint32_t h) {
    const uint32_t A[4] = {0xDB4F0B91u, 0xBBE05633u, 0xA0F2EC77u, 0x89E18285u};
    const uint32_t n = frame + 1u;
    return (float)((n * A[i] + h) >> 8) * 5.9604644775390625e-8f;      // 2^-24
}

// One record per thread: set k, pixel (x, y).  Every product and sum is rounded on its own
// (the library is built without contraction); the order is DESIGN.md section 29.3's.
__global__ void __launch_bounds__(256) pt_make_rays_kernel(MakeRays m, float4* out) {
    const size_t set = (size_t)m.width * m.height;
    const size_t gi = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gi >= set * m.n_sets) return;
    const uint32_t k = (uint32_t)(gi / set);
    const uint32_t p = (uint32_t)(gi - (size_t)k * set);
    const int y = (int)(p / (uint32_t)m.width), x = (int)(p - (uint32_t)y * (uint32_t)m.width);
    const uint32_t frame = m.first_frame + k;
    float u[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint32_t h = 0u;
        if (m.per_pixel) { uint32_t seed = 4u * p + (uint32_t)i; h = wang_hash(seed); }
        u[i] = make_rays_u(frame, i, h);
    }
    const f3 E = mk3(m.eye[0], m.eye[1], m.eye[2]), L = mk3(m.llc[0], m.llc[1], m.llc[2]);
    const f3 Hh = mk3(m.hor[0], m.hor[1], m.hor[2]), Vv = mk3(m.ver[0], m.ver[1], m.ver[2]);
    float s = (float)x / (float)m.width, t = (float)y / (float)m.height;
    if (m.aa_width > 0.0f) {
        s = s + ((u[0] - 0.5f) * m.aa_width) / (float)m.width;
        t = t + ((u[1] - 0.5f) * m.aa_width) / (float)m.height;
    }
    f3 O = E, D = mk3(0.f, 0.f, 0.f);
    if (m.model == PT_CAM_PINHOLE) {
        f3 Lc = L, Hc = Hh, Vc = Vv;
        if (m.lens_radius > 0.0f) {
            const f3 c = sub(add(add(L, smul(0.5f, Hh)), smul(0.5f, Vv)), E);
            const float sc = m.focus_distance / sqrtf(dot(c, c));
            const float r = m.lens_radius * sqrtf(u[2]);
            const float phi = 6.2831855f * u[3];
            float sn, cs;
            pnm_sincos(phi, sn, cs);
            const float a = r * cs, bq = r * sn;
            O = add(add(E, smul(a, divs(Hh, sqrtf(dot(Hh, Hh))))), smul(bq, divs(Vv, sqrtf(dot(Vv, Vv)))));
            Lc = add(E, muls(sub(L, E), sc));
            Hc = muls(Hh, sc);
            Vc = muls(Vv, sc);
        }
        D = normalize(sub(add(add(Lc, smul(s, Hc)), smul(t, Vc)), O));
    } else {
        const f3 f = normalize(cross(Vv, Hh));
        if (m.model == PT_CAM_ORTHO) {
            O = add(add(L, smul(s, Hh)), smul(t, Vv));
            D = f;
        } else {
            const f3 rr = normalize(Hh), uu = normalize(Vv);
            if (m.model == PT_CAM_EQUIRECT) {
                const float phi = (s - 0.5f) * 6.2831855f, theta = (t - 0.5f) * 3.1415927f;
                float sp, cp, st, ct;
                pnm_sincos(phi, sp, cp);
                pnm_sincos(theta, st, ct);
                D = normalize(add(add(smul(ct * sp, rr), smul(st, uu)), smul(ct * cp, f)));
            } else {
                const float a = 2.0f * s - 1.0f, bq = 2.0f * t - 1.0f;
                const float rho = sqrtf(a * a + bq * bq);
                if (rho > 1.0f) {
                    O = mk3(0.f, 0.f, 0.f);           // no ray: six zeros
                } else if (rho == 0.0f) {
                    D = f;
                } else {
                    const float theta = rho * ((m.fov_deg * 0.017453292f) * 0.5f);
                    float st, ct;
                    pnm_sincos(theta, st, ct);
                    const f3 q = add(smul(a / rho, rr), smul(bq / rho, uu));
                    D = normalize(add(smul(st, q), smul(ct, f)));
                }
            }
        }
    }
    float4* o = out + 2 * ((size_t)k * (size_t)m.frame_stride + p);
    o[0] = make_float4(O.x, O.y, O.z, 0.f);
    o[1] = make_float4(D.x, D.y, D.z, 0.f);
}
