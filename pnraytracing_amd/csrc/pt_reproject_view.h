// pnraytracing_amd/csrc/pt_reproject_view.h -- temporal reprojection under the camera models of
// pnrt_make_rays (pnrt_reproject_view): pt_reproject_kernel (pt_reproject.h) with view A's
// image-plane algebra replaced by the closed-form inverse of an orthographic, equirectangular or
// fisheye view's centre rays.  Defined bit for bit in DESIGN.md section 31.2;
// tests/reproject_view_ref.py restates it in numpy.  A pinhole view A is pt_reproject_kernel's.
//
// The kernel keeps pt_reproject_kernel's shape: one lane per pixel of B, a wave per 8x8 tile,
// striding over the tiles; the taps, the blend and the counts are pt_reproject.h's functions.  The
// model is a template parameter: an instantiation holds its own inverse alone -- no per-lane
// branch on a uniform, and the orthographic one no pnm_atan2 at all.
#pragma once
#include "pt_rays.h"
#include "pt_reproject.h"

// ra's camera is view A's: the twelve floats of its pnrt_ray_camera.  fov_deg: a fisheye's.
// (the fisheye's inverse holds three more live values across the gathers: at 7 waves it would spill one register)
template <int MODEL>
__global__ void __launch_bounds__(REPROJECT_BLOCK, MODEL == PT_CAM_FISHEYE ? REPROJECT_WAVES - 1 : REPROJECT_WAVES)
pt_reproject_view_kernel(ReprojectArgs ra, float fov_deg, const float4* acc, const float4* mom, const float4* pos_a,
                         const float4* nrm_a, const float4* pos_b, const float4* nrm_b, float4* acc_out, float4* mom_out,
                         ReprojectCounts* counts) {
    static_assert(MODEL == PT_CAM_ORTHO || MODEL == PT_CAM_EQUIRECT || MODEL == PT_CAM_FISHEYE, "pinhole: pt_reproject_kernel");
    const int p = threadIdx.x;
    const int W = ra.width, H = ra.height;
    const f3 E = mk3(ra.eye[0], ra.eye[1], ra.eye[2]), L = mk3(ra.llc[0], ra.llc[1], ra.llc[2]);
    const f3 Hh = mk3(ra.hor[0], ra.hor[1], ra.hor[2]), Vv = mk3(ra.ver[0], ra.ver[1], ra.ver[2]);
    // (pt_make_rays_kernel's basis)
    const f3 f = normalize(cross(Vv, Hh));
    [[maybe_unused]] const f3 r = normalize(Hh), u = normalize(Vv);
    [[maybe_unused]] const f3 Nv = cross(Hh, Vv);
    [[maybe_unused]] const float NN = dot(Nv, Nv);
    [[maybe_unused]] const float half_fov = (fov_deg * 0.017453292f) * 0.5f;
    const float tol2 = ra.position_tolerance * ra.position_tolerance;
    uint32_t n_reprojected = 0, n_disoccluded = 0, n_missed = 0, max_frames = 0;
    unsigned long long sum_frames = 0;
    for (uint32_t tile = blockIdx.x; tile < ra.n_tiles; tile += gridDim.x) {
        const int ty = (int)(tile / (uint32_t)ra.tiles_x), tx = (int)(tile - (uint32_t)ty * ra.tiles_x);
        const int x = tx * 8 + (p & 7), y = ty * 8 + (p >> 3);
        if (x >= W || y >= H) continue;                      // beyond the right or top edge
        const size_t pix = (size_t)y * W + x;
        const float4 pb = pos_b[pix], nb = nrm_b[pix];
        float4 out_acc = make_float4(0.f, 0.f, 0.f, 0.f), out_mom = make_float4(0.f, 0.f, 0.f, 0.f);
        if (pb.w == 0.0f) {                                  // a primary miss of the new view, or a pixel without a ray
            n_missed += 1;
        } else {
            const f3 P = mk3(pb.x, pb.y, pb.z);
            float s, t, dd;
            bool front = true;
            if constexpr (MODEL == PT_CAM_ORTHO) {
                const f3 q = sub(P, L);
                s = dot(cross(q, Vv), Nv) / NN;
                t = dot(cross(Hh, q), Nv) / NN;
                const float z = dot(q, f);
                front = z > 0.0f;
                dd = z * z;
            } else {
                const f3 d = sub(P, E);
                const float X = dot(d, r), Y = dot(d, u), Z = dot(d, f);
                dd = dot(d, d);
                if constexpr (MODEL == PT_CAM_EQUIRECT) {
                    const float phi = pnm_atan2(X, Z);
                    const float theta = pnm_atan2(Y, sqrtf(X * X + Z * Z));
                    s = phi / 6.2831855f + 0.5f;
                    t = theta / 3.1415927f + 0.5f;
                } else {
                    const float hyp = sqrtf(X * X + Y * Y);
                    const float theta = pnm_atan2(hyp, Z);
                    const float rho = theta / half_fov;
                    float a = 0.0f, b = 0.0f;
                    if (hyp != 0.0f) {                       // (NaN: the quotients are NaN, as every test wants them)
                        a = rho * (X / hyp);
                        b = rho * (Y / hyp);
                    }
                    s = (a + 1.0f) * 0.5f;
                    t = (b + 1.0f) * 0.5f;
                }
            }
            const float fx = s * (float)W, fy = t * (float)H;
            // (every comparison is false for NaN)
            constexpr bool WRAPX = MODEL == PT_CAM_EQUIRECT;
            const bool taps = front && fx >= -1.0f && (WRAPX ? fx <= (float)W : fx < (float)W) && fy >= -1.0f && fy < (float)H;
            uint32_t n1;
            if (reproject_taps<WRAPX>(ra, taps, fx, fy, tol2 * dd, P, nb, acc, mom, pos_a, nrm_a, out_acc, out_mom, n1)) {
                n_reprojected += 1;
                sum_frames += n1;
                max_frames = n1 > max_frames ? n1 : max_frames;
            } else {
                n_disoccluded += 1;
            }
        }
        acc_out[pix] = out_acc;
        mom_out[pix] = out_mom;
    }
    reproject_commit(n_reprojected, n_disoccluded, n_missed, sum_frames, max_frames, counts);
}
