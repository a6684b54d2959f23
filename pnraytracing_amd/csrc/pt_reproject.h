// pnraytracing_amd/csrc/pt_reproject.h -- temporal reprojection (pnrt_reproject; not in
// the reference, whose redraw starts the image again from one sample: main.cpp:592-596):
// after a camera move the accumulation and moments images of the old view A are resampled
// into the new view B, through the guide images of both, and history that belongs to
// another surface is rejected.  Defined bit for bit in DESIGN.md section 25;
// tests/reproject_ref.py restates it in numpy.
//
// One lane per pixel of B, a wave per 8x8 tile (pt_adaptive.h's tile arithmetic), so the
// four bilinear taps of a wave gather from a compact 2-D footprint of A's images.  A wave
// strides over the tiles and keeps its counts in registers; they are combined across the
// lanes once, and lane 0 issues the block's integer atomics -- on one of REPROJECT_SLOTS
// records, each in a cache line of its own, which the host adds up: with one record for all
// blocks the atomics on its line took as long as the rest of the kernel.
#pragma once
#include "pt_moments.h"

struct ReprojectArgs {
    float eye[3], llc[3], hor[3], ver[3];     // camera A, the view the history was rendered with
    float normal_min, position_tolerance;
    uint32_t max_history;
    int width, height, tiles_x;
    uint32_t n_tiles;
};

// what the host reads back (zeroed before the launch): REPROJECT_SLOTS partial records
struct alignas(128) ReprojectCounts {
    unsigned long long n_reprojected, n_disoccluded, n_missed, sum_frames;
    uint32_t max_frames, reserved;
};

#define REPROJECT_BLOCK 64        // one wave = one tile at a time
#define REPROJECT_MAX_GRID 8192   // (256 CUs x 4 SIMDs x the kernel's 7 waves: 7168 resident)
// Waves per SIMD the kernels are compiled for (72 VGPRs): what pt_reproject_kernel has always had, stated
// since the taps became a function -- inlined, its registers came out at 73.
#define REPROJECT_WAVES 7
#define REPROJECT_SLOTS 64

// Steps 3 and 4, shared by pt_reproject_kernel and pt_reproject_view_kernel
// (pt_reproject_view.h): the four bilinear taps around (fx, fy) of view A's images, their validity
// tests and the normalised blend.  taps: the projection's own test (in front, in range); lim:
// tol^2 * |d|^2; P, nb: the hit and the normal record of B's pixel.  true: out_acc / out_mom hold the
// reprojected pixel and n1 its capped frame count; false: disoccluded, nothing written.
// WRAPX (an equirectangular view A: DESIGN.md 31.2): the tap column wraps around the image
// instead of being tested against it; the clamp behind the wrap only keeps the address of a tap
// of weight 0 (column W + 1 at fx == W) inside a one-column image.
template <bool WRAPX>
PN_DEV bool reproject_taps(const ReprojectArgs& ra, bool taps, float fx, float fy, float lim, const f3& P, const float4& nb,
                           const float4* acc, const float4* mom, const float4* pos_a, const float4* nrm_a, float4& out_acc,
                           float4& out_mom, uint32_t& n1) {
    const int W = ra.width, H = ra.height;
    const float flx = taps ? floorf(fx) : 0.0f, fly = taps ? floorf(fy) : 0.0f;
    const int x0 = (int)flx, y0 = (int)fly;          // -1 .. W - 1 (WRAPX: W), -1 .. H - 1
    const float a = fx - flx, b = fy - fly;
    const float wgt[4] = {(1.0f - a) * (1.0f - b), a * (1.0f - b), (1.0f - a) * b, a * b};
    // all four taps' records at clamped (always in-bounds) addresses, then the tests
    float4 ta[4], tm[4];
    bool valid[4];
    bool any = false;
    float wsum = 0.0f;
    uint32_t nmin = 0xFFFFFFFFu;
    for (int i = 0; i < 4; ++i) {
        int xi = x0 + (i & 1);
        const int yi = y0 + (i >> 1);
        if (WRAPX) xi = xi < 0 ? xi + W : (xi >= W ? xi - W : xi);
        const bool inside = taps && (WRAPX || (xi >= 0 && xi < W)) && yi >= 0 && yi < H;
        const int xc = xi < 0 ? 0 : (xi >= W ? W - 1 : xi), yc = yi < 0 ? 0 : (yi >= H ? H - 1 : yi);
        const size_t at = (size_t)yc * W + xc;
        const float4 pa = pos_a[at], na = nrm_a[at];
        tm[i] = mom[at];
        ta[i] = acc[at];
        const f3 e = sub(mk3(pa.x, pa.y, pa.z), P);
        const uint32_t n = __float_as_uint(tm[i].w);
        valid[i] = inside && wgt[i] > 0.0f && pa.w == 1.0f && na.w == nb.w &&
                   dot(mk3(na.x, na.y, na.z), mk3(nb.x, nb.y, nb.z)) >= ra.normal_min && dot(e, e) <= lim && n >= 1u;
        if (valid[i]) {
            any = true;
            wsum = wsum + wgt[i];
            nmin = n < nmin ? n : nmin;
        }
    }
    if (!any) return false;
    float cx = 0.0f, cy = 0.0f, cz = 0.0f, mean = 0.0f, s2 = 0.0f;
    for (int i = 0; i < 4; ++i) {
        if (!valid[i]) continue;
        const float r = wgt[i] / wsum;
        const uint32_t n = __float_as_uint(tm[i].w);
        cx = cx + r * ta[i].x;
        cy = cy + r * ta[i].y;
        cz = cz + r * ta[i].z;
        mean = mean + r * tm[i].x;
        s2 = s2 + r * (tm[i].y / (float)(n - 1u > 1u ? n - 1u : 1u));
    }
    n1 = nmin < ra.max_history ? nmin : ra.max_history;
    out_acc = make_float4(cx, cy, cz, 1.0f);
    out_mom = make_float4(mean, s2 * (float)(n1 - 1u), 0.0f, __uint_as_float(n1));
    return true;
}

// A wave's counts, combined across its lanes; lane 0 adds them to the block's record.
PN_DEV void reproject_commit(uint32_t n_reprojected, uint32_t n_disoccluded, uint32_t n_missed, unsigned long long sum_frames,
                             uint32_t max_frames, ReprojectCounts* counts) {
    n_reprojected = moments_wave_sum(n_reprojected);
    n_disoccluded = moments_wave_sum(n_disoccluded);
    n_missed = moments_wave_sum(n_missed);
    sum_frames = moments_wave_sum(sum_frames);
    max_frames = moments_wave_max(max_frames);
    if (threadIdx.x != 0) return;
    counts += blockIdx.x % REPROJECT_SLOTS;
    if (n_reprojected) {
        atomicAdd(&counts->n_reprojected, (unsigned long long)n_reprojected);
        atomicAdd(&counts->sum_frames, sum_frames);
        atomicMax(&counts->max_frames, max_frames);
    }
    if (n_disoccluded) atomicAdd(&counts->n_disoccluded, (unsigned long long)n_disoccluded);
    if (n_missed) atomicAdd(&counts->n_missed, (unsigned long long)n_missed);
}

// acc / mom / pos_a / nrm_a: view A (read).  pos_b / nrm_b: view B's guides (read).
// acc_out / mom_out: the resampled images (other buffers than acc / mom: lanes gather
// from their neighbours' pixels).
__global__ void __launch_bounds__(REPROJECT_BLOCK, REPROJECT_WAVES)
pt_reproject_kernel(ReprojectArgs ra, const float4* acc, const float4* mom, const float4* pos_a, const float4* nrm_a,
                    const float4* pos_b, const float4* nrm_b, float4* acc_out, float4* mom_out, ReprojectCounts* counts) {
    const int p = threadIdx.x;
    const int W = ra.width, H = ra.height;
    const f3 eye = mk3(ra.eye[0], ra.eye[1], ra.eye[2]);
    const f3 hor = mk3(ra.hor[0], ra.hor[1], ra.hor[2]), ver = mk3(ra.ver[0], ra.ver[1], ra.ver[2]);
    const f3 L = sub(mk3(ra.llc[0], ra.llc[1], ra.llc[2]), eye);
    const f3 Nv = cross(hor, ver);
    const float LN = dot(L, Nv), NN = dot(Nv, Nv);
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
        if (pb.w == 0.0f) {                                  // a primary miss of the new view
            n_missed += 1;
        } else {
            const f3 P = mk3(pb.x, pb.y, pb.z);
            const f3 d = sub(P, eye);
            const float k = LN / dot(d, Nv);
            const f3 q = sub(smul(k, d), L);
            const float s = dot(cross(q, ver), Nv) / NN;
            const float t = dot(cross(hor, q), Nv) / NN;
            const float fx = s * (float)W, fy = t * (float)H;
            // (k - k == 0: finite; every comparison is false for NaN)
            const bool taps = k > 0.0f && (k - k) == 0.0f && fx >= -1.0f && fx < (float)W && fy >= -1.0f && fy < (float)H;
            uint32_t n1;
            if (reproject_taps<false>(ra, taps, fx, fy, tol2 * dot(d, d), P, nb, acc, mom, pos_a, nrm_a, out_acc, out_mom, n1)) {
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
