// pnraytracing_amd/csrc/pt_denoise.h -- the denoised preview (pnrt_denoise): the
// edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) on the
// albedo-demodulated accumulation image, guided by the first-hit images of
// pt_guides.h.  Every float operation and its order is the text of DESIGN.md
// section 20 ("Guide images and the denoised preview"); tests/atrous_ref.py
// restates the same text in numpy, and the two agree bit for bit.
//
// pt_denoise_prep, once per pnrt_denoise: per pixel one compact guide record
//   g0 = (N.xyz, pass-through flag 1 / 0), g1 = (P.xyz, 0)
// and the demodulated colour c = accum.rgb / max(albedo.rgb, 1/256).
// One pass per level: 25 taps at spacing 2^level, three 16-byte loads a tap (g0, g1,
// colour) -- from an LDS tile with halo at the spacings 1, 2, 4 (pt_denoise_pass_lds),
// through the caches at 8 and 16 (pt_denoise_pass) -- ping-pong between two images;
// the last pass multiplies the albedo back and copies the pass-through pixels from
// the accumulation image.  A wave covers an 8x8-pixel tile (the order of pt_wf.h
// wf_coords), a block 16x16.
#pragma once
#include "pt_guides.h"

#define DN_ALBEDO_MIN 0.00390625f      // 1 / 256

struct DenoiseParams {
    int width, height;
    float inv_c, inv_n, inv_p;     // 1 / sigma^2 of the pass (colour: sigma_color * 2^-pass)
    int step;                      // tap spacing 2^pass
};

PN_DEV bool dn_coords(const DenoiseParams& d, int& x, int& y) {
    const int w = (int)(threadIdx.x >> 6), l = (int)(threadIdx.x & 63u);
    x = (int)blockIdx.x * 16 + (w & 1) * 8 + (l & 7);
    y = (int)blockIdx.y * 16 + (w >> 1) * 8 + (l >> 3);
    return x < d.width && y < d.height;
}

__global__ void __launch_bounds__(256) pt_denoise_prep(DenoiseParams d, const float* materials, int n_materials,
                                                       const float4* accum, const float4* pos, const float4* nrm,
                                                       const float4* alb, float4* guide, float4* col) {
    int x, y;
    if (!dn_coords(d, x, y)) return;
    const size_t i = (size_t)y * d.width + x;
    const float4 a = accum[i], p = pos[i], n = nrm[i], al = alb[i];
    bool pass = p.w == 0.0f;                      // a miss
    if (!pass) {                                  // a hit on an emissive material
        const int mat = (int)n.w;
        f3 em = mk3(0.f, 0.f, 0.f);
        if (mat >= 0 && mat < n_materials) em = mk3(materials[18 * (size_t)mat], materials[18 * (size_t)mat + 1], materials[18 * (size_t)mat + 2]);
        pass = guide_emissive(em);
    }
    guide[2 * i] = make_float4(n.x, n.y, n.z, pass ? 1.0f : 0.0f);
    guide[2 * i + 1] = make_float4(p.x, p.y, p.z, 0.f);
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!pass) {
        c.x = a.x / fmax_(al.x, DN_ALBEDO_MIN);
        c.y = a.y / fmax_(al.y, DN_ALBEDO_MIN);
        c.z = a.z / fmax_(al.z, DN_ALBEDO_MIN);
    }
    col[i] = c;
}

PN_DEV float dn_dist2(float4 q, float4 p) {
    const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
    return (dx * dx + dy * dy) + dz * dz;
}

// One tap: its weight and its share of the sums.
PN_DEV void dn_tap(const DenoiseParams& d, float hw, float4 t0, float4 t1, float4 tc, float4 g0, float4 g1, float4 c,
                   float& sw, float& sx, float& sy, float& sz) {
    const float e = (dn_dist2(tc, c) * d.inv_c + dn_dist2(t0, g0) * d.inv_n) + dn_dist2(t1, g1) * d.inv_p;
    const float w = hw * pnm_exp2(-e);
    sw = sw + w;
    sx = sx + w * tc.x;
    sy = sy + w * tc.y;
    sz = sz + w * tc.z;
}
// LAST: the final level -- remodulate, alpha 1 (step 5)
template <bool LAST>
PN_DEV float4 dn_result(float sw, float sx, float sy, float sz, const float4* alb, size_t i) {
    float4 r = make_float4(sx / sw, sy / sw, sz / sw, 0.f);
    if (LAST) {
        const float4 al = alb[i];
        r.x = r.x * fmax_(al.x, DN_ALBEDO_MIN);
        r.y = r.y * fmax_(al.y, DN_ALBEDO_MIN);
        r.z = r.z * fmax_(al.z, DN_ALBEDO_MIN);
        r.w = 1.0f;
    }
    return r;
}

// One level with the taps fetched through the caches (any spacing; the spacings 4..16).
// LAST: pass-through pixels are copied from the accumulation image
template <bool LAST>
__global__ void __launch_bounds__(256) pt_denoise_pass(DenoiseParams d, const float4* guide, const float4* src,
                                                       float4* dst, const float4* accum, const float4* alb) {
    int x, y;
    if (!dn_coords(d, x, y)) return;
    const size_t i = (size_t)y * d.width + x;
    const float4 g0 = guide[2 * i];
    if (g0.w != 0.0f) {                           // pass-through (no later pass reads its colour)
        if (LAST) dst[i] = accum[i];
        return;
    }
    const float4 g1 = guide[2 * i + 1], c = src[i];
    const float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    float sw = 0.f, sx = 0.f, sy = 0.f, sz = 0.f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int yy = y + dy * d.step;
        if (yy < 0 || yy >= d.height) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int xx = x + dx * d.step;
            if (xx < 0 || xx >= d.width) continue;
            const size_t j = (size_t)yy * d.width + xx;
            const float4 t0 = guide[2 * j], t1 = guide[2 * j + 1], tc = src[j];
            if (t0.w != 0.0f) continue;           // a pass-through tap: weight exactly 0
            dn_tap(d, h[dy + 2] * h[dx + 2], t0, t1, tc, g0, g1, c, sw, sx, sy, sz);
        }
    }
    dst[i] = dn_result<LAST>(sw, sx, sy, sz, alb, i);
}

// The same level for the spacings 1, 2 and 4, where a 16x16 block's taps overlap:
// the block stages its tile and a halo of 2 * STEP pixels -- (16 + 4 STEP)^2 entries
// of 48 B: 19, 27 and 48 KiB -- in LDS once, and the 25 taps read LDS.  An entry
// outside the image carries the pass-through flag, so it is skipped like one.  The
// same operations in the same order as pt_denoise_pass: the same bits.  Measured
// at 1080p against pt_denoise_pass at the same spacing: 0.11 vs 0.26 ms (prep +
// spacing 1), 0.07 vs 0.20 (2), 0.10 vs 0.18 (4); spacing 8 would need 108 KiB a
// block, 16 more than a CU has.
#ifndef DN_LDS_MAX_STEP
#define DN_LDS_MAX_STEP 4      // 0: every spacing through pt_denoise_pass (the A/B baseline)
#endif
template <int STEP, bool LAST>
__global__ void __launch_bounds__(256) pt_denoise_pass_lds(DenoiseParams d, const float4* guide, const float4* src,
                                                           float4* dst, const float4* accum, const float4* alb) {
    constexpr int T = 16 + 4 * STEP;
    __shared__ float4 s_g0[T * T], s_g1[T * T], s_c[T * T];
    const int x0 = (int)blockIdx.x * 16 - 2 * STEP, y0 = (int)blockIdx.y * 16 - 2 * STEP;
    for (int k = (int)threadIdx.x; k < T * T; k += 256) {
        const int ty = k / T, tx = k - ty * T;
        const int gx = x0 + tx, gy = y0 + ty;
        float4 a = make_float4(0.f, 0.f, 0.f, 1.0f), b = make_float4(0.f, 0.f, 0.f, 0.f), cc = b;
        if (gx >= 0 && gx < d.width && gy >= 0 && gy < d.height) {
            const size_t j = (size_t)gy * d.width + gx;
            a = guide[2 * j]; b = guide[2 * j + 1]; cc = src[j];
        }
        s_g0[k] = a; s_g1[k] = b; s_c[k] = cc;
    }
    __syncthreads();
    int x, y;
    if (!dn_coords(d, x, y)) return;
    const size_t i = (size_t)y * d.width + x;
    const int kc = (y - y0) * T + (x - x0);
    const float4 g0 = s_g0[kc];
    if (g0.w != 0.0f) {
        if (LAST) dst[i] = accum[i];
        return;
    }
    const float4 g1 = s_g1[kc], c = s_c[kc];
    const float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    float sw = 0.f, sx = 0.f, sy = 0.f, sz = 0.f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int k = kc + dy * STEP * T + dx * STEP;
            const float4 t0 = s_g0[k];
            if (t0.w != 0.0f) continue;           // pass-through, or outside the image
            dn_tap(d, h[dy + 2] * h[dx + 2], t0, s_g1[k], s_c[k], g0, g1, c, sw, sx, sy, sz);
        }
    }
    dst[i] = dn_result<LAST>(sw, sx, sy, sz, alb, i);
}
