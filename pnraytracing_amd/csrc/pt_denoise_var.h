// pnraytracing_amd/csrc/pt_denoise_var.h -- the variance-guided denoised preview
// (pnrt_denoise_variance): the a-trous filter of pt_denoise.h with the edge-stopping
// function of SVGF (Schied et al. 2017, section 4.4) in place of the global colour
// sigma.  The luminance difference between tap and centre is measured in units of
// the centre pixel's own standard error, which comes from a variance image filtered
// alongside the colour; its start is the variance of the mean luminance that the
// sample moments (pt_moments.h) hold.  Every float operation and its order is the
// text of DESIGN.md section 24.2; tests/atrous_var_ref.py restates the same text in
// numpy, and the two agree bit for bit.
//
// The variance rides in the colour image's fourth channel (0 and unused in
// pt_denoise.h), so a tap stays three 16-byte loads, the guide records are those of
// pt_denoise_prep, and the LDS tiles stay at 19, 27 and 48 KiB.  A non-last pass
// writes nothing for a pass-through pixel, so the ping-pong image holds stale data
// there: whether a neighbour or a tap counts is decided from the guide record's
// flag alone, never from the colour image.
#pragma once
#include "pt_denoise.h"
#include "pt_moments.h"

#define DNV_EPS 9.5367431640625e-07f   // 2^-20

struct DenoiseVarParams {
    int width, height;
    float sigma_v, inv_n, inv_p;   // sigma_variance (not scaled per pass); 1 / sigma^2 of normal and position
    int step;                      // tap spacing 2^pass
};

PN_DEV bool dnv_coords(const DenoiseVarParams& d, int& x, int& y) {
    DenoiseParams b{};
    b.width = d.width; b.height = d.height;
    return dn_coords(b, x, y);
}

// Steps 1-3: the guide record of pt_denoise_prep, and col = (c0, v0).
__global__ void __launch_bounds__(256) pt_denoise_var_prep(DenoiseVarParams d, const float* materials, int n_materials,
                                                           const float4* accum, const float4* pos, const float4* nrm,
                                                           const float4* alb, const float4* moments, float4* guide,
                                                           float4* col) {
    int x, y;
    if (!dnv_coords(d, x, y)) return;
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
        const float4 m = make_float4(fmax_(al.x, DN_ALBEDO_MIN), fmax_(al.y, DN_ALBEDO_MIN), fmax_(al.z, DN_ALBEDO_MIN), 0.f);
        c.x = a.x / m.x;
        c.y = a.y / m.y;
        c.z = a.z / m.z;
        const float4 mo = moments[i];
        const uint32_t cnt = __float_as_uint(mo.w);
        if (cnt >= 2u) {                          // the variance of the mean luminance, in demodulated units
            const float lm = moments_luma(m);
            c.w = ((mo.y / (float)(cnt - 1u)) / (float)cnt) / (lm * lm);
        } else {                                  // unmeasured: a standard error as large as the value
            const float l = moments_luma(c);
            c.w = l * l;
        }
    }
    col[i] = c;
}

// Step 5a's scale from the prefilter's sums: one division, one square root and one
// reciprocal per pixel and pass.
PN_DEV float dnv_scale(const DenoiseVarParams& d, float G, float K) {
    const float g = G / K;
    return 1.0f / (d.sigma_v * sqrtf(g) + DNV_EPS);
}

// One tap (step 5b): its weight and its share of the sums.  lc: the centre's luminance.
PN_DEV void dnv_tap(const DenoiseVarParams& d, float hw, float r, float4 t0, float4 t1, float4 tc, float4 g0, float4 g1,
                    float lc, float& sw, float& sx, float& sy, float& sz, float& sv) {
    const float e = (fabsf(moments_luma(tc) - lc) * r + dn_dist2(t0, g0) * d.inv_n) + dn_dist2(t1, g1) * d.inv_p;
    const float w = hw * pnm_exp2(-e);
    sw = sw + w;
    sx = sx + w * tc.x;
    sy = sy + w * tc.y;
    sz = sz + w * tc.z;
    sv = sv + (w * w) * tc.w;
}
// Step 5c; LAST: the final level -- remodulate, alpha 1 (step 6)
template <bool LAST>
PN_DEV float4 dnv_result(float sw, float sx, float sy, float sz, float sv, const float4* alb, size_t i) {
    float4 r = make_float4(sx / sw, sy / sw, sz / sw, 0.f);
    if (LAST) {
        const float4 al = alb[i];
        r.x = r.x * fmax_(al.x, DN_ALBEDO_MIN);
        r.y = r.y * fmax_(al.y, DN_ALBEDO_MIN);
        r.z = r.z * fmax_(al.z, DN_ALBEDO_MIN);
        r.w = 1.0f;
    } else {
        r.w = sv / (sw * sw);
    }
    return r;
}

// One level with the taps fetched through the caches (the spacings 8 and 16).  The
// eight off-centre neighbours of the prefilter are extra loads: a flag and a
// variance each, 4 bytes both.
template <bool LAST>
__global__ void __launch_bounds__(256) pt_denoise_var_pass(DenoiseVarParams d, const float4* guide, const float4* src,
                                                           float4* dst, const float4* accum, const float4* alb) {
    int x, y;
    if (!dnv_coords(d, x, y)) return;
    const size_t i = (size_t)y * d.width + x;
    const float4 g0 = guide[2 * i];
    if (g0.w != 0.0f) {                           // pass-through (its colour and variance are never read)
        if (LAST) dst[i] = accum[i];
        return;
    }
    const float4 g1 = guide[2 * i + 1], c = src[i];
    const float kk[3] = {0.25f, 0.5f, 0.25f};
    float G = 0.f, K = 0.f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int yy = y + dy;
        if (yy < 0 || yy >= d.height) continue;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int xx = x + dx;
            if (xx < 0 || xx >= d.width) continue;
            const size_t j = (size_t)yy * d.width + xx;
            if (guide[2 * j].w != 0.0f) continue;
            const float k = kk[dy + 1] * kk[dx + 1];
            G = G + k * src[j].w;
            K = K + k;
        }
    }
    const float r = dnv_scale(d, G, K), lc = moments_luma(c);
    const float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    float sw = 0.f, sx = 0.f, sy = 0.f, sz = 0.f, sv = 0.f;
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
            dnv_tap(d, h[dy + 2] * h[dx + 2], r, t0, t1, tc, g0, g1, lc, sw, sx, sy, sz, sv);
        }
    }
    dst[i] = dnv_result<LAST>(sw, sx, sy, sz, sv, alb, i);
}

// The same level for the spacings 1, 2 and 4 from the LDS tile of pt_denoise_pass_lds
// (same size, same halo of 2 * STEP >= 2 pixels, which holds the prefilter's +-1
// neighbours).  An entry outside the image carries the pass-through flag, so the
// prefilter and the taps skip it like one.  The same operations in the same order
// as pt_denoise_var_pass: the same bits.
template <int STEP, bool LAST>
__global__ void __launch_bounds__(256) pt_denoise_var_pass_lds(DenoiseVarParams d, const float4* guide, const float4* src,
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
    if (!dnv_coords(d, x, y)) return;
    const size_t i = (size_t)y * d.width + x;
    const int kc = (y - y0) * T + (x - x0);
    const float4 g0 = s_g0[kc];
    if (g0.w != 0.0f) {
        if (LAST) dst[i] = accum[i];
        return;
    }
    const float4 g1 = s_g1[kc], c = s_c[kc];
    const float kk[3] = {0.25f, 0.5f, 0.25f};
    float G = 0.f, K = 0.f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int k = kc + dy * T + dx;
            if (s_g0[k].w != 0.0f) continue;      // pass-through, or outside the image
            const float kw = kk[dy + 1] * kk[dx + 1];
            G = G + kw * s_c[k].w;
            K = K + kw;
        }
    }
    const float r = dnv_scale(d, G, K), lc = moments_luma(c);
    const float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    float sw = 0.f, sx = 0.f, sy = 0.f, sz = 0.f, sv = 0.f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int k = kc + dy * STEP * T + dx * STEP;
            const float4 t0 = s_g0[k];
            if (t0.w != 0.0f) continue;           // pass-through, or outside the image
            dnv_tap(d, h[dy + 2] * h[dx + 2], r, t0, s_g1[k], s_c[k], g0, g1, lc, sw, sx, sy, sz, sv);
        }
    }
    dst[i] = dnv_result<LAST>(sw, sx, sy, sz, sv, alb, i);
}
