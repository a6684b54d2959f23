// pnraytracing_amd/csrc/pt_denoise.h -- the denoised previews (pnrt_denoise and
// pnrt_denoise_variance): the edge-avoiding a-trous wavelet filter (Dammertz et al.
// 2010) on the albedo-demodulated accumulation image, guided by the first-hit images of
// pt_guides.h.  The filter is written once; VAR selects the variance-guided one, whose
// own steps are in pt_denoise_var.h.  Every float operation and its order is the text
// of DESIGN.md section 20 ("Guide images and the denoised preview") and, for VAR,
// section 24.2; tests/atrous_ref.py and tests/atrous_var_ref.py restate the same texts
// in numpy, and the kernels agree with them bit for bit.
//
// pt_denoise_prep<VAR>, once per call: per pixel one compact guide record
//   g0 = (N.xyz, pass-through flag 1 / 0), g1 = (P.xyz, 0)
// and the demodulated colour c = accum.rgb / max(albedo.rgb, 1/256); VAR: c.w = the
// variance image's start.
// pt_denoise_pass<VAR, STEP, LAST>, one per level: 25 taps at spacing 2^level, three
// 16-byte loads a tap (g0, g1, colour) -- from an LDS tile with halo at the spacings 1,
// 2, 4 (STEP = the spacing), through the caches at 8 and 16 (STEP = 0) -- ping-pong
// between two images; the last pass multiplies the albedo back and copies the
// pass-through pixels from the accumulation image.  A wave covers an 8x8-pixel tile (the
// order of pt_wf.h wf_coords), a block 16x16.
#pragma once
#include "pt_guides.h"
#include "pt_denoise_var.h"

#define DN_ALBEDO_MIN 0.00390625f      // 1 / 256

struct DenoiseParams {
    int width, height;
    // colour: what the exponent's colour term is scaled with -- 1 / sigma^2 of the pass (sigma_color *
    // 2^-pass); VAR: sigma_variance (not scaled per pass).  inv_n, inv_p: 1 / sigma^2 of normal and position
    float colour, inv_n, inv_p;
    int step;                      // tap spacing 2^pass
};

PN_DEV bool dn_coords(const DenoiseParams& d, int& x, int& y) {
    const int w = (int)(threadIdx.x >> 6), l = (int)(threadIdx.x & 63u);
    x = (int)blockIdx.x * 16 + (w & 1) * 8 + (l & 7);
    y = (int)blockIdx.y * 16 + (w >> 1) * 8 + (l >> 3);
    return x < d.width && y < d.height;
}

// moments: the sample moments (VAR; unused otherwise)
template <bool VAR>
__global__ void __launch_bounds__(256) pt_denoise_prep(DenoiseParams d, const float* materials, int n_materials,
                                                       const float4* accum, const float4* pos, const float4* nrm,
                                                       const float4* alb, const float4* moments, float4* guide,
                                                       float4* col) {
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
        const float4 m = make_float4(fmax_(al.x, DN_ALBEDO_MIN), fmax_(al.y, DN_ALBEDO_MIN), fmax_(al.z, DN_ALBEDO_MIN), 0.f);
        c.x = a.x / m.x;
        c.y = a.y / m.y;
        c.z = a.z / m.z;
        if constexpr (VAR) c.w = dnv_start(m, c, moments[i]);
    }
    col[i] = c;
}

PN_DEV float dn_dist2(float4 q, float4 p) {
    const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
    return (dx * dx + dy * dy) + dz * dz;
}

struct DnSums { float w, x, y, z, v; };      // v: the variance filter's fifth sum

// One tap: its weight from the exponent's colour term ec and
// the guide records, and its share of the sums.
template <bool VAR>
PN_DEV void dn_tap(const DenoiseParams& d, float hw, float ec, float4 t0, float4 t1, float4 tc, float4 g0, float4 g1,
                   DnSums& s) {
    const float e = (ec + dn_dist2(t0, g0) * d.inv_n) + dn_dist2(t1, g1) * d.inv_p;
    const float w = hw * pnm_exp2(-e);
    s.w = s.w + w;
    s.x = s.x + w * tc.x;
    s.y = s.y + w * tc.y;
    s.z = s.z + w * tc.z;
    if (VAR) s.v = s.v + (w * w) * tc.w;
}
// The level's pixel (20.2 step 5; 24.2 steps 5c and 6).  LAST: the final level -- remodulate, alpha 1
template <bool VAR, bool LAST>
PN_DEV float4 dn_result(const DnSums& s, const float4* alb, size_t i) {
    float4 r = make_float4(s.x / s.w, s.y / s.w, s.z / s.w, 0.f);
    if (LAST) {
        const float4 al = alb[i];
        r.x = r.x * fmax_(al.x, DN_ALBEDO_MIN);
        r.y = r.y * fmax_(al.y, DN_ALBEDO_MIN);
        r.z = r.z * fmax_(al.z, DN_ALBEDO_MIN);
        r.w = 1.0f;
    } else if (VAR) {
        r.w = s.v / (s.w * s.w);
    }
    return r;
}

// One pixel (x, y) of one level.  tap(xx, yy, j, t0, t1, tc) fetches the records of the
// pixel (xx, yy), which is pixel j of the image, and returns false for one to skip: a
// pass-through pixel (weight exactly 0).  BOUNDS: a pixel outside the image is skipped
// before it is fetched (otherwise tap answers false for it and does not look at j).  VAR: the 3x3 prefilter of the variance (step 5a) reads the
// +-1 neighbours' flags and variances through tap too.
// LAST: a pass-through pixel is copied from the accumulation image (no later pass reads
// its colour, so the other passes write nothing).
template <bool VAR, bool BOUNDS, bool LAST, class Tap>
PN_DEV void dn_pixel(const DenoiseParams& d, int x, int y, int spacing, Tap tap, float4* dst, const float4* accum,
                     const float4* alb) {
    const size_t i = (size_t)y * d.width + x;
    auto outside = [](int v, int n) { return BOUNDS && (v < 0 || v >= n); };
    // (unsigned: inside the image no term is negative, and the signed form costs the kernels that
    // fetch by j an extension of the width's sign per row, 22 VALU instructions)
    auto pixel = [&](int xx, int yy) { return (size_t)(uint32_t)yy * (uint32_t)d.width + (uint32_t)xx; };
    float4 g0, g1, c;
    if (!tap(x, y, i, g0, g1, c)) {
        if (LAST) dst[i] = accum[i];
        return;
    }
    float r = 0.f, lc = 0.f;
    if constexpr (VAR) {
        const float kk[3] = {0.25f, 0.5f, 0.25f};
        float G = 0.f, K = 0.f;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const int yy = y + dy;
            if (outside(yy, d.height)) continue;
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int xx = x + dx;
                if (outside(xx, d.width)) continue;
                float4 t0, t1, tc;
                if (!tap(xx, yy, pixel(xx, yy), t0, t1, tc)) continue;
                const float k = kk[dy + 1] * kk[dx + 1];
                G = G + k * tc.w;
                K = K + k;
            }
        }
        r = dnv_scale(d.colour, G, K);
        lc = moments_luma(c);
    }
    const float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    DnSums s = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int yy = y + dy * spacing;
        if (outside(yy, d.height)) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int xx = x + dx * spacing;
            if (outside(xx, d.width)) continue;
            float4 t0, t1, tc;
            if (!tap(xx, yy, pixel(xx, yy), t0, t1, tc)) continue;
            const float ec = VAR ? dnv_colour_term(tc, lc, r) : dn_dist2(tc, c) * d.colour;
            dn_tap<VAR>(d, h[dy + 2] * h[dx + 2], ec, t0, t1, tc, g0, g1, s);
        }
    }
    dst[i] = dn_result<VAR, LAST>(s, alb, i);
}

// One level.  STEP = 1, 2, 4: the level of that spacing, where a 16x16 block's taps
// overlap: the block stages its tile and a halo of 2 * STEP pixels (>= 2, so it holds
// the prefilter's +-1 neighbours) -- (16 + 4 STEP)^2 entries of 48 B: 19, 27 and 48 KiB
// -- in LDS once, and the taps read LDS.  An entry outside the image carries the
// pass-through flag, so it is skipped like one.  STEP = 0: any spacing (d.step), the
// taps fetched through the caches; VAR: the prefilter's eight off-centre neighbours are
// extra loads there, a flag and a variance each, 4 bytes both.  The same operations in
// the same order either way: the same bits.  Measured at 1080p, LDS against the caches
// at the same spacing: 0.11 vs 0.26 ms (prep + spacing 1), 0.07 vs 0.20 (2), 0.10 vs
// 0.18 (4); spacing 8 would need 108 KiB a block, 16 more than a CU has.
#ifndef DN_LDS_MAX_STEP
#define DN_LDS_MAX_STEP 4      // the largest spacing through LDS; 0: every spacing through the caches (the A/B baseline)
#endif
template <bool VAR, int STEP, bool LAST>
__global__ void __launch_bounds__(256) pt_denoise_pass(DenoiseParams d, const float4* guide, const float4* src,
                                                       float4* dst, const float4* accum, const float4* alb) {
    int x, y;
    if constexpr (STEP > 0) {
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
        if (!dn_coords(d, x, y)) return;
        const int kc = (y - y0) * T + (x - x0);
        dn_pixel<VAR, false, LAST>(d, x, y, STEP, [&](int xx, int yy, size_t j, float4& t0, float4& t1, float4& tc) {
            const int k = kc + (yy - y) * T + (xx - x);     // (from the pixel's own entry: a constant offset once unrolled)
            t0 = s_g0[k];
            if (t0.w != 0.0f) return false;
            t1 = s_g1[k]; tc = s_c[k];
            return true;
        }, dst, accum, alb);
    } else {
        if (!dn_coords(d, x, y)) return;
        dn_pixel<VAR, true, LAST>(d, x, y, d.step, [&](int xx, int yy, size_t j, float4& t0, float4& t1, float4& tc) {
            // (the compiler moves the loads of a tap's t1 and tc behind the flag test itself; written
            // that way, as above, the four kernels of this branch take 3 to 5 VGPRs more)
            t0 = guide[2 * j]; t1 = guide[2 * j + 1]; tc = src[j];
            return t0.w == 0.0f;
        }, dst, accum, alb);
    }
}
