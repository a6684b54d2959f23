// pnraytracing_amd/csrc/pt_denoise_var.h -- what the variance-guided denoised preview
// (pnrt_denoise_variance) has of its own: the a-trous filter of pt_denoise.h with the
// edge-stopping function of SVGF (Schied et al. 2017, section 4.4) in place of the
// global colour sigma.  The luminance difference between tap and centre is measured in
// units of the centre pixel's own standard error, which comes from a variance image
// filtered alongside the colour; its start is the variance of the mean luminance that
// the sample moments (pt_moments.h) hold.  Every float operation and its order is the
// text of DESIGN.md section 24.2; tests/atrous_var_ref.py restates the same text in
// numpy, and the two agree bit for bit.
//
// The variance rides in the colour image's fourth channel (0 and unused by the fixed
// filter), so a tap stays three 16-byte loads, the guide records are the same, and the
// LDS tiles stay at 19, 27 and 48 KiB.  A non-last pass writes nothing for a
// pass-through pixel, so the ping-pong image holds stale data there: whether a
// neighbour or a tap counts is decided from the guide record's flag alone, never from
// the colour image.
//
// Here: the variance image's start (step 3), the scale from the 3x3 prefilter's sums
// (5a) and the colour term of a tap's exponent (5b).  The kernels, the prefilter's loop
// and the fifth sum are pt_denoise.h's, under its VAR switch.
#pragma once
#include "pt_moments.h"

#define DNV_EPS 9.5367431640625e-07f   // 2^-20

// Step 3: the start of the variance image.  m: the clamped albedo the colour was divided
// by, c: the demodulated colour, mo: the pixel's sample moments.
PN_DEV float dnv_start(float4 m, float4 c, float4 mo) {
    const uint32_t cnt = __float_as_uint(mo.w);
    if (cnt >= 2u) {                              // the variance of the mean luminance, in demodulated units
        const float lm = moments_luma(m);
        return ((mo.y / (float)(cnt - 1u)) / (float)cnt) / (lm * lm);
    }
    const float l = moments_luma(c);              // unmeasured: a standard error as large as the value
    return l * l;
}

// Step 5a's scale from the prefilter's sums: one division, one square root and one
// reciprocal per pixel and pass.
PN_DEV float dnv_scale(float sigma_v, float G, float K) {
    const float g = G / K;
    return 1.0f / (sigma_v * sqrtf(g) + DNV_EPS);
}

// Step 5b: the colour term of a tap's exponent.  lc: the centre's luminance, r: dnv_scale.
PN_DEV float dnv_colour_term(float4 tc, float lc, float r) { return fabsf(moments_luma(tc) - lc) * r; }
