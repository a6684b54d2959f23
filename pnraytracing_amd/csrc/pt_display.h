// pnraytracing_amd/csrc/pt_display.h -- the display transform and the luminance
// histogram behind auto exposure (pnrt_display, pnrt_luma_histogram_read; the
// reference shows the clamped accumulation through render.frag and has neither a
// tone curve nor an exposure).  Defined bit for bit in DESIGN.md section 26;
// tests/display_ref.py restates it in numpy.
//
// Display: a float4 image, row 0 = bottom, to one RGBA8 image.  Per channel
//   v = c * exposure;  s = v > 0 ? v : 0;  s = min(s, 65536);  t = tone(s);
//   t = min(t, 1);  u = transfer(t);  q = (uint8)floor(u * 255 + 0.5);  alpha 255
// every product and sum rounded on its own (-ffp-contract=off).
#pragma once
#include "pt_moments.h"

#define DISPLAY_TONE_CLAMP 0
#define DISPLAY_TONE_REINHARD 1
#define DISPLAY_TONE_ACES 2
#define DISPLAY_TRANSFER_LINEAR 0
#define DISPLAY_TRANSFER_SRGB 1

#define DISPLAY_BLOCK 256
#define DISPLAY_PIXELS_PER_LANE 4   // 4 x 16 B in, one 16 B store out

template <int TONE, int TRANSFER>
PN_DEV uint32_t display_channel(float c, float exposure, float w2) {
    const float v = c * exposure;
    float s = (v > 0.0f) ? v : 0.0f;             // NaN, negatives and -0 become +0
    s = fminf(s, 65536.0f);
    float t;
    if (TONE == DISPLAY_TONE_REINHARD) t = (s * (1.0f + s / w2)) / (1.0f + s);
    else if (TONE == DISPLAY_TONE_ACES) t = (s * (2.51f * s + 0.03f)) / (s * (2.43f * s + 0.59f) + 0.14f);
    else t = s;
    t = fminf(t, 1.0f);
    float u = t;
    if (TRANSFER == DISPLAY_TRANSFER_SRGB) {
        u = (t <= 0.0031308f) ? 12.92f * t : 1.055f * pnm_pow(t, __uint_as_float(0x3ED55555u)) - 0.055f;
        u = fminf(u, 1.0f);
    }
    return (uint32_t)floorf(u * 255.0f + 0.5f);
}

template <int TONE, int TRANSFER>
PN_DEV uint32_t display_pixel(float4 c, float exposure, float w2) {
    return display_channel<TONE, TRANSFER>(c.x, exposure, w2) | (display_channel<TONE, TRANSFER>(c.y, exposure, w2) << 8) |
           (display_channel<TONE, TRANSFER>(c.z, exposure, w2) << 16) | 0xFF000000u;
}

// A lane converts four consecutive pixels of the OUTPUT image, which is one flat
// run of npix words whatever the width: the 16-byte store is always aligned, and a
// group that crosses a row end simply reads its pixels from two source rows (rows
// are flipped, pixels within a row are not, so a row's loads and stores stay
// contiguous).  The last group of an image whose pixel count is no multiple of
// four stores word by word.  npix < 2^31 (the host checks), so no index wraps.
template <int TONE, int TRANSFER>
__global__ void __launch_bounds__(DISPLAY_BLOCK)
pt_display_kernel(const float4* __restrict__ src, uint32_t* __restrict__ dst, uint32_t width, uint32_t height, uint32_t npix,
                  int bottom_first, float exposure, float w2) {
    const uint32_t o0 = (blockIdx.x * DISPLAY_BLOCK + threadIdx.x) * DISPLAY_PIXELS_PER_LANE;
    if (o0 >= npix) return;
    uint32_t oy = o0 / width, x = o0 - oy * width;
    // all four loads first, so that they are in flight together; a pixel past the end of
    // the image reads the last pixel again and is not stored
    float4 c[DISPLAY_PIXELS_PER_LANE];
#pragma unroll
    for (int k = 0; k < DISPLAY_PIXELS_PER_LANE; ++k) {
        const bool in = o0 + (uint32_t)k < npix;
        const uint32_t cy = in ? oy : height - 1u, cx = in ? x : width - 1u;
        const uint32_t sy = bottom_first ? cy : height - 1u - cy;
        c[k] = src[(size_t)sy * width + cx];
        if (++x == width) { x = 0u; ++oy; }
    }
    uint32_t q[DISPLAY_PIXELS_PER_LANE];
#pragma unroll
    for (int k = 0; k < DISPLAY_PIXELS_PER_LANE; ++k) q[k] = display_pixel<TONE, TRANSFER>(c[k], exposure, w2);
    if (o0 + DISPLAY_PIXELS_PER_LANE <= npix) {
        *reinterpret_cast<uint4*>(dst + o0) = make_uint4(q[0], q[1], q[2], q[3]);
    } else {
#pragma unroll
        for (int k = 0; k < DISPLAY_PIXELS_PER_LANE; ++k)
            if (o0 + (uint32_t)k < npix) dst[o0 + k] = q[k];
    }
}

// ---- the luminance histogram ---------------------------------------------------------
// 16 bins per octave over 2^-16 .. 2^16 from the bits of Y alone: the exponent and the
// top four mantissa bits, (bits >> 19) - 1776 clamped to 0 .. 511 (1.0 -> 256).
#define LUMA_BINS 512
// A block ends with one global atomic per non-zero bin, all blocks on the same few hundred
// addresses: with 2 048 blocks of 256 lanes those atomics were most of the kernel's time
// (DESIGN.md section 26.4), so the blocks are large and few.
#define LUMA_HIST_BLOCK 1024
#define LUMA_HIST_MAX_BLOCKS 512
// One LDS histogram per block (0) or one per wave (1).  Rendered images put most pixels
// into a few bins, where the waves of a block collide on one LDS word; measured in
// DESIGN.md section 26 (tools/display_bench.py builds the other layout to compare).
#ifndef LUMA_HIST_PER_WAVE
#define LUMA_HIST_PER_WAVE 0
#endif

struct LumaHist {               // the device record: pnrt_luma_histogram's layout
    unsigned long long n_pixels, n_counted;
    unsigned long long bins[LUMA_BINS];
};

PN_DEV int luma_bin(float y) {
    const int b = (int)(__float_as_uint(y) >> 19) - 1776;
    return b < 0 ? 0 : (b > LUMA_BINS - 1 ? LUMA_BINS - 1 : b);
}

// Over the rows of a shard selector: a grid-stride loop, LDS atomics into the block's
// (or the wave's) histogram, then one 64-bit global atomic per non-zero bin.  Every
// field is an integer sum, so the record does not depend on the block order.
// total = rows * width < 2^31 (the host checks), so i + stride does not wrap.
__global__ void __launch_bounds__(LUMA_HIST_BLOCK)
pt_luma_hist_kernel(const float4* __restrict__ src, LumaHist* out, uint32_t width, uint32_t rows, int band, int n_shards,
                    int shard) {
    constexpr int kCopies = LUMA_HIST_PER_WAVE ? LUMA_HIST_BLOCK / 64 : 1;
    __shared__ uint32_t s_bins[kCopies][LUMA_BINS];
    __shared__ uint32_t s_cnt[2];
    for (int b = threadIdx.x; b < kCopies * LUMA_BINS; b += LUMA_HIST_BLOCK) (&s_bins[0][0])[b] = 0u;
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0u;
    __syncthreads();
    uint32_t* mine = s_bins[LUMA_HIST_PER_WAVE ? (threadIdx.x >> 6) : 0];
    const uint32_t total = rows * width;
    const uint32_t stride = gridDim.x * LUMA_HIST_BLOCK;
    uint32_t n_pixels = 0, n_counted = 0;
    auto fetch = [&](uint32_t i) {
        const uint32_t r = i / width, x = i - r * width;
        const int y = shard_row((int)r, band, n_shards, shard);
        return src[(size_t)y * width + x];
    };
    auto count = [&](float4 c) {
        const float Y = moments_luma(c);
        n_pixels += 1u;
        if (Y > 0.0f && Y < pnm_inf()) {         // (NaN fails the first comparison)
            n_counted += 1u;
            atomicAdd(&mine[luma_bin(Y)], 1u);
        }
    };
    // two pixels a turn, both loads before either is counted
    for (uint32_t i = blockIdx.x * LUMA_HIST_BLOCK + threadIdx.x; i < total; i += 2u * stride) {
        const bool two = i + stride < total;
        const float4 a = fetch(i), b = fetch(two ? i + stride : i);
        count(a);
        if (two) count(b);
    }
    n_pixels = moments_wave_sum(n_pixels);
    n_counted = moments_wave_sum(n_counted);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&s_cnt[0], n_pixels);
        atomicAdd(&s_cnt[1], n_counted);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < LUMA_BINS; b += LUMA_HIST_BLOCK) {
        uint32_t v = 0u;
#pragma unroll
        for (int k = 0; k < kCopies; ++k) v += s_bins[k][b];
        if (v) atomicAdd(&out->bins[b], (unsigned long long)v);
    }
    if (threadIdx.x == 0 && s_cnt[0]) {
        atomicAdd(&out->n_pixels, (unsigned long long)s_cnt[0]);
        if (s_cnt[1]) atomicAdd(&out->n_counted, (unsigned long long)s_cnt[1]);
    }
}
