// pnraytracing_amd/csrc/pt_moments.h -- per-pixel sample moments of the frames'
// luminance and the convergence measure read from them (pnrt_enable_moments,
// pnrt_read_error, pnrt_convergence; not in the reference, which shows the
// accumulation image and counts frames: main.cpp:613-628).  Defined bit for bit
// in DESIGN.md section 21; tests/moments_ref.py restates it in numpy.
//
// The moments image: one float4 per pixel, row 0 = bottom,
//   x = mean of the frames' luminance Y      y = M2, the sum of squared deviations
//   z = 0 (reserved)                         w = n, the frames folded in (uint32 bits)
// updated per frame, in frame order, by Welford's recurrence.
#pragma once
#include "pt_passes.h"

// Rec. 709 luminance of a frame's colour, every operation rounded (no contraction)
PN_DEV float moments_luma(float4 c) { return ((0.2126f * c.x) + (0.7152f * c.y)) + (0.0722f * c.z); }

// The clamped relative standard error of a pixel with n >= 2 frames:
// sqrt(var / n) / max(mean, 1/256), at most 65535 (the comparison also catches NaN).
PN_DEV float moments_error(float mean, float m2, uint32_t n) {
    const float var = m2 / (float)(n - 1u);
    const float sem = sqrtf(var / (float)n);
    const float e = sem / fmaxf(mean, 1.0f / 256.0f);
    return (e <= 65535.0f) ? e : 65535.0f;
}

// pt_blend_kernel (pt_passes.h) with the moments update in the same pass over the
// colour buffer: the blend arithmetic is that kernel's, operation for operation, so
// the accumulation image is bit-identical; the moment state stays in registers over
// the batch's frames (one record read and one record write per pixel).
__global__ void pt_blend_moments_kernel(FrameParams fp, const float4* colors, float4* accum, float4* moments,
                                        int chunk_frames, uint32_t first_frame) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= fp.rows * fp.width) return;
    int lr = i / fp.width, px = i - lr * fp.width;
    int py = shard_row(lr, fp.band, fp.n_shards, fp.shard);
    size_t pix = (size_t)py * fp.width + px;
    float4 acc = accum[pix];
    const float4 m = moments[pix];
    float mean = m.x, m2 = m.y;
    uint32_t n = __float_as_uint(m.w);
    for (int k = 0; k < chunk_frames; ++k) {
        float4 c = colors[((size_t)k * fp.rows + lr) * fp.width + px];
        const uint32_t frame = first_frame + (uint32_t)k;
        float a = 1.0f / (float)(frame + 1u);
        acc.x = mixf(acc.x, c.x, a);
        acc.y = mixf(acc.y, c.y, a);
        acc.z = mixf(acc.z, c.z, a);
        acc.w = 1.0f;
        const float y = moments_luma(c);
        if (frame == 0u) { n = 0u; mean = 0.0f; m2 = 0.0f; }   // frame 0 overwrites the accumulation (a = 1)
        n += (n != 0xFFFFFFFFu) ? 1u : 0u;
        const float d = y - mean;
        mean = mean + d * (1.0f / (float)n);
        m2 = m2 + d * (y - mean);
    }
    accum[pix] = acc;
    moments[pix] = make_float4(mean, m2, 0.0f, __uint_as_float(n));
}

// e_c of every pixel of the image; +inf where fewer than two frames were folded in
__global__ void __launch_bounds__(256) pt_moments_error_kernel(const float4* moments, float* err, uint32_t npix) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const float4 m = moments[i];
    const uint32_t n = __float_as_uint(m.w);
    err[i] = n < 2u ? __uint_as_float(0x7f800000u) : moments_error(m.x, m.y, n);
}

// The device record of one pnrt_convergence call (the host writes the identities
// before the launch: zeros, and 0xFFFFFFFF for the minimum).  Every field is an
// integer combined by an order-independent atomic (sum, max, min), so the
// statistics are the same bits whatever order the blocks arrive in.
struct MomentsStats {
    unsigned long long n_pixels, n_measured, n_above, sum_q16;
    uint32_t max_error_bits;    // e_c >= 0: its bits order as unsigned
    uint32_t min_frames, max_frames;
    uint32_t reserved;
};

#define MOMENTS_REDUCE_BLOCK 256

template <class T>
PN_DEV T moments_wave_sum(T v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
PN_DEV uint32_t moments_wave_max(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t w = (uint32_t)__shfl_xor((int)v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}

// Statistics over the rows of a shard selector: lanes accumulate privately over a
// grid-stride loop, waves combine with cross-lane moves, the block's waves through
// LDS, and one lane issues the block's atomics.
__global__ void __launch_bounds__(MOMENTS_REDUCE_BLOCK)
pt_moments_reduce_kernel(const float4* moments, MomentsStats* out, int width, int rows, int band, int n_shards, int shard,
                         float threshold) {
    const size_t total = (size_t)rows * width;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    unsigned long long n_pixels = 0, n_measured = 0, n_above = 0, sum_q16 = 0;
    uint32_t max_bits = 0, min_frames = 0xFFFFFFFFu, max_frames = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int r = (int)(i / width), x = (int)(i - (size_t)r * width);
        const int y = shard_row(r, band, n_shards, shard);
        const float4 m = moments[(size_t)y * width + x];
        const uint32_t n = __float_as_uint(m.w);
        n_pixels += 1;
        min_frames = n < min_frames ? n : min_frames;
        max_frames = n > max_frames ? n : max_frames;
        if (n >= 2u) {
            const float e = moments_error(m.x, m.y, n);
            const uint32_t eb = __float_as_uint(e);
            n_measured += 1;
            n_above += e > threshold ? 1 : 0;
            sum_q16 += (unsigned long long)(uint32_t)(e * 65536.0f);
            max_bits = eb > max_bits ? eb : max_bits;
        }
    }
    n_pixels = moments_wave_sum(n_pixels);
    n_measured = moments_wave_sum(n_measured);
    n_above = moments_wave_sum(n_above);
    sum_q16 = moments_wave_sum(sum_q16);
    max_bits = moments_wave_max(max_bits);
    min_frames = ~moments_wave_max(~min_frames);
    max_frames = moments_wave_max(max_frames);

    constexpr int kWaves = MOMENTS_REDUCE_BLOCK / 64;
    __shared__ unsigned long long s_sum[kWaves][4];
    __shared__ uint32_t s_max[kWaves][3];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
        s_sum[wave][0] = n_pixels; s_sum[wave][1] = n_measured; s_sum[wave][2] = n_above; s_sum[wave][3] = sum_q16;
        s_max[wave][0] = max_bits; s_max[wave][1] = min_frames; s_max[wave][2] = max_frames;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < kWaves; ++w) {
        n_pixels += s_sum[w][0]; n_measured += s_sum[w][1]; n_above += s_sum[w][2]; sum_q16 += s_sum[w][3];
        max_bits = s_max[w][0] > max_bits ? s_max[w][0] : max_bits;
        min_frames = s_max[w][1] < min_frames ? s_max[w][1] : min_frames;
        max_frames = s_max[w][2] > max_frames ? s_max[w][2] : max_frames;
    }
    if (n_pixels == 0) return;             // (a block past the end of the rows)
    atomicAdd(&out->n_pixels, n_pixels);
    atomicAdd(&out->n_measured, n_measured);
    atomicAdd(&out->n_above, n_above);
    atomicAdd(&out->sum_q16, sum_q16);
    atomicMax(&out->max_error_bits, max_bits);
    atomicMin(&out->min_frames, min_frames);
    atomicMax(&out->max_frames, max_frames);
}
