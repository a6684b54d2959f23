// pnraytracing_amd/csrc/pt_adaptive.h -- adaptive sampling (pnrt_render_adaptive; not
// in the reference, which renders every pixel every frame: main.cpp:612-613): a call
// renders only the pixels whose relative standard error (pt_moments.h) is still above
// a threshold.  Defined bit for bit in DESIGN.md section 22; tests/adaptive_ref.py
// restates it in numpy.
//
//   mask     one wave per 8x8 tile of (x, local row): the lanes' predicates, balloted
//   scan     exclusive scan of the tiles' "any pixel active" flags (pt_bvh.h bvh_scan_kernel)
//   scatter  the active-tile list {tile, mask}, in increasing tile order
//   gen / shade   pt_wf.h's kernels, instantiated with the slot -> pixel mapping through
//            the list (WfAdapt); the trace kernel sees path entries only
//   blend    one lane per (list entry, pixel): the moments update of section 21 and the
//            progressive mean with the pixel's own frame count
#pragma once
#include "pt_moments.h"
#include "pt_wf.h"

// what the host reads back after the mask step (zeroed before it)
struct AdaptCounts {
    unsigned long long n_active_pixels;
    uint32_t n_active_tiles, reserved;
};

#define ADAPT_MASK_BLOCK 256      // 4 waves = 4 tiles per block

// A pixel is active iff n < m || e_c > threshold (m >= 2: an unmeasured pixel is
// active and moments_error is never asked about n < 2); pixels beyond the frame's
// right edge or the selector's last row never are.
__global__ void __launch_bounds__(ADAPT_MASK_BLOCK)
pt_adaptive_mask_kernel(const float4* moments, int width, int rows, int band, int n_shards, int shard, int tiles_x,
                        uint32_t n_tiles, float threshold, uint32_t m, unsigned long long* masks, int* flags) {
    const uint32_t tile = blockIdx.x * (ADAPT_MASK_BLOCK / 64) + (threadIdx.x >> 6);     // wave-uniform
    if (tile >= n_tiles) return;
    const int p = threadIdx.x & 63;
    const int ty = (int)(tile / (uint32_t)tiles_x), tx = (int)(tile - (uint32_t)ty * tiles_x);
    const int x = tx * 8 + (p & 7), lr = ty * 8 + (p >> 3);
    bool active = false;
    if (x < width && lr < rows) {
        const int y = shard_row(lr, band, n_shards, shard);
        const float4 r = moments[(size_t)y * width + x];
        const uint32_t n = __float_as_uint(r.w);
        active = n < m || moments_error(r.x, r.y, n) > threshold;
    }
    const unsigned long long mask = __ballot(active);
    if (p == 0) {
        masks[tile] = mask;
        flags[tile] = mask != 0ull ? 1 : 0;
    }
}

// entry offs[t] of the list for every active tile t (offs: the exclusive scan of flags,
// so the list is in increasing tile order whatever order the blocks run in)
__global__ void __launch_bounds__(256)
pt_adaptive_scatter_kernel(const unsigned long long* masks, const int* flags, const int* offs, uint32_t n_tiles, WfTile* list,
                           AdaptCounts* counts) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t pixels = 0;
    if (t < n_tiles) {
        if (flags[t]) {
            WfTile e;
            e.tile = t; e.pad = 0u; e.mask = masks[t];
            list[offs[t]] = e;                  // offs[t] < the number of flagged tiles <= n_tiles: the list's capacity
            pixels = (uint32_t)__popcll(e.mask);
        }
        if (t == n_tiles - 1) counts->n_active_tiles = (uint32_t)(offs[t] + flags[t]);      // the scan's total
    }
    // the active pixels: one integer atomic per wave of 64 tiles (one per active tile from
    // the mask kernel -- 16 196 on one address for a half-active 1080p frame -- made the
    // mask step 0.275 ms instead of 0.092 ms)
    pixels = moments_wave_sum(pixels);
    if ((threadIdx.x & 63) == 0 && pixels != 0u) atomicAdd(&counts->n_active_pixels, (unsigned long long)pixels);
}

// ---- the wavefront kernels over an adaptive batch's slots: pt_wf.h's, instantiated
// with the list as their trailing argument -- pt_wf_gen_setup<WfAdapt> and
// pt_wf_shade_setup<FINAL, WfAdapt> (timed as PNRT_K_GEN / PNRT_K_SHADE)

// ---- blend: section 21.1's moments update, and the progressive mean with the weight
// 1 / (float)n of the pixel's own count after the increment (pt_blend_kernel's mixf
// otherwise).  One lane per (list entry, pixel of the tile); the pixel's records stay
// in registers over the batch's frames.
__global__ void __launch_bounds__(256)
pt_blend_adaptive_kernel(FrameParams fp, WfAdapt ad, int tiles_x, const float4* colors, float4* accum, float4* moments,
                         int chunk_frames, uint32_t first_frame) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t a = i >> 6;
    const int p = (int)(i & 63u);
    if (a >= ad.n_tiles) return;
    const WfTile e = ad.tiles[a];
    if (!((e.mask >> p) & 1ull)) return;
    const int ty = (int)(e.tile / (uint32_t)tiles_x), tx = (int)(e.tile - (uint32_t)ty * tiles_x);
    const int px = tx * 8 + (p & 7), lr = ty * 8 + (p >> 3);
    if (px >= fp.width || lr >= fp.rows) return;             // (never active: the mask kernel's rule)
    const int py = shard_row(lr, fp.band, fp.n_shards, fp.shard);
    const size_t pix = (size_t)py * fp.width + px;
    float4 acc = accum[pix];
    const float4 m = moments[pix];
    float mean = m.x, m2 = m.y;
    uint32_t n = __float_as_uint(m.w);
    for (int k = 0; k < chunk_frames; ++k) {
        const float4 c = colors[((size_t)a * chunk_frames + k) * 64 + p];
        const uint32_t frame = first_frame + (uint32_t)k;
        const float y = moments_luma(c);
        if (frame == 0u) { n = 0u; mean = 0.0f; m2 = 0.0f; }
        n += (n != 0xFFFFFFFFu) ? 1u : 0u;
        const float w = 1.0f / (float)n;
        acc.x = mixf(acc.x, c.x, w);
        acc.y = mixf(acc.y, c.y, w);
        acc.z = mixf(acc.z, c.z, w);
        acc.w = 1.0f;
        const float d = y - mean;
        mean = mean + d * w;
        m2 = m2 + d * (y - mean);
    }
    accum[pix] = acc;
    moments[pix] = make_float4(mean, m2, 0.0f, __uint_as_float(n));
}
