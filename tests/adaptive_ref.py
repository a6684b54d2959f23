"""TEST INFRASTRUCTURE: DESIGN.md section 22 (adaptive sampling, pnrt_render_adaptive)
restated in float32 numpy on top of tests/moments_ref.py: the activity predicate, the
8x8 tiles over (x, local row) and their list, the per-pixel moments update with the
blend weight 1 / (float)n, and the statistics record -- what pt_adaptive.h must
compute, bit for bit."""
from __future__ import annotations

import numpy as np

import moments_ref as R

F = np.float32
U = np.uint32
TILE = 8
SLOT_MAX = (1 << 28) - 1          # path slots of one batch
MAX_CHUNK_FRAMES = 128


def selector_rows(height: int, band: int = 1, n_shards: int = 1, shard: int = 0) -> np.ndarray:
    """The image rows of a shard selector in local-row order (pnrt_pack_rows' order)."""
    y = np.arange(height)
    return y[(y // band) % n_shards == shard]


def active(moments: np.ndarray, threshold: float, min_frames: int) -> np.ndarray:
    """(H, W) bool: n < m || e_c > threshold with m = max(min_frames, 2); an unmeasured
    pixel (e_c = +inf there, n < 2 <= m) is active."""
    m = max(int(min_frames), 2)
    n = R.frames_of(moments)
    return (n < U(min(m, 0xFFFFFFFF))) | (R.error(moments) > F(threshold))


def tile_list(mask_local: np.ndarray) -> list:
    """[(tile index, 64-bit mask)] of the active tiles of a (rows, W) bool array in local-row
    order, increasing tile index; bit p of a mask is pixel (p & 7, p >> 3) of the tile."""
    rows, width = mask_local.shape
    tx_n, ty_n = (width + TILE - 1) // TILE, (rows + TILE - 1) // TILE
    padded = np.zeros((ty_n * TILE, tx_n * TILE), bool)      # beyond the edges: never active
    padded[:rows, :width] = mask_local
    out = []
    for ty in range(ty_n):
        for tx in range(tx_n):
            blk = padded[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE].reshape(-1)
            m = sum(1 << int(p) for p in np.flatnonzero(blk))
            if m:
                out.append((ty * tx_n + tx, m))
    return out


def plan(n_active_tiles: int, n_frames: int, cap_frames: int | None = None):
    """(frames_per_batch, n_batches) of a call: the plan of 64 * n_active_tiles path slots
    per frame (cap_frames: what PNRT_BATCH_BYTES allows, when the context has a cap)."""
    if n_frames == 0 or n_active_tiles == 0:
        return 0, 0
    fit = min(MAX_CHUNK_FRAMES, SLOT_MAX // (64 * n_active_tiles))
    chunk = min(n_frames, fit)
    if cap_frames is not None:
        chunk = max(1, min(chunk, cap_frames))
    return chunk, -(-n_frames // chunk)


def render(accum: np.ndarray, moments: np.ndarray, colors, frame_numbers, threshold: float, min_frames: int,
           band: int = 1, n_shards: int = 1, shard: int = 0, cap_frames: int | None = None):
    """One pnrt_render_adaptive call whose frames have the colour images `colors`:
    -> (accumulation, moments, stats).  The mask is evaluated once, on `moments`; an active
    pixel gets every frame in order (section 21.1's update, then the blend with
    a = 1 / (float)n of its own count after the increment); an inactive pixel keeps both
    records, bit for bit."""
    height, width = moments.shape[:2]
    rows = selector_rows(height, band, n_shards, shard)
    mask = np.zeros((height, width), bool)
    mask[rows] = active(moments, threshold, min_frames)[rows]
    tiles = tile_list(mask[rows]) if len(rows) else []
    fpb, nb = plan(len(tiles), len(frame_numbers), cap_frames)
    stats = {"n_pixels": int(len(rows) * width), "n_active_pixels": int(mask.sum()),
             "n_tiles": ((width + TILE - 1) // TILE) * ((len(rows) + TILE - 1) // TILE), "n_active_tiles": len(tiles),
             "frames_per_batch": fpb, "n_batches": nb}
    assert stats["n_active_pixels"] == sum(bin(m).count("1") for _, m in tiles)
    acc, mom = np.array(accum, F), np.array(moments, F)
    if not tiles:
        return acc, mom, stats
    new_acc, new_mom = acc.copy(), mom.copy()
    for c, f in zip(colors, frame_numbers):
        c = np.asarray(c, F)
        new_mom = R.update(new_mom, [c], [f])
        a = (F(1) / R.frames_of(new_mom).astype(F)).astype(F)[..., None]
        new_acc[..., :3] = ((new_acc[..., :3] * (F(1) - a).astype(F)).astype(F) + (c[..., :3] * a).astype(F)).astype(F)
        new_acc[..., 3] = 1
    acc[mask] = new_acc[mask]
    mom[mask] = new_mom[mask]
    return acc, mom, stats
