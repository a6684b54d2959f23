"""Generate tests/golden/shader_fixtures.json + shader_samples.npz: what the
reference's OWN shader text computes (run where the reference tree is present;
tests only read the outputs).

oracle/_ref/shader_driver is shaders/ray_tracing.comp translated to C++ by
oracle/shader/translate.py and compiled against oracle/shader/glsl_shim.hpp
(oracle/shader/Makefile).  For every case of tests/shader_pin.py this records
  * functions: the sha256 of the input words and of the driver's output words
    (NaNs canonical), and the first SAMPLE output records in full,
  * images: the sha256 of the driver's RGBA32F accumulation image; the image
    itself (RGB; alpha is 1 everywhere) for the cases the GPU test compares
    against, every fourth row for the others.
Recorded results only: numbers, no program text.

Usage:  python tests/golden/make_shader_golden.py
"""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import shader_pin as SP  # noqa: E402


def main():
    if not os.path.exists(SP.DRIVER):
        subprocess.run(["make", "-C", os.path.join(REPO, "oracle", "shader")], check=True)
    fixtures = {"seed": SP.SEED, "sample": SP.SAMPLE, "functions": {}, "images": {}}
    samples = {}
    cfgs = SP.fn_scenes()
    blobs = {k: SP.scene_blob(c) for k, c in cfgs.items()}
    for name, (fn, key, words) in SP.fn_cases(cfgs).items():
        out = SP.canonical(fn, SP.driver_fn(cfgs[key], fn, words, blob=blobs[key]))
        fixtures["functions"][name] = {"fn": fn, "scene": key, "n": len(words), "words": int(out.size),
                                       "in_sha256": SP.sha(words), "out_sha256": SP.sha(out)}
        samples[f"fn/{name}"] = out[:SP.SAMPLE]
        print(f"{name:40s} {out.size:8d} words", flush=True)
    for name, (build, gpu) in SP.image_cases().items():
        cfg, first, n = build()
        img = SP.driver_image(cfg, first, n)
        assert np.all(img[..., 3] == 1.0), name
        w = SP.canonical(-1, img.view(np.uint32).reshape(-1, 4))
        fixtures["images"][name] = {"width": cfg.width, "height": cfg.height, "depth": cfg.max_depth, "first": first,
                                    "frames": n, "words": int(w.size), "sha256": SP.sha(w), "full": bool(gpu)}
        samples[f"img/{name}"] = img[..., :3] if gpu else img[::4, :, :3]
        print(f"{name:40s} {cfg.width}x{cfg.height} depth {cfg.max_depth} frames {first}+{n} mean {img[..., :3].mean():.5f}",
              flush=True)
    json.dump(fixtures, open(os.path.join(HERE, "shader_fixtures.json"), "w"), indent=1)
    np.savez_compressed(os.path.join(HERE, "shader_samples.npz"), **samples)
    print("wrote shader_fixtures.json, shader_samples.npz")


if __name__ == "__main__":
    main()
