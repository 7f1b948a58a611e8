#!/usr/bin/env python3
"""Cost of camera views (ow_render_view / ow_render_view_async, kernels k_height_bound + k_render_view) on 1024^2 x 4 cascades, against the
ray cast on the very same pixel rays (ow_raycast_surface_async, k_raycast_surface: one wave per ray).

Image sizes 320 x 200, 1280 x 720 and 1920 x 1080; the reference scene's camera (main.tscn:120, fov 75, far 4000), the default options with
the distance falloff around the camera; after 10 ticks.  Each size runs a warm-up and `--steps` enqueues of the render (RGBA8 only, and RGBA8
plus records) and of the ray cast over the image's pixel rays (formed on the host from the documented formula), timed with torch events on
the generator's stream.  Prints one JSON line per size and form: time per call, ns per pixel, the hit / truncated shares, and whether the
render's t equals the ray cast's.  Kernel times come from a `rocprofv3 --kernel-trace --stats` run of this script.
    python scripts/render_bench.py [--steps 5] [--sizes 320x200,1280x720,1920x1080] [--out FILE]"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from godotoceanwaves_amd import UPDATE_DELTA, WaveCascadeParameters, WaveGenerator, _lib, cascade_preset  # noqa: E402

N, CASCADES = 1024, 4
POSITION = (0.0, 10.0, -25.0)
BASIS = (-0.996195, -0.0151344, 0.0858316, 0.0, 0.984807, 0.173648, -0.0871557, 0.172987, -0.981061)
FOV, FAR = 75.0, 4000.0


def pixel_rays(width, height):
    """the rays of include/ocean_waves.h ow_render_view's formula in FP32 (the kernel's own differ by rounding only)"""
    B = np.asarray(BASIS, np.float32).reshape(3, 3)
    th = np.float32(math.tan(math.radians(FOV) / 2))
    aspect = np.float32(width) / np.float32(height)
    i = np.arange(width, dtype=np.float32)[None, :]
    j = np.arange(height, dtype=np.float32)[:, None]
    x = ((2 * (i + np.float32(0.5))) / np.float32(width) - 1) * aspect * th + 0 * j
    y = (1 - (2 * (j + np.float32(0.5))) / np.float32(height)) * th + 0 * i
    d = np.stack([x, y, -np.ones_like(x)], axis=-1).reshape(-1, 3) @ B.T
    return WaveGenerator.rays(np.broadcast_to(np.float32(POSITION), d.shape), d, FAR)


def timed(stream, steps, fn):
    import torch
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        e0.record(stream)
        for _ in range(steps):
            fn()
        e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / steps * 1e3


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--sizes", default="320x200,1280x720,1920x1080")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    stream = torch.cuda.Stream()
    gen = WaveGenerator()
    gen.map_size = N
    gen.stream = stream.cuda_stream
    gen.init_gpu(CASCADES)
    params = [WaveCascadeParameters(**cascade_preset(i)) for i in range(CASCADES)]
    gen.run(UPDATE_DELTA, params, 10)
    gen.sync()
    sc = np.array([(1 / p.tile_length[0], 1 / p.tile_length[1], p.displacement_scale, p.normal_scale) for p in params], np.float32)
    opts = {"falloff": True}
    ray_opts = {"falloff_center": (POSITION[0], POSITION[2])}
    lines = []
    for size in a.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        cam = WaveGenerator.camera(POSITION, BASIS, FOV, w, h, FAR)
        count = w * h
        rgba_dev = torch.zeros((count, 4), dtype=torch.uint8, device="cuda:0")
        rec_dev = torch.zeros((count, WaveGenerator.RENDER_PIXEL.itemsize), dtype=torch.uint8, device="cuda:0")
        rays = pixel_rays(w, h)
        rays_dev = torch.from_numpy(rays.view(np.uint8).copy()).to("cuda:0")
        hits_dev = torch.zeros((count, WaveGenerator.RAYCAST_HIT.itemsize), dtype=torch.uint8, device="cuda:0")
        us = {"render_rgba": timed(stream, a.steps, lambda: gen.render_view_async(cam, sc, rgba_dev, None, opts)),
              "render_rgba_records": timed(stream, a.steps, lambda: gen.render_view_async(cam, sc, rgba_dev, rec_dev, opts)),
              "raycast": timed(stream, a.steps, lambda: gen.raycast_surface_async(rays_dev, sc, hits_dev, ray_opts))}
        rec = np.frombuffer(rec_dev.cpu().numpy().tobytes(), WaveGenerator.RENDER_PIXEL)
        hits = np.frombuffer(hits_dev.cpu().numpy().tobytes(), WaveGenerator.RAYCAST_HIT)
        st = rec["status"]
        stats = {"size": size, "pixels": count, "hit_share": float(((st & _lib.OW_RAY_HIT) != 0).mean()),
                 "truncated_share": float(((st & _lib.OW_RAY_TRUNCATED) != 0).mean()),
                 "raycast_samples_per_ray": float(hits["samples"].mean()), "raycast_rounds_per_ray": float(hits["rounds"].mean()),
                 "slab_half_height": float(hits["slab_half_height"][0]), "status_equals_raycast": bool((st == hits["status"]).mean() > 0.999),
                 "t_within_1e-3_of_raycast": float((np.abs(rec["t"] - hits["t"]) <= 1e-3).mean())}
        for form, t in us.items():
            line = dict(stats, form=form, us_per_call=round(t, 1), ns_per_pixel=round(t * 1e3 / count, 1))
            lines.append(line)
            print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
