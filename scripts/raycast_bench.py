#!/usr/bin/env python3
"""Cost of ray casts (ow_raycast_surface / ow_raycast_surface_async, kernels k_height_bound + k_raycast_surface) on 1024^2 x 4 cascades.

Ray counts 1, 64, 4 Ki and 64 Ki; three families of camera rays over [-500, 500]^2: steep (from 20 m, 30-80 degrees down), grazing (from
2 m, 1-5 degrees down) and high (from 300 m, 10-80 degrees down), default options.  Each case runs `--steps` calls through the synchronous
form (host arrays: copy in, both kernels, records out, synchronise; host clock) and the asynchronous one (device buffers, torch events
around the call on the generator's stream).  Prints one JSON line per case and form: time per call, the rounds and samples per ray, the hit,
truncated and converged shares.  Kernel times come from a `rocprofv3 --kernel-trace --stats` run of this script.
    python scripts/raycast_bench.py [--steps 10] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from godotoceanwaves_amd import UPDATE_DELTA, WaveCascadeParameters, WaveGenerator, _lib, cascade_preset  # noqa: E402

N, CASCADES = 1024, 4
COUNTS = (1, 64, 4096, 65536)
FAMILIES = {"steep": (20.0, 20.0, 30.0, 80.0), "grazing": (2.0, 2.0, 1.0, 5.0), "high": (300.0, 300.0, 10.0, 80.0)}


def rays(family, count, seed):
    hlo, hhi, alo, ahi = FAMILIES[family]
    rng = np.random.default_rng(seed)
    a = np.radians(rng.uniform(alo, ahi, count))
    az = rng.uniform(0, 2 * np.pi, count)
    o = np.stack([rng.uniform(-500, 500, count), rng.uniform(hlo, hhi, count), rng.uniform(-500, 500, count)], axis=1)
    return WaveGenerator.rays(o, np.stack([np.cos(a) * np.cos(az), -np.sin(a), np.cos(a) * np.sin(az)], axis=1), 5000.0)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
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
    lines = []
    for family in FAMILIES:
        for count in COUNTS:
            r = rays(family, count, seed=count)
            out = gen.raycast_surface(r, sc)   # warm-up, and the statistics
            st = out["status"]
            stats = {"family": family, "rays": count, "rounds_per_ray": float(out["rounds"].mean()), "samples_per_ray": float(out["samples"].mean()),
                     "hit_share": float(((st & _lib.OW_RAY_HIT) != 0).mean()), "truncated_share": float(((st & _lib.OW_RAY_TRUNCATED) != 0).mean()),
                     "converged_share_of_hits": float(out["query"]["converged"][(st & _lib.OW_RAY_HIT) != 0].mean()) if (st & 1).any() else 0.0,
                     "slab_half_height": float(out["slab_half_height"][0])}
            t0 = time.perf_counter()
            for _ in range(a.steps):
                gen.raycast_surface(r, sc)
            sync_us = (time.perf_counter() - t0) / a.steps * 1e6
            rays_dev = torch.from_numpy(r.view(np.uint8).copy()).to("cuda:0")
            out_dev = torch.zeros((count, WaveGenerator.RAYCAST_HIT.itemsize), dtype=torch.uint8, device="cuda:0")
            gen.raycast_surface_async(rays_dev, sc, out_dev)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                e0.record(stream)
                for _ in range(a.steps):
                    gen.raycast_surface_async(rays_dev, sc, out_dev)
                e1.record(stream)
            e1.synchronize()
            async_us = e0.elapsed_time(e1) / a.steps * 1e3
            same = np.frombuffer(out_dev.cpu().numpy().tobytes(), WaveGenerator.RAYCAST_HIT).tobytes() == out.tobytes()
            for form, us in (("sync", sync_us), ("async", async_us)):
                line = dict(stats, form=form, us_per_call=round(us, 1))
                if form == "async":
                    line["equals_sync"] = same
                lines.append(line)
                print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
