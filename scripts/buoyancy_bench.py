#!/usr/bin/env python3
"""Cost of buoyancy (ow_buoyancy / ow_buoyancy_async, kernels k_buoyancy_points + k_buoyancy_bodies) on 1024^2 x 4 cascades.

Cases (bodies x hull points per body): 64 x 64, 1 Ki x 64 and 4 Ki x 256; boxes of 4 x 4 x 4 or 8 x 4 x 8 points, scattered over
[-500, 500]^2 at the water line.  Every physics step advances the maps by one tick and moves every body 0.5 m (and turns it 0.01 rad),
the situation the warm start is for.  Each case runs `--steps` such steps four ways: cold or warm start (OW_BUOYANCY_WARM_START), through
the synchronous form (host arrays: copy in, kernels, results and per-point records out, synchronise; host clock) or the asynchronous one
(device buffers, torch events around the call on the generator's stream).  Prints one JSON line per case and mode: time per call, mean
Newton iterations and evaluations per point, the converged share.  `--mode cold|warm` restricts the run to one start, so that a
`rocprofv3 --kernel-trace --stats` run sees one kind of k_buoyancy_points launch.
    python scripts/buoyancy_bench.py [--steps 20] [--mode both|cold|warm] [--out FILE]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from godotoceanwaves_amd import UPDATE_DELTA, WaveCascadeParameters, WaveGenerator, cascade_preset  # noqa: E402

N, CASCADES = 1024, 4
CASES = [(64, (4, 4, 4)), (1024, (4, 4, 4)), (4096, (8, 4, 8))]


def scene(count, divisions, seed):
    rng = np.random.default_rng(seed)
    bodies = np.zeros(count, WaveGenerator.BUOYANCY_BODY)
    hulls = []
    for i in range(count):
        h = WaveGenerator.box_hull((4.0, 2.0, 8.0), divisions, body=i)
        a = rng.uniform(0, 2 * math.pi)
        c, s = math.cos(a), math.sin(a)
        bodies[i]["transform"][:9] = (c, 0, s, 0, 1, 0, -s, 0, c)   # a heading about y
        bodies[i]["transform"][9:] = (rng.uniform(-500, 500), 0.0, rng.uniform(-500, 500))
        bodies[i]["point_offset"], bodies[i]["point_count"] = len(h) * i, len(h)
        bodies[i]["linear_drag"], bodies[i]["quadratic_drag"] = 0.5, 0.1
        hulls.append(h)
    heading = rng.uniform(0, 2 * math.pi, count)
    step = np.stack([np.cos(heading), np.zeros(count), np.sin(heading)], axis=1).astype(np.float32) * 0.5
    return bodies, np.concatenate(hulls), step


def move(bodies, step):
    bodies["transform"][:, 9:] += step
    t = bodies["transform"][:, :9].reshape(-1, 3, 3).astype(np.float64)
    c, s = math.cos(0.01), math.sin(0.01)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    bodies["transform"][:, :9] = (t @ R).reshape(-1, 9).astype(np.float32)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--mode", choices=("both", "cold", "warm"), default="both")
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
    starts = ("cold", "warm") if a.mode == "both" else (a.mode,)
    lines = []
    for nb, div in CASES:
        for start in starts:
            opts = {"warm_start": True} if start == "warm" else None
            # synchronous form: host arrays; the per-point records come back too (the warm start needs them on the host)
            bodies, hull, step = scene(nb, div, nb)
            pts = np.zeros(len(hull), WaveGenerator.BUOYANCY_POINT)
            sync_s, it, ev, cv = [], [], [], []
            for k in range(a.steps + 1):
                gen.run(UPDATE_DELTA, params, 1)
                gen.sync()
                move(bodies, step)
                t0 = time.perf_counter()
                gen.buoyancy(bodies, hull, sc, opts, points=pts)
                if k > 0:   # the first call is a cold start either way (and grows the scratch)
                    sync_s.append(time.perf_counter() - t0)
                    it.append(pts["iterations"].mean())
                    ev.append(pts["evaluations"].mean())
                    cv.append(pts["converged"].mean())
            # asynchronous form: everything resident on the device, one pose upload per step
            bodies, hull, step = scene(nb, div, nb)
            dev = lambda x: torch.from_numpy(np.frombuffer(x.tobytes(), np.uint8).copy()).to("cuda:0")   # noqa: E731
            bodies_dev, hull_dev = dev(bodies), dev(hull)
            res_dev = torch.zeros(nb * 64, dtype=torch.uint8, device="cuda:0")
            pts_dev = torch.zeros(len(hull) * 64, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            async_ms = []
            for k in range(a.steps + 1):
                gen.run(UPDATE_DELTA, params, 1)
                move(bodies, step)
                host = torch.from_numpy(np.frombuffer(bodies.tobytes(), np.uint8).copy()).pin_memory()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(stream):
                    bodies_dev.copy_(host, non_blocking=True)
                    e0.record(stream)
                    gen.buoyancy_async(bodies_dev, hull_dev, sc, res_dev, pts_dev, opts)
                    e1.record(stream)
                gen.sync()
                e1.synchronize()
                if k > 0:
                    async_ms.append(e0.elapsed_time(e1))
            line = {"map_size": N, "cascades": CASCADES, "bodies": nb, "points_per_body": len(hull) // nb, "points": len(hull), "start": start,
                    "steps": a.steps, "sync_us": round(float(np.median(sync_s)) * 1e6, 1), "async_us": round(float(np.median(async_ms)) * 1e3, 1),
                    "mean_iterations": round(float(np.mean(it)), 3), "mean_evaluations": round(float(np.mean(ev)), 3),
                    "converged": round(float(np.mean(cv)), 5), "bytes_back_sync": nb * 64 + len(hull) * 64, "bytes_back_async_results": nb * 64}
            print(json.dumps(line), flush=True)
            lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
