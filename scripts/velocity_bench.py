#!/usr/bin/env python3
"""Cost of the velocity layers (ow_update_velocity: k_velocity_pass1 + k_velocity_pass2) per map size and layer count, and of the consumers
that read them (ow_query_velocity, ow_buoyancy with OW_BUOYANCY_WATER_VELOCITY) at 1024^2 x 4.

ow_update_velocity: every step runs one update_all tick (all layers stale again), then the refresh, timed by torch events on the generator's
stream around the call alone (device time of the two launch pairs, up to four cascades per pair at 2048^2).  The consumers: host clock per
synchronous call, 64 Ki query points / 1 Ki bodies x 64 hull points, the layers current (only the query kernel runs).  One JSON line per
case.  `--sizes` / `--counts` restrict the sweep (a `rocprofv3 --kernel-trace --stats` run of one shape).
    python scripts/velocity_bench.py [--steps 20] [--sizes 128,256,512,1024,2048] [--counts 1,4,8] [--no-consumers] [--out FILE]"""
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

BYTES_PER_TEXEL = 52  # h0 (8) + omega (4) read, two packed layers written and read back (2 x 2 x 8), RGBA16F out (8)


def make(n, count, stream=None):
    g = WaveGenerator()
    g.map_size = n
    if stream is not None:
        g.stream = stream
    g.init_gpu(max(2, count))
    return g, [WaveCascadeParameters(**cascade_preset(i % 8)) for i in range(count)]


def refresh_case(n, count, steps):
    import torch
    s = torch.cuda.Stream()
    g, p = make(n, count, s.cuda_stream)
    times = []
    with torch.cuda.stream(s):
        for k in range(steps + 2):
            g.update_all(UPDATE_DELTA, p)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            g.update_velocity(range(count))
            b.record(s)
            b.synchronize()
            if k >= 2:
                times.append(a.elapsed_time(b) * 1e3)
    computed, skipped = g.velocity_stats()
    g.free()
    us = float(np.median(times))
    texels = n * n * count
    return {"case": "update_velocity", "n": n, "layers": count, "us_median": round(us, 2), "us_min": round(min(times), 2),
            "us_per_layer": round(us / count, 2), "bytes_per_texel": BYTES_PER_TEXEL,
            "fraction_of_8TBps": round(texels * BYTES_PER_TEXEL / (us * 1e-6) / 8e12, 3), "layers_computed": computed, "layers_skipped": skipped}


def consumer_cases(steps):
    n, count = 1024, 4
    g, p = make(n, count)
    g.run(UPDATE_DELTA, p, 3)
    sc = np.array([(1 / q.tile_length[0], 1 / q.tile_length[1], q.displacement_scale, q.normal_scale) for q in p], np.float32)
    rng = np.random.default_rng(1)
    xz = rng.uniform(-500, 500, (65536, 2)).astype(np.float32)
    g.update_velocity()
    out = []
    for label, fn in (("query_surface", lambda: g.query_surface(xz, sc)), ("query_velocity", lambda: g.query_velocity(xz, sc))):
        fn()
        t = []
        for _ in range(steps):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e6)
        out.append({"case": label, "n": n, "layers": count, "points": len(xz), "us_median": round(float(np.median(t)), 1)})
    bodies = np.zeros(1024, WaveGenerator.BUOYANCY_BODY)
    hulls = []
    for i in range(len(bodies)):
        h = WaveGenerator.box_hull((4.0, 2.0, 8.0), (4, 4, 4), body=i)
        a = rng.uniform(0, 2 * math.pi)
        c, s = math.cos(a), math.sin(a)
        bodies[i]["transform"][:9] = (c, 0, s, 0, 1, 0, -s, 0, c)
        bodies[i]["transform"][9:] = (rng.uniform(-500, 500), 0.0, rng.uniform(-500, 500))
        bodies[i]["point_offset"], bodies[i]["point_count"] = len(h) * i, len(h)
        bodies[i]["linear_drag"], bodies[i]["quadratic_drag"] = 0.5, 0.1
        hulls.append(h)
    hull = np.concatenate(hulls)
    for label, opts in (("buoyancy", None), ("buoyancy_water_velocity", {"water_velocity": True})):
        g.buoyancy(bodies, hull, sc, opts)
        t = []
        for _ in range(steps):
            t0 = time.perf_counter()
            g.buoyancy(bodies, hull, sc, opts)
            t.append((time.perf_counter() - t0) * 1e6)
        out.append({"case": label, "n": n, "layers": count, "bodies": len(bodies), "points": len(hull), "us_median": round(float(np.median(t)), 1)})
    g.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--sizes", default="128,256,512,1024,2048")
    ap.add_argument("--counts", default="1,4,8")
    ap.add_argument("--no-consumers", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for n in (int(v) for v in a.sizes.split(",")):
        for c in (int(v) for v in a.counts.split(",")):
            if n == 2048 and c > 4:
                continue  # 2048^2 x 8: the frame scratch alone is gigabytes; the refresh runs pairs of four anyway
            rows.append(refresh_case(n, c, a.steps))
            print(json.dumps(rows[-1]), flush=True)
    if not a.no_consumers:
        for r in consumer_cases(a.steps):
            rows.append(r)
            print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
