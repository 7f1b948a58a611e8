#!/usr/bin/env python3
"""Cost of the water-height query (ow_query_surface / ow_query_surface_async, kernel k_query_surface) on 1024^2 x 4 cascades.

Cases: 4 Ki, 64 Ki and 1 Mi points, uniformly random in [-500, 500]^2 or spatially coherent (a square grid in row order over the same
square: 64 x 64, 256 x 256, 1024 x 1024), each through the synchronous form (host arrays: copy in, kernel, copy out, synchronise) and the
asynchronous one (device buffers, torch events around `--reps` back-to-back calls).  Prints one JSON line per case: time per call, queries/s,
mean Newton iterations and evaluations of F, the converged share, and the bytes a query reads as its evaluation count implies.  Run it
under `rocprofv3 --kernel-trace --stats` for the kernel's own time (k_query_surface in the stats file).
    python scripts/query_bench.py [--reps 20] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from godotoceanwaves_amd import UPDATE_DELTA, WaveCascadeParameters, WaveGenerator, cascade_preset  # noqa: E402

N, CASCADES = 1024, 4
TAP_BYTES = 32            # one bilinear tap: two 16-byte row loads (four RGBA16F texels)
SAMPLE_TAPS = 1 + 1 + 4   # the record's sample at p, per cascade: displacement, normal, and the bicubic filter's four taps of the normal map


def points(count, coherent):
    if coherent:
        side = int(round(count ** 0.5))
        g = (np.arange(side) + 0.5) * (1000.0 / side) - 500.0
        X, Z = np.meshgrid(g, g)
        return np.stack([X.ravel(), Z.ravel()], axis=1).astype(np.float32)
    return np.random.default_rng(count).uniform(-500, 500, (count, 2)).astype(np.float32)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    stream = torch.cuda.Stream()   # the generator enqueues on this stream (ow_config.stream), so that events on it bracket the async calls
    gen = WaveGenerator()
    gen.map_size = N
    gen.stream = stream.cuda_stream
    gen.init_gpu(CASCADES)
    params = [WaveCascadeParameters(**cascade_preset(i)) for i in range(CASCADES)]
    gen.run(UPDATE_DELTA, params, 10)
    gen.sync()
    sc = np.array([(1 / p.tile_length[0], 1 / p.tile_length[1], p.displacement_scale, p.normal_scale) for p in params], np.float32)
    lines = []
    for count in (4096, 65536, 1 << 20):
        for coherent in (False, True):
            xz = points(count, coherent)
            rec = gen.query_surface(xz, sc)   # warm-up, grows the scratch; also the statistics
            t0 = time.perf_counter()
            for _ in range(a.reps):
                gen.query_surface(xz, sc)
            sync_s = (time.perf_counter() - t0) / a.reps
            xz_dev = torch.from_numpy(xz).to("cuda:0")
            out_dev = torch.empty((count, WaveGenerator.SURFACE_QUERY.itemsize), dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            gen.query_surface_async(xz_dev, sc, out_dev)
            gen.sync()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.reps):
                gen.query_surface_async(xz_dev, sc, out_dev)
            e1.record(stream)
            gen.sync()
            e1.synchronize()
            async_s = e0.elapsed_time(e1) * 1e-3 / a.reps
            same = np.frombuffer(out_dev.cpu().numpy().tobytes(), WaveGenerator.SURFACE_QUERY).tobytes() == rec.tobytes()
            evals = float(rec["evaluations"].mean())
            read_bytes = (evals * CASCADES + SAMPLE_TAPS * CASCADES) * TAP_BYTES + 8
            line = {"map_size": N, "cascades": CASCADES, "points": count, "layout": "grid" if coherent else "random",
                    "sync_us": round(sync_s * 1e6, 1), "async_us": round(async_s * 1e6, 1),
                    "sync_queries_per_s": round(count / sync_s), "async_queries_per_s": round(count / async_s),
                    "mean_iterations": round(float(rec["iterations"].mean()), 3), "mean_evaluations": round(evals, 3),
                    "converged": round(float(rec["converged"].mean()), 5), "bytes_read_per_query": round(read_bytes, 1),
                    "bytes_written_per_query": WaveGenerator.SURFACE_QUERY.itemsize,
                    "async_read_GBps": round(count * read_bytes / async_s * 1e-9, 1), "async_equals_sync": same}
            print(json.dumps(line), flush=True)
            lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
