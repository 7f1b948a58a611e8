"""Developer tool (not part of bench.py): what one frame of 4 substeps of a floating-body set costs on 1024^2 x 4 maps, three ways:
  (a) host loop   the way examples/buoyancy_host.c does it: per substep upload the pose records, ow_buoyancy_async, ow_sync, read the results
                  back, integrate on the CPU (NumPy, vectorised over the bodies)
  (b) split       ow_bodies_step with OW_FLAG_BODIES_SPLIT: per substep one lane per hull point, then one wave per body
  (c) fused       ow_bodies_step with OW_FLAG_BODIES_FUSED: one wave per body, the four substeps in one launch
for body counts 1 .. 16384 and hulls of 16 .. 4096 points (sets of more than --max-points hull points are skipped).  The maps stand still
while a case is timed.  Per case: --warmup frames, then --regions regions of --frames frames, each region closed by one synchronisation
(the host loop synchronises every substep by construction); the median region is reported with the fastest and slowest (the spread).
(a) is the baseline of every claim, taken in the same process on the same device.

    python scripts/bench_bodies.py [--out profiles/bodies_step.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from godotoceanwaves_amd import WaveCascadeParameters  # noqa: E402
from godotoceanwaves_amd.presets import UPDATE_DELTA, cascade_preset  # noqa: E402
from godotoceanwaves_amd.wave_generator import WaveGenerator as W  # noqa: E402

SUBSTEPS, DT = 4, 1.0 / 240.0
OPTS = {"warm_start": True}


def scene(num_bodies, points, seed=0):
    rng = np.random.default_rng(seed)
    st = np.zeros(num_bodies, W.RIGID_BODY)
    size = (2.0, 1.0, 2.0)
    mass, iinv = W.box_mass_properties(size, 512.5)
    st["position"] = np.stack([rng.uniform(-400, 400, num_bodies), rng.uniform(-0.3, 0.3, num_bodies), rng.uniform(-400, 400, num_bodies)], axis=1)
    st["orientation"][:, 3] = 1.0
    st["mass"], st["inverse_inertia"] = mass, iinv
    st["linear_drag"], st["quadratic_drag"] = 3.0, 0.5
    st["point_offset"], st["point_count"] = np.arange(num_bodies) * points, points
    hull = np.zeros(num_bodies * points, W.HULL_POINT)
    one = rng.uniform(-0.5, 0.5, (points, 3)) * size
    hull["local"] = np.tile(one, (num_bodies, 1))
    hull["volume"] = np.prod(size) / points
    hull["half_height"] = 0.5 * (np.prod(size) / points) ** (1 / 3)
    hull["body"] = np.repeat(np.arange(num_bodies), points)
    return st, hull


def generator(kernels):
    gen = W()
    gen.map_size = 1024
    gen.bodies_kernels = kernels
    gen.init_gpu(4)
    params = [WaveCascadeParameters(**cascade_preset(ci)) for ci in range(4)]
    gen.run(UPDATE_DELTA, params, 3)
    gen.sync()
    sc = np.array([(1 / p.tile_length[0], 1 / p.tile_length[1], p.displacement_scale, p.normal_scale) for p in params], np.float32)
    return gen, sc


def regions(frame, sync, warmup, count, frames):
    for _ in range(warmup):
        frame()
    sync()
    out = []
    for _ in range(count):
        t0 = time.perf_counter()
        for _ in range(frames):
            frame()
        sync()
        out.append((time.perf_counter() - t0) / frames * 1e6)
    return np.median(out), min(out), max(out)


def device_step(gen, sc, st, hull, args):
    s = gen.bodies_create(st, hull)
    r = regions(lambda: gen.bodies_step(s, sc, SUBSTEPS, DT, OPTS), gen.sync, args.warmup, args.regions, args.frames)
    gen.bodies_destroy(s)
    return r


def host_loop(gen, sc, st, hull, args):
    import torch
    state = st.copy()
    records = np.zeros(len(st), W.BUOYANCY_BODY)
    records["point_offset"], records["point_count"] = st["point_offset"], st["point_count"]
    records["linear_drag"], records["quadratic_drag"] = st["linear_drag"], st["quadratic_drag"]
    dev = lambda x: torch.from_numpy(np.frombuffer(x.tobytes(), np.uint8).copy()).to("cuda:0")   # noqa: E731
    hull_dev, rec_dev = dev(hull), dev(records)
    res_dev = torch.zeros(len(st) * 64, dtype=torch.uint8, device="cuda:0")
    pts_dev = torch.zeros(len(hull) * 64, dtype=torch.uint8, device="cuda:0")
    g = float(np.float32(9.81))

    def frame():
        for _ in range(SUBSTEPS):
            x, y, z, w = state["orientation"].T
            R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                          2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1)
            records["transform"][:, :9], records["transform"][:, 9:] = R, state["position"]
            records["linear_velocity"], records["angular_velocity"] = state["linear_velocity"], state["angular_velocity"]
            rec_dev.copy_(torch.from_numpy(records.view(np.uint8).reshape(-1)))
            gen.buoyancy_async(rec_dev, hull_dev, sc, res_dev, pts_dev, OPTS)
            gen.sync()
            res = res_dev.cpu().numpy().view(W.BUOYANCY_RESULT)
            Rm = R.reshape(-1, 3, 3)
            a = (res["force"] + state["applied_force"]) / state["mass"][:, None]
            a[:, 1] -= g
            state["linear_velocity"] += DT * a
            tau = res["torque"] + state["applied_torque"]
            b = np.einsum("nij,ni->nj", Rm, tau) * state["inverse_inertia"]
            state["angular_velocity"] += DT * np.einsum("nij,nj->ni", Rm, b)
            state["position"] += DT * state["linear_velocity"]
            wx, wy, wz = state["angular_velocity"].T
            dq = np.stack([wx * w + wy * z - wz * y, wy * w + wz * x - wx * z, wz * w + wx * y - wy * x, -(wx * x + wy * y + wz * z)], axis=1)
            q = state["orientation"] + 0.5 * DT * dq
            state["orientation"] = q / np.sqrt((q * q).sum(axis=1))[:, None]

    return regions(frame, gen.sync, min(args.warmup, 3), args.regions, max(2, args.frames // 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bodies", type=int, nargs="*", default=[1, 16, 256, 4096, 16384])
    ap.add_argument("--points", type=int, nargs="*", default=[16, 64, 256, 1024, 4096])
    ap.add_argument("--max-points", type=int, default=1 << 22)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.cuda.init()   # before the library opens the device: torch brings a HIP runtime of its own
    fused, sc = generator("fused")
    split, _ = generator("split")
    lines = ["# scripts/bench_bodies.py: microseconds per frame of %d substeps (dt %.6f s, warm start) on 1024^2 x 4 maps; median of %d regions of %d frames "
             "[fastest .. slowest]; (a) host loop = the baseline" % (SUBSTEPS, DT, args.regions, args.frames),
             "%7s %7s | %30s | %30s | %30s | %9s %9s" % ("bodies", "points", "(a) host loop", "(b) split", "(c) fused", "a/c", "b/c")]
    print("\n".join(lines), flush=True)
    for nb in args.bodies:
        for npts in args.points:
            if nb * npts > args.max_points:
                continue
            st, hull = scene(nb, npts)
            a = host_loop(fused, sc, st, hull, args)
            b = device_step(split, sc, st, hull, args)
            c = device_step(fused, sc, st, hull, args)
            fmt = lambda r: "%9.1f [%8.1f .. %8.1f]" % r   # noqa: E731
            line = "%7d %7d | %30s | %30s | %30s | %9.2f %9.2f" % (nb, npts, fmt(a), fmt(b), fmt(c), a[0] / c[0], b[0] / c[0])
            lines.append(line)
            print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
