"""The cost of ray casts against the floating bodies: ow_cast_bodies_async for 1, 64 and 65536 rays against 256 and 4096 twelve-triangle
crates of a body set (at the poses it was created with) on 1024^2 x 4 maps, with the bounding spheres (cull 0) and without (cull -1), next to ow_raycast_surface_async on the
same rays as a yardstick, and the scene cast (the water cast, then the solid cast on its records).  Run it on a GPU; without one it fails.
Every crate count is measured in a child process of its own under its own time limit (the parent never opens the device).

Each figure is the median of 5 REGIONS of `reps` calls between two events on the context's stream (a caller's stream, so that the events and
the launches share it), after 2 regions of warm-up; reps is 20, or 3 where a call takes milliseconds.  There is no threshold: the figures
are a record.
    python scripts/solid_cast_cost.py [out.txt]          what profiles/solid_cast_1024x4.txt holds"""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REGIONS, WARMUP = 5, 2
SPACING, CRATE = 5.0, (2.0, 1.0, 2.0)
SIDES = (16, 64)             # 256 and 4096 crates
RAYS = (1, 64, 65536)
LIMIT = 240                  # seconds for each child


def crates(W, side):
    """side^2 crates of examples/solid_draw_host.c's kind on a grid about the origin, four hull points each"""
    import numpy as np
    per, rho = 4, 1025.0
    volume = CRATE[0] * CRATE[1] * CRATE[2]
    mass = 0.5 * rho * volume
    n = side * side
    st, hull = np.zeros(n, W.RIGID_BODY), np.zeros(n * per, W.HULL_POINT)
    b = np.arange(n)
    st["position"] = np.stack([(b % side - (side - 1) / 2) * SPACING, np.full(n, 0.3), (b // side - (side - 1) / 2) * SPACING], axis=1)
    st["orientation"] = (0, 0, 0, 1)
    st["mass"] = mass
    st["inverse_inertia"] = (12.0 / (mass * (CRATE[1] ** 2 + CRATE[2] ** 2)), 12.0 / (mass * (CRATE[0] ** 2 + CRATE[2] ** 2)),
                             12.0 / (mass * (CRATE[0] ** 2 + CRATE[1] ** 2)))
    st["linear_drag"], st["quadratic_drag"] = 3.0, 0.5
    st["point_offset"], st["point_count"] = b * per, per
    k = np.arange(n * per)
    hull["local"] = np.stack([((k % 2) - 0.5) * CRATE[0] / 2, np.zeros(n * per), ((k // 2 % 2) - 0.5) * CRATE[2] / 2], axis=1)
    hull["volume"], hull["half_height"], hull["body"] = volume / per, CRATE[1] / 2, k // per
    return st, hull


def child(side):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    from godotoceanwaves_amd import _lib, solid_cast as SC
    from godotoceanwaves_amd.presets import UPDATE_DELTA
    from godotoceanwaves_amd.wave_generator import WaveGenerator as W
    from scenes import box, make_gen, scales_of
    stream = torch.cuda.Stream()
    gen, params = make_gen(1024, [0, 1, 2, 3], stream=stream.cuda_stream)
    sc = scales_of(params)
    solid = gen.solid_create(*box(CRATE))
    bodies = gen.bodies_create(*crates(W, side))
    half = side * SPACING / 2
    rng = np.random.default_rng(5)
    n = max(RAYS)
    o = np.stack([rng.uniform(-half, half, n), rng.uniform(3.0, 40.0, n), rng.uniform(-half, half, n)], axis=1)
    aim = np.stack([rng.uniform(-half, half, n), np.zeros(n), rng.uniform(-half, half, n)], axis=1)
    rays = W.rays(o, aim - o, 2000.0)
    rays_dev = torch.from_numpy(rays.view(np.uint8).copy()).to("cuda:0")
    water_dev = torch.zeros(n * W.RAYCAST_HIT.itemsize, dtype=torch.uint8, device="cuda:0")
    out_dev = torch.zeros(n * SC.SOLID_HIT.itemsize, dtype=torch.uint8, device="cuda:0")
    print(f"device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, HIP {torch.version.hip}")
    with torch.cuda.stream(stream):
        gen.run(UPDATE_DELTA, params, 4)
        gen.raycast_surface_async(rays_dev, sc, water_dev)
        SC.raycast_solids_async(gen, solid, bodies, rays_dev, out_dev, water_dev)
    stream.synchronize()
    st = SC.raycast_solids_stats(gen)
    rec = np.frombuffer(out_dev.cpu().numpy().tobytes(), SC.SOLID_HIT)
    wet = np.frombuffer(water_dev.cpu().numpy().tobytes(), W.RAYCAST_HIT)
    print(f"{side * side} crates {SPACING:.0f} m apart on 1024^2 x 4 maps, {n} rays from 3 .. 40 m up: the water is hit by {((wet['status'] & _lib.OW_RAY_HIT) != 0).mean():.3f} "
          f"of them, a crate (no farther than the water) by {((rec['status'] & _lib.OW_RAY_SOLID) != 0).mean():.3f}; a ray's sphere test passes "
          f"{st['sphere_tests_passed'] / n:.2f} crates of {side * side - st['skipped_instances']}, {st['pairs_tested'] / n:.1f} pairs a ray")

    def region(launch, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            a.record(stream)
            for _ in range(reps):
                launch()
            b.record(stream)
        stream.synchronize()
        return a.elapsed_time(b) * 1e3 / reps      # microseconds per call

    def measure(launch, reps):
        for _ in range(WARMUP):
            region(launch, reps)
        return [region(launch, reps) for _ in range(REGIONS)]

    row = lambda v, reps: f"median {statistics.median(v):10.2f} us ({REGIONS} regions of {reps}: " + " ".join(f"{x:.2f}" for x in v) + ")"   # noqa: E731
    for count in RAYS:
        heavy = count * side * side >= 1 << 24
        calls = (("ow_cast_bodies_async, cull  0   ", lambda: SC.raycast_solids_async(gen, solid, bodies, rays_dev, out_dev, ray_count=count), 20),
                 ("ow_cast_bodies_async, cull -1   ", lambda: SC.raycast_solids_async(gen, solid, bodies, rays_dev, out_dev, options={"cull": -1}, ray_count=count),
                  3 if heavy else 20),
                 ("ow_raycast_surface_async        ", lambda: gen.raycast_surface_async(rays_dev, sc, water_dev, count=count), 20),
                 ("the water cast, then the solids ", lambda: (gen.raycast_surface_async(rays_dev, sc, water_dev, count=count),
                                                                SC.raycast_solids_async(gen, solid, bodies, rays_dev, out_dev, water_dev, ray_count=count)), 20))
        for name, launch, reps in calls:
            print(f"{side * side:5d} crates {count:6d} rays  {name}: {row(measure(launch, reps), reps)}")
    gen.solid_destroy(solid)
    gen.bodies_destroy(bodies)
    gen.free()


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(int(sys.argv[2]))
        return
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "solid_cast_1024x4.txt")
    text = "ray casts against the floating bodies: scripts/solid_cast_cost.py (microseconds per asynchronous call on 1024^2 x 4 maps)\n"
    for side in SIDES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(side)], capture_output=True, text=True, timeout=LIMIT)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"the measurement of {side * side} crates failed (exit status {r.returncode}): nothing is written")
        text += r.stdout
    with open(out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
