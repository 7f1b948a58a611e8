"""The cost of the sun shadows: a 2048^2 map of 256 crates (ow_shadow_map_begin + ow_shadow_map_cast from a body set's resident poses), and
ow_shadow_apply_async at 5 taps with water receiving over the 1280 x 720 records of ow_mesh_draw_async's and ow_solid_draw_async's picture
of the reference scene (256^2 x 3, main.tscn's camera and sun), next to ow_solid_draw_async and ow_environment_apply_async on the same
picture as yardsticks.  Run it on a GPU; without one it fails.  The measurement runs in a child process under its own time limit (the
parent never opens the device).

Each figure is the median of 5 REGIONS of REPS launches between two events on the context's stream (a caller's stream, so that the events
and the launches share it), after 3 regions of warm-up.  A launch of a pass or of the solid draw is preceded by a device-to-device copy
that restores the records from a pristine copy -- a pass leaves its status bit behind and a second pass over the same records would do
nothing --; the restoring copy alone is timed the same way and subtracted.  There is no threshold: the figures are a record.
    python scripts/shadow_cost.py [out.txt]          what profiles/shadow_1024x4.txt holds"""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTH, HEIGHT, STEPS, REGIONS, REPS, WARMUP = 1280, 720, 20, 5, 20, 3
MAP_SIZE, SIDE, SPACING = 2048, 16, 5.0          # 256 crates, 5 m apart
FRAME = dict(center=(0.0, 0.0, 17.5), half_extent=50.0, depth_range=100.0)
CRATE = (2.0, 1.0, 2.0)
LIMIT = 300                  # seconds for the child


def crates(W):
    """SIDE^2 crates of examples/shadow_host.c's kind on a grid about FRAME's centre"""
    import numpy as np
    per, rho = 4 * 2 * 4, 1025.0
    volume = CRATE[0] * CRATE[1] * CRATE[2]
    mass = 0.5 * rho * volume
    n = SIDE * SIDE
    st, hull = np.zeros(n, W.RIGID_BODY), np.zeros(n * per, W.HULL_POINT)
    for b in range(n):
        st[b]["position"] = ((b % SIDE - (SIDE - 1) / 2) * SPACING, 0.3, FRAME["center"][2] + (b // SIDE - (SIDE - 1) / 2) * SPACING)
        st[b]["orientation"] = (0, 0, 0, 1)
        st[b]["mass"] = mass
        st[b]["inverse_inertia"] = (12.0 / (mass * (CRATE[1] ** 2 + CRATE[2] ** 2)), 12.0 / (mass * (CRATE[0] ** 2 + CRATE[2] ** 2)),
                                    12.0 / (mass * (CRATE[0] ** 2 + CRATE[1] ** 2)))
        st[b]["linear_drag"], st[b]["quadratic_drag"] = 3.0, 0.5
        st[b]["point_offset"], st[b]["point_count"] = b * per, per
        k = b * per
        for i in range(4):
            for j in range(2):
                for l in range(4):
                    hull[k]["local"] = ((i + 0.5) * (CRATE[0] / 4) - CRATE[0] / 2, (j + 0.5) * (CRATE[1] / 2) - CRATE[1] / 2, (l + 0.5) * (CRATE[2] / 4) - CRATE[2] / 2)
                    hull[k]["volume"], hull[k]["half_height"], hull[k]["body"] = volume / per, CRATE[1] / 2 / 2, b
                    k += 1
    return st, hull


def child():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    from godotoceanwaves_amd import _lib
    from godotoceanwaves_amd.presets import UPDATE_DELTA
    from godotoceanwaves_amd.wave_generator import WaveGenerator as W
    from scenes import box, grid, make_gen, REF_BASIS, scales_of
    stream = torch.cuda.Stream()
    gen, params = make_gen(256, [0, 1, 2], stream=stream.cuda_stream)
    sc = scales_of(params)
    cam = W.camera((0.0, 10.0, -25.0), REF_BASIS, 75.0, WIDTH, HEIGHT, 4000.0)
    origin = W.clipmap_origin(cam.position, 4.0)
    rec = torch.zeros((WIDTH * HEIGHT, W.RENDER_PIXEL.itemsize), dtype=torch.uint8, device="cuda:0")
    mesh = gen.mesh_create(*grid(128, 4.0))
    solid = gen.solid_create(*box(CRATE))
    bodies = gen.bodies_create(*crates(W))
    shadow = gen.shadow_map_create(MAP_SIZE)
    opts = dict(filter_taps=5, receive_water=True)
    print(f"device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, HIP {torch.version.hip}")
    with torch.cuda.stream(stream):
        for _ in range(STEPS):
            gen.update_all(UPDATE_DELTA, params)
            gen.bodies_step(bodies, sc, 4, UPDATE_DELTA / 4, {"warm_start": True})
        gen.mesh_draw_async(mesh, cam, origin, sc, None, rec, {"falloff": True, "cull_back": True})
        water_only = rec.clone()
        gen.solid_draw_async(solid, bodies, cam, None, rec)
        pristine = rec.clone()
        gen.shadow_map_begin(shadow, FRAME)
        gen.shadow_map_cast(shadow, solid, bodies)
        gen.shadow_apply_async(shadow, cam, rec, None, opts)
    stream.synchronize()
    st = gen.shadow_stats(shadow)
    depth = gen.shadow_map_read(shadow)
    covered = depth != np.float32(3.4028235e38)
    before = np.frombuffer(pristine.cpu().numpy().tobytes(), W.RENDER_PIXEL)
    after = np.frombuffer(rec.cpu().numpy().tobytes(), W.RENDER_PIXEL)
    hit, crate = (before["status"] & _lib.OW_RAY_HIT) != 0, (before["status"] & _lib.OW_RAY_SOLID) != 0
    dark = (after["diffuse"] < before["diffuse"]).any(-1)
    assert (((after["status"] & _lib.OW_RAY_SHADOWED) != 0) == hit).all()
    print(f"map {MAP_SIZE} x {MAP_SIZE} over {2 * FRAME['half_extent']:.0f} m, {SIDE * SIDE} crates: {st['drawn']} triangles cast, {st['culled']} culled, "
          f"{int(covered.sum())} texels covered ({covered.mean():.4f} of the map)")
    print(f"records {WIDTH} x {HEIGHT} ({WIDTH * HEIGHT * 128 / 1e6:.0f} MB): receivers in {hit.mean():.3f} of the picture, crates in {crate.mean():.3f}, "
          f"sun dimmed in {dark.mean():.3f}")

    def region(launch, restore):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            a.record(stream)
            for _ in range(REPS):
                if restore is not None:
                    rec.copy_(restore, non_blocking=True)
                if launch:
                    launch()
            b.record(stream)
        stream.synchronize()
        return a.elapsed_time(b) * 1e3 / REPS      # microseconds per launch

    def measure(launch, restore):
        for _ in range(WARMUP):
            region(launch, restore)
        return [region(launch, restore) for _ in range(REGIONS)]

    def cast():
        gen.shadow_map_begin(shadow, FRAME)
        gen.shadow_map_cast(shadow, solid, bodies)

    def cast_wave():
        gen.shadow_map_begin(shadow, dict(FRAME, lane_box=-1))
        gen.shadow_map_cast(shadow, solid, bodies)

    built = measure(cast, None)
    built_wave = measure(cast_wave, None)
    cast()
    copy = measure(None, pristine)
    apply5 = measure(lambda: gen.shadow_apply_async(shadow, cam, rec, None, opts), pristine)
    apply1 = measure(lambda: gen.shadow_apply_async(shadow, cam, rec, None, dict(opts, filter_taps=1)), pristine)
    apply9 = measure(lambda: gen.shadow_apply_async(shadow, cam, rec, None, dict(opts, filter_taps=9)), pristine)
    solids = measure(lambda: gen.solid_draw_async(solid, bodies, cam, None, rec), water_only)
    env = measure(lambda: gen.environment_apply_async(cam, rec), pristine)
    base = statistics.median(copy)
    row = lambda v, off: f"median {statistics.median(v) - off:8.2f} us ({REGIONS} regions of {REPS}: " + " ".join(f"{x - off:.2f}" for x in v) + ")"   # noqa: E731
    print(f"ow_shadow_map_begin + ow_shadow_map_cast:                 {row(built, 0.0)}")
    print(f"the same with lane_box -1 (every triangle to the wave):   {row(built_wave, 0.0)}")
    print(f"restoring copy alone:                                     {row(copy, 0.0)}")
    print("per launch beyond the copy:")
    for name, v in (("ow_shadow_apply_async, 5 taps ", apply5), ("ow_shadow_apply_async, 1 tap  ", apply1), ("ow_shadow_apply_async, 9 taps ", apply9),
                    ("ow_solid_draw_async           ", solids), ("ow_environment_apply_async    ", env)):
        print(f"{name}: {row(v, base)}")
    for h, fn in ((shadow, gen.shadow_map_destroy), (solid, gen.solid_destroy), (bodies, gen.bodies_destroy), (mesh, gen.mesh_destroy)):
        fn(h)
    gen.free()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child()
        return
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "shadow_1024x4.txt")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, timeout=LIMIT)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit(f"the measurement failed (exit status {r.returncode}): nothing is written")
    text = "sun shadows: scripts/shadow_cost.py (a 2048^2 map of 256 crates; the pass next to ow_solid_draw and ow_environment_apply on the same records)\n" + r.stdout
    with open(out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
