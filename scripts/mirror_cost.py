"""The cost of the floating bodies' reflections: ow_mirror_apply_async over the 1280 x 720 records of ow_mesh_draw_async's and
ow_solid_draw_async's picture of the reference scene (256^2 x 3, main.tscn's camera), with 256 and with 4 096 twelve-triangle crates, with
and without culling, next to
  the floor      ow_radiance_light_apply_async on the same records (what the pass does where no body is met), and
  the baseline   what there was before the pass: the mirror rays of all casting water pixels uploaded, then ow_cast_bodies_async over them
                 (one 64-lane wave a ray); shading the hits would come on top.
Run it on a GPU; without one it fails.  The measurement runs in a child process under its own time limit (the parent never opens the device).

Each figure is the median of 5 REGIONS of launches between two events on the context's stream (a caller's stream, so that the events and
the launches share it), after 3 regions of warm-up.  A launch of a pass is preceded by a device-to-device copy that restores the records
from a pristine copy -- a pass leaves its status bit behind and a second pass over the same records would do nothing --; the restoring
copy alone is timed the same way and subtracted.  The clocks are rocm-smi's reading before and after, where the tool is there.  There is no
threshold: the figures are a record.
    python scripts/mirror_cost.py [out.txt]          what profiles/mirror_1024x4.txt holds"""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mist_cost import clocks                                                    # noqa: E402
from shadow_cost import CRATE, HEIGHT, REGIONS, STEPS, WARMUP, WIDTH            # noqa: E402  (the same picture)

FIELDS = ((16, 5.0), (64, 3.0))     # side x side crates, metres apart: 256 over 80 m, 4 096 over 192 m, both from 8 m in front of the camera on
LIMIT = 600                         # seconds for the child


def crates(W, side, spacing):
    """side^2 crates of examples/shadow_host.c's kind on a grid that begins 8 m in front of the camera"""
    import numpy as np
    per, rho = 4 * 2 * 4, 1025.0
    volume = CRATE[0] * CRATE[1] * CRATE[2]
    mass = 0.5 * rho * volume
    n = side * side
    st, hull = np.zeros(n, W.RIGID_BODY), np.zeros(n * per, W.HULL_POINT)
    for b in range(n):
        st[b]["position"] = ((b % side - (side - 1) / 2) * spacing, 0.3, -17.0 + (b // side) * spacing)
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
    from godotoceanwaves_amd import _lib, mirror, solid_cast
    from godotoceanwaves_amd.presets import UPDATE_DELTA
    from godotoceanwaves_amd.wave_generator import WaveGenerator as W
    from scenes import box, example_panorama, grid, make_gen, REF_BASIS, scales_of
    stream = torch.cuda.Stream()
    gen, params = make_gen(256, [0, 1, 2], stream=stream.cuda_stream)
    sc = scales_of(params)
    cam = W.camera((0.0, 10.0, -25.0), REF_BASIS, 75.0, WIDTH, HEIGHT, 4000.0)
    origin = W.clipmap_origin(cam.position, 4.0)
    rec = torch.zeros((WIDTH * HEIGHT, W.RENDER_PIXEL.itemsize), dtype=torch.uint8, device="cuda:0")
    mesh = gen.mesh_create(*grid(128, 4.0))
    solid = gen.solid_create(*box(CRATE))
    sky = gen.sky_create(example_panorama())
    radiance = gen.radiance_create(sky)
    dark = (0.0, 0.0, 0.0)
    print(f"device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, HIP {torch.version.hip}")
    print("before: " + clocks())

    def region(launch, restore, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            a.record(stream)
            for _ in range(reps):
                if restore is not None:
                    rec.copy_(restore, non_blocking=True)
                if launch:
                    launch()
            b.record(stream)
        stream.synchronize()
        return a.elapsed_time(b) * 1e3 / reps      # microseconds per launch

    def measure(launch, restore, reps):
        for _ in range(WARMUP):
            region(launch, restore, reps)
        return [region(launch, restore, reps) for _ in range(REGIONS)]

    row = lambda v, off, reps: f"median {statistics.median(v) - off:9.2f} us ({REGIONS} regions of {reps}: " + " ".join(f"{x - off:.2f}" for x in v) + ")"   # noqa: E731
    for side, spacing in FIELDS:
        n = side * side
        reps = 20 if n <= 256 else 4
        bodies = gen.bodies_create(*crates(W, side, spacing))
        with torch.cuda.stream(stream):
            for _ in range(STEPS):
                gen.update_all(UPDATE_DELTA, params)
                gen.bodies_step(bodies, sc, 4, UPDATE_DELTA / 4, {"warm_start": True})
            gen.mesh_draw_async(mesh, cam, origin, sc, None, rec, {"falloff": True, "cull_back": True, "ambient_color": dark})
            gen.solid_draw_async(solid, bodies, cam, None, rec, {"ambient_color": dark})
            pristine = rec.clone()
            mirror.mirror_apply_async(gen, radiance, cam, rec, solid, bodies)
        stream.synchronize()
        st = mirror.mirror_stats(gen)
        before = np.frombuffer(pristine.cpu().numpy().tobytes(), W.RENDER_PIXEL)
        after = np.frombuffer(rec.cpu().numpy().tobytes(), W.RENDER_PIXEL)
        water = ((before["status"] & _lib.OW_RAY_HIT) != 0) & ((before["status"] & _lib.OW_RAY_SOLID) == 0)
        mirrored = (after["status"] & _lib.OW_RAY_MIRROR) != 0
        assert np.isfinite(after["color"]).all() and int(mirrored.sum()) == st["rays_hit"]
        print(f"\n{n} crates {spacing:g} m apart; records {WIDTH} x {HEIGHT} ({WIDTH * HEIGHT * 128 / 1e6:.0f} MB): water in {water.mean():.3f} of the picture, "
              f"crates in {((before['status'] & _lib.OW_RAY_SOLID) != 0).mean():.3f}")
        print(f"one pass: {st['pixels']} pixels, {st['rays_cast']} mirror rays, {st['sphere_tests_passed']} sphere tests passed "
              f"({st['sphere_tests_passed'] / max(st['rays_cast'], 1):.2f} a ray), {st['pairs_tested']} pairs, {st['rays_hit']} rays hit "
              f"({st['rays_hit'] / max(st['rays_cast'], 1):.4f})")
        # the baseline's rays: position and R = 2 (N . V) N - V of every casting record, formed on the host
        pos, nrm = before["position"].astype(np.float32), before["normal"].astype(np.float32)
        casting = water & ((before["status"] & (_lib.OW_RAY_FROM_BELOW | _lib.OW_RAY_ENVIRONMENT | _lib.OW_RAY_SKY_LIT)) == 0) & np.isfinite(nrm).all(-1) & (nrm != 0).any(-1)
        relv = pos - np.float32(cam.position[:])
        view = -relv / np.linalg.norm(relv, axis=-1, keepdims=True)
        refl = 2.0 * (nrm * view).sum(-1, keepdims=True) * nrm - view
        rays = W.rays(pos[casting], refl[casting], 200.0)
        rays_host = torch.from_numpy(np.frombuffer(rays.tobytes(), np.uint8).copy()).pin_memory()
        rays_dev = torch.zeros(len(rays) * W.RAY.itemsize, dtype=torch.uint8, device="cuda:0")
        hits_dev = torch.zeros(len(rays) * solid_cast.SOLID_HIT.itemsize, dtype=torch.uint8, device="cuda:0")

        def upload():
            rays_dev.copy_(rays_host, non_blocking=True)

        def cast():
            solid_cast.raycast_solids_async(gen, solid, bodies, rays_dev, hits_dev, ray_count=len(rays))

        with torch.cuda.stream(stream):
            upload()
            cast()
        stream.synchronize()
        found = np.frombuffer(hits_dev.cpu().numpy().tobytes(), solid_cast.SOLID_HIT)
        print(f"the baseline's cast: {len(rays)} rays, {int(((found['status'] & _lib.OW_RAY_HIT) != 0).sum())} hit")
        copy = measure(None, pristine, reps)
        base = statistics.median(copy)
        gathered = measure(lambda: mirror.mirror_apply_async(gen, radiance, cam, rec, solid, bodies), pristine, reps)
        uncull = measure(lambda: mirror.mirror_apply_async(gen, radiance, cam, rec, solid, bodies, options=dict(cull=-1)), pristine, reps) if n <= 256 else None
        nobody = measure(lambda: mirror.mirror_apply_async(gen, radiance, cam, rec), pristine, reps)
        floor = measure(lambda: gen.sky_light_apply_async(radiance, cam, rec), pristine, reps)
        up = measure(upload, None, reps)
        casts = measure(cast, None, reps)
        print(f"restoring copy alone:                       {row(copy, 0.0, reps)}")
        print("per launch beyond the copy:")
        for name, v in (("ow_mirror_apply_async                      ", gathered), ("ow_mirror_apply_async, cull -1 (no culling)", uncull),
                        ("ow_mirror_apply_async, no bodies           ", nobody), ("ow_radiance_light_apply_async (the floor)  ", floor)):
            if v is not None:
                print(f"{name}: {row(v, base, reps)}")
        print("the baseline, per launch:")
        print(f"upload of the mirror rays (pinned host memory): {row(up, 0.0, reps)}")
        print(f"ow_cast_bodies_async over them                : {row(casts, 0.0, reps)}")
        print(f"ratio, baseline (upload + cast) over the pass : {(statistics.median(up) + statistics.median(casts)) / (statistics.median(gathered) - base):.2f}")
        gen.bodies_destroy(bodies)
    print("\nafter:  " + clocks())
    for h, fn in ((radiance, gen.radiance_destroy), (sky, gen.sky_destroy), (solid, gen.solid_destroy), (mesh, gen.mesh_destroy)):
        fn(h)
    gen.free()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child()
        return
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mirror_1024x4.txt")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, timeout=LIMIT)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit(f"the measurement failed (exit status {r.returncode}): nothing is written")
    text = ("reflections of the floating bodies: scripts/mirror_cost.py (1280 x 720 records; the pass next to ow_radiance_light_apply, its floor, and to "
            "ow_cast_bodies_async over uploaded mirror rays, the route there was before)\n" + r.stdout)
    with open(out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
