"""The cost of the light from the sky: ow_radiance_create for a 2048 x 1024 panorama (the defaults: level 0 at 1024 x 512, six levels, 64
samples), and ow_radiance_light_apply_async next to ow_environment_apply_async on the same 1280 x 720 records of ow_mesh_draw_async's picture
of the reference scene (256^2 x 3, main.tscn's camera).  Run it on a GPU; without one it fails.  The measurement runs in a child process
under its own time limit (the parent never opens the device).

Each figure is the median of 5 REGIONS.  A region of the build is one ow_radiance_create + ow_radiance_destroy, timed with the host clock (the
create ends in the handle life cycle's synchronisation).  A region of a pass is REPS launches between two events on the context's stream
(a caller's stream, so that the events and the launches share it), each launch preceded by a device-to-device copy that restores the
records from a pristine copy -- a pass leaves its status bit behind and a second pass over the same records would do nothing --; the
restoring copy alone is timed the same way and subtracted.  There is no threshold: the figures are a record.
    python scripts/sky_light_cost.py [out.txt]          what profiles/sky_light_1024x4.txt holds"""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTH, HEIGHT, STEPS, REGIONS, REPS, WARMUP = 1280, 720, 20, 5, 20, 3
SKY_WIDTH, SKY_HEIGHT = 2048, 1024
LIMIT = 300                  # seconds for the child


def panorama(w, h):
    import numpy as np
    j, i = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    img = np.zeros((h, w, 4), np.uint8)
    img[..., 0] = 40 + 150 * j // (h - 1)
    img[..., 1] = 90 + 120 * j // (h - 1) + 20 * np.abs(2 * i - w) // w
    img[..., 2] = 230 - 100 * j // (h - 1)
    img[..., 3] = 255
    return img


def child():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    from godotoceanwaves_amd import _lib
    from godotoceanwaves_amd.presets import UPDATE_DELTA
    from godotoceanwaves_amd.wave_generator import WaveGenerator as W
    from scenes import grid, make_gen, REF_BASIS, scales_of
    stream = torch.cuda.Stream()
    gen, params = make_gen(256, [0, 1, 2], stream=stream.cuda_stream)
    sc = scales_of(params)
    cam = W.camera((0.0, 10.0, -25.0), REF_BASIS, 75.0, WIDTH, HEIGHT, 4000.0)
    origin = W.clipmap_origin(cam.position, 4.0)
    rec = torch.zeros((WIDTH * HEIGHT, W.RENDER_PIXEL.itemsize), dtype=torch.uint8, device="cuda:0")
    mesh = gen.mesh_create(*grid(128, 4.0))
    sky = gen.sky_create(panorama(SKY_WIDTH, SKY_HEIGHT))
    print(f"device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, HIP {torch.version.hip}")

    # the build
    gen.radiance_destroy(gen.radiance_create(sky))          # warm-up: code objects
    build = []
    for _ in range(REGIONS):
        gen.sync()
        t0 = time.perf_counter()
        radiance = gen.radiance_create(sky)
        build.append((time.perf_counter() - t0) * 1e3)
        if len(build) < REGIONS:
            gen.radiance_destroy(radiance)
    sizes = [gen.radiance_level(radiance, k).shape[:2] for k in range(radiance.levels)]
    print(f"ow_radiance_create, {SKY_WIDTH} x {SKY_HEIGHT} panorama, levels " + ", ".join(f"{w} x {h}" for h, w in sizes) +
          f", 64 samples: median {statistics.median(build):.3f} ms of {REGIONS} regions (" + " ".join(f"{v:.3f}" for v in build) + "), host clock, synchronised")

    # the passes
    with torch.cuda.stream(stream):
        gen.run(UPDATE_DELTA, params, STEPS)
        gen.mesh_draw_async(mesh, cam, origin, sc, None, rec, {"falloff": True, "cull_back": True, "ambient_color": (0.0, 0.0, 0.0)})
        pristine = rec.clone()
        gen.sky_light_apply_async(radiance, cam, rec)
    stream.synchronize()
    status = np.frombuffer(rec.cpu().numpy().tobytes(), W.RENDER_PIXEL)["status"]
    hit = (status & _lib.OW_RAY_HIT) != 0
    assert (((status & _lib.OW_RAY_SKY_LIT) != 0) == hit).all()
    print(f"records {WIDTH} x {HEIGHT} ({WIDTH * HEIGHT * 128 / 1e6:.0f} MB), water in {hit.mean():.3f} of the picture")

    def region(launch):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            a.record(stream)
            for _ in range(REPS):
                rec.copy_(pristine, non_blocking=True)
                if launch:
                    launch()
            b.record(stream)
        stream.synchronize()
        return a.elapsed_time(b) * 1e3 / REPS      # microseconds per launch

    def measure(launch):
        for _ in range(WARMUP):
            region(launch)
        return [region(launch) for _ in range(REGIONS)]

    copy = measure(None)
    light = measure(lambda: gen.sky_light_apply_async(radiance, cam, rec))
    env = measure(lambda: gen.environment_apply_async(cam, rec, sky))
    base = statistics.median(copy)
    print(f"restoring copy alone:          median {base:8.2f} us of {REGIONS} regions of {REPS} (" + " ".join(f"{v:.2f}" for v in copy) + ")")
    for name, v in (("ow_radiance_light_apply_async", light), ("ow_environment_apply_async   ", env)):
        print(f"{name}: median {statistics.median(v) - base:8.2f} us per launch beyond the copy ({REGIONS} regions of {REPS}: " + " ".join(f"{x - base:.2f}" for x in v) + ")")
    gen.radiance_destroy(radiance)
    gen.sky_destroy(sky)
    gen.mesh_destroy(mesh)
    gen.free()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child()
        return
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sky_light_1024x4.txt")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, timeout=LIMIT)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit(f"the measurement failed (exit status {r.returncode}): nothing is written")
    text = ("light from the sky: scripts/sky_light_cost.py (the build of a radiance pyramid; the pass next to ow_environment_apply on the same records)\n" + r.stdout)
    with open(out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
