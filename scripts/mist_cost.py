"""The cost of the height mist: ow_mist_apply_async at 64 slices over the 1280 x 720 records of ow_mesh_draw_async's and
ow_solid_draw_async's picture of the reference scene (256^2 x 3, main.tscn's camera and sun), with the 2048^2 shadow map of 256 crates
(scripts/shadow_cost.py's) and without a map, next to ow_environment_apply_async and ow_shadow_apply_async on the same records as
yardsticks.  Run it on a GPU; without one it fails.  The measurement runs in a child process under its own time limit (the parent never
opens the device).

Each figure is the median of 5 REGIONS of REPS launches between two events on the context's stream (a caller's stream, so that the events
and the launches share it), after 3 regions of warm-up.  A launch of a pass is preceded by a device-to-device copy that restores the
records from a pristine copy -- a pass leaves its status bit behind and a second pass over the same records would do nothing --; the
restoring copy alone is timed the same way and subtracted.  The clocks are rocm-smi's reading before and after, where the tool is there.
There is no threshold: the figures are a record.
    python scripts/mist_cost.py [out.txt]          what profiles/mist_1024x4.txt holds"""
import os
import shutil
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from shadow_cost import crates, CRATE, FRAME, HEIGHT, MAP_SIZE, REGIONS, REPS, SIDE, STEPS, WARMUP, WIDTH   # noqa: E402  (the same scene)

SLICES = 64
LIMIT = 300                  # seconds for the child


def clocks():
    """the device's current clocks as rocm-smi prints them (read only), or a note that the tool is not there"""
    exe = shutil.which("rocm-smi") or "/opt/rocm/bin/rocm-smi"
    if not os.path.exists(exe):
        return "clocks: rocm-smi not found"
    try:
        r = subprocess.run([exe, "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=30)
    except (OSError, subprocess.TimeoutExpired):
        return "clocks: rocm-smi did not answer"
    rows = [line.strip() for line in r.stdout.splitlines() if "clock level" in line and ("sclk" in line or "mclk" in line or "fclk" in line)]
    return "clocks: " + ("; ".join(rows) if rows else "not reported")


def child():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    from godotoceanwaves_amd import _lib, mist
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
    opts = dict(slices=SLICES)
    print(f"device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, HIP {torch.version.hip}")
    print("before: " + clocks())
    with torch.cuda.stream(stream):
        for _ in range(STEPS):
            gen.update_all(UPDATE_DELTA, params)
            gen.bodies_step(bodies, sc, 4, UPDATE_DELTA / 4, {"warm_start": True})
        gen.mesh_draw_async(mesh, cam, origin, sc, None, rec, {"falloff": True, "cull_back": True})
        gen.solid_draw_async(solid, bodies, cam, None, rec)
        pristine = rec.clone()
        gen.shadow_map_begin(shadow, FRAME)
        gen.shadow_map_cast(shadow, solid, bodies)
        mist.mist_apply_async(gen, cam, rec, shadow, None, opts)
    stream.synchronize()
    st = mist.mist_stats(gen)
    before = np.frombuffer(pristine.cpu().numpy().tobytes(), W.RENDER_PIXEL)
    after = np.frombuffer(rec.cpu().numpy().tobytes(), W.RENDER_PIXEL)
    assert ((after["status"] & _lib.OW_RAY_MIST) != 0).all() and np.isfinite(after["color"]).all()
    hit = (before["status"] & _lib.OW_RAY_HIT) != 0
    total = WIDTH * HEIGHT * SLICES
    print(f"map {MAP_SIZE} x {MAP_SIZE} over {2 * FRAME['half_extent']:.0f} m, {SIDE * SIDE} crates; records {WIDTH} x {HEIGHT} "
          f"({WIDTH * HEIGHT * 128 / 1e6:.0f} MB), hits in {hit.mean():.3f} of the picture; {SLICES} slices")
    print(f"one pass: {st['pixels']} pixels, {st['slices_fetched']} of {total} slices read the map ({st['slices_fetched'] / total:.3f}), "
          f"{st['slices_shadowed']} found shadowed ({st['slices_shadowed'] / total:.4f})")

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

    copy = measure(None, pristine)
    with_map = measure(lambda: mist.mist_apply_async(gen, cam, rec, shadow, None, opts), pristine)
    without = measure(lambda: mist.mist_apply_async(gen, cam, rec, None, None, opts), pristine)
    most = measure(lambda: mist.mist_apply_async(gen, cam, rec, shadow, None, dict(slices=256)), pristine)
    env = measure(lambda: gen.environment_apply_async(cam, rec), pristine)
    shade = measure(lambda: gen.shadow_apply_async(shadow, cam, rec, None, dict(filter_taps=5, receive_water=True)), pristine)
    base = statistics.median(copy)
    row = lambda v, off: f"median {statistics.median(v) - off:8.2f} us ({REGIONS} regions of {REPS}: " + " ".join(f"{x - off:.2f}" for x in v) + ")"   # noqa: E731
    print(f"restoring copy alone:                    {row(copy, 0.0)}")
    print("per launch beyond the copy:")
    for name, v in (("ow_mist_apply_async, 64 slices, the map ", with_map), ("ow_mist_apply_async, 64 slices, no map  ", without),
                    ("ow_mist_apply_async, 256 slices, the map", most), ("ow_environment_apply_async              ", env),
                    ("ow_shadow_apply_async, 5 taps           ", shade)):
        print(f"{name}: {row(v, base)}")
    print("after:  " + clocks())
    for h, fn in ((shadow, gen.shadow_map_destroy), (solid, gen.solid_destroy), (bodies, gen.bodies_destroy), (mesh, gen.mesh_destroy)):
        fn(h)
    gen.free()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child()
        return
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "mist_1024x4.txt")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, timeout=LIMIT)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit(f"the measurement failed (exit status {r.returncode}): nothing is written")
    text = ("height mist: scripts/mist_cost.py (1280 x 720 records, 64 slices, the 2048^2 map of 256 crates; the pass next to "
            "ow_environment_apply and ow_shadow_apply on the same records)\n" + r.stdout)
    with open(out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
