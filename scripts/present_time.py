"""The cost of the finishing stage at a 1920 x 1080 output: ow_environment_apply_async and ow_present_async over ow_mesh_draw_async's picture of
the reference scene (256^2 x 3, main.tscn's camera, a 1024 x 512 procedural panorama, the scene's fog and present settings), with downsample
1 (records 1920 x 1080) and downsample 2 (records 3840 x 2160).  Each size is measured by a child process of its own under its own time
limit (the parent never opens the device); a child that fails ends the run.  Events on the context's stream (a caller's stream, so that
the events and the launches share it), the median of REPS launches after a warm-up; the records are restored from a pristine copy before
every launch of the pass, outside the events, because a pass leaves OW_RAY_ENVIRONMENT behind and a second pass over the same records
would do nothing.  Next to each time: the bytes of distinct 128-byte lines the kernel touches (computed from the shapes: a record is one
line) and that traffic over the time as a fraction of the plain-copy rate README.md cites (0.785 of 8 TB/s).  There is no threshold: the
figures are a record; the 1920 x 1080 records nearly fit the Infinity Cache, so those figures are partly warm-cache ones (NOTE below).
    python scripts/present_time.py [out.txt]          what profiles/present_time.txt holds"""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT_WIDTH, OUT_HEIGHT, STEPS, REPS, WARMUP = 1920, 1080, 20, 20, 3
COPY_RATE = 0.785 * 8.0e12   # bytes per second: README.md's "0.78-0.79 of 8 TB/s, the part's copy ceiling"
LIMIT = 300                  # seconds per child
NOTE = ("note: at 1920 x 1080 the 265 MB of records largely fit the 256 MB Infinity Cache, and each timed launch follows a launch (the restoring copy, or the "
        "previous present) that has just touched them, so the downsample-1 figures are partly warm-cache figures (hence a rate above the copy rate); "
        "the 3840 x 2160 figures (1062 MB) are the ones representative of DRAM")


def panorama(w=1024, h=512):
    import numpy as np
    j, i = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    img = np.zeros((h, w, 4), np.uint8)
    img[..., 0] = 40 + 150 * j // (h - 1)
    img[..., 1] = 90 + 120 * j // (h - 1) + 20 * np.abs(2 * i - w) // w
    img[..., 2] = 230 - 100 * j // (h - 1)
    img[..., 3] = 255
    return img


def lines(nbytes):
    return (nbytes + 127) // 128 * 128


def child(s):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    from godotoceanwaves_amd import _lib
    from godotoceanwaves_amd.presets import UPDATE_DELTA
    from godotoceanwaves_amd.wave_generator import WaveGenerator as W
    from scenes import grid, make_gen, REF_BASIS, scales_of
    width, height = OUT_WIDTH * s, OUT_HEIGHT * s
    stream = torch.cuda.Stream()
    gen, params = make_gen(256, [0, 1, 2], stream=stream.cuda_stream)
    sc = scales_of(params)
    cam = W.camera((0.0, 10.0, -25.0), REF_BASIS, 75.0, width, height, 4000.0)
    origin = W.clipmap_origin(cam.position, 4.0)
    records, out = width * height, OUT_WIDTH * OUT_HEIGHT
    rec = torch.zeros((records, W.RENDER_PIXEL.itemsize), dtype=torch.uint8, device="cuda:0")
    rgba = torch.zeros((out, 4), dtype=torch.uint8, device="cuda:0")
    linear = torch.zeros((out, 4), dtype=torch.float32, device="cuda:0")
    mesh = gen.mesh_create(*grid(128, 4.0))
    pano = panorama()
    sky = gen.sky_create(pano)
    present = {"downsample": s}
    with torch.cuda.stream(stream):
        gen.run(UPDATE_DELTA, params, STEPS)
        gen.mesh_draw_async(mesh, cam, origin, sc, None, rec, {"falloff": True, "cull_back": True})
        pristine = rec.clone()
        gen.environment_apply_async(cam, rec, sky)
        gen.present_async(cam, rec, rgba, linear, present)
    stream.synchronize()
    print(f"device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, HIP {torch.version.hip}")
    status = np.frombuffer(rec.cpu().numpy().tobytes(), W.RENDER_PIXEL)["status"]
    hit = (status & _lib.OW_RAY_HIT) != 0
    assert ((status & _lib.OW_RAY_ENVIRONMENT) != 0).all() and np.isfinite(linear.cpu().numpy()).all()
    print(f"downsample {s}: records {width} x {height} ({records * 128 / 1e6:.0f} MB), output {OUT_WIDTH} x {OUT_HEIGHT}; sky pixels {1 - hit.mean():.3f} of the picture")

    def timed(launch, before=None):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
        with torch.cuda.stream(stream):
            for _ in range(WARMUP):
                if before:
                    before()
                launch()
            for a, b in ev:
                if before:
                    before()
                a.record(stream)
                launch()
                b.record(stream)
        stream.synchronize()
        return [a.elapsed_time(b) * 1e3 for a, b in ev]

    def report(name, us, read, written):
        med = statistics.median(us)
        rate = (read + written) / (med * 1e-6)
        print(f"{name}: median {med:.1f} us, min {min(us):.1f}, max {max(us):.1f} over {REPS} launches; distinct 128-byte lines: {read} B read + {written} B written; "
              f"{rate / 1e12:.2f} TB/s = {rate / COPY_RATE:.2f} of the plain-copy rate ({COPY_RATE / 1e12:.2f} TB/s)")

    us = timed(lambda: gen.environment_apply_async(cam, rec, sky), lambda: rec.copy_(pristine))
    report("ow_environment_apply_async (k_environment_apply)", us, records * 128 + lines(pano.size), records * 128)
    us = timed(lambda: gen.present_async(cam, rec, rgba, linear, present))
    report(f"ow_present_async (k_present<{s}>), RGBA8 and linear out", us, records * 128, lines(out * 4) + lines(out * 16))
    us = timed(lambda: gen.present_async(cam, rec, rgba, None, present))
    report(f"ow_present_async (k_present<{s}>), RGBA8 only", us, records * 128, lines(out * 4))
    us = timed(lambda: rec.copy_(pristine))
    report("a device-to-device copy of the records, for scale", us, records * 128, records * 128)
    gen.sky_destroy(sky)
    gen.mesh_destroy(mesh)
    gen.free()


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--step":
        return child(int(sys.argv[2]))
    out = open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, "w")

    def say(line):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()
    say(f"ow_environment_apply_async and ow_present_async at a {OUT_WIDTH} x {OUT_HEIGHT} output over ow_mesh_draw_async's picture, 256^2 x 3, the reference "
        f"camera, a 1024 x 512 panorama, the scene's fog and present settings (scripts/present_time.py)")
    say(NOTE)
    for k, s in enumerate((1, 2)):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", str(s)], capture_output=True, text=True, timeout=LIMIT)
        except subprocess.TimeoutExpired:
            say(f"downsample {s}: no result within {LIMIT} s; stopping")
            return 1
        if r.returncode != 0:
            say(f"downsample {s}: failed with status {r.returncode}; stopping\n{r.stderr[-2000:]}")
            return 1
        for line in r.stdout.splitlines():
            if k == 0 or not line.startswith("device:"):
                say(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
