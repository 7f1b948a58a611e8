"""The cost of ow_solid_draw_async at 1280 x 720 over a mesh picture of the reference scene (1024^2 x 3, main.tscn's camera): 256 and 4 096
crates of 2 x 1 x 2 m floating on a grid in front of the camera, next to the ow_mesh_draw_async that produced the picture.  Each of the three
is measured by a child process of its own under its own time limit (the parent never opens the device); a child that fails ends the run.
Events on the context's stream (a caller's stream, so that the events and the launches share it), the median of REPS launches after a warm-up.
There is no threshold: the figures are a record.
    python scripts/solid_draw_time.py [out.txt]          what profiles/solid_draw.txt holds"""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTH, HEIGHT, STEPS, REPS, WARMUP = 1280, 720, 30, 40, 5
LIMIT = 240     # seconds per child


def crates(count, spacing):
    """`count` crates on a square grid `spacing` metres apart that starts 4 m in front of the camera's foot point, dropped from 0.3 m"""
    import numpy as np
    from godotoceanwaves_amd.wave_generator import WaveGenerator as W
    from scenes import crate, make_bodies
    side = int(round(count ** 0.5))
    items = [crate(origin=((k % side - 0.5 * (side - 1)) * spacing, 0.3, -21.0 + (k // side) * spacing), divisions=(2, 2, 2), kl=3.0, kq=0.5) for k in range(count)]
    st, hull = make_bodies(items)
    assert len(st) == count and W.RIGID_BODY.itemsize == st.dtype.itemsize and np.isfinite(st["mass"]).all()
    return st, hull


def child(step):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    from godotoceanwaves_amd import _lib
    from godotoceanwaves_amd.presets import UPDATE_DELTA
    from godotoceanwaves_amd.wave_generator import WaveGenerator as W
    from scenes import box, grid, make_gen, REF_BASIS, scales_of
    count = {"mesh": 256, "solid256": 256, "solid4096": 4096}[step]
    stream = torch.cuda.Stream()
    gen, params = make_gen(1024, [0, 1, 2], stream=stream.cuda_stream)
    sc = scales_of(params)
    cam = W.camera((0.0, 10.0, -25.0), REF_BASIS, 75.0, WIDTH, HEIGHT, 4000.0)
    origin = W.clipmap_origin(cam.position, 4.0)
    pixels = WIDTH * HEIGHT
    rgba = torch.zeros((pixels, 4), dtype=torch.uint8, device="cuda:0")
    rec = torch.zeros((pixels, W.RENDER_PIXEL.itemsize), dtype=torch.uint8, device="cuda:0")
    mesh = gen.mesh_create(*grid(128, 4.0))
    bodies = gen.bodies_create(*crates(count, 6.0 if count == 256 else 3.0))
    solid = gen.solid_create(*box((2.0, 1.0, 2.0)))
    opts = {"falloff": True, "cull_back": True}
    with torch.cuda.stream(stream):
        for _ in range(STEPS):
            gen.update_all(UPDATE_DELTA, params)
            gen.bodies_step(bodies, sc, 2, UPDATE_DELTA / 2, {"warm_start": True})
        gen.mesh_draw_async(mesh, cam, origin, sc, rgba, rec, opts)
        gen.solid_draw_async(solid, bodies, cam, rgba, rec)
    stream.synchronize()
    print(f"device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, HIP {torch.version.hip}")
    if step != "mesh":
        records = np.frombuffer(rec.cpu().numpy().tobytes(), W.RENDER_PIXEL)
        st = gen.solid_draw_stats()
        share = ((records["status"] & _lib.OW_RAY_SOLID) != 0).mean()
        print(f"{count} crates, {count * 12} triangles: {st['drawn']} drawn, {st['culled']} culled, {st['skipped_instances']} instances skipped; "
              f"pixels that show a crate {share:.4f}; scratch {st['scratch_bytes']} B")

    def once():
        if step == "mesh":
            gen.mesh_draw_async(mesh, cam, origin, sc, rgba, rec, opts)
        else:
            gen.solid_draw_async(solid, bodies, cam, rgba, rec)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
    with torch.cuda.stream(stream):
        for _ in range(WARMUP):
            once()
        for a, b in ev:
            a.record(stream)
            once()
            b.record(stream)
    stream.synchronize()
    us = [a.elapsed_time(b) * 1e3 for a, b in ev]
    what = (f"ow_mesh_draw_async (the picture underneath, {128 * 128 * 2} triangles)" if step == "mesh" else
            f"ow_solid_draw_async, {count} crates (k_solid_clear, k_solid_vertices, k_solid_raster, k_solid_resolve)")
    print(f"{what}: median {statistics.median(us):.1f} us, min {min(us):.1f}, max {max(us):.1f} over {REPS} launches")
    gen.solid_destroy(solid)
    gen.bodies_destroy(bodies)
    gen.mesh_destroy(mesh)
    gen.free()


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--step":
        return child(sys.argv[2])
    out = open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, "w")

    def say(line):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()
    say(f"ow_solid_draw_async at {WIDTH} x {HEIGHT} over ow_mesh_draw_async's picture, 1024^2 x 3, the reference camera, crates stepped {STEPS} times "
        f"(scripts/solid_draw_time.py)")
    for k, step in enumerate(("solid256", "solid4096", "mesh")):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step], capture_output=True, text=True, timeout=LIMIT)
        except subprocess.TimeoutExpired:
            say(f"{step}: no result within {LIMIT} s; stopping")
            return 1
        if r.returncode != 0:
            say(f"{step}: failed with status {r.returncode}; stopping\n{r.stderr[-2000:]}")
            return 1
        for line in r.stdout.splitlines():
            if k == 0 or not line.startswith("device:"):
                say(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
