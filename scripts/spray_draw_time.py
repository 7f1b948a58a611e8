"""The cost of ow_billboard_draw_async at 1920 x 1080 on the reference scene (1024^2 x 3, main.tscn's camera, ow_spray_options_default's
32 768 particles) after one emitter cycle, next to the ow_mesh_draw_async it composites over and to a hipMemcpyAsync of the bytes the blend
kernel must read and write, as the floor.  Each of the three is measured by a child process of its own under its own time limit (the
parent never opens the device); a child that fails ends the run.  Events on the context's stream (a caller's stream, so that the events and
the launches share it), the median of REPS launches after a warm-up.
    python scripts/spray_draw_time.py [out.txt]          what profiles/spray_draw.txt holds"""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTH, HEIGHT, STEPS, REPS, WARMUP = 1920, 1080, 300, 40, 5
LIMIT = 240     # seconds per child
PIXEL_READ, PIXEL_WRITE = 40, 36     # k_billboard_blend per pixel: t, status, two 16-byte vectors in; the vectors and the RGBA8 word out


def child(step):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ctypes as C
    import numpy as np
    import torch
    from godotoceanwaves_amd.presets import UPDATE_DELTA
    from godotoceanwaves_amd.wave_generator import WaveGenerator as W
    from scenes import example_textures, grid, make_gen, REF_BASIS, scales_of
    stream = torch.cuda.Stream()
    gen, params = make_gen(1024, [0, 1, 2], stream=stream.cuda_stream)
    sc = scales_of(params)
    cam = W.camera((0.0, 10.0, -25.0), REF_BASIS, 75.0, WIDTH, HEIGHT, 4000.0)
    origin = W.clipmap_origin(cam.position, 4.0)
    count = WIDTH * HEIGHT
    rgba = torch.zeros((count, 4), dtype=torch.uint8, device="cuda:0")
    rec = torch.zeros((count, W.RENDER_PIXEL.itemsize), dtype=torch.uint8, device="cuda:0")
    mesh = gen.mesh_create(*grid(128, 4.0))
    spray = gen.spray_create()
    material = gen.spray_material_create(*example_textures())
    opts = {"falloff": True, "cull_back": True}
    with torch.cuda.stream(stream):
        for _ in range(STEPS):
            gen.update_all(UPDATE_DELTA, params)
            gen.spray_step(spray, UPDATE_DELTA, sc)
        gen.mesh_draw_async(mesh, cam, origin, sc, rgba, rec, opts)
        gen.spray_draw_async(spray, material, cam, rgba, rec)
    stream.synchronize()
    print(f"device: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, HIP {torch.version.hip}")
    if step == "spray":
        records = np.frombuffer(rec.cpu().numpy().tobytes(), W.RENDER_PIXEL)
        st = gen.spray_draw_stats()
        frags = records["reserved"][:, 1]
        print(f"live particles {gen.spray_live_count(spray)} of {spray.amount}; billboards drawn {st['drawn']}, culled {st['culled']}; "
              f"fragments per pixel: mean {frags.mean():.4f}, max {int(frags.max())}, pixels with spray {(frags > 0).mean():.4f}; scratch {st['scratch_bytes']} B")
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    src = torch.zeros(count * PIXEL_READ, dtype=torch.uint8, device="cuda:0")
    dst = torch.zeros(count * PIXEL_READ, dtype=torch.uint8, device="cuda:0")

    def once():
        if step == "spray":
            gen.spray_draw_async(spray, material, cam, rgba, rec)
        elif step == "mesh":
            gen.mesh_draw_async(mesh, cam, origin, sc, rgba, rec, opts)
        else:
            assert hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), count * PIXEL_READ, 3, stream.cuda_stream) == 0     # device to device
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
    what = {"spray": "ow_billboard_draw_async (clear, k_billboard_setup, k_billboard_blend)", "mesh": "ow_mesh_draw_async (the four launches it composites over)",
            "copy": f"hipMemcpyAsync, device to device, {count * PIXEL_READ} B ({PIXEL_READ} B per pixel: what k_billboard_blend reads; it writes {PIXEL_WRITE})"}[step]
    print(f"{what}: median {statistics.median(us):.1f} us, min {min(us):.1f}, max {max(us):.1f} over {REPS} launches")
    gen.spray_material_destroy(material)
    gen.spray_destroy(spray)
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
    say(f"ow_billboard_draw_async at {WIDTH} x {HEIGHT}, 1024^2 x 3, the reference camera and emitter after {STEPS} steps of 1/50 s (scripts/spray_draw_time.py)")
    for k, step in enumerate(("spray", "mesh", "copy")):
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
