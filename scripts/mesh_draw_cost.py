"""The cost of ow_mesh_draw against ow_render_view at 1024^2 x 4: the clipmap fixture (tests/golden/clipmap_low_inner.npz) where main.gd
puts it for the reference camera (main.tscn:120), the falloff around the camera, at 320 x 200, 1280 x 720 and 1920 x 1080; the raster
kernel's per-lane / cooperative threshold (lane_box) swept; medians of repeated regions after a warm-up, with the spread.
    python scripts/mesh_draw_cost.py [out.txt]          the table profiles/mesh_draw_1024x4.txt holds
    python scripts/mesh_draw_cost.py trace              five draws per size and nothing else: the workload for a kernel trace"""
import os, sys, time, statistics
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from godotoceanwaves_amd.presets import UPDATE_DELTA
from godotoceanwaves_amd.wave_generator import WaveGenerator as W
from scenes import make_gen, scales_of
REF_BASIS = (-0.996195, -0.0151344, 0.0858316, 0.0, 0.984807, 0.173648, -0.0871557, 0.172987, -0.981061)
only = sys.argv[1] if len(sys.argv) > 1 else "all"
out = open(only if only not in ("all", "trace") else os.devnull, "w")
def say(*a):
    line = " ".join(str(x) for x in a); print(line, flush=True); out.write(line + "\n"); out.flush()
gen, params = make_gen(1024, [0, 1, 2, 3])
gen.run(UPDATE_DELTA, params, 4)
sc = scales_of(params)
z = np.load(os.path.join(ROOT, "tests", "golden", "clipmap_low_inner.npz"))
mesh = gen.mesh_create(z["vertices"], z["triangles"])
def region(fn, reps):
    gen.sync(); t0 = time.perf_counter()
    for _ in range(reps): fn()
    gen.sync(); return (time.perf_counter() - t0) / reps * 1e3
def measure(fn, reps, regions=7):
    for _ in range(2): fn()
    v = [region(fn, reps) for _ in range(regions)]
    return statistics.median(v), min(v), max(v)
for w, h in ((320, 200), (1280, 720), (1920, 1080)):
    cam = W.camera((0.0, 10.0, -25.0), REF_BASIS, 75.0, w, h, 4000.0)
    origin = W.clipmap_origin(cam.position, 4.0)
    rgba = torch.zeros((w * h, 4), dtype=torch.uint8, device="cuda:0")
    rec = torch.zeros((w * h, 128), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    opts = {"falloff": True}
    if only == "trace":
        for _ in range(5): gen.mesh_draw_async(mesh, cam, origin, sc, rgba, rec, opts)
        gen.sync(); continue
    gen.mesh_draw(mesh, cam, origin, sc, opts, pixels=False)
    st = gen.mesh_stats(mesh)
    say(f"{w}x{h} stats {st}")
    for lb in (0, -1, 1, 2, 8, 16, 64):
        o = dict(opts, lane_box=lb)
        med, lo, hi = measure(lambda: gen.mesh_draw_async(mesh, cam, origin, sc, rgba, rec, o), 20)
        gen.mesh_draw(mesh, cam, origin, sc, o, pixels=False); s2 = gen.mesh_stats(mesh)
        say(f"{w}x{h} mesh_draw_async rgba+records lane_box={lb:3d} median {med:.3f} ms (min {lo:.3f} max {hi:.3f}) per_lane {s2['per_lane']} cooperative {s2['cooperative']}")
    med, lo, hi = measure(lambda: gen.mesh_draw_async(mesh, cam, origin, sc, rgba, None, opts), 20)
    say(f"{w}x{h} mesh_draw_async rgba only median {med:.3f} ms (min {lo:.3f} max {hi:.3f})")
    med, lo, hi = measure(lambda: gen.mesh_draw(mesh, cam, origin, sc, opts, pixels=False), 5)
    say(f"{w}x{h} mesh_draw (host rgba, synchronous) median {med:.3f} ms (min {lo:.3f} max {hi:.3f})")
    med, lo, hi = measure(lambda: gen.render_view_async(cam, sc, rgba, rec, opts), 2, 5)
    say(f"{w}x{h} render_view_async rgba+records median {med:.3f} ms (min {lo:.3f} max {hi:.3f})")
med, lo, hi = measure(lambda: gen.mesh_displace(mesh, origin, sc, {"falloff_center": (0.0, -25.0)}), 10)
say(f"mesh_displace (vertex stage, {mesh.num_vertices} vertices, host copy, synchronous) median {med:.3f} ms (min {lo:.3f} max {hi:.3f})")
gen.mesh_destroy(mesh)
