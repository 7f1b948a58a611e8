"""The comparisons that carry assertions, and the interface checks every feature makes of its part of include/ocean_waves.h, each written
once: what differs per feature (names, phrases, expected sizes) is passed in by the feature's test."""
import math
import os
import re
import subprocess

import numpy as np

import helpers as H
import query_twin
import render_twin
from cpu_builds import cpu_query, ROOT
from device_maps import DISP_REPORTED, half_to_f32, NORM_REPORTED
from godotoceanwaves_amd import _lib
from godotoceanwaves_amd.wave_generator import WaveGenerator as W
from scenes import BELOW, DEFAULTS, G, HIT, NO_TRIANGLE, RAY_TOL, RHO, slope_factor, TRUNC, uniforms_of, unit
from velocity_twin import phases, velocity_twin

HEADER = open(os.path.join(ROOT, "include", "ocean_waves.h")).read()


def fp32_slack(disp, scales, p):
    """how far an FP32 evaluation of |p + f D_xz(p) - q| may sit from the FP64 one at the same p: the texture coordinate p * s * N is
    rounded twice (2^-23 relative), which moves each cascade's interpolant by that many texels times its largest texel step, plus the
    rounding of the position and of the sums (a few ulp of |p| and of |D|)"""
    d = query_twin.as_f64(disp)
    sc = np.asarray(scales, np.float64)
    n = d.shape[1]
    r = np.abs(np.asarray(p, np.float64)).max(axis=1)
    per_texel = sum(sc[i, 2] * max(np.abs(np.diff(d[i][..., [0, 2]], axis=a)).max() for a in (0, 1)) for i in range(len(sc)))
    return 2e-5 + r * 2.0 ** -21 + r * sc[:, :2].max() * n * 2.0 ** -22 * per_texel


def check_against_twin(out, disp, scales, xz, tol=1e-3, center=None):
    assert all(np.isfinite(out[f]).all() for f in ("p", "residual", "falloff", "height", "normal"))
    assert all(np.isfinite(out["sample"][f]).all() for f in ("displacement", "gradient", "gradient_scaled", "foam", "gradient_fragment"))
    r64 = query_twin.residual(disp, scales, out["p"], xz, center)
    slack = fp32_slack(disp, scales, out["p"])
    c = out["converged"].astype(bool)
    assert (r64[c] <= tol + slack[c]).all(), (r64[c] - tol - slack[c]).max()
    assert (out["residual"][c] <= tol).all()
    assert (out["residual"][~c] > tol).all()
    assert (np.abs(out["residual"][~c] - r64[~c]) <= slack[~c]).all()
    assert np.array_equal(out["world_xz"], np.asarray(xz, np.float32))
    return c


def assert_same_records(got, want, what):
    for f in got.dtype.names:
        assert got[f].tobytes() == want[f].tobytes(), (what, f)


def check_records(L, qh, d, m, sc, rays, out, options=None):
    """what every record holds: no NaN / Inf, the embedded query is harness_query's at the hit bit for bit, the residual is g there,
    the position is o + t d^, and zeros without a hit"""
    o = dict(options or {})
    for f in ("t", "position", "residual", "slab_half_height", "t_enter", "t_exit"):
        assert np.isfinite(out[f]).all(), f
    hit = (out["status"] & HIT) != 0
    if hit.any():
        pos = out["position"][hit]
        want = cpu_query(qh, d, m, sc, pos[:, [0, 2]], max_iterations=o.get("max_iterations", 0), tolerance=o.get("query_tolerance", 0.0),
                         falloff_center=o.get("falloff_center"))
        assert out["query"][hit].tobytes() == want.tobytes()
        wl = np.float32(o.get("water_level", 0.0))
        assert np.array_equal(out["residual"][hit], pos[:, 1] - (wl + want["height"]))
        dn = unit(rays["direction"][hit])
        assert np.array_equal(pos, rays["origin"][hit] + out["t"][hit][:, None] * dn)
        assert ((out["t"][hit] >= out["t_enter"][hit]) & (out["t"][hit] <= out["t_exit"][hit])).all()
    assert not out[~hit]["query"].tobytes().strip(b"\0")
    assert (out["t"][~hit] == 0).all() and (out["residual"][~hit] == 0).all()
    return hit


def check_texel_centres(out, disp, norm):
    """ow_sample_surface records at the centres of every texel of one 128^2 cascade with map scales (1/128, 1/128, 1, 1), row by row: both
    weights are 0, so the displacement, the plain gradient and the plain foam are the texel's own half-words widened, by value (a -0 may
    come back as +0: a + b * 0 with b * 0 = +0).  Returns the patterns that came back so."""
    d, m = np.asarray(disp, np.uint16).reshape(-1, 4), np.asarray(norm, np.uint16).reshape(-1, 4)
    assert len(out) == len(d) == len(m)
    got = np.concatenate([out["displacement"], out["gradient"], out["foam"][:, None]], axis=1)
    bits = np.concatenate([d[:, DISP_REPORTED], m[:, NORM_REPORTED]], axis=1)
    same = got == half_to_f32(bits)
    assert same.all(), (bits[~same][:8], got[~same][:8])
    return np.unique(bits[same])


def check_calm_hits(out, rays, h):
    """scenes.calm_hit_rays over a calm sea: every ray hits at the analytic t = h / -d^.y within the ray tolerance, on the slab's floor"""
    assert (out["status"] == HIT).all()
    dn = unit(rays["direction"]).astype(np.float64)
    t_star = h / -dn[:, 1]
    assert np.abs(out["t"] - t_star).max() <= RAY_TOL + 1e-6 * t_star.max()
    assert (np.abs(out["residual"]) <= RAY_TOL * slope_factor(dn, 0.0) + 1e-5).all()
    assert (out["slab_half_height"] == np.float32(0.01)).all() and (out["query"]["height"] == 0).all()
    assert (out["rounds"] <= 1 + 4).all() and (out["samples"] >= 2).all()


def check_calm_misses(out, wl):
    """scenes.calm_miss_rays over a calm sea at water level wl = -0.5, cast with max_samples = 64"""
    assert wl == -0.5
    st = out["status"]
    assert st[0] == 0 and out["samples"][0] == 0                   # upward from above the slab: never enters it
    assert st[1] == 0 and out["samples"][1] == 0                   # horizontal, above the slab
    assert st[2] == HIT and abs(out["t"][2] - 5.5 * np.sqrt(2)) <= RAY_TOL
    assert st[3] == 0 and out["samples"][3] == 0                   # horizontal, just above the slab (0.01 m)
    assert st[4] == HIT | BELOW and abs(out["t"][4] - 2.5 * np.sqrt(2)) <= RAY_TOL   # from below, surfacing
    assert st[5] == BELOW and out["samples"][5] == 0               # from below, going down: never enters the slab
    assert st[6] == BELOW | TRUNC and out["samples"][6] == 64 and out["rounds"][6] == 1   # inside the slab, horizontal, 5 km
    assert st[7] == 0 and out["samples"][7] == 0                   # stops 10 m short of the water
    assert st[8] == BELOW | TRUNC                                  # on the plane: g = 0 is not above; 100 m is 401 samples


def buoyancy_twin(disp, scales, bodies, hull, p, options=None):
    """The model restated in FP64 with NumPy at the undisplaced points p the solver found: per-body force, torque and submerged volume"""
    o = dict(options or {})
    rho, g, wl = o.get("density", RHO), o.get("gravity", G), o.get("water_level", 0.0)
    F = np.zeros((len(bodies), 3))
    Tq = np.zeros((len(bodies), 3))
    SV = np.zeros(len(bodies))
    H = query_twin.displacement(disp, scales, p)[:, 1] * query_twin.falloff(p, o.get("falloff_center"))
    for b, body in enumerate(bodies):
        sl = slice(body["point_offset"], body["point_offset"] + body["point_count"])
        B = body["transform"][:9].astype(np.float64).reshape(3, 3)
        org = body["transform"][9:].astype(np.float64)
        r = hull[sl]["local"].astype(np.float64) @ B.T
        w = r + org
        d = wl + H[sl] - w[:, 1]
        hh = hull[sl]["half_height"].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            s = np.where(hh > 0, np.clip((d + hh) / (2 * hh), 0, 1), (d > 0).astype(np.float64))
        sv = hull[sl]["volume"].astype(np.float64) * s
        u = body["linear_velocity"].astype(np.float64) + np.cross(body["angular_velocity"].astype(np.float64), r)
        un = np.linalg.norm(u, axis=1)
        drag = (rho * sv)[:, None] * (float(body["linear_drag"]) * u + float(body["quadratic_drag"]) * un[:, None] * u)
        f = -drag
        f[:, 1] += rho * g * sv
        F[b], Tq[b], SV[b] = f.sum(0), np.cross(r, f).sum(0), sv.sum()
    return F, Tq, SV


VELOCITY_FLOOR = 2e-5


def check_layer(gen, i, floor=VELOCITY_FLOOR, m=None, calm=False):
    """layer i of V against the twin at the layer's own words; returns the worst ratio to the allowance.
    floor: the record's floor where it is not FLOOR (tests/test_velocity_layers.py); m: the twin's unit phasors as a function of the FP32
    phases (the long-session cases); calm: a sea whose layer may lie below FP16's range -- no non-triviality check"""
    got = gen.velocity_map(i)
    h0, om = gen.get_spectrum(i)
    _, mod, _ = gen.get_push_constants(i)
    want = velocity_twin(h0, om, mod, m=None if m is None else m(phases(om, mod)))
    assert np.all(got[..., 3].view(np.uint16) == 0)
    assert np.isfinite(got.astype(np.float32)).all()
    r = H.fp16_close(got[..., :3], want.astype(np.float16), ulps=1, rel_floor=floor)
    assert r <= 1.0, (i, r)
    assert calm or np.abs(want).max() > 1e-3  # the layer is not trivially zero
    return r


def check_composite(rgba, rec, options=None):
    """what every image holds: finite records, sky without a hit, the composite and the RGBA8 rule"""
    for f in W.RENDER_PIXEL.names:
        if f not in ("status", "reserved"):
            assert np.isfinite(rec[f]).all(), f
    hit = (rec["status"] & HIT) != 0
    sky = np.asarray(dict(DEFAULTS, **(options or {}))["sky_color"], np.float32)
    amb = np.asarray(dict(DEFAULTS, **(options or {}))["ambient_color"], np.float32)
    assert (rec["color"][~hit] == sky).all()
    zeroed = rec[~hit].copy()
    zeroed["status"] = 0
    zeroed["color"] = 0
    assert not zeroed.tobytes().strip(b"\0")
    want = rec["albedo"] * (rec["diffuse"] + amb) + rec["specular"][..., None]
    assert np.array_equal(rec["color"][hit], want[hit])
    assert np.array_equal(rgba, render_twin.rgba8(rec["color"]))
    assert not rec["reserved"].any()
    return hit


def check_picture(pic, num_triangles, options=None):
    """check_composite's rules -- finite records, sky and zeros without a hit, the composite, the RGBA8 rule -- with
    reserved[0] the triangle's index + 1, and the counters adding up"""
    rgba, rec, vis = pic["rgba"], pic["rec"], pic["vis"]
    for f in W.RENDER_PIXEL.names:
        if f not in ("status", "reserved"):
            assert np.isfinite(rec[f]).all(), f
    hit = (rec["status"] & HIT) != 0
    o = dict(DEFAULTS, **{k: v for k, v in (options or {}).items() if k in DEFAULTS})
    sky, amb = np.asarray(o["sky_color"], np.float32), np.asarray(o["ambient_color"], np.float32)
    assert (rec["color"][~hit] == sky).all()
    zeroed = rec[~hit].copy()
    zeroed["status"] = 0
    zeroed["color"] = 0
    assert not zeroed.tobytes().strip(b"\0")
    want = rec["albedo"] * (rec["diffuse"] + amb) + rec["specular"][..., None]
    assert np.array_equal(rec["color"][hit], want[hit])
    assert np.array_equal(rgba, render_twin.rgba8(rec["color"]))
    assert not rec["reserved"][..., 1:].any()
    assert np.array_equal(hit, vis != NO_TRIANGLE)
    assert np.array_equal(rec["reserved"][..., 0][hit], (vis[hit] & np.uint64(0xFFFFFFFF)).astype(np.uint32) + 1) and not rec["reserved"][..., 0][~hit].any()
    assert (rec["reserved"][..., 0] <= num_triangles).all()
    assert int(pic["counters"].sum()) == num_triangles, pic["counters"]
    return hit


def calm_plane(cam, near, half=32.0):
    """a camera over the square |x|, |z| <= half of the plane y = 0, in FP64: per pixel the ray's t to the plane (inf where it does not go
    down) and the point there, whether the pixel is asked (its ray passes more than 1e-4 m from the square's edge, the near plane and
    max_distance) and whether it has a hit"""
    o = np.asarray(list(cam.position), np.float64)
    dirs = render_twin.pixel_directions(list(cam.basis), cam.fov_y_degrees, cam.width, cam.height)
    fwd = -np.asarray(list(cam.basis), np.float64).reshape(3, 3)[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(dirs[..., 1] < 0, -o[1] / dirs[..., 1], np.inf)
        pos = o + t[..., None] * dirs
        depth = t * (dirs @ fwd)
    finite = np.isfinite(t)
    margin = np.where(finite, np.minimum.reduce([half - np.abs(pos[..., 0]), half - np.abs(pos[..., 2]), depth - near, cam.max_distance - depth]), -1.0)
    asked = ~finite | (np.abs(margin) > 1e-4)
    want = finite & (margin > 0)
    return t, pos, asked, want


def assert_same_picture(got, want, what):
    """a mesh draw (scenes.gpu_mesh_draw, cpu_builds.cpu_mesh_draw): vertex records, visibility words, pixel records, RGBA and counters"""
    for f in W.MESH_VERTEX.names:
        assert got["vertices"][f].tobytes() == want["vertices"][f].tobytes(), (what, "vertex", f)
    assert got["vis"].tobytes() == want["vis"].tobytes(), (what, "visibility words")
    for f in W.RENDER_PIXEL.names:
        assert got["rec"][f].tobytes() == want["rec"][f].tobytes(), (what, f)
    assert got["rgba"].tobytes() == want["rgba"].tobytes(), what
    assert list(got["counters"]) == list(want["counters"]), what


SHADE_TOL = H.TOL_F32   # 1e-4: the project's FP32 parity tolerance


def compare_with_twin(rec, cam, options):
    """every hit pixel against the twin fed the record's own inputs; absolute for the terms bounded by 1, relative to max(1, |twin|) for
    diffuse and specular.  Returns the largest error per term."""
    hit = (rec["status"] & HIT) != 0
    r = rec[hit]
    twin = render_twin.shade(r["gradient_fragment"], r["foam_fragment"], r["wave_height"], r["position"], list(cam.position), list(cam.basis),
                    uniforms_of(options))
    worst = {}
    for k in ("foam_factor", "albedo", "normal", "fresnel", "roughness", "color", "diffuse", "specular"):
        assert np.isfinite(twin[k]).all(), k
        err = np.abs(r[k].astype(np.float64) - twin[k])
        if k in ("diffuse", "specular"):
            err = err / np.maximum(1.0, np.abs(twin[k]))
        worst[k] = float(err.max())
    return worst, int(hit.sum())


def assert_same_image(got, want, what):
    (g_rgba, g_rec), (w_rgba, w_rec) = got, want
    for f in W.RENDER_PIXEL.names:
        assert g_rec[f].tobytes() == w_rec[f].tobytes(), (what, f)
    assert g_rgba.tobytes() == w_rgba.tobytes(), what


def same_picture(a, b, what):
    assert a["rgba"].tobytes() == b["rgba"].tobytes(), what
    if a["rec"] is not None or b["rec"] is not None:
        for f in W.RENDER_PIXEL.names:
            assert a["rec"][f].tobytes() == b["rec"][f].tobytes(), (what, f)


def same_records(a, b, what):
    for f in W.RENDER_PIXEL.names:
        assert a[f].tobytes() == b[f].tobytes(), (what, f)


def fnv1a(b):
    h = 1469598103934665603
    for x in np.frombuffer(b, np.uint8).tolist():
        h = ((h ^ x) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def mirror_schedule(n, frames):
    """the schedule of examples/c_consumer.c / examples/wave_generator_host.cpp through the Python mirror:
    (layers handed off, checksum, surface samples along the 64-point line)"""
    from godotoceanwaves_amd import WaveCascadeParameters, WaveGenerator
    tile, wind, dirs = [88.0, 57.0, 16.0], [10.0, 5.0, 20.0], [20.0, 15.0, 20.0]
    fetch, spread, whitecap, foam = [150.0, 150.0, 550.0], [0.2, 0.4, 0.4], [0.5, 0.5, 0.25], [8.0, 0.0, 3.0]
    params = [WaveCascadeParameters(tile_length=(tile[i], tile[i]), wind_speed=wind[i], wind_direction=dirs[i], fetch_length=fetch[i],
                                    spread=spread[i], whitecap=whitecap[i], foam_amount=foam[i],
                                    spectrum_seed=(1000 + 17 * i, -2000 + 31 * i), time=120.0 + math.pi * i) for i in range(3)]
    gen = WaveGenerator()
    gen.map_size = n
    gen.init_gpu(3)
    total, in_flight, handed = 0, -1, 0

    def take(layer):
        d, m = gen.readback_wait(layer)
        return (fnv1a(d.tobytes()) + 31 * fnv1a(m.tobytes()) + layer) & 0xFFFFFFFFFFFFFFFF

    for _ in range(frames):
        if gen.pass_num_cascades_remaining == 0:
            gen.update(1.0 / 50.0, params)
        if in_flight >= 0:
            total ^= take(in_flight)
            handed += 1
        layer = gen.pass_num_cascades_remaining - 1
        gen._process()
        gen.readback_begin([layer])
        in_flight = layer
    total ^= take(in_flight)
    handed += 1
    xz = np.stack([-40.0 + 1.25 * np.arange(64), 7.5 + 0.5 * np.arange(64)], axis=1).astype(np.float32)
    return handed, total, gen.sample_surface(xz, [(1 / t, 1 / t, 1.0, 1.0) for t in tile])


def check_against_mirror(stdout, n, frames):
    out = dict(kv.split("=") for kv in stdout.split())
    handed, total, s = mirror_schedule(n, frames)
    assert int(out["layers_handed_off"]) == handed == frames
    assert int(out["checksum"], 16) == total
    lo, hi = out["wave_height"].strip("[]").split(",")
    assert abs(float(lo) - float(s["displacement"][:, 1].min())) < 1e-4 and abs(float(hi) - float(s["displacement"][:, 1].max())) < 1e-4
    assert int(out["spray_active"]) == int(s["spray_active"].sum())
    if "spectra_generated" in out:   # (examples/c_consumer.c asks ow_spectrum_stats: one spectrum per cascade, none regenerated)
        assert int(out["spectra_generated"]) == 3 and int(out["spectra_skipped"]) == 0


DOC = open(os.path.join(ROOT, "INTEGRATION.md")).read()


SHIM = DOC.split("## 2. C# (P/Invoke)")[1].split("## 3. Plain C")[0]


C_SIZES = {"float": 4, "double": 8, "int32_t": 4, "uint32_t": 4, "void *": 8, "size_t": 8, "uint64_t": 8}


CS_SIZES = {"float": 4, "double": 8, "int": 4, "uint": 4, "IntPtr": 8, "nuint": 8, "ulong": 8}


def strip_comments(text):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def c_functions():
    """name -> (return type, number of parameters) for every function the header declares"""
    out = {}
    for m in re.finditer(r"^([A-Za-z_][A-Za-z0-9_ \*]*?)\b(ow_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", strip_comments(HEADER), flags=re.M | re.S):
        ret, name, args = m.group(1).strip(), m.group(2), " ".join(m.group(3).split())
        out[name] = (ret, 0 if args in ("", "void") else args.count(",") + 1)
    return out


def c_struct_fields(name):
    body = re.search(r"typedef struct %s \{(.*?)\}\s*%s\s*;" % (name, name), strip_comments(HEADER), flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        m = re.match(r"(void \*|[A-Za-z_][A-Za-z0-9_]*)\s*(.*)$", decl)
        ctype, names = m.group(1), m.group(2)
        for n in names.split(","):
            d = re.match(r"\s*([A-Za-z_][A-Za-z0-9_]*)(\[(\w+)\])?\s*$", n)
            count = d.group(3)
            if count is not None and not count.isdigit():
                count = re.search(r"#define %s (\d+)" % count, HEADER).group(1)
            fields.append((d.group(1), C_SIZES[ctype] * int(count or 1)))
    return fields


def cs_struct_fields(name):
    body = re.search(r"struct %s \{(.*?)\n\}" % name, strip_comments(SHIM), flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.replace("public", "").split())
        if not decl:
            continue
        fixed = decl.startswith("fixed ")
        decl = decl[len("fixed "):] if fixed else decl
        ctype, names = decl.split(" ", 1)
        for n in names.split(","):
            m = re.match(r"\s*([A-Za-z_][A-Za-z0-9_]*)(\[(\d+)\])?\s*$", n)
            fields.append((m.group(1), CS_SIZES[ctype] * int(m.group(3) or 1)))
    return fields


def check_declared_and_bound(lib, names):
    """the header declares each function outside its comments, the ctypes table has it and the loaded library resolves it; returns the
    header without its block comments, for the checks a feature adds"""
    text = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES
        assert getattr(lib, name)
    return text


def exported_symbols():
    """the ow_* functions the built library exports"""
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    return set(re.findall(r" T (ow_[a-z0-9_]+)", out))


def check_csharp_binds(names, returns=r"\w+", indexed=True):
    """the C# text binds each function (with this return type) and, where `indexed`, section 7's index names it"""
    for name in names:
        assert re.search(r"\[DllImport\(Lib\)\]\s*public static extern %s %s\(" % (returns, name), SHIM), name
        if indexed:
            assert "`%s`" % name in DOC.split("## 7. Index")[1], name
