"""An FP64 twin of the floating bodies' reflections, written from the definition in include/ocean_waves.h and the header text of
godotoceanwaves_amd/csrc/ow_mirror.h: the sky pass's twin (tests/sky_light_twin.py) up to radiance, the ray cast's brute-force twin
(tests/solid_cast_twin.py) for the mirror ray of every casting record, the body's colour, the fade, the mix, and the rest of the sky pass.
The mirror ray is the record's FP32 position and the twin's own mirror direction narrowed to FP32 (the definition's ray is an FP32 ray)."""
import numpy as np

import sky_light_twin as SL
import solid_cast_twin as SC
from scenes import W

HIT, MIRROR = 1, 512
FLT_MAX = 3.4028234663852886e38


def mirror(records, cam_words, opts, pyr, shape, tf, flags=None):
    """opts: the option record's values (FP32 values as Python numbers, two_sided a bool).  dict of color [H][W][3] (float64), status, cast
    (the records that cast), hit, pair (instance * triangles + triangle, -1 without a hit), t64, unambiguous, body (C), weight, radiance (radiance'
    where a body is mirrored) and rays (the RAY records of the casting records, in row-major order)"""
    h, w = records.shape
    sky = SL.sky_light(records, cam_words, opts, pyr)
    tf = np.ascontiguousarray(tf, np.float32).reshape(-1, 12)
    nt = len(np.asarray(shape[1]).reshape(-1, 3))
    cast = sky["mirror"] & (len(tf) > 0)
    out = dict(cast=cast, hit=np.zeros((h, w), bool), pair=np.full((h, w), -1), t64=np.zeros((h, w)), unambiguous=np.ones((h, w), bool),
               body=np.zeros((h, w, 3)), weight=np.zeros((h, w)), radiance=sky["radiance"].copy(), sky=sky)
    status = sky["status"].copy()
    if cast.any():
        rays = W.rays(records["position"][cast], sky["reflect"][cast].astype(np.float32), float(opts["max_distance"]))
        c = SC.cast(shape, tf, rays, two_sided=bool(opts.get("two_sided")), flags=flags)
        out["rays"] = rays
        n = c["normal"]
        light = np.float64(opts["light_direction"])
        light = (light / np.linalg.norm(light)).astype(np.float32).astype(np.float64)
        ndl = np.maximum(n @ light, 0.0)
        e = SL.tap(pyr["E"], np.where(c["hit"][:, None], n, np.array([0.0, 1.0, 0.0])))
        body = np.float64(opts["body_color"]) * ((np.float64(opts["light_color"]) * ndl[:, None] + np.float64(opts["ambient_color"])) + e * float(opts["ambient_energy"]))
        T, fb = float(opts["max_distance"]), float(opts["fade_begin"])
        fade = np.where(c["t64"] <= fb, 1.0, (T - c["t64"]) / (T - fb))
        wgt = float(opts["opacity"]) * fade
        ok = c["hit"] & np.isfinite(body).all(axis=1) & (np.abs(body) <= FLT_MAX).all(axis=1)
        rad = sky["radiance"][cast]
        rad = np.where(ok[:, None], rad * (1.0 - wgt[:, None]) + body * wgt[:, None], rad)
        out["radiance"][cast] = rad
        out["hit"][cast] = c["hit"]
        out["pair"][cast] = np.where(c["hit"], c["instance"] * nt + c["triangle"], -1)
        out["t64"][cast] = c["t64"]
        out["unambiguous"][cast] = c["unambiguous"]
        out["body"][cast] = np.where(ok[:, None], body, 0.0)
        out["weight"][cast] = np.where(ok, wgt, 0.0)
        st = status[cast]
        status[cast] = np.where(ok, st | MIRROR, st)
    # the rest of the sky pass on radiance'
    env = sky["env"]
    f0 = 0.16 * float(opts["specular"]) ** 2
    scale = env[..., 0] * f0 + env[..., 1] * min(max(50.0 * f0, 0.0), 1.0)
    spec = np.where(sky["mirror"][..., None], out["radiance"] * scale[..., None] * float(opts["reflection_energy"]), 0.0)
    color = records["color"].astype(np.float64)
    col = color + sky["ambient"] + spec
    col = np.where(np.isfinite(col) & (np.abs(col) <= FLT_MAX), col, color)
    out["color"] = np.where(sky["todo"][..., None], col, color)
    out["status"] = status
    out["spec"] = spec
    return out


def pair_t(shape, tf, ray, pair):
    """the FP64 t of one (instance, triangle) pair along one RAY record, from the FP32 world vertices and p_k = w_k - o in FP32"""
    v, tri = np.ascontiguousarray(shape[0], np.float32).reshape(-1, 3), np.ascontiguousarray(shape[1], np.int32).reshape(-1, 3)
    nt = len(tri)
    wv = SC.world_vertices(v, np.ascontiguousarray(tf, np.float32).reshape(-1, 12)[pair // nt][None])[0][tri[pair % nt]]
    o = ray["origin"].astype(np.float32)
    p = (wv - o[None]).astype(np.float64)
    d = SC.unit(ray["direction"][None])[0].astype(np.float64)
    N = SC.cross(p[1] - p[0], p[2] - p[0])
    return float(SC.dot(p[0], N) / SC.dot(d, N))
