"""An FP64 NumPy twin of the height mist (include/ocean_waves.h ow_mist_*), written from the definition in the header's text and not from
godotoceanwaves_amd/csrc/ow_mist.h: the rays, the medium's closed form, the slices, the depth compares with what makes one ambiguous, and
the pixel.  Everything is float64 from the FP32 inputs; nothing here is rounded to FP32 on the way."""
import numpy as np

import shadow_twin as ST

HIT, MIST = 1, 256
FLIP = 1e-4             # metres: a depth compare this close to flipping is ambiguous
LN2 = 0.6931471805599453


def f32(v):
    return np.asarray(np.float32(v), np.float64)


def rays(cam_words, width, height):
    """(origin [3], unit directions [H][W][3]) of the camera whose resolved 15 floats are cam_words"""
    c = np.asarray(cam_words, np.float64)
    o, B, th, aspect = c[0:3], c[3:12].reshape(3, 3), c[12], c[13]
    i, j = np.meshgrid(np.arange(width), np.arange(height))
    x = ((2.0 * (i + 0.5)) / width - 1.0) * aspect * th
    y = (1.0 - (2.0 * (j + 0.5)) / height) * th
    local = np.stack([x, y, -np.ones_like(x)], -1)
    d = local @ B.T
    return o, d / np.linalg.norm(d, axis=-1, keepdims=True)


def phi(x):
    x = np.asarray(x, np.float64)
    safe = np.where(x > 0, x, 1.0)
    return np.where(x > 0, -np.expm1(-safe) / safe, 1.0)


def integral(k, h0, dy, t):
    """I(t): the weight w(h) = 1 for h <= 0, exp(-k h) above, along h(s) = h0 + s dy over [0, t]; per segment as length x mean weight"""
    h0, dy, t = np.broadcast_arrays(np.asarray(h0, np.float64), np.asarray(dy, np.float64), np.asarray(t, np.float64))
    h1 = h0 + t * dy
    crosses = (h0 < 0) != (h1 < 0)
    with np.errstate(all="ignore"):
        tc = np.where(crosses & (dy != 0), -h0 / np.where(dy != 0, dy, 1.0), 0.0)
    tc = np.clip(tc, 0.0, t)
    # [0, tc] on the side of h0, [tc, t] on the side of h1; without a crossing tc = 0 and the first segment is empty
    def segment(length, ha, hb):
        lo, hi = np.minimum(ha, hb), np.maximum(ha, hb)
        below = hi <= 0
        lo = np.maximum(lo, 0.0)
        return np.where(below, length, length * np.exp(-k * lo) * phi(k * (hi - lo)))
    first = np.where(crosses, segment(tc, h0, np.zeros_like(h0)), 0.0)
    second = np.where(crosses, segment(t - tc, np.zeros_like(h0), h1), segment(t, h0, h1))
    return first + second


def transmittance(extinction, k, h0, dy, t):
    return np.exp(-extinction * integral(k, h0, dy, t))


def phase(g, c):
    q = 1.0 + g * g - 2.0 * g * c
    return (1.0 - g * g) / (q * np.sqrt(q))


def lit_at(fr, depth, s, t, d, bias_m):
    """one compare per point: lit outside the footprint, beyond 2 depth_range, or where d - bias <= D"""
    n = fr["size"]
    inside = (s >= 0) & (s < n) & (t >= 0) & (t < n) & (d <= 2.0 * fr["depth_range"])
    i, j = np.clip(np.floor(s), 0, n - 1).astype(int), np.clip(np.floor(t), 0, n - 1).astype(int)
    return ~inside | (d - bias_m <= depth[j, i])


def apply(cam_words, records, options, frame=None, depth=None):
    """The pass on (H, W) records.  options: dict of the FP32 option values (sun_direction any length, slices resolved).  frame: shadow_twin's
    frame, depth: the map's [size][size] float32 depths (FLT_MAX where empty), or None for no map.  Returns a dict of color, status, A, B, S,
    shadowed (slices per pixel) and ambiguous (a pixel with a compare within FLIP metres of flipping)."""
    rec = np.asarray(records)
    H, W = rec.shape
    o, d = rays(cam_words, W, H)
    ext, k = float(f32(options["extinction"])), float(f32(options["height_falloff"])) * LN2
    base, length = float(f32(options["base_height"])), float(f32(options["length"]))
    g, sky_affect, N = float(f32(options["anisotropy"])), float(f32(options["sky_affect"])), int(options["slices"])
    sun = f32(options["sun_direction"])
    sun = sun / np.linalg.norm(sun)
    albedo, sun_color, ambient = f32(options["albedo"]), f32(options["sun_color"]), f32(options["ambient_color"])
    todo = (rec["status"] & MIST) == 0
    hit = (rec["status"] & HIT) != 0
    rt = rec["t"].astype(np.float64)
    t_end = np.where(hit, np.minimum(np.where(rt > 0, rt, 0.0), length), length)
    h0, dy = o[1] - base, d[..., 1]
    T = lambda t: transmittance(ext, k, h0, dy, t)      # noqa: E731
    A = 1.0 - T(t_end)
    B = np.zeros((H, W))
    shadowed = np.zeros((H, W), np.int64)
    ambiguous = np.zeros((H, W), bool)
    if depth is not None and frame is not None:
        D = np.asarray(depth, np.float64)
        bias_m = float(f32(options.get("shadow_bias", 0.0))) * frame["w"]
        eps_st = FLIP * frame["k"]
        for n in range(N):
            ta, tb = t_end * (n / N) ** 2, t_end * ((n + 1) / N) ** 2
            m = 0.5 * (ta + tb)
            p = o + m[..., None] * d
            s, t, dep = ST.project(frame, p)
            lit = lit_at(frame, D, s, t, dep, bias_m)
            for ds in (-eps_st, eps_st):
                for dt in (-eps_st, eps_st):
                    for dd in (-FLIP, FLIP):
                        ambiguous |= lit_at(frame, D, s + ds, t + dt, dep + dd, bias_m) != lit
            B += np.where(lit, 0.0, T(ta) - T(tb))
            shadowed += ~lit
        B = np.clip(B, 0.0, A)
    c = np.einsum("hwk,k->hw", d, sun)
    p = phase(g, c)
    S = albedo * (sun_color * (p * (A - B))[..., None] + ambient * A[..., None])
    scale = np.where(hit, 1.0, sky_affect)
    A_used, S = A * scale, S * scale[..., None]
    color = rec["color"].astype(np.float64)
    with np.errstate(all="ignore"):
        out = color * (1.0 - A_used)[..., None] + S
    out = np.where(np.isfinite(out), out, S)
    out = np.where(todo[..., None], out, color)
    return dict(color=out, status=np.where(todo, rec["status"] | MIST, rec["status"]), A=A, B=B, S=S, shadowed=np.where(todo, shadowed, 0),
                ambiguous=ambiguous & todo, t_end=t_end, ray=d)
