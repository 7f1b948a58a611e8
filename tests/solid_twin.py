"""FP64 twin of the solid draw (include/ocean_waves.h ow_solid_*), written from the definition in the header and not from
godotoceanwaves_amd/csrc/ow_solid.h: numpy over whole images, one (instance, triangle) pair at a time.

A pixel is AMBIGUOUS -- set aside by the comparison -- where FP32 rounding may legitimately decide otherwise than FP64 does:
  * its centre lies within EDGE_PIXELS of the boundary of a front-facing (or, two-sided, any) triangle whose depth there is in range, or
    such a triangle's depth is within DEPTH_GAP (relative) of the near plane or of the far distance;
  * the two nearest covering pairs, or the nearest one and the background record's t, lie within DEPTH_GAP (relative) of each other.
"""
import math

import numpy as np

EDGE_PIXELS = 1e-3   # pixels
DEPTH_GAP = 1e-5     # relative: a hundred FP32 roundings
HIT, SOLID = 1, 16
DEFAULT_NEAR = 0.05
DEFAULTS = dict(color=(0.45, 0.30, 0.15), light_direction=(0.321197, 0.18296, 0.929171), light_color=(1.0, 1.0, 1.0), ambient_color=(0.05, 0.08, 0.10),
                background_color=(0.0, 0.0, 0.0))


def pixel_xy(cam):
    """x, y of every pixel's ray (x, y, -1), [H][W] each"""
    w, h = int(cam.width), int(cam.height)
    th = math.tan(math.radians(float(cam.fov_y_degrees)) / 2.0)
    aspect = w / h
    i, j = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    return (2.0 * (i + 0.5) / w - 1.0) * aspect * th, (1.0 - 2.0 * (j + 0.5) / h) * th, (2.0 / w * aspect * th, -2.0 / h * th)


def draw(vertices, triangles, transforms, cam, options=None, records=None, skip=None):
    """dict over the [H][W] image: solid (a solid is drawn), covered (some pair covers the centre, whatever the depth test says), ambiguous,
    triangle and instance (index + 1 of the winner, 0 where none is drawn), t, position, normal, color (of every pixel)"""
    o = dict(DEFAULTS)
    o.update(options or {})
    near = o.get("near", 0.0)
    near = near if near > 0.0 else DEFAULT_NEAR
    two_sided = bool(o.get("two_sided"))
    v = np.asarray(vertices, np.float32).astype(np.float64).reshape(-1, 3)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    tf = np.asarray(transforms, np.float32).astype(np.float64).reshape(-1, 12)
    h, w = int(cam.height), int(cam.width)
    x, y, (gx, gy) = pixel_xy(cam)
    rlen = np.sqrt(x * x + y * y + 1.0)
    far = float(cam.max_distance)
    cam_o = np.array(list(cam.position), np.float64)
    cam_b = np.array(list(cam.basis), np.float64).reshape(3, 3)
    light = np.asarray(o["light_direction"], np.float64)
    light = light / np.linalg.norm(light)

    best = np.full((h, w), np.inf)
    second = np.full((h, w), np.inf)
    win = np.full((h, w), -1, np.int64)
    covered = np.zeros((h, w), bool)
    ambiguous = np.zeros((h, w), bool)
    pos = np.zeros((h, w, 3))
    nrm = np.zeros((h, w, 3))
    for inst, t in enumerate(tf):
        if not np.isfinite(t).all() or (skip is not None and skip[inst]):
            continue
        world = v @ t[:9].reshape(3, 3).T + t[9:]
        view = (world - cam_o) @ cam_b           # B^T (w - o), per row
        for k, (a, b, c) in enumerate(tri):
            pair = inst * len(tri) + k
            w0, w1, w2 = world[a], world[b], world[c]
            v0, v1, v2 = view[a], view[b], view[c]
            if not (np.isfinite(world[[a, b, c]]).all() and np.isfinite(view[[a, b, c]]).all()):
                continue
            n = (np.cross(v1, v2), np.cross(v2, v0), np.cross(v0, v1))
            big_n = np.cross(v1 - v0, v2 - v0)
            det = float(v0 @ big_n)
            if det == 0.0 or (det > 0.0 and not two_sided):
                continue
            sg = -1.0 if det < 0.0 else 1.0
            e = [x * ni[0] + y * ni[1] - ni[2] for ni in n]
            rn = x * big_n[0] + y * big_n[1] - big_n[2]
            with np.errstate(divide="ignore", invalid="ignore"):
                s = det / rn
                dist = []     # the centre's signed distance to each edge, in pixels, positive inside
                for ei, ni in zip(e, n):
                    g = math.hypot(ni[0] * gx, ni[1] * gy)
                    dist.append(sg * ei / g if g > 0.0 else np.where(sg * ei >= 0.0, np.inf, -np.inf))
            m = np.minimum(np.minimum(dist[0], dist[1]), dist[2])
            in_depth = (sg * rn > 0.0) & (s > near) & (s <= far)
            hit = (m >= 0.0) & in_depth
            close = (sg * rn > 0.0) & (s > near * (1.0 - DEPTH_GAP)) & (s <= far * (1.0 + DEPTH_GAP))
            ambiguous |= (np.abs(m) < EDGE_PIXELS) & close
            ambiguous |= (m > -EDGE_PIXELS) & (sg * rn > 0.0) & ((np.abs(s - near) <= DEPTH_GAP * near) | (np.abs(s - far) <= DEPTH_GAP * far))
            covered |= hit
            d = np.where(hit, s * rlen, np.inf)
            better = d < best
            second = np.where(better, best, np.minimum(second, d))
            best = np.where(better, d, best)
            win = np.where(better, pair, win)
            if better.any():
                se = e[0] + e[1] + e[2]
                with np.errstate(divide="ignore", invalid="ignore"):
                    p = (e[0] / se)[..., None] * w0 + (e[1] / se)[..., None] * w1 + (e[2] / se)[..., None] * w2
                pos = np.where(better[..., None], p, pos)
                nn = np.cross(w1 - w0, w2 - w0)
                nn = nn / np.linalg.norm(nn) * (-1.0 if det > 0.0 else 1.0)
                nrm = np.where(better[..., None], nn, nrm)
    with np.errstate(invalid="ignore"):
        ambiguous |= covered & np.isfinite(second) & (second - best <= DEPTH_GAP * best)
    solid = covered.copy()
    color = np.empty((h, w, 3))
    color[:] = np.asarray(o["background_color"], np.float64)
    if records is not None:
        bg_hit = (records["status"] & HIT) != 0
        bg_t = records["t"].astype(np.float64)
        solid &= ~bg_hit | (best <= bg_t)
        with np.errstate(invalid="ignore"):
            ambiguous |= covered & bg_hit & (np.abs(best - bg_t) <= DEPTH_GAP * bg_t)
        color = records["color"].astype(np.float64)
    ndl = np.maximum(nrm @ light, 0.0)
    diffuse = ndl[..., None] * np.asarray(o["light_color"], np.float64)
    shaded = np.asarray(o["color"], np.float64) * (diffuse + np.asarray(o["ambient_color"], np.float64))
    color = np.where(solid[..., None], shaded, color)
    ntri = max(len(tri), 1)
    return dict(solid=solid, covered=covered, ambiguous=ambiguous, triangle=np.where(solid, win % ntri + 1, 0), instance=np.where(solid, win // ntri + 1, 0),
                t=np.where(solid, best, 0.0), position=np.where(solid[..., None], pos, 0.0), normal=np.where(solid[..., None], nrm, 0.0), color=color,
                diffuse=np.where(solid[..., None], diffuse, 0.0))


def rgba8(color):
    """(int)(clamp(c, 0, 1) * 255 + 0.5) per channel in FP32, alpha 255: ow_render_view's packing"""
    c = np.asarray(color, np.float32)
    v = np.where(c > 0, np.where(c < 1, c, np.float32(1)), np.float32(0)).astype(np.float32)
    out = np.full(c.shape[:-1] + (4,), 255, np.uint8)
    out[..., :3] = (v * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)
    return out
