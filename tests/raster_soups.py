"""Triangle soups for the shared walk of the three triangle draws (csrc/ow_raster.h raster_wave under k_mesh_raster, k_solid_raster and
k_shadow_raster), and the three draws behind one set of calls.  tests/test_raster_edges.py holds the boxed CPU builds and the device to
the brute-force passes of the harnesses (harness_*_cover_all) on them.

Everything is placed where a test wants it: the maps are zero, so a vertex's world position is its local position; the camera stands at
the origin with the identity basis and a 90 degree field of view, so view space is world space and pixel (u, v) at view depth z is
X = (u - W / 2) z / (H / 2), Y = (H / 2 - v) z / (H / 2), Z = -z; the light shines straight down on a frame of half_extent = size / 2
about the origin, so texel (s, t) at light depth d is X = s - size / 2, Z = size / 2 - t, Y = depth_range - d.  A soup is written in
these raster units -- [T][3][3] of (u, v, depth), the centre of pixel or texel i at i + 0.5 -- and placed by a target; the families that
reach behind the camera are written in view space.  A case is a placed soup V [T][3][3] float32 and the origins [n][3] it is drawn at:
instances for the solid draw and the cast, copies for the mesh, pair n T + t either way.  Seeds are fixed.

Nothing here asserts about the code under test and nothing here builds."""
import numpy as np

from cpu_builds import cpu_mesh_draw, cpu_shadow_cast, cpu_solid_draw
from scenes import bare_context, blank_records, gpu_mesh_draw, level_camera, NEAR, NO_TRIANGLE

FAR = 200.0                       # the camera's max_distance
DEPTH_RANGE = 50.0                # the frame's: depths are cast up to 100
PICTURES = ((1, 1), (8, 8), (9, 7), (37, 21), (64, 40), (160, 96))
MAPS = (16, 64, 257)
LANE_BOXES = (0, -1, 1, 64)       # the default (4), everything to the wave, one centre, everything to its lane
ZERO_N = 128
ZERO_MAPS = np.zeros((1, ZERO_N, ZERO_N, 4), np.uint16)
ZERO_SCALES = np.array([(1 / 64.0, 1 / 64.0, 1.0, 1.0)], np.float32)
LANE, WAVE = 2, 3                 # a set-up's kind: ow_mesh.h kTriLane, kTriWave and ow_shadow.h's
ONE_ORIGIN = np.zeros((1, 3), np.float32)
SHADOW_EMPTY = 0x7f7fffff


# ---- the three draws -------------------------------------------------------------------------------------------------------------------------

def soup(V):
    V = np.ascontiguousarray(V, np.float32).reshape(-1, 3, 3)
    return V.reshape(-1, 3), np.arange(3 * len(V), dtype=np.int32).reshape(-1, 3)


def translations(origins):
    tf = np.zeros((len(origins), 12), np.float32)
    tf[:, 0] = tf[:, 4] = tf[:, 8] = 1.0
    tf[:, 9:] = origins
    return tf


class BareContext:
    """a context whose maps are never read: the solid draw's and the cast's"""

    def __init__(self):
        self.gen = bare_context()

    def free(self):
        self.gen.free()


class Picture:
    """the camera's side: what the mesh and the solid draw share"""
    sizes = PICTURES
    odd, large = (37, 21), (160, 96)              # no multiple of 8 either way; room for a box of 65 centres
    tie_size = (37, 21)
    empty = NO_TRIANGLE

    def place(self, P, size):
        P = np.asarray(P, np.float64)
        w, h = size
        z = P[..., 2]
        return np.stack([(P[..., 0] - w / 2) / (h / 2) * z, (h / 2 - P[..., 1]) / (h / 2) * z, -z], -1).astype(np.float32)

    def shift(self, sideways, nearer):
        return (sideways, 0.0, nearer)            # towards the camera: the view depth falls

    def depths(self):
        return 2.2 * NEAR, 0.45 * FAR

    def camera(self, size):
        return level_camera(size[0], size[1], fov=90.0, max_distance=FAR)


class Mesh(Picture):
    name = "mesh"

    def flat(self, V, origins):
        """the copies one after the other, each vertex l + o in FP32: solid_world's sum under a translation"""
        V, o = np.asarray(V, np.float32), np.asarray(origins, np.float32)
        return (V[None] + o[:, None, None, :]).astype(np.float32).reshape(-1, 3, 3)

    def cpu(self, L, V, origins, size, lane_box, brute=False):
        out = cpu_mesh_draw(L, ZERO_MAPS, ZERO_MAPS, ZERO_SCALES, soup(self.flat(V, origins)), (0.0, 0.0, 0.0), self.camera(size), {"lane_box": lane_box}, brute)
        if brute == "setups":
            return out
        out.update(words=out["vis"], lane=int(out["counters"][2]), wave=int(out["counters"][3]), drawn=int(out["counters"][2] + out["counters"][3]))
        return out

    def context(self):
        from device_maps import written_context
        return written_context(ZERO_N, 1)

    def gpu(self, ctx, V, origins, size, lane_box):
        handle = ctx.gen.mesh_create(*soup(self.flat(V, origins)))
        out = gpu_mesh_draw(ctx.gen, handle, self.camera(size), (0.0, 0.0, 0.0), ZERO_SCALES, {"lane_box": lane_box})
        ctx.gen.mesh_destroy(handle)
        out.update(words=out["vis"], drawn=int(out["counters"][2] + out["counters"][3]))
        return out


class Solid(Picture):
    name = "solid"

    def cpu(self, L, V, origins, size, lane_box, brute=False):
        cam = self.camera(size)
        out = cpu_solid_draw(L, soup(V), translations(origins), cam, {"two_sided": True, "lane_box": lane_box}, blank_records(cam), brute=brute)
        if brute != "setups":
            out.update(words=out["vis"])
        return out

    def context(self):
        return BareContext()

    def gpu(self, ctx, V, origins, size, lane_box):
        """the draw keeps its visibility words to itself: the records carry them (t is the depth along the ray, reserved the pair)"""
        cam = self.camera(size)
        h = ctx.gen.solid_create(*soup(V))
        rgba, rec = ctx.gen.solid_draw_instances(h, translations(origins), cam, {"two_sided": True, "lane_box": lane_box}, pixels=blank_records(cam))
        st = ctx.gen.solid_draw_stats()
        ctx.gen.solid_destroy(h)
        return dict(rgba=rgba, rec=rec, words=None, drawn=st["drawn"])


class Shadow:
    name = "shadow"
    sizes = tuple((s, s) for s in MAPS)
    odd, large = (257, 257), (257, 257)
    tie_size = (64, 64)
    empty = np.uint64(SHADOW_EMPTY)

    def place(self, P, size):
        P = np.asarray(P, np.float64)
        return np.stack([P[..., 0] - size[0] / 2, DEPTH_RANGE - P[..., 2], size[0] / 2 - P[..., 1]], -1).astype(np.float32)

    def shift(self, sideways, nearer):
        return (sideways, nearer, 0.0)            # towards the light: the light depth falls

    def depths(self):
        return 1.0, 1.9 * DEPTH_RANGE

    def frame(self, size, lane_box):
        return dict(light_direction=(0.0, 1.0, 0.0), half_extent=size[0] / 2, depth_range=DEPTH_RANGE, center=(0.0, 0.0, 0.0), cast_both_sides=True,
                    lane_box=lane_box)

    def cpu(self, L, V, origins, size, lane_box, brute=False):
        out = cpu_shadow_cast(L, self.frame(size, lane_box), size[0], soup(V), translations(origins), brute)
        if brute != "setups":
            out.update(words=out["map"].astype(np.uint64), rec=None, rgba=None)
        return out

    context = Solid.context

    def gpu(self, ctx, V, origins, size, lane_box):
        m, solid = ctx.gen.shadow_map_create(size[0]), ctx.gen.solid_create(*soup(V))
        ctx.gen.shadow_map_begin(m, self.frame(size, lane_box))
        ctx.gen.shadow_map_cast_instances(m, solid, translations(origins))
        words, st = ctx.gen.shadow_map_read(m).view(np.uint32).astype(np.uint64), ctx.gen.shadow_stats(m)
        ctx.gen.solid_destroy(solid)
        ctx.gen.shadow_map_destroy(m)
        return dict(words=words, rec=None, rgba=None, drawn=st["drawn"])


TARGETS = {t.name: t for t in (Mesh(), Solid(), Shadow())}


# ---- random soups ----------------------------------------------------------------------------------------------------------------------------

def log_uniform(rng, lo, hi, shape):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), shape))


def scattered(rng, count, size, depth_lo, depth_hi, side_lo=0.01, side_hi=None, centre=(-0.25, 1.25)):
    """raster units: centres over the picture and a quarter of it around, sides from a hundredth of a centre's spacing to four pictures,
    vertex depths within a factor of two of a log-uniform one"""
    w, h = size
    side = log_uniform(rng, side_lo, side_hi or 4.0 * max(w, h), (count, 1, 1))
    c = np.stack([rng.uniform(centre[0] * w, centre[1] * w, count), rng.uniform(centre[0] * h, centre[1] * h, count)], -1)[:, None, :]
    uv = c + side * rng.uniform(-1.0, 1.0, (count, 3, 2))
    d = log_uniform(rng, depth_lo, depth_hi, (count, 1)) * rng.uniform(0.5, 2.0, (count, 3))
    return np.concatenate([uv, d[..., None]], -1)


def ulps(value, k):
    """float32 `value` moved k units in the last place"""
    bits = np.full(np.shape(k), np.float32(value)).view(np.int32) + np.asarray(k, np.int32)
    return bits.view(np.float32)


def view_families(rng, count, size):
    """the camera's: in front at any size (some beyond max_distance), across the near plane or the camera, vertices within 4 ulp of
    near, vertices within 4 ulp of max_distance, and slivers seen nearly edge-on; placed, [count][3][3] float32 each"""
    pic = TARGETS["mesh"]
    front = pic.place(scattered(rng, count, size, 2.0 * NEAR, 0.8 * FAR), size)
    across = np.stack([rng.uniform(-3.0, 3.0, (count, 3)), rng.uniform(-3.0, 3.0, (count, 3)),
                       -np.where(rng.random((count, 3)) < 0.5, rng.uniform(-2.0, 2.0, (count, 3)), rng.uniform(-0.2, 0.2, (count, 3)))], -1).astype(np.float32)
    across[::3] *= (10.0 ** rng.uniform(1.0, 4.0, (len(across[::3]), 1, 1))).astype(np.float32)   # up to 30 km: the crossing points' rounding is pixels wide
    P = scattered(rng, count, size, NEAR, 4.0 * NEAR, side_hi=float(max(size)))
    at_near = rng.random((count, 3)) < 0.6
    at_near[:, 0] = True
    P[..., 2] = np.where(at_near, ulps(NEAR, rng.integers(-4, 5, (count, 3))).astype(np.float64), P[..., 2])
    near = pic.place(P, size)
    near[..., 2] = -P[..., 2].astype(np.float32)                    # the view depths to the bit
    P = scattered(rng, count, size, 1.0, 2.0, side_lo=0.5, side_hi=float(max(size)))
    P[..., 2] = ulps(FAR, rng.integers(-4, 5, (count, 3)))             # the other plane the depth is tested against
    far = pic.place(P, size)
    far[..., 2] = -P[..., 2].astype(np.float32)
    V = pic.place(scattered(rng, count, size, 4.0 * NEAR, 0.3 * FAR), size).astype(np.float64)
    a, b = rng.uniform(0.2, 2.0, (2, count, 1))
    scale = np.abs(V).max(axis=(1, 2))[:, None]
    eps = rng.choice([0.0, 1e-6, 1e-4, 1e-3, 1e-2], (count, 1))
    V[:, 2] = a * V[:, 0] + b * V[:, 1] + eps * scale * rng.uniform(-1.0, 1.0, (count, 3))     # in the plane through the camera, or nearly
    return dict(front=front, across=across, near=near, far=far, slivers=V.astype(np.float32))


def light_families(rng, count, size):
    """the light's: sub-texel, map-wide, partly and wholly off the footprint, and depths around 2 depth_range (and in front of the frame's
    near plane); placed"""
    sh = TARGETS["shadow"]
    n = size[0]
    sub = scattered(rng, count, size, 1.0, DEPTH_RANGE, side_hi=1.0, centre=(0.0, 1.0))
    wide = scattered(rng, count, size, 1.0, DEPTH_RANGE, side_lo=0.5 * n, side_hi=3.0 * n)
    off = scattered(rng, count, size, 1.0, DEPTH_RANGE, side_lo=0.1, side_hi=0.5 * n, centre=(-0.6, 1.6))
    deep = scattered(rng, count, size, 1.0, DEPTH_RANGE, side_lo=0.5, side_hi=1.0 * n)
    edge = ulps(2.0 * DEPTH_RANGE, rng.integers(-4, 5, (count, 3))).astype(np.float64)
    deep[..., 2] = np.where(rng.random((count, 3)) < 0.6, edge, rng.uniform(-0.2, 2.4, (count, 3)) * DEPTH_RANGE)
    V = sh.place(deep, size)
    return dict(sub=sh.place(sub, size), wide=sh.place(wide, size), off=sh.place(off, size), deep=V)


def families(target, rng, count, size):
    return light_families(rng, count, size) if target.name == "shadow" else view_families(rng, count, size)


# ---- placed triangles: candidates, and the ones whose set-up has the wanted property ---------------------------------------------------------------

def corners(rng, count, size, side_lo, side_hi, depth):
    """right triangles with axis-parallel legs of side_lo .. side_hi centres, their corners anywhere within two centres of the picture"""
    w, h = size
    e = rng.uniform(side_lo, side_hi, (count, 2)) * rng.choice([-1.0, 1.0], (count, 2))
    c = np.stack([rng.uniform(-2.0, w + 2.0, count), rng.uniform(-2.0, h + 2.0, count)], -1)
    uv = np.stack([c, c + e * [1.0, 0.0], c + e * [0.0, 1.0]], 1)
    d = np.broadcast_to(rng.uniform(depth[0], depth[1], (count, 1, 1)), (count, 3, 1))
    return np.concatenate([uv, d], -1)


def sides_of(setups):
    return setups["x1"] - setups["x0"] + 1, setups["y1"] - setups["y0"] + 1


def take(P, mask, k):
    at = np.flatnonzero(mask)[:k]
    return P[at]


def placed_sides(target, draw, size, lane_box, seed):
    """boxes whose longer side is exactly lane_box centres (the last the lane walks) and lane_box + 1 (the first for the wave), four of each
    (a one-centre box: the corner pixels' among them, the only ones shadow_setup leaves)"""
    rng = np.random.default_rng(seed)
    P = np.concatenate([corner_points(size), corners(rng, 6000, size, max(lane_box - 2.5, 0.01), lane_box + 1.5, (2.0, 20.0))])
    sx, sy = sides_of(draw(target.place(P, size))["setups"])
    drawn = (sx > 0) & (sy > 0)
    longer = np.maximum(sx, sy)
    return np.concatenate([take(P, drawn & (longer == lane_box), 4), take(P, drawn & (longer == lane_box + 1), 4)])


PLACED_RESIDUES = (7, 0, 1)


def placed_edges(target, draw, size, seed):
    """for each of x0, x1, y0, y1 and each residue 7, 0, 1 (mod 8) two triangles whose box has that edge there, boxes clamped at the last
    column and the last row, and one-centre boxes in the four corner pixels"""
    rng = np.random.default_rng(seed)
    w, h = size
    P = np.concatenate([corners(rng, 8000, size, 0.05, 0.6 * max(w, h), (2.0, 20.0)), corners(rng, 4000, size, 0.05, 0.45, (2.0, 20.0)), corner_points(size)])
    s = draw(target.place(P, size))["setups"]
    drawn = s["kind"] >= LANE
    keep = [take(P, drawn & (s[e] % 8 == r), 2) for e in ("x0", "x1", "y0", "y1") for r in PLACED_RESIDUES]
    sx, sy = sides_of(s)
    keep.append(take(P, drawn & (s["x1"] == w - 1) & (sx > 2), 2))
    keep.append(take(P, drawn & (s["y1"] == h - 1) & (sy > 2), 2))
    for x, y in ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)):
        keep.append(take(P, drawn & (s["x0"] == x) & (s["x1"] == x) & (s["y0"] == y) & (s["y1"] == y), 1))
    return np.concatenate(keep)


def corner_points(size):
    """a vertex on the centre of each corner pixel and the rest outside the picture: the only one-centre boxes shadow_setup's floor and ceil
    leave (tri_setup's ceil and floor have them around any small triangle)"""
    w, h = size
    out = []
    for x, y, dx, dy in ((0, 0, -1, -1), (w - 1, 0, 1, -1), (0, h - 1, -1, 1), (w - 1, h - 1, 1, 1)):
        c = (x + 0.5, y + 0.5)
        out.append([(c[0], c[1], 5.0), (c[0] + 1.5 * dx, c[1], 5.0), (c[0], c[1] + 1.5 * dy, 5.0)])
    return np.array(out, np.float64)


# ---- wave layouts ----------------------------------------------------------------------------------------------------------------------------

def small_and_big(rng, count, size, big_at):
    """`count` triangles: those at big_at with a box of a dozen centres a side or more (the wave's at the default lane_box), the others with
    a box of one to four (a lane's: longer than one spacing either way, so it holds a centre, and under two, so shadow_setup's floor and
    ceil leave at most four)"""
    w, h = size
    P = np.zeros((count, 3, 3))
    for k in range(count):
        big = k in big_at
        side = rng.uniform(14.0, 0.8 * min(w, h)) if big else rng.uniform(1.2, 1.9)
        c = (rng.uniform(1.0, w - 1.0 - side), rng.uniform(1.0, h - 1.0 - side))
        P[k, :, :2] = [c, (c[0] + side, c[1] + 0.3 * side), (c[0] + 0.4 * side, c[1] + side)]
        P[k, :, 2] = rng.uniform(2.0, 20.0)
    return P


def wave_layouts(size, seed):
    """name -> (raster-unit soup, origins): three 64-triangle waves (all for the wave; only lane 0's; only lane 63's), 63, 64, 65 and 129
    triangles with only the last one for the wave (the last lane of a partial wave beside lanes without a triangle, lane 0 of a wave of
    its own), and 43 triangles at 3 origins (an instance straddles the first wave's end and another the second's)"""
    rng = np.random.default_rng(seed)
    out = {"64 for the wave": (small_and_big(rng, 64, size, set(range(64))), ONE_ORIGIN),
           "lane 0 alone": (small_and_big(rng, 64, size, {0}), ONE_ORIGIN), "lane 63 alone": (small_and_big(rng, 64, size, {63}), ONE_ORIGIN)}
    for count in (63, 64, 65, 129):
        out["%d, the last for the wave" % count] = (small_and_big(rng, count, size, {count - 1}), ONE_ORIGIN)
    out["43 x 3"] = (small_and_big(rng, 43, size, {42}), None)        # the origins are the target's: see instance_origins
    return out


def instance_origins(target):
    return np.array([target.shift(0.0, 0.0), target.shift(0.03, 0.01), target.shift(-0.02, 0.02)], np.float32)


# ---- ties and contention ---------------------------------------------------------------------------------------------------------------------

TIE_TRIANGLES, TIE_COPIES = 43, 100          # 4 300 pairs: 68 waves


def ties(size, seed):
    """43 triangles of every size at 100 equal origins: every pair ties with its 99 copies, bit for bit, over 68 waves"""
    rng = np.random.default_rng(seed)
    return scattered(rng, TIE_TRIANGLES, size, 2.0, 20.0, side_lo=0.5, side_hi=float(max(size)), centre=(0.1, 0.9)), np.zeros((TIE_COPIES, 3), np.float32)


LAYERS = (64, 64)                            # triangles a copy, copies: 4 096 layers
LAYER_SIZE = (16, 16)


def layers(target):
    """4 096 parallel layers that each fill the 16 x 16 picture, pair p's depth 10 - 0.001 p or so: every word ends at the last pair's,
    through 4 095 other values on the way when the pairs come in order"""
    w, h = LAYER_SIZE
    P = np.zeros((LAYERS[0], 3, 3))
    P[:, :, :2] = [(-6.0 * w, -5.0 * h), (8.0 * w, -5.0 * h), (0.5 * w, 9.0 * h)]
    P[:, :, 2] = (10.0 - 0.001 * np.arange(LAYERS[0]))[:, None]
    origins = np.array([target.shift(0.0, 0.064 * k) for k in range(LAYERS[1])], np.float32)
    return P, origins


def orders(count, seed):
    rng = np.random.default_rng(seed)
    return {"given": np.arange(count), "reversed": np.arange(count)[::-1], "shuffled": rng.permutation(count)}


# ---- closed sheets ---------------------------------------------------------------------------------------------------------------------------

SHEETS = ((8, (9, 7)), (8, (37, 21)), (33, (37, 21)), (33, (160, 96)), (64, (37, 21)), (64, (64, 40)))     # cells a side, picture
SHEET_MARGIN = 3.0


def sheet(target, cells, size, seed):
    """a grid of cells^2 cells over the picture and three centres around it, every inner vertex moved by up to a quarter of a cell either
    way (no cell folds) and given a depth of its own: (raster-unit soup [2 cells^2][3][3], the grid vertices of every triangle
    [2 cells^2][3])"""
    rng = np.random.default_rng(seed)
    w, h = size
    m = SHEET_MARGIN
    u, v = np.meshgrid(np.linspace(-m, w + m, cells + 1), np.linspace(-m, h + m, cells + 1))
    inner = np.zeros_like(u, bool)
    inner[1:-1, 1:-1] = True
    u = u + inner * rng.uniform(-0.25, 0.25, u.shape) * (w + 2 * m) / cells
    v = v + inner * rng.uniform(-0.25, 0.25, v.shape) * (h + 2 * m) / cells
    lo, hi = target.depths()
    grid = np.stack([u, v, log_uniform(rng, lo, hi, u.shape)], -1).reshape(-1, 3)
    r, q = np.meshgrid(np.arange(cells), np.arange(cells), indexing="ij")
    a = (r * (cells + 1) + q).ravel()
    b, d, e = a + 1, a + cells + 1, a + cells + 2
    flip = rng.random(len(a)) < 0.5                                   # either diagonal
    first = np.where(flip[:, None], np.stack([a, d, e], 1), np.stack([a, d, b], 1))
    second = np.where(flip[:, None], np.stack([a, e, b], 1), np.stack([b, d, e], 1))
    idx = np.stack([first, second], 1).reshape(-1, 3)
    return grid[idx], idx
