"""Maps a test wrote, under the read side's kernels: a context over caller-owned map buffers (WaveGenerator.external_maps) that a test
fills with any FP16 bytes, and the written inputs tests/test_written_maps.py (the CPU builds) and tests/test_written_maps_gpu.py (the
device) share -- every finite FP16 pattern for the device's loads, one-texel spikes for k_height_bound, non-finite heights.

What the host code asks of a context that has never ticked (csrc/ow_points_host.hip, ow_consumer_host.hip, ow_mesh_host.hip): the point,
ray, view and mesh calls check their arguments, the cascade count against the context's and the layers' fault flags, and then read the map
buffers as they are; only the velocity calls ask for computed layers (velocity_refresh: pc_valid, OW_ERR_STATE).  ow_create zeroes the map
buffers -- max(2, cascades) layers of them, which is what a caller's buffers must hold -- and synchronises.  So a written context never
ticks: it is created, written, and read.

Nothing here asserts about the code under test and nothing here builds."""
import numpy as np

from godotoceanwaves_amd.wave_generator import WaveGenerator, WaveGenerator as W
from scenes import look

# ---- the context ---------------------------------------------------------------------------------------------------------------------------


class WrittenContext:
    """gen: a WaveGenerator whose displacement and normal maps are this object's torch buffers, on this object's stream"""

    def __init__(self, n, cascades):
        import torch
        self.n, self.cascades = n, cascades
        layers = max(2, cascades)                 # ow_create's own count: it zeroes that many layers of a caller's buffers
        self.stream = torch.cuda.Stream()
        self.disp = torch.zeros((layers, n, n, 4), dtype=torch.int16, device="cuda")
        self.norm = torch.zeros_like(self.disp)
        torch.cuda.synchronize()
        self.gen = WaveGenerator()
        self.gen.map_size = n
        self.gen.stream = self.stream.cuda_stream
        self.gen.external_maps = (self.disp.data_ptr(), self.norm.data_ptr())
        self.gen.init_gpu(cascades)
        assert self.gen.descriptors["displacement_map"].rid == self.disp.data_ptr()

    def write(self, disp_u16, norm_u16):
        """host arrays [cascades][n][n][4] of uint16 over the maps, ordered on the context's stream; returns them for the CPU builds"""
        import torch
        shape = (self.cascades, self.n, self.n, 4)
        d, m = np.ascontiguousarray(disp_u16, np.uint16), np.ascontiguousarray(norm_u16, np.uint16)
        assert d.shape == shape and m.shape == shape, (d.shape, m.shape, shape)
        with torch.cuda.stream(self.stream):
            self.disp[:self.cascades].copy_(torch.from_numpy(d.view(np.int16).copy()))
            self.norm[:self.cascades].copy_(torch.from_numpy(m.view(np.int16).copy()))
        self.stream.synchronize()
        return d, m

    def free(self):
        self.gen.free()


def written_context(n, cascades):
    return WrittenContext(n, cascades)


# ---- A. every finite FP16 value ------------------------------------------------------------------------------------------------------------

FP16_N = 128                       # 128^2 texels of four half-words: exactly 65 536
FP16_SCALES = np.array([(1 / 128, 1 / 128, 1.0, 1.0)], np.float32)    # one texel per metre: x = c + 0.5 is texel c's centre, exactly
FINITE_PATTERNS = 65536 - 2048
# the half-words of a texel that a record of ow_sample_surface reports unmixed at a texel centre: displacement x, y, z of the displacement
# layer; gradient x, y and foam (w) of the normal layer
DISP_REPORTED, NORM_REPORTED = [0, 1, 2], [0, 1, 3]


def fp16_layout(reverse=False, seed=20261020):
    """(displacement, normal) layers [1][128][128][4] of uint16.  The displacement layer is a seeded permutation of the 65 536 patterns.
    The normal layer is a second one, drawn so that the 16 384 patterns the first puts into w, which no record reports, sit in x, y or w
    of the second: every pattern is then in a reported half-word of one of the layers.  The non-finite patterns (exponent 31) are zero.
    reverse: the same texels in the opposite order (the half-words of a texel keep their places)."""
    rng = np.random.default_rng(seed)
    first = rng.permutation(65536).astype(np.uint16)
    hidden = first[3::4]
    at = np.arange(65536)
    reported = rng.permutation(at[at % 4 != 2])
    second = np.zeros(65536, np.uint16)
    second[reported[:len(hidden)]] = hidden
    second[np.concatenate([reported[len(hidden):], at[at % 4 == 2]])] = rng.permutation(np.concatenate([first[0::4], first[1::4], first[2::4]]))
    assert np.array_equal(np.sort(second), np.arange(65536))
    out = []
    for flat in (first, second):
        texels = flat.reshape(-1, 4)[::-1] if reverse else flat.reshape(-1, 4)
        layer = np.ascontiguousarray(texels).reshape(1, FP16_N, FP16_N, 4).copy()
        layer[(layer & 0x7c00) == 0x7c00] = 0
        out.append(layer)
    return tuple(out)


def texel_points(offset):
    """(x, z) = (c + offset, r + offset) for every texel (r, c), row by row: 0.5 is the centres (both weights 0), 1.0 the corners between
    four texels (both weights 0.5)"""
    r, c = np.meshgrid(np.arange(FP16_N), np.arange(FP16_N), indexing="ij")
    return np.stack([c.ravel() + offset, r.ravel() + offset], axis=1).astype(np.float32)


def half_to_f32(u16):
    return np.asarray(u16, np.uint16).view(np.float16).astype(np.float32)


# ---- B. the height bound ---------------------------------------------------------------------------------------------------------------------

BOUND_SIZES = (128, 512)           # 8 192 texel pairs: one trip of k_height_bound's loop, a partial grid; 131 072: two trips of the full grid
BOUND_SEED = 7


def bound_scales(n):
    """three cascades with texels of 0.5 m, 0.625 m and 0.375 m and displacement scales that differ: a bound word taken from another
    cascade's layer gives another slab"""
    return np.array([(1 / (n * t), 1 / (n * t), sz, 1.0) for t, sz in ((0.5, 1.0), (0.625, 0.75), (0.375, 0.5))], np.float32)


def f16_bits(v):
    return int(np.float16(v).view(np.uint16))


def spike_texels(n):
    """the first texel and the odd one of its pair, the last pair, at 512^2 the last pair of the loop's first trip (65 536 lanes) and the
    first of its second, and a seeded one"""
    t = [0, 1, n * n - 2, n * n - 1]
    if n == 512:
        t += [131071, 131072]
    return t + [int(np.random.default_rng(BOUND_SEED + n).integers(2, n * n - 2))]


class BoundCase:
    """maps [3][n][n][4], their scales, the spikes (cascade, texel, D_y bits) and where their texels' centres lie in the world"""

    def __init__(self, name, n, spikes, fill=0, options=None, rays=None):
        self.name, self.n, self.spikes, self.fill, self.options, self.own_rays = name, n, spikes, fill, options, rays
        self.scales = bound_scales(n)

    def maps(self, without=()):
        """without: the indices of the spikes left out (their texels' D_y zero)"""
        d = np.zeros((3, self.n * self.n, 4), np.uint16)
        m = np.zeros((3, self.n * self.n, 4), np.uint16)
        if self.fill:
            d[..., [0, 2, 3]] = self.fill
            m[...] = self.fill
        for k, (c, texel, bits) in enumerate(self.spikes):
            if k not in without:
                d[c, texel, 1] = bits
        shape = (3, self.n, self.n, 4)
        return d.reshape(shape), m.reshape(shape)

    def maxima(self):
        """the largest |D_y| per cascade, as float32"""
        out = np.zeros(3, np.float32)
        for c, _, bits in self.spikes:
            v = np.abs(half_to_f32(np.uint16(bits)))
            out[c] = out[c] if v <= out[c] else v          # a NaN stays
        return out

    def slab(self):
        """ow_raycast.h slab_half_height on the known maxima, in float32 operation for operation"""
        H = np.float32(0.0)
        for c in range(3):
            H = np.float32(H + np.float32(self.maxima()[c] * np.abs(self.scales[c, 2])))
        with np.errstate(over="ignore", invalid="ignore"):
            hw = np.float32(np.float32(H * np.float32(1.0 + 0.0009765625)) + np.float32(1e-2))
        return hw if np.isfinite(hw) else np.float32(3.4028235e38)

    def shift(self):
        """the constant horizontal displacement of the filled maps: the water drawn at world (x, z) is the map at (x, z) - shift"""
        if not self.fill:
            return 0.0
        return float(sum(np.float32(half_to_f32(np.uint16(self.fill)) * sz) for sz in self.scales[:, 2]))

    def world(self, k):
        """(x, z, height) of spike k: its texel's centre as the surface shows it, and the height there"""
        c, texel, bits = self.spikes[k]
        size = 1.0 / (float(self.scales[c, 0]) * self.n)
        r, col = divmod(texel, self.n)
        return (col + 0.5) * size + self.shift(), (r + 0.5) * size + self.shift(), float(half_to_f32(np.uint16(bits))) * float(self.scales[c, 2])

    def rays(self):
        """a dozen rays shared among the spikes: straight down on each, from two heights and with a direction that is no unit vector, down
        beside it (inside its texel neighbourhood and three texels away), slanted onto it, up from below, horizontal at y = 2 across it"""
        if self.own_rays is not None:
            return self.own_rays
        o, d, T = [], [], []
        per = 12 // len(self.spikes)
        for k in range(len(self.spikes)):
            x, z, _ = self.world(k)
            size = 1.0 / (float(self.scales[self.spikes[k][0], 0]) * self.n)
            variants = [((x, 10, z), (0, -1, 0), 100), ((x - 5, 2, z), (1, 0, 0), 20), ((x + 0.3 * size, 10, z - 0.2 * size), (0, -1, 0), 100),
                        ((x - 6, 6, z), (1, -1, 0), 40), ((x, 50, z), (0, -2, 0), 100), ((x + 3 * size, 10, z), (0, -1, 0), 100),
                        ((x, -10, z), (0, 1, 0), 100), ((x, 2, z - 5), (0, 0, 3), 20), ((x, 6, z + 6), (0, -1, -1), 40),
                        ((x - 0.4 * size, 30, z + 0.4 * size), (0, -1, 0), 100), ((x - 5, 2, z + 0.5 * size), (1, 0, 0), 20),
                        ((x + 2, 4.5, z), (-1, -1, 0), 40)]
            for org, direction, far in variants[:per]:
                o.append(org), d.append(direction), T.append(far)
        return W.rays(o, d, T)

    def camera(self):
        """8 x 8 pixels looking down at the last spike from 8 m: 2.8 m of water across, the spike's texels in the middle"""
        x, z, _ = self.world(len(self.spikes) - 1)
        return look(position=(x, 8.0, z), yaw_deg=0.0, pitch_deg=-89.9, fov=20.0, width=8, height=8, max_distance=40.0)


def bound_cases(n):
    """every case of one map size: the spike of 3.0 at each texel of spike_texels in each cascade, three spikes at once, a negative one, and
    a map full of 1000.0 but for D_y"""
    texels = spike_texels(n)
    cases = [BoundCase(f"{n}: cascade {c}, texel {t}", n, [(c, t, f16_bits(3.0))]) for c in range(3) for t in texels]
    rng = np.random.default_rng(BOUND_SEED + 1000 + n)
    a, b, c = (int(v) for v in rng.integers(0, n * n, 3))
    cases.append(BoundCase(f"{n}: 1.0, 2.0 and 4.0 at once", n, [(0, a, f16_bits(1.0)), (1, b, f16_bits(2.0)), (2, c, f16_bits(4.0))]))
    cases.append(BoundCase(f"{n}: a spike of -3.0", n, [(1, b, f16_bits(-3.0))]))
    cases.append(BoundCase(f"{n}: 1000.0 everywhere but in D_y", n, [(0, a, f16_bits(0.5))], fill=f16_bits(1000.0)))
    return cases


NON_FINITE = (0x7c00, 0xfc00, 0x7e00)      # +Inf, -Inf, a NaN
NON_FINITE_OPTIONS = {"max_samples": 64}


def non_finite_case(bits, n=128):
    """one texel of cascade 0 whose D_y is not finite; the four rays stay far from it (its texel is the middle one: 32 m away), so their
    samples are finite and only the bound sees it.  64 samples at 0.25 m bound every march at 16 m."""
    rays = W.rays([(1, 3, 1), (2, 20, 1), (1, 2, 2), (2, -3, 2)], [(0, -1, 0), (0, -1, 0), (1, 0, 0), (0, 2, 0)], [100, 100, 100, 100])
    return BoundCase(f"D_y = {bits:#06x}", n, [(0, (n // 2) * n + n // 2, bits)], options=NON_FINITE_OPTIONS, rays=rays)
