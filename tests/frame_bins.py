"""Inputs, FP64 twin driver and metrics of the frame kernels' bin-by-bin tests (tests/test_frame_bins.py on the CPU,
tests/test_frame_bins_gpu.py on the device, scripts/frame_bin_margins.py).  Test infrastructure only.

The parity tests compare a whole channel in the max norm on JONSWAP spectra, where one wave number of N^2 carries about 1 / (4 N) of the
channel's maximum: a single bin can be entirely wrong below 1e-4.  Here the frame kernels (modulate, two row transforms, transpose, unpack)
are fed spectra that WE choose -- unit-modulus random phases on a chosen support, so that every bin of the support weighs the same -- and
compared with the FP64 twin (tests/np_twin.py) fed with the same FP32 h0 and the same FP32 phase omega * t:
  * spatially, per channel, relative to the maximum of the channel's GROUP in the twin (a channel that is zero for an input is then held
    against its neighbours instead of being exempt), and
  * per bin (white input, the channels that are linear in the spectrum): the spectrum of the error against the spectrum of the twin."""
import ctypes as C
import functools

import numpy as np

import helpers as H
import np_twin as T
from godotoceanwaves_amd.presets import DEPTH
from oracle import oracle as O
from godotoceanwaves_amd import WaveCascadeParameters, WaveGenerator
from godotoceanwaves_amd.presets import cascade_preset, UPDATE_DELTA

T_FRAME = 37.25   # s: the time of the compared tick (phases up to ~170 rad at the Nyquist wave number of 2 rad/m)
PHI_BIN = 1e-2    # the per-bin metric's floor, relative to the rms over all bins of the twin's spectrum
UNPACK = dict(whitecap=0.5, grow=0.02 * 5.0 * 7.5, decay=0.02 * 5.0 * 1.15)   # one update of 1/50 s with foam_amount 5 (wave_generator.gd:104-106)

DISPLACEMENT, DERIVATIVE = (0, 1, 2), (3, 4, 5, 7)   # the two groups of the spatial metric (helpers.CHANNELS; channel 7 as jacobian - 1)
SPATIAL_CHANNELS = DISPLACEMENT + DERIVATIVE
BIN_CHANNELS = ("hx", "hy", "hz", "dhx_dx", "dhy_dx")   # linear in the spectrum; dhy_dx = grad_x (1 + |dhx_dx|)


def tiles(n):
    """(square, non-square) tile lengths in m with a Nyquist wave number of about 2 rad/m: L ~ pi N / 2 (402 x 300 at 256^2, 1608 x 1200 at 1024^2)"""
    L = float(round(np.pi * n / 2))
    return (L, L), (L, float(round(0.75 * L)))


def _phases(n, seed):
    rng = np.random.default_rng(seed)
    return np.exp(2j * np.pi * rng.random((n, n)))


def white(n, seed):
    """every texel"""
    return _phases(n, seed)


def lines(n, seed):
    """texel row 0 and texel column 0 (the two Nyquist lines), with the corner texel (0, 0)"""
    m = np.zeros((n, n), bool)
    m[0, :] = m[:, 0] = True
    return np.where(m, _phases(n, seed), 0)


def axes(n, seed):
    """texel row N/2 and texel column N/2: ky = 0 and kx = 0, with the DC texel (where k is the regularisation 1e-6 alone)"""
    m = np.zeros((n, n), bool)
    m[n // 2, :] = m[:, n // 2] = True
    return np.where(m, _phases(n, seed), 0)


def point_sets(n):
    """name -> the (y, x) texels of one sparse input: single texels on and off the special lines, and one asymmetric pair"""
    h = n // 2
    return {"corner": [(0, 0)], "dc": [(h, h)], "row0_kx0": [(0, h)], "col0_ky0": [(h, 0)], "row0_x5": [(0, 5)], "col0_y5": [(5, 0)],
            "pair": [(3, n - 5), (n - 7, 11)]}


def points(n, seed, name):
    ph = _phases(n, seed)
    out = np.zeros((n, n), complex)
    for y, x in point_sets(n)[name]:
        out[y, x] = ph[y, x]
    return out


def inputs(n):
    """name -> (kind, function of (n, seed)): kind is "white" or "sparse" (the bound's kind)"""
    out = {"white": ("white", white), "lines": ("sparse", lines), "axes": ("sparse", axes)}
    for name in point_sets(n):
        out["point_" + name] = ("sparse", lambda n_, seed, name=name: points(n_, seed, name))
    return out


def h0_mirror(h0):
    """conj(h0(-k)): the other half of the reference's spectrum texel"""
    return np.conj(H.mirror(h0))


def spectrum_texels(h0):
    """complex64 [n][n] -> the reference's float4 texels [n][n][4] (h0(k), conj(h0(-k))), as ow_get_spectrum returns them"""
    h0 = np.asarray(h0, np.complex64)
    m = h0_mirror(h0)
    return np.ascontiguousarray(np.stack([h0.real, h0.imag, m.real, m.imag], axis=-1), np.float32)


def twin_fields(h0, omega32, t32, tile, depth=DEPTH):
    """the FP64 twin's four transformed layers with the unpack sign applied: FP32 h0 (complex64 [n][n]), FP32 dispersion plane and FP32
    time, widened; the phase is the FP32 product omega * t (spectrum_modulate.glsl:65), as test_full_size_properties forms it"""
    h0 = np.asarray(h0, np.complex64).astype(np.complex128)
    n = h0.shape[0]
    t32 = np.float32(t32)
    phase32 = np.asarray(omega32, np.float32) * t32
    return T.ifft2_ref(T.modulate(n, tile, depth, float(t32), h0, h0_mirror(h0), omega=phase32.astype(np.float64) / float(t32)))


def twin_channels(h0, omega32, t32, tile, whitecap, grow, decay, depth=DEPTH, layers=None):
    """the eight FP64 channels [n][n][8] after one tick from a zero foam plane (layers: transformed layers to unpack instead, for mutants)"""
    out = twin_fields(h0, omega32, t32, tile, depth) if layers is None else layers
    return T.unpack(out, whitecap, grow, decay)


def scale_input(unit, omega32, t32, tile, depth=DEPTH):
    """unit-modulus input -> complex64 h0, scaled by ONE FP32 factor so that the largest of the twin's five derivative fields (dhy_dx, dhy_dz,
    dhx_dx, dhz_dz, dhz_dx) has maximum 0.5: FP16 stays in range and every term of the Jacobian and the gradients is of order one"""
    unit = np.asarray(unit, np.complex64)
    n = unit.shape[0]
    u = unit.astype(np.complex128)
    x = T.modulate(n, tile, depth, float(np.float32(t32)), u, h0_mirror(u), omega=np.asarray(omega32, np.float64))
    o = np.fft.ifft2(x[1:].astype(np.complex64), axes=(-2, -1)) * np.float32(n * n)   # (the peak alone is wanted: single precision will do)
    peak = max(np.abs(o[0].imag).max(), np.abs(o[1].real).max(), np.abs(o[1].imag).max(), np.abs(o[2].real).max(), np.abs(o[2].imag).max())
    if peak == 0:   # the DC texel alone: kx = ky = 0 and every derivative field vanishes -- the elevation hy = h is all there is: its maximum 0.5
        peak = np.abs(np.fft.ifft2(x[0].astype(np.complex64)) * np.float32(n * n)).max()
    return (unit * np.float32(0.5 / peak)).astype(np.complex64)


def condition_self_mirrored(unit, omega32, t32):
    """A texel that mirrors onto itself -- (0, 0), (0, N/2), (N/2, 0), (N/2, N/2) -- holds h = 2 Re(h0 m), m = exp(i omega t): with a random
    phase that can cancel (seen: cos = 7e-4), the scale makes up for it, and the 2e-7 of an FP32 sincos then shows as 3e-5 of the only mode
    there is -- in the oracle as in the kernels.  The single-texel inputs are no test of that: their self-mirrored texels get the phase at
    which h0 m has equal parts, arg = pi / 4, at t32 (still unit modulus)."""
    unit = np.array(unit, np.complex128)
    n = unit.shape[0]
    for y, x in ((0, 0), (0, n // 2), (n // 2, 0), (n // 2, n // 2)):
        if unit[y, x] != 0:
            unit[y, x] = np.exp(1j * (np.pi / 4 - float(np.float32(omega32[y, x]) * np.float32(t32))))
    return unit


def make_input(n, name, seed, omega32, t32, tile):
    """input `name` as the tests feed it: the unit-modulus pattern (single texels conditioned: condition_self_mirrored), scaled (scale_input)"""
    unit = inputs(n)[name][1](n, seed)
    if name.startswith("point_"):
        unit = condition_self_mirrored(unit, omega32, t32)
    return scale_input(unit, omega32, t32, tile)


def oracle_channels(h0, t32, tile, whitecap, grow, decay, depth=DEPTH):
    """the FP32 oracle on the same h0: spectrum_modulate -> ifft2 -> unpack from a zero foam plane, [n][n][8] FP32 (its omega is its own)"""
    n = h0.shape[0]
    x = O.spectrum_modulate(n, tile, depth, np.float32(t32), spectrum_texels(h0))
    return O.unpack(n, O.ifft2(n, O.fft_butterfly(n), x), whitecap, grow, decay)[2]


class EmulFrame(C.Structure):
    """CascadeFrame of ow_device.h as tests/emul/emul.cpp takes it"""
    _fields_ = [(f, C.c_float) for f in ("tile_x", "tile_y", "time", "whitecap", "foam_grow_rate", "foam_decay")] + [("cascade", C.c_int32), ("pad0", C.c_int32)]


EMUL_ENTRIES = {   # entry point of tests/emul/emul.cpp -> the sizes it accepts, up to 1024^2
    "emul_frame": (128, 256, 512, 1024), "emul_frame_compact": (256, 512, 1024), "emul_frame_lp0": (128, 256, 512), "emul_frame_lp1": (256, 512)}


@functools.lru_cache(maxsize=1)
def emul_library():
    E = H.emul_library()
    f32p, u16p = np.ctypeslib.ndpointer(np.float32, flags="C"), np.ctypeslib.ndpointer(np.uint16, flags="C")
    E.emul_frame.argtypes = [C.c_int, f32p, f32p, C.POINTER(EmulFrame), f32p, u16p, u16p, u16p, f32p]
    E.emul_frame_compact.argtypes = E.emul_frame.argtypes
    E.emul_frame_lp.argtypes = [C.c_int, C.c_int] + E.emul_frame.argtypes[1:]
    return E


def emul_channels(entry, h0, omega32, t32, tile, whitecap, grow, decay):
    """the device's lane code on the CPU (tests/emul/emul.cpp), entry point `entry` of EMUL_ENTRIES, one tick from a zero foam plane:
    ([n][n][8] FP32, displacement bits, normal bits)"""
    E = emul_library()
    n = h0.shape[0]
    h0a = np.ascontiguousarray(np.stack([h0.real, h0.imag], axis=-1), np.float32)
    cf = EmulFrame(tile[0], tile[1], np.float32(t32), whitecap, np.float32(grow), np.exp(-np.float32(decay), dtype=np.float32), 0, 0)
    Tb, foam = np.zeros(n * n * 4 * 2, np.float32), np.zeros(n * n, np.uint16)
    disp, norm, f32 = np.zeros((n, n, 4), np.uint16), np.zeros((n, n, 4), np.uint16), np.zeros((n, n, 8), np.float32)
    args = (h0a, np.ascontiguousarray(omega32, np.float32), C.byref(cf), Tb, disp, norm, foam, f32)
    rc = E.emul_frame_lp(n, int(entry[-1]), *args) if entry.startswith("emul_frame_lp") else getattr(E, entry)(n, *args)
    assert rc == 0, f"{entry} does not take {n}^2"
    return f32, disp, norm


SEED = 20261018


@functools.lru_cache(maxsize=2)
def cpu_case(n, tile_index, name):
    """(tile, h0 complex64, the oracle's FP32 omega, the twin's channels) of input `name` on the square (0) or the non-square (1) tile at
    t = T_FRAME: computed once, shared by everything that is compared with it, and left unchanged"""
    tile = tiles(n)[tile_index]
    om = O.omega(n, tile, DEPTH)
    h0 = make_input(n, name, SEED + tile_index, om, T_FRAME, tile)
    r = twin_channels(h0, om, T_FRAME, tile, **UNPACK)
    for a in (h0, om, r):
        a.setflags(write=False)
    return tile, h0, om, r


def _group(c):
    return DISPLACEMENT if c in DISPLACEMENT else DERIVATIVE


def _plane(a, c):
    v = np.asarray(a[..., c], np.float64)
    return v - 1.0 if c == 7 else v


def spatial(a, r):
    """per non-foam channel: max|a - r| / the maximum over the channel's group in the twin r ({hx, hy, hz}; {grad_x, grad_y, dhx_dx,
    jacobian - 1}) -> dict name -> figure"""
    gmax = {g: max(np.abs(_plane(r, c)).max() for c in g) for g in (DISPLACEMENT, DERIVATIVE)}
    if gmax[DERIVATIVE] == 0:   # the DC texel alone (scale_input): held against what every other input scales its derivative fields to
        gmax[DERIVATIVE] = 0.5
    return {H.CHANNELS[c]: float(np.abs(_plane(a, c) - _plane(r, c)).max() / gmax[_group(c)]) for c in SPATIAL_CHANNELS}


def linear_channel(a, name):
    """one of BIN_CHANNELS from the eight channels, FP64"""
    a = np.asarray(a)
    if name == "dhy_dx":
        return a[..., 3].astype(np.float64) * (1.0 + np.abs(a[..., 5].astype(np.float64)))
    return a[..., H.CHANNELS.index(name)].astype(np.float64)


def per_bin(a, r, channels=BIN_CHANNELS, phi=PHI_BIN):
    """per linear channel: max over ALL bins k of E(k) / (S(k) + phi rms_k S), E = |fft2(a - r)| / N^2, S = |fft2(r)| / N^2 in FP64.  The
    channels are real, so the half plane of rfft2 holds every bin's magnitude; rms_k S over the full plane follows from Parseval.  phi only
    keeps the bins whose multiplier vanishes (uy = 0 for hx, DC) from dividing by zero.  -> dict name -> (figure, (ky, kx) bin of the worst)"""
    out = {}
    for name in channels:
        ra, rr = linear_channel(a, name), linear_channel(r, name)
        nn = rr.size
        E = np.abs(np.fft.rfft2(ra - rr)) / nn
        S = np.abs(np.fft.rfft2(rr)) / nn
        rms = np.sqrt((rr ** 2).sum()) / nn
        ratio = E / (S + phi * rms)
        i = int(np.argmax(ratio))
        out[name] = (float(ratio.flat[i]), tuple(int(v) for v in np.unravel_index(i, ratio.shape)))
    return out


def bounds(n):
    """dict(spatial_white, spatial_sparse, bin_white) for size n (helpers.FRAME_BIN_BOUNDS)"""
    return H.FRAME_BIN_BOUNDS[n]


def worst_ratio(a, r, n, kind, bin_channels=BIN_CHANNELS, margin=1.0):
    """every figure of an input divided by its bound -> (worst ratio, description, dict of the figures); > 1 fails.  kind: "white" or "sparse";
    margin: the family's factor on the bounds (1 unless profiles/frame_bin_margins.txt derives another)"""
    b = bounds(n)
    figs = {"spatial " + k: v for k, v in spatial(a, r).items()}
    ratios = {k: v / (margin * (b["spatial_white"] if kind == "white" else b["spatial_sparse"])) for k, v in figs.items()}
    if kind == "white" and bin_channels:
        for k, (v, at) in per_bin(a, r, bin_channels).items():
            figs["bin " + k] = v
            ratios["bin " + k] = v / (margin * b["bin_white"])
    k = max(ratios, key=ratios.get)
    return ratios[k], f"{k}: {figs[k]:.3g} ({ratios[k]:.2f} of its bound)", figs


# ---- teeth: faults of the kind the kernels can have, applied in FP64; each must push a metric above its bound ----
def compact_layers(h0, omega32, t32, tile, mutant=None, depth=DEPTH):
    """compact_pipeline of tests/test_compact_math.py (the algebra of the compact intermediate: three layers, the two Nyquist lines in closed
    form) on the twin's inputs -- FP32 h0, the FP32 phase omega * t -- returning the four transformed layers as np_twin.ifft2_ref does.
    mutant: None, or
      "corner_generic"  the corner texel's closed forms Q1[0], Q2[0], Q3[0] left at the generic row-0 expressions
      "no_P"            P(ky) dropped from the derived i ky T0 + P
      "no_conjugate"    one mirrored row of T1 taken without the conjugate"""
    h0 = np.asarray(h0, np.complex64).astype(np.complex128)
    n = h0.shape[0]
    idy, idx = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    kx = (idx - n * 0.5) * 2 * np.pi / tile[0]
    ky = (idy - n * 0.5) * 2 * np.pi / tile[1]
    k = np.hypot(kx, ky) + 1e-6
    ux, uy = kx / k, ky / k
    m = np.exp(1j * (np.asarray(omega32, np.float32) * np.float32(t32)).astype(np.float64))
    h = h0 * m + h0_mirror(h0) * np.conj(m)
    Z0, Z1, Z2 = 1j * (1 + uy) * h, 1j * ux * h, 1j * kx * (1 - ux) * h
    col = idx == 0
    Z1 = np.where(col, 0, Z1)
    Z2 = np.where(col, ux * (ky - 1j * kx) * h, Z2)
    P = ((kx + 1j * ux) * h)[:, 0] if mutant != "no_P" else np.zeros(n)
    Tm = [np.fft.ifft(Z, axis=1) * n for Z in (Z0, Z1, Z2)]
    Q1, Q2, Q3 = -ky[0] * uy[0] * h[0], (1j * ux[0] - ky[0]) * h[0], (1j * kx[0] * (1 - ux[0]) + ky[0] * ux[0]) * h[0]
    if mutant != "corner_generic":
        Q1[0] = ((-ky * uy + kx + 1j * ux) * h)[0, 0]
        Q2[0] = (-ky * (1 + 1j * ux) * h)[0, 0]
        Q3[0] = (-1j * kx * ux * h)[0, 0]
    R = [None] + [np.fft.ifft(q) * n for q in (Q1, Q2, Q3)]
    kyv = ky[:, 0]
    c1 = Tm[1].copy()
    c1[1:n // 2] = np.conj(Tm[1][n - np.arange(1, n // 2)])
    if mutant == "no_conjugate":
        c1[n // 4 + 3] = Tm[1][n - (n // 4 + 3)]
    G = [Tm[0].copy(), 1j * kyv[:, None] * Tm[0] + P[:, None], (1 - kyv)[:, None] * c1, Tm[2].copy()]
    for j in (1, 2, 3):
        G[j][0] = R[j]
    F = [np.fft.ifft(g, axis=0).T * n for g in G]   # [x'][y]
    return np.stack([F[0], F[2].real + 1j * F[1].imag, F[3].real + 1j * F[1].real, F[3].imag + 1j * F[2].imag])


def _twin_mutant(h0, omega32, t32, tile, mutate):
    """the twin with `mutate` applied to its modulated layers [layer][y][x]"""
    h0 = np.asarray(h0, np.complex64).astype(np.complex128)
    phase32 = np.asarray(omega32, np.float32) * np.float32(t32)
    x = T.modulate(h0.shape[0], tile, DEPTH, float(np.float32(t32)), h0, h0_mirror(h0), omega=phase32.astype(np.float64) / float(np.float32(t32)))
    mutate(x)
    return T.unpack(T.ifft2_ref(x), **{"whitecap": UNPACK["whitecap"], "grow": UNPACK["grow"], "decay": UNPACK["decay"]})


def _jonswap_blindness(n, mutate):
    """today's metric -- the max norm over a channel, preset 2 at the same size -- of the same mutant on the twin: the worst non-foam channel"""
    from godotoceanwaves_amd.presets import UPDATE_DELTA, cascade_preset
    p = cascade_preset(2)
    h0, h0m = T.spectrum(n, H.twin_params(H.spectrum_pc(p)))
    x = T.modulate(n, p["tile_length"], DEPTH, p["time"] + UPDATE_DELTA, h0, h0m)
    r = T.unpack(T.ifft2_ref(x), **UNPACK)
    mutate(x)
    a = T.unpack(T.ifft2_ref(x), **UNPACK)
    return max(H.relmax(a[..., c], r[..., c]) for c in SPATIAL_CHANNELS)


def teeth(n=256):
    """rows (mutant, input, worst ratio to the bounds, which figure, today's metric on preset 2 or None) -- tests/test_frame_bins.py asserts
    on them, scripts/frame_bin_margins.py prints them"""
    def one_bin(x):
        x[0, n // 3, n // 5] *= 1 + 2e-3

    def one_column(x):
        x[:, :, n // 2 + 37] *= np.exp(1j * 1e-3)

    def sign_row(a):
        a = a.copy()
        a[7, :, :6] *= -1   # texel row 7: the checkerboard shifted by one
        return a

    rows = []
    for label, name, make, blind in [
            ("1 one bin of layer 0 scaled by 1 + 2e-3", "white", lambda c: _twin_mutant(c[1], c[2], T_FRAME, c[0], one_bin), one_bin),
            ("2 corner texel: generic row-0 forms for Q1..Q3[0]", "lines", lambda c: twin_channels(None, None, None, None, **UNPACK, layers=compact_layers(c[1], c[2], T_FRAME, c[0], "corner_generic")), None),
            ("2 corner texel: generic row-0 forms for Q1..Q3[0]", "point_corner", lambda c: twin_channels(None, None, None, None, **UNPACK, layers=compact_layers(c[1], c[2], T_FRAME, c[0], "corner_generic")), None),
            ("3 P(ky) dropped from i ky T0 + P", "lines", lambda c: twin_channels(None, None, None, None, **UNPACK, layers=compact_layers(c[1], c[2], T_FRAME, c[0], "no_P")), None),
            ("4 one column of bins rotated by exp(1e-3 i)", "white", lambda c: _twin_mutant(c[1], c[2], T_FRAME, c[0], one_column), one_column),
            ("5 one mirrored row of T1 without the conjugate", "white", lambda c: twin_channels(None, None, None, None, **UNPACK, layers=compact_layers(c[1], c[2], T_FRAME, c[0], "no_conjugate")), None),
            ("6 unpack's sign checkerboard shifted in one texel row", "point_pair", lambda c: sign_row(c[3]), None)]:
        case = cpu_case(n, 1, name)
        worst, what, _ = worst_ratio(make(case), case[3], n, inputs(n)[name][0])
        rows.append(dict(mutant=label, input=name, ratio=worst, what=what, today=None if blind is None else _jonswap_blindness(n, blind)))
    return rows


PATHS = [
    (128, 2, "update_all", "standard", "standard", 1),
    (128, 2, "update_all", "layer_parallel", "layer_parallel", 1),
    (256, 2, "update_all", "layer_parallel_compact", "layer_parallel_compact", 1),
    (256, 2, "run", None, "tick_groups_compact", 3),
    (512, 2, "update_all", "compact", "compact", 1),
    (1024, 2, "update_all", "standard", "standard", 1),        # the 1024^2 plan
    (1024, 2, "update_all", None, "compact", 1),
    (1024, 2, "run", None, "tick_pairs_compact", 3),
    (1024, 2, "lookahead", None, "compact", 4),                  # update_all x 4 with one delta: the last tick's pass 1 was computed ahead
    (2048, 1, "update_all", None, "compact", 1),                 # split-plan pass 1, half-table pass 2
    (2048, 1, "run", None, "tick_pairs_compact", 3),             # the split tick pairs
]


def _inputs(n):
    return list(inputs(n)) if n in (256, 1024) else ["white", "lines"]


def gpu_cases():
    """grouped by size and input, the paths innermost: the twin of an input is shared by the paths that reach the same FP32 time"""
    out = []
    for n in sorted({p[0] for p in PATHS}):
        for name in _inputs(n):
            out += [(name,) + p for p in PATHS if p[0] == n]
    return out


def _tile(n, cascades, i):
    """the square tile on the even cascades, the non-square one on the odd ones (and on a lone cascade)"""
    return tiles(n)[i % 2 if cascades > 1 else 1]


def _seed(i):
    return SEED + 10 * i


def _context(n, cascades, kernels, ticks_after):
    """a context whose spectra are resident (one tick of preset records on the case's tiles) and whose records are clean; the record times
    reach FB.T_FRAME with the last tick of the path"""
    gen = WaveGenerator()
    gen.map_size = n
    gen.debug_f32 = True
    gen.kernels = kernels
    gen.init_gpu(max(2, cascades))
    params = [WaveCascadeParameters(**dict(cascade_preset(i), tile_length=_tile(n, cascades, i), time=T_FRAME - (1 + ticks_after) * UPDATE_DELTA))
              for i in range(cascades)]
    gen.update_all(UPDATE_DELTA, params)
    assert not any(p.should_generate_spectrum for p in params)
    return gen, params


_REFERENCES = {}


def _reference(n, tile, name, seed, t32, om, whitecap, grow, decay):
    """(the twin's channels, the oracle's foam) of one injected input: computed once per FP32 time and dispersion plane and left unchanged
    (the last four are kept: the cases are ordered by input)"""
    key = (n, tile, name, seed, np.float32(t32).tobytes(), H.digest(om), whitecap, grow, decay)
    if key not in _REFERENCES:
        while len(_REFERENCES) >= 4:
            _REFERENCES.pop(next(iter(_REFERENCES)))
        h0 = _h0(n, tile, name, seed)
        r = twin_channels(h0, om, t32, tile, whitecap, grow, decay)
        r.setflags(write=False)
        _REFERENCES[key] = (r, oracle_channels(h0, t32, tile, whitecap, grow, decay)[..., 6].copy())
    return _REFERENCES[key]


@functools.lru_cache(maxsize=4)
def _h0(n, tile, name, seed):
    """the input, scaled with the layer's dispersion plane at FB.T_FRAME (the scale need not follow the tick's own FP32 time)"""
    from oracle import oracle as O
    h0 = make_input(n, name, seed, O.omega(n, tile, DEPTH), T_FRAME, tile)
    h0.setflags(write=False)
    return h0


def run_gpu_case(name, n, cascades, path, kernels, ticks):
    """the procedure of one case -> (kernel family of the last launch, look-ahead hits of the last tick, per cascade a dict of what was read
    back and the references); scripts/frame_bin_margins.py prints the figures of the same runs"""
    gen, params = _context(n, cascades, kernels, ticks)
    try:
        h0 = []
        for i in range(cascades):
            h0.append(_h0(n, _tile(n, cascades, i), name, _seed(i)))
            # (the dispersion plane: kept on cascade 0, the layer's own handed back on the others -- the twin takes what ow_get_spectrum returns)
            gen.debug_set_spectrum(i, h0[i], None if i == 0 else gen.get_spectrum(i)[1])
        if path == "lookahead":
            for _ in range(ticks - 1):
                gen.update_all(UPDATE_DELTA, params)
        hits = gen.lookahead_stats()[0]
        for i in range(cascades):
            gen.set_normal_map(i, np.zeros((n, n, 4), np.float16))
        if path == "run":
            gen.run(UPDATE_DELTA, params, ticks)
        else:
            gen.update_all(UPDATE_DELTA, params)
        gen.sync()
        assert not any(p.should_generate_spectrum for p in params)
        out = []
        for i, p in enumerate(params):
            tile = _tile(n, cascades, i)
            spec, om = gen.get_spectrum(i)
            disp, norm = gen.get_maps(i)
            r, foam = _reference(n, tile, name, _seed(i), np.float32(p.time), om, float(np.float32(p.whitecap)), float(np.float32(p.foam_grow_rate)),
                                 float(np.float32(p.foam_decay_rate)))
            out.append(dict(tile=tile, h0=h0[i], spectrum=spec, f32=gen.get_maps_f32(i), disp=disp, norm=norm, twin=r, oracle_foam=foam))
        return gen.last_kernel_family(), gen.lookahead_stats()[0] - hits, out
    finally:
        gen.free()
