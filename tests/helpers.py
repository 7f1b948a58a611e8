"""Shared helpers of the test-suite: error metrics and oracle drivers."""
import ctypes as C
import hashlib
import json
import math
import os
import sys

import numpy as np

from godotoceanwaves_amd.presets import DEPTH, UPDATE_DELTA, cascade_preset
from oracle import oracle as O
from oracle import ref as R

CHANNELS = ["hx", "hy", "hz", "grad_x", "grad_y", "dhx_dx", "foam", "jacobian"]
# north_star tolerance: 1e-4 relative FP32, taken per channel in the max norm (element-wise relative
# error is meaningless at zero crossings)
TOL_F32 = 1e-4
# foam is RECURRENT FP16 state (fft_unpack.glsl:61): a 1e-7 difference in the Jacobian can flip one FP16
# rounding, so the pre-quantisation foam may differ by one FP16 ulp of the [0,1] state
TOL_FOAM_ABS = 2.0 ** -10
# SHA-256 digests of what the reference's own shaders computed (oracle/_ref), written by tests/golden/make_ref_digests.py: the
# bit-exact pins hold where the reference checkout is absent too
REF_DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_digests.json")


def digest(a):
    """dtype, shape and every byte of an array: two arrays with the same digest are bit-identical"""
    a = np.ascontiguousarray(a)
    return hashlib.sha256(f"{a.dtype.str}{a.shape}".encode() + a.tobytes()).hexdigest()


def ref_digests(section):
    with open(REF_DIGESTS) as f:
        return json.load(f)[section]


def relmax(a, b):
    """max|a-b| / max|b| (max-norm relative error)"""
    a, b = np.asarray(a), np.asarray(b)
    kind = np.complex128 if (np.iscomplexobj(a) or np.iscomplexobj(b)) else np.float64
    a, b = a.astype(kind), b.astype(kind)
    den = np.abs(b).max()
    return float(np.abs(a - b).max() / (den if den > 0 else 1.0))


def fp16_close(a_bits_or_f16, b_bits_or_f16, ulps=1, rel_floor=1e-5):
    """|a-b| <= ulps * spacing_fp16(|b|) + rel_floor * max|b| per channel (last axis); returns worst ratio.
    One FP16 ulp alone is meaningless near zero crossings (the ulp shrinks with the value while the FP32 error of
    a 1024-point transform does not), hence the floor relative to the channel maximum: 1e-5, ten times tighter
    than the 1e-4 FP32 tolerance of north_star.  That the FP16 maps are EXACTLY the round-to-nearest-even
    quantisation of the FP32 channels is checked separately (quantisation_exact)."""
    a = np.asarray(a_bits_or_f16).view(np.float16)
    b = np.asarray(b_bits_or_f16).view(np.float16)
    af, bf = a.astype(np.float64), b.astype(np.float64)
    spacing = np.spacing(np.abs(b)).astype(np.float64)
    chmax = np.abs(bf).reshape(-1, bf.shape[-1]).max(axis=0)
    allowed = ulps * spacing + rel_floor * chmax
    return float((np.abs(af - bf) / allowed).max())


def quantisation_exact(f32, disp_bits, norm_bits):
    """The RGBA16F maps must be bit for bit the RTE quantisation of the pre-quantisation FP32 channels
    [hx,hy,hz,gx,gy,dhx_dx,foam,J]: displacement = (hx,hy,hz), normal = (gx,gy,dhx_dx,foam)."""
    d = np.asarray(disp_bits).view(np.uint16)
    n = np.asarray(norm_bits).view(np.uint16)
    q = np.asarray(f32, np.float32).astype(np.float16).view(np.uint16)
    return bool(np.array_equal(d[..., :3], q[..., 0:3]) and np.array_equal(n[..., :4], q[..., 3:7]))


def set_params(cstruct, preset):
    for k, v in preset.items():
        if k == "tile_length":
            cstruct.tile_length[0], cstruct.tile_length[1] = v
        elif k == "spectrum_seed":
            cstruct.spectrum_seed[0], cstruct.spectrum_seed[1] = v
        else:
            setattr(cstruct, k, v)
    cstruct.should_generate_spectrum = 1


def oracle_generator(n, cascade_ids, native=False):
    g = O.Generator(n, len(cascade_ids), DEPTH, native=native)
    for i, ci in enumerate(cascade_ids):
        set_params(g.params[i], cascade_preset(ci))
    return g


def spectrum_pc(preset):
    U, F = preset["wind_speed"], preset["fetch_length"] * 1e3
    return O.make_pc(preset["spectrum_seed"], preset["tile_length"], np.float32(O.jonswap_alpha(U, F)),
                     np.float32(O.jonswap_peak(U, F)), U, np.float32(math.radians(preset["wind_direction"])), DEPTH,
                     preset["swell"], preset["detail"], preset["spread"])


def record_pc(rec, depth=DEPTH):
    """The spectrum push constants of one parameter record, packed as the runtime packs them (ow_schedule.hip pack_spectrum, after
    wave_generator.gd:69-71): wind speed and fetch clamped to 1e-4 (the exported setters), alpha and the peak frequency from the FP64 values,
    deg_to_rad in FP64, every scalar narrowed to FP32 only at the pack."""
    U, F = max(rec["wind_speed"], 1e-4), max(rec["fetch_length"], 1e-4) * 1e3
    return O.make_pc(rec["spectrum_seed"], rec["tile_length"], O.jonswap_alpha(U, F), O.jonswap_peak(U, F), U,
                     rec["wind_direction"] * (math.pi / 180.0), depth, rec["swell"], rec["detail"], rec["spread"])


def pc_words(pc):
    """the first twelve words of the spectrum push-constant block (ow_get_push_constants), as uint32"""
    f = [pc.tile_length[0], pc.tile_length[1], pc.alpha, pc.peak_frequency, pc.wind_speed, pc.angle, pc.depth, pc.swell, pc.detail, pc.spread]
    return np.concatenate([np.array([pc.seed[0], pc.seed[1]], np.int64).astype(np.uint32), np.array(f, np.float32).view(np.uint32)])


def twin_params(pc):
    """the same push constants as the FP64 truth twin's parameters (tests/np_twin.py): the FP32 values, widened"""
    return dict(seed=(pc.seed[0], pc.seed[1]), tile_length=(pc.tile_length[0], pc.tile_length[1]), alpha=pc.alpha,
                peak_frequency=pc.peak_frequency, wind_speed=pc.wind_speed, angle=pc.angle, depth=pc.depth, swell=pc.swell,
                detail=pc.detail, spread=pc.spread)


def spectrum_records(fuzzed=14, seed=20261016):
    """(name, record) of the spectrum texel tests (tests/test_spectrum_texels.py, scripts/spectrum_margins.py): the eight presets, the ten
    range-edge presets (tests/edge_presets.py) and `fuzzed` records drawn by scripts/fuzz_parity.draw_case (FP64 scalars, random seeds,
    non-square tiles in about 40 % of them) -- 32 in all, four contexts of eight cascades."""
    from edge_presets import edge_presets
    scripts = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts")
    if scripts not in sys.path:
        sys.path.insert(0, scripts)
    import fuzz_parity
    out = [(f"preset{i}", cascade_preset(i)) for i in range(8)] + sorted(edge_presets().items())
    rng = np.random.default_rng(seed)
    recs = []
    while len(recs) < fuzzed:
        recs += fuzz_parity.draw_case(rng)["records"]
    return out + [(f"fuzz{i}", r) for i, r in enumerate(recs[:fuzzed])]


def spectrum_references(n, pcs, workers=4):
    """per push-constant block: (the oracle's texels [n][n][4] FP32, the FP64 twin's h0 [n][n] complex128, the oracle's omega [n][n] FP32,
    np_twin.direction_ulp_sensitivity [n][n]),
    computed in parallel (the oracle's ctypes calls and NumPy's array operations release the interpreter lock)"""
    import np_twin
    from concurrent.futures import ThreadPoolExecutor

    def one(pc):
        tp = twin_params(pc)
        return (O.spectrum_compute(n, pc), np_twin.amplitude(n, tp), O.omega(n, (pc.tile_length[0], pc.tile_length[1]), pc.depth),
                np_twin.direction_ulp_sensitivity(n, tp))
    with ThreadPoolExecutor(max_workers=workers) as ex:
        return list(ex.map(one, pcs))


def device_spectra(n, recs):
    """one context of len(recs) cascades, one update_all: per slot (h0 texels [n][n][4] through ow_get_spectrum, omega [n][n], the spectrum
    push-constant words of the launch)"""
    from godotoceanwaves_amd import WaveCascadeParameters, WaveGenerator
    gen = WaveGenerator()
    gen.map_size = n
    gen.init_gpu(max(2, len(recs)))
    try:
        gen.update_all(UPDATE_DELTA, [WaveCascadeParameters(**r) for r in recs])
        gen.sync()
        return [gen.get_spectrum(i) + (gen.get_push_constants(i)[0],) for i in range(len(recs))]
    finally:
        gen.free()


# ---- per-texel metric (the spectrum spans tens of orders of magnitude: a max-norm is set by the few texels at the peak) ----
# The spectrum's bounds (tests/test_spectrum_texels.py, tests/test_emul.py, scripts/spectrum_margins.py).  Each is about four times the worst
# value measured on the MI355X over every size and record of spectrum_records (profiles/spectrum_margins.txt); the measured value is noted.
SPEC_PHI = 1e-7             # the floor, relative to the plane's maximum (tests/test_spectrum_texels.py says why)
SPEC_ABS_FLOOR = float(np.sqrt(np.finfo(np.float32).tiny))   # 1.1e-19: the amplitude is the square root of an FP32 energy, subnormal below this
SPEC_RHO_ORACLE = 3e-6      # k_spectrum vs the oracle, per texel (measured 6.7e-7)
SPEC_KAPPA = 2.0            # k_spectrum vs the FP64 twin: this many times the literal form's own error ...
SPEC_RHO_TWIN = 1.5e-6      # ... plus this much of |twin| (measured 3.9e-7)
SPEC_RHO_LITERAL = 5e-6     # the oracle vs the FP64 twin (measured 1.2e-6)
SPEC_ARG_ULPS = 4.0         # ulps of theta - angle allowed on top, times np_twin.direction_ulp_sensitivity (the wind's null direction; measured 0.98)
# The frame kernels' bounds on injected spectra (tests/frame_bins.py, tests/test_frame_bins.py, tests/test_frame_bins_gpu.py): per size, FOUR times the
# ORACLE's own worst error against the FP64 twin (the measured value is noted; profiles/frame_bin_margins.txt) over all seven non-foam channels,
# every input of the kind and both tiles -- the factor covers a transform of another radix, another summation order and the Cody-Waite sincos_phase
# (2e-7).  spatial_*: max|a - twin| over the maximum of the channel's group; bin_white: the per-bin ratio (phi = frame_bins.PHI_BIN).
# tests/test_frame_bins.py holds the oracle within a quarter of each, so the constants cannot drift from their source.
FRAME_BIN_BOUNDS = {
    128: dict(spatial_white=2.4e-6, spatial_sparse=5.8e-6, bin_white=4.3e-4),    # measured 5.79e-7, 1.43e-6, 1.07e-4
    256: dict(spatial_white=2.5e-6, spatial_sparse=6.9e-6, bin_white=4.9e-4),    # measured 6.19e-7, 1.71e-6, 1.22e-4
    512: dict(spatial_white=2.8e-6, spatial_sparse=7.6e-6, bin_white=5.5e-4),    # measured 7.00e-7, 1.88e-6, 1.37e-4
    1024: dict(spatial_white=3.2e-6, spatial_sparse=8.9e-6, bin_white=8.6e-4),   # measured 7.79e-7, 2.21e-6, 2.13e-4
    2048: dict(spatial_white=3.9e-6, spatial_sparse=1.7e-6, bin_white=1.15e-3),  # measured 9.58e-7, 4.09e-7, 2.86e-4 (white and lines only; bins of hy, hz, dhx_dx)
}
# a kernel family whose legitimate rounding needs more than a bound gets a factor here, with its error model in profiles/frame_bin_margins.txt
FRAME_BIN_FAMILY_MARGIN = {}


def texel_margins(a, r, rho, phi, extra=0.0, per_ulp=None, ulps=0.0, abs_floor=0.0):
    """a, r: planes with the channel on the last axis (complex channels compare as complex numbers).  Per texel and channel
        ratio = |a - r| / (extra + (rho + ulps per_ulp) |r| + phi max|r|)      (max over the channel's plane)
    over the texels with |r| >= phi max|r| (and >= abs_floor) -- the ones below the floor may differ freely (they must be finite: checked by
    the caller).
    extra: an absolute allowance per texel (or 0); per_ulp: a relative allowance per texel and ulp of something the formulas cannot
    evaluate more closely in FP32 (np_twin.direction_ulp_sensitivity), of which `ulps` are allowed.
    Returns dict(worst: max ratio, at: its index, floor_share: share of all texel-channels that need the floor term,
    over_share: share of all texel-channels with a ratio above 1, rho_needed: the smallest rho with every ratio <= 1 at this phi,
    ulps_needed: the smallest `ulps` with every ratio <= 1 at this rho and phi)."""
    a = np.asarray(a)
    r = np.asarray(r)
    kind = np.complex128 if (np.iscomplexobj(a) or np.iscomplexobj(r)) else np.float64
    err = np.abs(a.astype(kind) - r.astype(kind))
    mag = np.abs(r.astype(kind))
    floor = np.maximum(phi * mag.reshape(-1, mag.shape[-1]).max(axis=0), abs_floor)
    live = (mag >= floor) & (mag > 0)
    cond = 0.0 if per_ulp is None else per_ulp * mag
    rel = extra + (rho * mag + ulps * cond)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(live, err / (rel + floor), 0.0)
        need = np.where(live, (err - extra - ulps * cond - floor) / mag, 0.0)
        need_ulps = np.where(live & (cond > 0), (err - extra - rho * mag - floor) / cond, 0.0) if per_ulp is not None else np.zeros(1)
    i = int(np.argmax(ratio))
    return dict(worst=float(ratio.flat[i]), at=np.unravel_index(i, ratio.shape), floor_share=float((live & (err > rel)).sum() / err.size),
                over_share=float((ratio > 1.0).sum() / err.size), rho_needed=max(0.0, float(need.max())),
                ulps_needed=max(0.0, float(need_ulps.max())))


def spectrum_margins(a, r, rho, sens, extra=0.0):
    """texel_margins with the spectrum's floor (SPEC_PHI of the plane's maximum, and SPEC_ABS_FLOOR) and SPEC_ARG_ULPS ulps of theta - angle
    (sens: np_twin.direction_ulp_sensitivity, per texel and channel)"""
    return texel_margins(a, r, rho, SPEC_PHI, extra=extra, per_ulp=sens, ulps=SPEC_ARG_ULPS, abs_floor=SPEC_ABS_FLOOR)


def zero_where_reference_is_not_finite(r, *planes):
    """The reference's own Box-Muller draws log(0) at a texel whose hash gives u1 = 0 (spectrum_compute.glsl:44-49; one texel of 2^31 --
    fuzz2 of spectrum_records at 2048^2): there its amplitude is not finite, and so must every other evaluation's be.  Asserts that each
    plane is non-finite exactly where r is, and returns r and the planes with those texels set to 0."""
    bad = ~np.isfinite(r)
    out = [np.where(bad, 0, r)]
    for a in planes:
        assert np.array_equal(~np.isfinite(a), bad), "non-finite texels where the reference has finite ones (or the other way round)"
        out.append(np.where(bad, 0, a))
    return out


def h0_complex(h0):
    """[n][n][4] FP32 spectrum texels -> [n][n][2] complex: (h0(k), conj(h0(-k)))"""
    h0 = np.asarray(h0, np.float32)
    return h0[..., 0::2] + 1j * h0[..., 1::2].astype(np.float64)


def mirror(plane):
    """plane[(N - y) % N][(N - x) % N]"""
    return np.roll(plane[::-1, ::-1], 1, axis=(0, 1))


# ---- the CPU emulation of the device code (tests/emul/emul.cpp over godotoceanwaves_amd/csrc/*.h) ----
class EmulSpectrumPC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("seed_x", "seed_y")] + \
               [(n, C.c_float) for n in ("tile_x", "tile_y", "alpha", "peak_frequency", "wind_speed", "angle", "depth", "swell", "detail", "spread")]


def emul_pc(pc):
    """an oracle SpectrumPC as the device struct"""
    return EmulSpectrumPC(pc.seed[0], pc.seed[1], pc.tile_length[0], pc.tile_length[1], pc.alpha, pc.peak_frequency, pc.wind_speed,
                          pc.angle, pc.depth, pc.swell, pc.detail, pc.spread)


def emul_library():
    """tests/emul/libemul.so, rebuilt when emul.cpp or a device header is newer"""
    from cpu_builds import compile_shared   # (cpu_builds imports this module)
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(here, "..", "godotoceanwaves_amd", "csrc")
    so = os.path.join(here, "emul", "libemul.so")
    srcs = [os.path.join(here, "emul", "emul.cpp")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        compile_shared(srcs[0], so)
    E = C.CDLL(so)
    f32p = np.ctypeslib.ndpointer(np.float32, flags="C")
    E.emul_spectrum.argtypes = [C.c_int, C.POINTER(EmulSpectrumPC), f32p, f32p, f32p]
    E.emul_spectrum_fast.argtypes = [C.c_int, C.POINTER(EmulSpectrumPC), f32p]
    return E


def emul_fast_h0(E, n, pc):
    """the kernel's form of the amplitude (spectrum_amplitude_fast) on the CPU: [n][n] complex"""
    out = np.zeros((n, n, 2), np.float32)
    E.emul_spectrum_fast(n, C.byref(emul_pc(pc)), out)
    return out[..., 0] + 1j * out[..., 1].astype(np.float64)


def ref_stages(c):
    """the stages test 1 pins, of an oracle generator (cascade 0) or of a RefCascade: the same arrays either way"""
    if isinstance(c, R.RefCascade):
        return {"spectrum": c.spectrum, "fft1": c.fft[1], "displacement": c.displacement, "normal": c.normal}
    return {"spectrum": c.spectrum(0), "fft1": c.fft_half1(0), "displacement": c.displacement(0), "normal": c.normal(0)}


def stage_digests(c):
    return {k: digest(v) for k, v in ref_stages(c).items()}


CASCADE_CASES = [(128, 0, 3), (128, 3, 2), (256, 2, 1), (512, 1, 1), (1024, 2, 1)]


def edge_cases():
    from edge_presets import edge_presets
    return sorted(edge_presets().items())


EDGE_FRAMES = 2
