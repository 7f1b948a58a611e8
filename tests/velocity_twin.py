"""The FP64 NumPy twin of the velocity layers V = dD/dt (godotoceanwaves_amd/csrc/ow_velocity_kernels.h), written from np_twin's modulate /
ifft2_ref / unpack conventions with hdot in place of h.  Test infrastructure: tests/test_water_velocity.py, tests/test_velocity_layers.py,
scripts/velocity_margins.py."""
import ctypes as C
import os

import numpy as np

import np_twin as NT
from cpu_builds import CSRC, HERE, compile_shared


def modulate_words(tile_length, time, depth=20.0):
    """the first four FP32 words of a layer's modulate push constants (ow_get_push_constants: tile_length, depth, time), as uint32"""
    return np.array([tile_length[0], tile_length[1], depth, time], np.float32).view(np.uint32)


def phases(omega, modulate_words):
    """the maps' own FP32 phase omega * t (spectrum_modulate.glsl:65), as FP32"""
    f = np.asarray(modulate_words, np.uint32).view(np.float32)
    return omega.astype(np.float32) * f[3]


def packed_layers(h0_texel, omega, modulate_words, m=None, empty_spare_half=False):
    """the two packed spectra [2][ky][kx] complex128 the transform runs on: hx + i hy and hz + i dhy_dx of hdot.
    m: the unit phasors exp(i omega t) per texel (default: exp of the FP32 product omega * t, in FP64).
    empty_spare_half: layer B as hz alone (what the kernels must NOT do: a mutant for the tests)."""
    n = omega.shape[0]
    f = np.asarray(modulate_words, np.uint32).view(np.float32)
    tile = (float(f[0]), float(f[1]))
    om = omega.astype(np.float64)
    h0 = h0_texel[..., 0].astype(np.float64) + 1j * h0_texel[..., 1]
    h0m = h0_texel[..., 2].astype(np.float64) + 1j * h0_texel[..., 3]
    if m is None:
        m = np.exp(1j * phases(omega, modulate_words).astype(np.float64))
    hdot = 1j * om * (h0 * m - h0m * np.conj(m))
    idy, idx = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    kx = (idx - n * 0.5) * 2 * np.pi / tile[0]
    ky = (idy - n * 0.5) * 2 * np.pi / tile[1]
    k = np.hypot(kx, ky) + 1e-6
    ux, uy = kx / k, ky / k
    hi = 1j * hdot
    spare = 0.0 if empty_spare_half else 1j * (hi * ky)
    return np.stack([hi * uy + 1j * hdot, hi * ux + spare])  # modulate's layers 0 and 1


def velocity_row_transform(h0_texel, omega, modulate_words, m=None):
    """the transform along kx alone, [layer][ky][y] complex128: what pass 1 leaves in the intermediate (rows, no 1/N)"""
    x = packed_layers(h0_texel, omega, modulate_words, m)
    return np.fft.ifft(x, axis=-1) * x.shape[-1]


def velocity_twin(h0_texel, omega, modulate_words, m=None, empty_spare_half=False):
    """V of one layer, FP64 [y][x][3]: the inputs are the resident spectrum (ow_get_spectrum's texel (h0(k), conj(h0(-k))) and omega) and the
    layer's FP32 push-constant words, the phase the FP32 product omega * t"""
    n = omega.shape[0]
    out = NT.ifft2_ref(packed_layers(h0_texel, omega, modulate_words, m, empty_spare_half))
    iy, ix = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    sign = 1.0 - 2.0 * ((ix & 1) ^ (iy & 1))
    o = out * sign
    return np.stack([o[0].real, o[0].imag, o[1].real], axis=-1)


def floor_needed(got_f16, want):
    """the smallest rel_floor at which helpers.fp16_close(got, want as FP16, ulps=1) passes: max over texels and channels of
    (|got - want16| - one FP16 ulp) / the channel's max|want16|"""
    a = np.asarray(got_f16).view(np.float16)[..., :3].astype(np.float64)
    b16 = np.asarray(want, np.float64).astype(np.float16)
    b = b16.astype(np.float64)
    chmax = np.abs(b).reshape(-1, 3).max(axis=0)
    over = np.abs(a - b) - np.spacing(np.abs(b16)).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(over <= 0, 0.0, over / chmax).max())  # (inf where a channel of the twin is all zeros and the layer is not)


# ---- the CPU lane emulation of the two kernels (tests/velocity/velocity_emul.cpp) ---------------------------------------------------

_EMUL = None


def emul_library():
    """tests/velocity/libvelocity_emul.so, rebuilt when velocity_emul.cpp or a device header is newer"""
    global _EMUL
    if _EMUL is not None:
        return _EMUL
    so = os.path.join(HERE, "velocity", "libvelocity_emul.so")
    srcs = [os.path.join(HERE, "velocity", "velocity_emul.cpp")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        compile_shared(srcs[0], so)
    E = C.CDLL(so)
    f32p = np.ctypeslib.ndpointer(np.float32, flags="C")
    E.velemul_layer.argtypes = [C.c_int, f32p, f32p, C.c_float, C.c_float, C.c_float, C.c_void_p, np.ctypeslib.ndpointer(np.uint16, flags="C")]
    E.velemul_expi.argtypes = [C.c_int, f32p, f32p]
    E.velemul_twiddles.argtypes = [C.c_int, f32p]
    _EMUL = E
    return E


def emul_layer(h0_texel, omega, modulate_words, intermediate=False):
    """both kernels on the CPU from the stored plane h0(k) (the texel's first half: the kernels read the mirrored texel themselves).
    Returns the FP16 layer [n][n][4], and with intermediate=True also the pass-1 intermediate [layer][ky][y] complex64"""
    E = emul_library()
    n = omega.shape[0]
    f = np.asarray(modulate_words, np.uint32).view(np.float32)
    plane = np.ascontiguousarray(h0_texel[..., :2], np.float32)
    out = np.zeros((n, n, 4), np.uint16)
    inter = np.zeros((2, n, n, 2), np.float32) if intermediate else None
    assert E.velemul_layer(n, plane, np.ascontiguousarray(omega, np.float32), float(f[0]), float(f[1]), float(f[3]),
                           inter.ctypes.data if intermediate else None, out) == 0
    layer = out.view(np.float16)
    return (layer, inter[..., 0] + 1j * inter[..., 1]) if intermediate else layer


def emul_phasors(phase_f32):
    """exp(i ph) as the kernels' expi_phase evaluates it from FP32 phases (CPU path: sincos_phase), widened to complex128"""
    E = emul_library()
    ph = np.ascontiguousarray(phase_f32, np.float32)
    m = np.zeros(ph.shape + (2,), np.float32)
    E.velemul_expi(ph.size, ph.reshape(-1), m.reshape(-1))
    return m[..., 0].astype(np.float64) + 1j * m[..., 1].astype(np.float64)
