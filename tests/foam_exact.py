"""The foam recurrence as an exact predictor, and the written foam planes it is fed with (tests/test_foam_exact.py).  Test infrastructure only.

Foam is the one state the frame kernels carry from tick to tick: normal.a, kept a second time in the context's private FP16 plane in pass 2's
lane order (ow_device.h Pass2::foam_index).  The debug image (OW_FLAG_DEBUG_F32) holds the FP32 Jacobian the kernel used as channel 7 and the
FP32 foam before quantisation as channel 6, so with the previous FP16 state known the new state is a handful of correctly rounded FP32
operations -- fft_unpack.glsl:55-66 as ow_device.h writes it three times (after_layer3, after_f3, unpack_texel) -- which NumPy reproduces bit
for bit, one rounding per step, per texel, all in np.float32:

    prev32 = prev_bits.view(float16) -> float32
    a      = prev32 * decay32
    fac    = -minimum(0, J - whitecap32)          J = channel 7, the kernel's own bits
    s      = a + fl32(fac * grow32)
    s      = 0 where s is NaN                     fmaxf(NaN, 0) = 0
    f32    = clip(s, 0, 1)                        channel 6
    bits   = f32 -> float16, round to nearest even   normal.a, and the next tick's prev

grow32 is float32(record.foam_grow_rate); decay32 is the host's own expf(-(float)record.foam_decay_rate) (ow_schedule.hip frame_of), taken from
the C library through ctypes: np.exp's float32 result may differ from glibc's in the last place, and the comparison is exact.

THE SIGN OF A ZERO.  A zero compares equal to a zero of the other sign, in channel 6 and in normal.a, and nowhere else: -0 * decay + (-0) is -0,
and fmaxf(-0, +0) is either zero as far as C says.  same_f32 / same_f16 count the texels that needed the allowance.

The written planes hold every one of the 65 536 FP16 patterns exactly once per 256^2 texels -- negative values, values above 1, both zeros,
subnormals, infinities and NaNs with their payloads -- in a seeded random order, so a texel read from the wrong place is almost surely
another value; larger maps tile the block with another permutation per block and per cascade, 128^2 maps take a quarter of one.

Nothing here asserts about the code under test and nothing here builds."""
import collections
import ctypes as C
import functools

import numpy as np

SEED = 20261021
BLOCK = 256                       # 256^2 texels: exactly 65 536

Record = collections.namedtuple("Record", "whitecap grow decay")   # the three FP32 constants of one cascade's unpack, as the kernels get them


@functools.lru_cache(maxsize=1)
def _expf():
    f = C.CDLL("libm.so.6").expf
    f.argtypes, f.restype = [C.c_float], C.c_float
    return f


def decay32(foam_decay_rate):
    """expf(-(float)foam_decay_rate) of the C library: the host's own (ow_schedule.hip frame_of)"""
    return np.float32(_expf()(float(-np.float32(foam_decay_rate))))


def foam_rates(delta, foam_amount):
    """(foam_grow_rate, foam_decay_rate) one update with `delta` arms, in FP64 (wave_generator.gd:104-106; ow_schedule.hip set_foam_rates)"""
    d = 10.0 - foam_amount
    return delta * foam_amount * 7.5, delta * (d if d > 0.5 else 0.5) * 1.15


def record(whitecap, foam_grow_rate, foam_decay_rate):
    return Record(np.float32(whitecap), np.float32(foam_grow_rate), decay32(foam_decay_rate))


def record_of(p):
    """the Record of a parameter object after the update that armed its rates (WaveCascadeParameters, or the oracle's record)"""
    return record(p.whitecap, p.foam_grow_rate, p.foam_decay_rate)


def half_to_f32(bits):
    return np.ascontiguousarray(bits, np.uint16).view(np.float16).astype(np.float32)


def factor(J, rec):
    """fac of the docstring: FP32, >= 0 (or -0)"""
    return -np.minimum(np.float32(0.0), np.asarray(J, np.float32) - rec.whitecap)


def predict(prev_bits, J, rec):
    """one tick -> (expected channel 6 as float32, expected normal.a as uint16), the shape of prev_bits"""
    with np.errstate(all="ignore"):
        a = half_to_f32(prev_bits) * rec.decay
        s = a + factor(J, rec) * rec.grow
        s = np.where(np.isnan(s), np.float32(0.0), s)
        f32 = np.minimum(np.maximum(s, np.float32(0.0)), np.float32(1.0))
        assert a.dtype == s.dtype == f32.dtype == np.float32
        return f32, f32.astype(np.float16).view(np.uint16)


def fold(prev_bits, Js, records):
    """the exact trajectory over len(Js) ticks: [(channel 6, normal.a)] per tick, tick k from tick k - 1's bits"""
    out, bits = [], np.ascontiguousarray(prev_bits, np.uint16)
    for J, rec in zip(Js, records):
        f32, bits = predict(bits, J, rec)
        out.append((f32, bits))
    return out


def product_is_subnormal(prev_bits, rec):
    """where prev32 * decay32 is a non-zero FP32 subnormal"""
    with np.errstate(all="ignore"):
        a = np.abs(half_to_f32(prev_bits) * rec.decay)
    return (a > 0) & (a < np.finfo(np.float32).tiny)


def growth(J, rec):
    """(share of texels with fac > 0, share with fac == 0)"""
    fac = factor(J, rec)
    return float((fac > 0).mean()), float((fac == 0).mean())


def _same(got, want, magnitude, accept=None):
    bad = got != want
    zeros = bad & ((got & magnitude) == 0) & ((want & magnitude) == 0)
    bad &= ~zeros
    if accept is not None:
        bad &= ~(accept & ((got & magnitude) == 0))
    return int(bad.sum()), int(zeros.sum())


def same_f32(got, want, zero_where=None):
    """(texels whose FP32 bits differ, texels that are zeros of different signs and so count as equal).  zero_where: a mask of texels at which a
    zero is accepted whatever is expected (an FP32-subnormal prediction that a flushing multiplier turns into zero)"""
    g, w = np.ascontiguousarray(got, np.float32).view(np.uint32), np.ascontiguousarray(want, np.float32).view(np.uint32)
    return _same(g, w, np.uint32(0x7FFFFFFF), zero_where)


def same_f16(got_bits, want_bits):
    """the same for FP16 bit patterns (float16 or uint16 arrays)"""
    g, w = np.ascontiguousarray(got_bits).view(np.uint16), np.ascontiguousarray(want_bits).view(np.uint16)
    return _same(g, w, np.uint16(0x7FFF))


# ---- the written planes ----------------------------------------------------------------------------------------------------------------------

def plane(n, cascade=0, reverse=False, seed=SEED):
    """uint16 [n][n]: every 256^2 block a permutation of the 65 536 patterns of its own (seeded by block and cascade); at 128^2 the quarter
    `cascade % 4` of one.  reverse: the same texels in the opposite order, as device_maps.fp16_layout has."""
    if n < BLOCK:
        assert n * n * 4 == BLOCK * BLOCK
        flat = np.random.default_rng([seed, cascade // 4, 0, 0]).permutation(65536).astype(np.uint16)
        out = flat[(cascade % 4) * n * n:(cascade % 4 + 1) * n * n].reshape(n, n)
    else:
        assert n % BLOCK == 0
        out = np.empty((n, n), np.uint16)
        for by in range(n // BLOCK):
            for bx in range(n // BLOCK):
                block = np.random.default_rng([seed, cascade, by, bx]).permutation(65536).astype(np.uint16)
                out[by * BLOCK:(by + 1) * BLOCK, bx * BLOCK:(bx + 1) * BLOCK] = block.reshape(BLOCK, BLOCK)
    return np.ascontiguousarray(out.reshape(-1)[::-1].reshape(n, n) if reverse else out)


def private_index(n):
    """[n][n] -> where the context's private plane keeps texel (row x', column y'): Pass2::foam_index, restated -- a lane t of row x' holds the
    sixteen texels y' = t + (n / 16) o side by side"""
    xp, yp = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    t = n // 16
    return xp * n + (yp % t) * 16 + yp // t


def to_private(bits):
    """a plane [n][n] in the private plane's order (flat, n * n)"""
    bits = np.ascontiguousarray(bits, np.uint16)
    out = np.empty(bits.size, np.uint16)
    out[private_index(bits.shape[0]).ravel()] = bits.ravel()
    return out


def from_private(foam, n):
    """the private plane (flat) as texels [n][n]"""
    return np.ascontiguousarray(np.asarray(foam, np.uint16)[private_index(n)])


def write_plane(gen, cascade, bits):
    """bits (uint16 [n][n]) become normal.a of `cascade` (and, through ow_set_normal_map's scatter, the private plane); channels 0..2 are left as
    read back.  The bits travel as a float16 VIEW: set_normal_map converts its argument with np.ascontiguousarray(..., np.float16), which
    would turn a uint16 array into the halves nearest to its integers."""
    norm = gen.get_maps(cascade)[1].view(np.uint16).copy()
    norm[..., 3] = bits
    gen.set_normal_map(cascade, norm.view(np.float16))
    return norm
