"""The frame arithmetic bin by bin on injected spectra, without a GPU: the FP32 oracle and the CPU emulation of the device's lane code
(tests/emul/emul.cpp) against the FP64 twin, in the metrics of tests/frame_bins.py -- every wave number weighs the same, and the special lines
(the two Nyquist lines, the axes kx = 0 and ky = 0, the corner and the DC texel) are fed alone.  The oracle's own error is where the bounds
come from (helpers.FRAME_BIN_BOUNDS = four times it); the emulation is held to the bounds the device is held to
(tests/test_frame_bins_gpu.py); the teeth show that faults of the kind a kernel can have -- which the max norm over a channel cannot see on
a JONSWAP spectrum -- fail."""
import numpy as np
import pytest

import frame_bins as FB
import helpers as H

SIZES = (128, 256, 512, 1024)
BINS_2048 = ("hy", "hz", "dhx_dx")   # what the device cases compare at 2048^2 (a few seconds of FP64 transforms)


def _cases():
    """(n, tile index, input, who): the oracle and every entry point of the emulation that takes the size, grouped by input so that the
    twin of an input is computed once (frame_bins.cpu_case keeps the last two)"""
    out = []
    for n in SIZES:
        for ti in (0, 1):
            for name in FB.inputs(n):
                out += [(n, ti, name, who) for who in ["oracle"] + [e for e, sizes in FB.EMUL_ENTRIES.items() if n in sizes]]
    for ti in (0, 1):
        out += [(2048, ti, name, "oracle") for name in ("white", "lines")]
    return out


@pytest.mark.parametrize("n,ti,name,who", _cases(), ids=[f"{n}-{'square' if ti == 0 else 'nonsquare'}-{name}-{who}" for n, ti, name, who in _cases()])
def test_against_the_twin(n, ti, name, who):
    """Every input on both tiles: spatially over the seven non-foam channels, per bin on the white input.  The oracle stays within a QUARTER
    of each bound (the bounds are four times its worst figure: they cannot drift from their source); the emulation of every kernel family
    within the bound.  Foam, one tick from a zero plane: helpers.TOL_FOAM_ABS."""
    tile, h0, om, r = FB.cpu_case(n, ti, name)
    kind = FB.inputs(n)[name][0]
    if who == "oracle":
        a = FB.oracle_channels(h0, FB.T_FRAME, tile, **FB.UNPACK)
    else:
        a, disp, norm = FB.emul_channels(who, h0, om, FB.T_FRAME, tile, **FB.UNPACK)
        assert H.quantisation_exact(a, disp, norm)
    worst, what, figs = FB.worst_ratio(a, r, n, kind, bin_channels=BINS_2048 if n == 2048 else FB.BIN_CHANNELS)
    print(f"{n}^2 tile {tile} {name} {who}: " + ", ".join(f"{k} {v:.2e}" for k, v in figs.items()))
    assert np.isfinite(a).all()
    assert worst <= (0.25 if who == "oracle" else 1.0), what
    assert np.abs(a[..., 6] - r[..., 6]).max() <= H.TOL_FOAM_ABS


def test_the_inputs_are_what_they_say():
    """unit modulus on the support and nothing off it; ONE factor scales an input so that the largest derivative field peaks at 0.5"""
    n = 128
    for name, (kind, fn) in FB.inputs(n).items():
        u = fn(n, 3)
        on = u != 0
        assert np.allclose(np.abs(u[on]), 1.0)
        want = {"white": n * n, "lines": 2 * n - 1, "axes": 2 * n - 1, "point_pair": 2}.get(name, 1)
        assert on.sum() == want, name
        tile, h0, om, r = FB.cpu_case(n, 1, name)
        assert np.array_equal(h0 != 0, FB.inputs(n)[name][1](n, FB.SEED + 1) != 0)
        o = FB.twin_fields(h0, om, FB.T_FRAME, tile)
        peak = max(np.abs(v).max() for v in (o[1].imag, o[2].real, o[2].imag, o[3].real, o[3].imag))
        if name == "point_dc":   # kx = ky = 0: no derivative field at all, the elevation alone
            assert peak == 0 and abs(np.abs(o[0].imag).max() - 0.5) < 1e-5
        else:
            assert abs(peak - 0.5) < 1e-5, (name, peak)
    assert FB.tiles(256) == ((402.0, 402.0), (402.0, 302.0)) and FB.tiles(1024)[0] == (1608.0, 1608.0)


def test_the_per_bin_metric_reads_one_bin():
    """a cosine of relative size eps added to one channel moves exactly that bin's ratio to eps S / (S + phi rms S), and no other's"""
    n = 128
    tile, h0, om, r = FB.cpu_case(n, 0, "white")
    y, x = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    S = np.abs(np.fft.rfft2(r[..., 1])) / n ** 2
    a = r.copy()
    a[..., 1] += 2 * 1e-3 * S[9, 17] * np.cos(2 * np.pi * (9 * y + 17 * x) / n)
    v, at = FB.per_bin(a, r, ("hy",))["hy"]
    rms = np.sqrt((r[..., 1] ** 2).sum()) / n ** 2
    assert at == (9, 17) and v == pytest.approx(1e-3 * S[9, 17] / (S[9, 17] + FB.PHI_BIN * rms), rel=1e-6)
    assert FB.per_bin(a, r, ("hx",))["hx"][0] < 1e-12


def test_teeth():
    """Each mutant pushes a metric above its bound on the input named; the two whole-array mutants (one bin scaled, one column of bins
    rotated) stay below today's 1e-4 in the max norm on preset 2 at the same size -- that metric does not see them."""
    rows = FB.teeth(256)
    for row in rows:
        print(f"{row['mutant']:55s} {row['input']:13s} {row['ratio']:10.3g} x bound ({row['what']})" +
              ("" if row["today"] is None else f"; max norm on preset 2: {row['today']:.2e}"))
    assert len(rows) == 7 and len({row["mutant"][0] for row in rows}) == 6
    for row in rows:
        assert row["ratio"] > 1.0, row
        if row["mutant"][0] in "14":
            assert row["today"] < H.TOL_F32, row
    # ... and the algebra they are applied to is the twin's, unmutated
    tile, h0, om, r = FB.cpu_case(256, 1, "lines")
    a = FB.twin_channels(None, None, None, None, **FB.UNPACK, layers=FB.compact_layers(h0, om, FB.T_FRAME, tile))
    assert FB.worst_ratio(a, r, 256, "sparse")[0] < 1e-6
