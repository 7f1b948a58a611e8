"""The frame kernels bin by bin on injected spectra (ow_debug_set_spectrum), every kernel family at the smallest shape it exists at, against
the FP64 twin in the metrics of tests/frame_bins.py -- the bounds come from the oracle's own error (helpers.FRAME_BIN_BOUNDS,
tests/test_frame_bins.py), never from the device.  A context generates its spectra once (one tick of preset records on the case's tile
lengths), gets a different input seed per cascade -- the square tile on cascade 0, the non-square one on cascade 1, so that a slot mix-up
shows --, a zero foam plane, and runs the path under test with clean records."""

import numpy as np
import pytest

import frame_bins as FB
import helpers as H
from godotoceanwaves_amd import WaveCascadeParameters, WaveGenerator, _lib
from godotoceanwaves_amd.presets import UPDATE_DELTA, cascade_preset
from frame_bins import _h0, _seed, _tile, gpu_cases as _cases, run_gpu_case as run_case

pytestmark = pytest.mark.gpu

# (n, cascades, path, kernels, family asserted, ticks of the path): the smallest shape at which each kernel exists
BINS_2048 = ("hy", "hz", "dhx_dx")


@pytest.mark.parametrize("name,n,cascades,path,kernels,family,ticks", _cases(),
                         ids=[f"{n}x{c}-{path}-{kernels or 'default'}-{name}" for name, n, c, path, kernels, family, ticks in _cases()])
def test_injected_spectrum(name, n, cascades, path, kernels, family, ticks):
    """ow_get_spectrum returns the injected h0 and its mirror bit for bit; both metrics against the twin within the oracle-derived bounds; the
    FP16 maps are the exact quantisation of the FP32 channels; foam after one tick from a zero plane within TOL_FOAM_ABS of the oracle's
    (through ow_run the compared tick is the last of three: foam is only bounded to [0, 1]); the launch took the family the case names."""
    got_family, hits, layers = run_case(name, n, cascades, path, kernels, ticks)
    assert got_family == family
    if path == "lookahead":
        assert hits > 0, "the last tick did not take the pass 1 computed ahead"
    margin = H.FRAME_BIN_FAMILY_MARGIN.get(family, 1.0)
    for i, d in enumerate(layers):
        assert np.array_equal(d["spectrum"].view(np.uint32), FB.spectrum_texels(d["h0"]).view(np.uint32)), "ow_get_spectrum is not the injected h0 and its mirror"
        f32 = d["f32"]
        worst, what, figs = FB.worst_ratio(f32, d["twin"], n, FB.inputs(n)[name][0], bin_channels=BINS_2048 if n == 2048 else FB.BIN_CHANNELS, margin=margin)
        print(f"{n}^2 cascade {i} tile {d['tile']} {name}: " + ", ".join(f"{k} {v:.2e}" for k, v in figs.items()))
        assert np.isfinite(f32).all()
        assert worst <= 1.0, f"cascade {i}: {what}"
        assert H.quantisation_exact(f32, d["disp"], d["norm"])
        if path != "run":
            assert np.abs(f32[..., 6] - d["oracle_foam"]).max() <= H.TOL_FOAM_ABS
        else:
            assert f32[..., 6].min() >= 0.0 and f32[..., 6].max() <= 1.0


# ---- the hook itself ----
def _small(kernels=None):
    n = 256
    gen = WaveGenerator()
    gen.map_size = n
    gen.debug_f32 = True
    gen.kernels = kernels
    gen.init_gpu(2)
    params = [WaveCascadeParameters(**dict(cascade_preset(i), tile_length=_tile(n, 2, i), time=FB.T_FRAME)) for i in range(2)]
    return n, gen, params


def test_hook_arguments_and_state():
    n, gen, params = _small()
    try:
        h0 = _h0(n, _tile(n, 2, 0), "white", _seed(0))
        with pytest.raises(_lib.OceanWavesError) as e:   # no spectrum has been generated: there are no push-constant words a clean record could match
            gen.debug_set_spectrum(0, h0)
        assert e.value.status == _lib.OW_ERR_STATE
        gen.update_all(UPDATE_DELTA, params[:1])          # cascade 0 alone: cascade 1 still has none
        gen.debug_set_spectrum(0, h0)
        with pytest.raises(_lib.OceanWavesError) as e:
            gen.debug_set_spectrum(1, h0)
        assert e.value.status == _lib.OW_ERR_STATE
        L = gen._lib
        assert L.ow_debug_set_spectrum(gen.context, 0, None, None) == _lib.OW_ERR_INVALID
        assert L.ow_debug_set_spectrum(gen.context, 2, h0.ctypes.data, None) == _lib.OW_ERR_INVALID and b"out of range" in L.ow_last_error()
        assert L.ow_debug_set_spectrum(gen.context, -1, h0.ctypes.data, None) == _lib.OW_ERR_INVALID
        assert np.array_equal(gen.get_spectrum(0)[0], FB.spectrum_texels(h0))
    finally:
        gen.free()


def test_injection_drops_what_was_computed_ahead():
    """three ticks with one delta leave pass 1 of the next ticks in the look-ahead queue, computed from the OLD spectrum: an injection followed by one more
    tick gives, bit for bit, the maps of a context that injected before those ticks"""
    n, a, pa = _small()
    _, b, pb = _small()
    try:
        h0 = [_h0(n, _tile(n, 2, i), "white", _seed(i)) for i in range(2)]
        zero = np.zeros((n, n, 4), np.float16)
        for gen, params, inject_after in ((a, pa, 3), (b, pb, 1)):
            for tick in range(1, 4):
                gen.update_all(UPDATE_DELTA, params)
                if tick == inject_after:
                    if gen is a:
                        assert gen.lookahead_stats()[1] > 0, "nothing was computed ahead: the case does not test what it says"
                    for i in range(2):
                        gen.debug_set_spectrum(i, h0[i])
            for i in range(2):
                gen.set_normal_map(i, zero)
            hits = gen.lookahead_stats()[0]
            gen.update_all(UPDATE_DELTA, params)
            gen.sync()
            assert (gen.lookahead_stats()[0] > hits) == (gen is b)   # a recomputes its pass 1; b takes the one it computed ahead from the injected spectrum
        for i in range(2):
            assert np.array_equal(a.get_maps_f32(i).view(np.uint32), b.get_maps_f32(i).view(np.uint32))
            for ma, mb in zip(a.get_maps(i), b.get_maps(i)):
                assert np.array_equal(ma.view(np.uint16), mb.view(np.uint16))
        assert pa[0].time == pb[0].time
    finally:
        a.free()
        b.free()


def test_injected_spectrum_stays_until_the_next_generation():
    """a dirty record that packs to the resident words keeps it (the flag is consumed: ow_spectrum_stats counts a skip); other words replace it"""
    n, gen, params = _small()
    try:
        gen.update_all(UPDATE_DELTA, params)
        h0 = _h0(n, _tile(n, 2, 0), "lines", _seed(0))
        gen.debug_set_spectrum(0, h0)
        want = FB.spectrum_texels(h0)
        generated, skipped = gen.spectrum_stats()
        params[0].whitecap = params[0].whitecap   # every setter raises the flag (wave_cascade_parameters.gd:32-35); the thirteen words do not change
        assert params[0].should_generate_spectrum
        gen.update_all(UPDATE_DELTA, params)
        gen.sync()
        assert gen.spectrum_stats() == (generated, skipped + 1) and np.array_equal(gen.get_spectrum(0)[0], want)
        params[0].wind_speed = 14.0
        gen.update_all(UPDATE_DELTA, params)
        gen.sync()
        assert gen.spectrum_stats() == (generated + 1, skipped + 1)
        got = gen.get_spectrum(0)[0]
        p = dict(cascade_preset(0), tile_length=_tile(n, 2, 0), wind_speed=14.0)
        from oracle import oracle as O
        assert not np.array_equal(got, want) and H.relmax(got, O.spectrum_compute(n, H.spectrum_pc(p))) < 2e-5
    finally:
        gen.free()
