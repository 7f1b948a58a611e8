"""The velocity kernels (godotoceanwaves_amd/csrc/ow_velocity_kernels.h: k_velocity_pass1 / k_velocity_pass2) off the square presets: non-square
tiles, the range-edge and fuzzed records, long-session phases, launch slots that are not their cascades -- and without a GPU.

CPU: tests/velocity/velocity_emul.cpp steps the lanes of a block through the kernels' own load, stage and epilogue functions (g++,
-ffp-contract=off); its layer and its pass-1 intermediate are held to the FP64 twin (tests/velocity_twin.py) from the oracle's spectrum, and the
twin itself is shown to tell the mistakes these tests are for.  GPU: the layers against the twin fed with the device's own spectrum and words.
The floors: FLOOR of tests/test_water_velocity.py for every record; a record with a floor of its own would be listed in FLOORS with the line of
profiles/velocity_margins.txt (scripts/velocity_margins.py) that measured it -- none needs one."""
import functools

import numpy as np
import pytest

import helpers as H
import velocity_twin as VT
from edge_presets import edge_presets
from godotoceanwaves_amd import WaveCascadeParameters, WaveGenerator
from godotoceanwaves_amd.presets import DEPTH, UPDATE_DELTA, cascade_preset
from oracle import oracle as O
from checks import check_layer, VELOCITY_FLOOR as FLOOR

SIZES = (128, 256, 512, 1024, 2048)
CALM = "calm_min_wind_short_fetch"
# record name -> its own floor (twice the device's measured need, never above H.TOL_F32), with the measurement cited.  Empty: on the MI355X
# no record at any size needs more than FLOOR (profiles/velocity_margins.txt, "floor needed").
FLOORS = {}
LONG_SESSIONS = [(1024, 2, 86400.0), (256, 7, 14400.0), (1024, 0, 3600.0)]  # tests/test_gpu_parity.py test_parity_holds_at_the_phases_of_a_long_session


def floor_of(name):
    f = FLOORS.get(name, FLOOR)
    assert f <= H.TOL_F32  # the cap: nothing beyond north_star's tolerance passes, whatever was measured
    return f


def is_calm(rec):
    """A fetch at the exported setter's clamped minimum (0.1 m): the whole FP32 spectrum underflows to +-0 and so does V (max|v| = 0, measured:
    profiles/velocity_margins.txt) -- calm_min_wind_short_fetch and fuzz10 of helpers.spectrum_records.  Decided by the record, not by the
    result: for these alone the layer's non-triviality check is replaced by finiteness and the metric."""
    return rec["fetch_length"] <= 1e-4


def record(name):
    """a record by name: 'presetN' or a range-edge preset"""
    return cascade_preset(int(name[6:])) if name.startswith("preset") else edge_presets()[name]


def extreme_records():
    """(name, record): the non-square tile, the largest phases, the wrapping seed at t = 0 exactly and the largest tile with the strongest wind"""
    e = edge_presets()
    assert e["wrapping_seed"]["time"] == 0.0 and e["non_square_tile"]["tile_length"][0] != e["non_square_tile"]["tile_length"][1]
    return [(k, e[k]) for k in ("non_square_tile", "late_time", "wrapping_seed", "gale_long_fetch")]


# ---- CPU: the lane emulation against the twin ----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def cpu_case(n, name):
    """the oracle's spectrum of a record, its words, the twin, its row transform, and the emulation's layer and intermediate (computed once)"""
    rec = record(name)
    pc = H.record_pc(rec)
    h0 = O.spectrum_compute(n, pc)
    om = O.omega(n, (pc.tile_length[0], pc.tile_length[1]), pc.depth)
    words = VT.modulate_words(rec["tile_length"], rec["time"], DEPTH)
    layer, inter = VT.emul_layer(h0, om, words, intermediate=True)
    out = dict(h0=h0, om=om, words=words, twin=VT.velocity_twin(h0, om, words), rows=VT.velocity_row_transform(h0, om, words), layer=layer, inter=inter)
    for v in out.values():
        v.setflags(write=False)
    return out


CPU_CASES = [(n, "non_square_tile") for n in SIZES] + [(n, name) for n in (128, 256, 512) for name in ("late_time", "wrapping_seed", "gale_long_fetch", "preset7")]


@pytest.mark.parametrize("n,name", CPU_CASES)
def test_emulated_layer_against_the_twin(n, name):
    c = cpu_case(n, name)
    got, want = c["layer"], c["twin"]
    assert np.all(got[..., 3].view(np.uint16) == 0)
    assert np.isfinite(got.astype(np.float32)).all()
    r = H.fp16_close(got[..., :3], want.astype(np.float16), ulps=1, rel_floor=floor_of(name))
    print(f"{name} {n}^2: emulated layer vs twin: ratio {r:.3f}, floor needed {VT.floor_needed(got, want):.2e}, max|v| {np.abs(want).max():.3g}")
    assert r <= 1.0, r
    assert np.abs(want).max() > 1e-3


@pytest.mark.parametrize("n,name", CPU_CASES)
def test_emulated_intermediate_against_the_twins_row_transform(n, name):
    """the transposed, tiled S layout on its own: pass 1 alone, un-tiled the way pass 2 reads it, against N ifft along kx -- the bound of
    tests/test_gpu_parity.py test_frame_parity_vs_oracle for the frame kernels' intermediate"""
    c = cpu_case(n, name)
    for layer in range(2):
        e = H.relmax(c["inter"][layer], c["rows"][layer])
        print(f"{name} {n}^2 layer {layer}: intermediate vs the twin's row transform {e:.2e}")
        assert e < 1e-5, (layer, e)


def test_twiddle_table_is_fp64_rounded_once():
    for n in SIZES:
        tw = np.zeros((n, 2), np.float32)
        VT.emul_library().velemul_twiddles(n, tw.reshape(-1))
        a = 2 * np.pi * np.arange(n) / n
        want = np.stack([np.cos(a), np.sin(a)], axis=-1)
        assert np.abs(tw - want).max() <= 2.0 ** -25  # half an FP32 ulp below 1
        assert tw[n // 4, 0] == 0.0 and tw[n // 2, 1] == 0.0 and tw[0, 0] == 1.0  # sincospi: exact at the quarter turns


def test_the_twin_has_teeth():
    """the mistakes the layer tests are for, made in the twin alone on the non-square record at 256^2: each must miss the true twin by at
    least ten times the allowance of the layer metric (a condition on this record, not a measurement)"""
    n, name = 256, "non_square_tile"
    c = cpu_case(n, name)
    h0, om, words, want = c["h0"], c["om"], c["words"], c["twin"].astype(np.float16)
    rec = record(name)
    unmirrored = h0.copy()
    unmirrored[..., 2], unmirrored[..., 3] = h0[..., 0], -h0[..., 1]  # conj(h0(k)) where conj(h0(-k)) belongs
    mutants = {
        "tile_x and tile_y exchanged": VT.velocity_twin(h0, om, VT.modulate_words(rec["tile_length"][::-1], rec["time"], DEPTH)),
        "the spare half of layer B left empty": VT.velocity_twin(h0, om, words, empty_spare_half=True),
        "the time word of another cascade": VT.velocity_twin(h0, om, VT.modulate_words(rec["tile_length"], cascade_preset(1)["time"], DEPTH)),
        "h0m un-mirrored": VT.velocity_twin(unmirrored, om, words),
    }
    for what, v in mutants.items():
        r = H.fp16_close(v.astype(np.float16), want, ulps=1, rel_floor=FLOOR)
        print(f"{what}: {r:.1f} times the allowance")
        assert r >= 10.0, (what, r)


def test_a_calm_sea_does_not_pass_vacuously():
    """the clamped minima of wind and fetch: the twin's layer lies below FP16's range (max|v| is printed and kept in
    profiles/velocity_margins.txt), so the metric compares zeros -- the layer must still be finite, w = 0, and within the metric"""
    c = cpu_case(256, CALM)
    got, want = c["layer"], c["twin"]
    print(f"{CALM} 256^2: max|v| of the twin {np.abs(want).max():.3e}, of the emulated layer {np.abs(got.astype(np.float64)).max():.3e}")
    assert np.isfinite(got.astype(np.float32)).all() and np.isfinite(want).all()
    assert np.all(got[..., 3].view(np.uint16) == 0)
    assert H.fp16_close(got[..., :3], want.astype(np.float16), ulps=1, rel_floor=FLOOR) <= 1.0
    # measured: this record's FP32 spectrum is +-0 in every texel (its energy underflows), max|v| = 0 -- what is left to go wrong is a NaN
    # from the wave-vector arithmetic (0 / k at the centre texel, 0 * omega) or a set w channel, both asserted above; signed zeros remain
    assert (np.abs(got[..., :3].astype(np.float32)) <= np.abs(want).max() + 2.0 ** -24).all()


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------

def make_context(n, recs, cascades=None):
    gen = WaveGenerator()
    gen.map_size = n
    gen.init_gpu(max(2, len(recs)) if cascades is None else cascades)
    return gen, [WaveCascadeParameters(**r) for r in recs]


@pytest.mark.gpu
@pytest.mark.parametrize("batch", range(4))
def test_every_record_at_256(batch):
    """helpers.spectrum_records(): the eight presets, the ten range-edge presets and the fuzzed FP64 records (about 40 % non-square), eight per
    context, one in every cascade slot; two ticks"""
    recs = H.spectrum_records()
    assert len(recs) == 32
    recs = recs[8 * batch:8 * batch + 8]
    gen, params = make_context(256, [r for _, r in recs])
    try:
        for _ in range(2):
            gen.update_all(UPDATE_DELTA, params)
        assert [name for name, rec in H.spectrum_records() if is_calm(rec)] == [CALM, "fuzz10"]
        for i, (name, rec) in enumerate(recs):
            r = check_layer(gen, i, floor=floor_of(name), calm=is_calm(rec))
            print(f"{name}: ratio {r:.3f}")
        assert gen.velocity_stats()[0] == len(recs)
    finally:
        gen.free()


@pytest.mark.gpu
@pytest.mark.parametrize("schedule", ["update_all", "run"])
@pytest.mark.parametrize("n", [128, 512, 1024, 2048])
def test_non_square_and_extreme_records_at_every_plan(n, schedule):
    """R0, W and THREADS differ per size (VelPlan): one tick through update_all and, in a context of its own, three through run"""
    recs = extreme_records()
    gen, params = make_context(n, [r for _, r in recs])
    try:
        if schedule == "update_all":
            gen.update_all(UPDATE_DELTA, params)
        else:
            gen.run(UPDATE_DELTA, params, 3)
        for i, (name, _) in enumerate(recs):
            r = check_layer(gen, i, floor=floor_of(name))
            print(f"{n}^2 {schedule} {name}: ratio {r:.3f}")
    finally:
        gen.free()


@pytest.mark.gpu
@pytest.mark.parametrize("n,ci,t0", LONG_SESSIONS)
def test_long_session_phases(n, ci, t0):
    """omega t of 1e5 .. 1e6 rad: sincos_phase's three-step reduction is inexact there, a property of the maps' own pass 1 that
    tests/test_gpu_parity.py accepts.  V is the derivative of what the maps hold, so the twin takes its unit phasors from the CPU build of
    expi_phase at the same FP32 phases, widened; the floor stays FLOOR.  (Its distance to the exact-m twin: profiles/velocity_margins.txt.)"""
    rec = dict(cascade_preset(ci), time=t0)
    gen, params = make_context(n, [rec])
    try:
        for _ in range(2):
            gen.update_all(UPDATE_DELTA, params)
        r = check_layer(gen, 0, m=VT.emul_phasors)
        print(f"{n}^2 preset {ci} t0 {t0}: ratio {r:.3f}")
    finally:
        gen.free()


def sparse_records():
    e = edge_presets()
    return [("non_square_tile", e["non_square_tile"]), ("preset1", cascade_preset(1)),
            ("preset5_non_square", dict(cascade_preset(5), tile_length=(137.0, 61.0), time=77.25)), ("late_time", e["late_time"])]


@pytest.mark.gpu
def test_sparse_masks_put_cascades_in_other_launch_slots():
    """VelocityArgs maps launch slots to layers: with the mask [1, 3] slot 0 computes layer 1 and slot 1 layer 3, each with its own tile
    lengths and time -- the content is checked, not only the counters"""
    recs = sparse_records()
    gen, params = make_context(256, [r for _, r in recs])
    try:
        gen.update_all(UPDATE_DELTA, params)
        gen.update_velocity([1, 3])
        assert gen.velocity_stats() == (2, 0)
        for i in (1, 3):
            check_layer(gen, i)  # (velocity_map: the layer is current, nothing is computed)
        assert gen.velocity_stats()[0] == 2
        c0, s0 = gen.velocity_stats()
        gen.update_velocity([0, 2, 3])
        assert gen.velocity_stats() == (c0 + 2, s0 + 1)
        for i in range(4):
            check_layer(gen, i)
        gen.velocity_ptrs()  # refreshes every computed layer: all are current
        assert gen.velocity_stats()[0] == 4
    finally:
        gen.free()


@pytest.mark.gpu
def test_sparse_masks_on_two_cascades_where_the_batch_fills_exactly():
    recs = sparse_records()[::3]  # the non-square tile and the largest phases
    gen, params = make_context(256, [r for _, r in recs])
    try:
        gen.update_all(UPDATE_DELTA, params)
        gen.update_velocity([0, 1])  # vel_slots = 2: one full launch pair
        assert gen.velocity_stats() == (2, 0)
        for i in range(2):
            check_layer(gen, i)
        assert gen.velocity_stats()[0] == 2
        gen.update_all(UPDATE_DELTA, params)
        gen.update_velocity([1])  # slot 0 computes layer 1
        assert gen.velocity_stats()[0] == 3
        check_layer(gen, 1)
        assert gen.velocity_stats()[0] == 3
        c0, s0 = gen.velocity_stats()
        gen.update_velocity([0, 1])
        assert gen.velocity_stats() == (c0 + 1, s0 + 1)
        for i in range(2):
            check_layer(gen, i)
    finally:
        gen.free()
