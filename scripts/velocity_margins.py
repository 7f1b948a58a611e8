#!/usr/bin/env python3
"""The floors the velocity layers need against the FP64 twin (tests/velocity_twin.py), for the cases of tests/test_velocity_layers.py: every
record of tests/helpers.spectrum_records at 256^2, the non-square and extreme records at the other plans (one tick of update_all, three of
run), and the long-session phases.  Per case it prints the smallest rel_floor at which helpers.fp16_close(layer, twin as FP16, ulps=1) passes
    * for the device's layer (k_velocity_pass1 / k_velocity_pass2 on the MI355X), and
    * for the CPU lane emulation (tests/velocity/velocity_emul.cpp: the same algorithm, contraction off, another compiler) fed the very same
      spectrum and words,
and then, without a device: max|v| of the calm record's twin, and for the long-session cases the distance between the twin with the unit
phasors of the CPU build of expi_phase and the twin with exact phasors, relative to max|v|.
    python scripts/velocity_margins.py [--emul]     >> profiles/velocity_margins.txt
--emul: no device; the spectrum is the oracle's, the words come from the record (the device column is left out).
The rule for the floors is in tests/test_velocity_layers.py (FLOORS)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import helpers as H  # noqa: E402
import velocity_twin as VT  # noqa: E402
from godotoceanwaves_amd.presets import DEPTH, UPDATE_DELTA, cascade_preset  # noqa: E402
from oracle import oracle as O  # noqa: E402

FLOOR = 2e-5  # tests/test_water_velocity.py
LONG_SESSIONS = [(1024, 2, 86400.0), (256, 7, 14400.0), (1024, 0, 3600.0)]
WORST = {}


def extreme_records():
    from edge_presets import edge_presets
    e = edge_presets()
    return [(k, e[k]) for k in ("non_square_tile", "late_time", "wrapping_seed", "gale_long_fetch")]


def oracle_inputs(n, rec, ticks):
    pc = H.record_pc(rec)
    t = rec["time"]
    for _ in range(ticks):
        t += UPDATE_DELTA
    return O.spectrum_compute(n, pc), O.omega(n, (pc.tile_length[0], pc.tile_length[1]), pc.depth), VT.modulate_words(rec["tile_length"], t, DEPTH)


def report(n, what, name, rec, h0, om, words, layer, m=None):
    want = VT.velocity_twin(h0, om, words, m=None if m is None else m(VT.phases(om, words)))
    e = VT.floor_needed(VT.emul_layer(h0, om, words), want)
    d = None if layer is None else VT.floor_needed(layer, want)
    f = np.asarray(words, np.uint32).view(np.float32)
    dev = "" if d is None else f" device {d:.2e}"
    flag = "" if max(d or 0.0, e) <= FLOOR else "   ABOVE FLOOR"
    print(f"{n:5d} {what:10s} {name:30s} tile {f[0]:8.3f} x {f[1]:8.3f} t {f[3]:10.3f} max|v| {np.abs(want).max():9.3e} | floor needed:{dev} emulation {e:.2e}{flag}", flush=True)
    for k, v in (("device", d), ("emulation", e)):
        if v is not None:
            WORST[k] = max(WORST.get(k, 0.0), v)


def run_context(n, what, recs, ticks, emul, m=None):
    if emul:
        for name, rec in recs:
            report(n, what, name, rec, *oracle_inputs(n, rec, ticks), None, m)
        return
    from godotoceanwaves_amd import WaveCascadeParameters, WaveGenerator
    gen = WaveGenerator()
    gen.map_size = n
    gen.init_gpu(max(2, len(recs)))
    try:
        params = [WaveCascadeParameters(**r) for _, r in recs]
        if what == "run":
            gen.run(UPDATE_DELTA, params, ticks)
        else:
            for _ in range(ticks):
                gen.update_all(UPDATE_DELTA, params)
        for i, (name, rec) in enumerate(recs):
            layer = gen.velocity_map(i)
            h0, om = gen.get_spectrum(i)
            report(n, what, name, rec, h0, om, gen.get_push_constants(i)[1], layer, m)
    finally:
        gen.free()


def main(argv):
    emul = "--emul" in argv
    who = "CPU emulation only, the oracle's spectrum" if emul else "MI355X and the CPU emulation, the device's spectrum and words"
    print(f"# floors needed by the velocity layers against the FP64 twin at one FP16 ulp ({who}); FLOOR = {FLOOR:g}")
    print("# size schedule record | tile, time word, max|v| of the twin | floor needed")
    recs = H.spectrum_records()
    for b in range(0, len(recs), 8):
        run_context(256, "update_all", recs[b:b + 8], 2, emul)
    for n in (128, 512, 1024, 2048):
        run_context(n, "update_all", extreme_records(), 1, emul)
        run_context(n, "run", extreme_records(), 3, emul)
    print("# long-session phases: the twin takes its unit phasors from the CPU build of expi_phase (sincos_phase) at the FP32 phases")
    for n, ci, t0 in LONG_SESSIONS:
        run_context(n, "update_all", [(f"preset{ci}_t{t0:g}", dict(cascade_preset(ci), time=t0))], 2, emul, m=VT.emul_phasors)
    print("# worst floor needed: " + ", ".join(f"{k} {v:.2e}" for k, v in WORST.items()))
    print("# without a device (the oracle's spectrum):")
    for n, ci, t0 in LONG_SESSIONS:
        h0, om, words = oracle_inputs(n, dict(cascade_preset(ci), time=t0), 2)
        exact = VT.velocity_twin(h0, om, words)
        own = VT.velocity_twin(h0, om, words, m=VT.emul_phasors(VT.phases(om, words)))
        ph = VT.phases(om, words)
        print(f"{n:5d} preset{ci} t0 {t0:g}: largest phase {float(ph.max()):.4g} rad; twin with expi_phase's phasors vs the exact-m twin: "
              f"{np.abs(own - exact).max() / np.abs(exact).max():.2e} of max|v| ({np.abs(exact).max():.3e} m/s)")
    from edge_presets import edge_presets
    h0, om, words = oracle_inputs(256, edge_presets()["calm_min_wind_short_fetch"], 0)
    print(f"  256 calm_min_wind_short_fetch: max|h0| {np.abs(h0).max():.3e} (FP32), max|v| of the twin {np.abs(VT.velocity_twin(h0, om, words)).max():.3e} m/s")


if __name__ == "__main__":
    main(sys.argv[1:])
