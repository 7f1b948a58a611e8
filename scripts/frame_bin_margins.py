#!/usr/bin/env python3
"""The frame kernels bin by bin on injected spectra (tests/frame_bins.py): for every size, input, tile and channel the figures of the FP32 oracle,
of the CPU emulation of the device's lane code (every entry point of tests/emul/emul.cpp that takes the size) and -- unless --no-device -- of the
device, per case of tests/test_frame_bins_gpu.py (the same runs: tests/frame_bins.py run_gpu_case), all against the FP64 twin; then the teeth table of
tests/test_frame_bins.py.  Columns: the spatial figure of the seven non-foam channels (max|a - twin| over the maximum of the channel's group),
then, on the white input, the per-bin ratio of the linear channels.
    python scripts/frame_bin_margins.py [--no-device] [n ...]     > profiles/frame_bin_margins.txt
helpers.FRAME_BIN_BOUNDS are four times the ORACLE's worst figure per size and kind, as this script prints them."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import frame_bins as FB  # noqa: E402
import helpers as H  # noqa: E402

SIZES = (128, 256, 512, 1024, 2048)
BINS_2048 = ("hy", "hz", "dhx_dx")


def figures(a, r, n, kind):
    sp = FB.spatial(a, r)
    pb = FB.per_bin(a, r, BINS_2048 if n == 2048 else FB.BIN_CHANNELS) if kind == "white" else {}
    return sp, {k: v for k, (v, _) in pb.items()}


def row(label, sp, pb):
    return f"{label} | " + " ".join(f"{sp[H.CHANNELS[c]]:.2e}" for c in FB.SPATIAL_CHANNELS) + (" | " + " ".join(f"{k} {v:.2e}" for k, v in pb.items()) if pb else "")


def note(worst, who, n, kind, sp, pb):
    w = worst.setdefault((who, n), dict(spatial_white=0.0, spatial_sparse=0.0, bin_white=0.0))
    w["spatial_" + kind] = max(w["spatial_" + kind], max(sp.values()))
    if pb:
        w["bin_white"] = max(w["bin_white"], max(pb.values()))


def main(argv):
    device = "--no-device" not in argv
    sizes = [int(a) for a in argv if not a.startswith("-")] or list(SIZES)
    print("# frame kernels on injected spectra vs the FP64 twin; t = %g s, phi = %g; bounds (helpers.FRAME_BIN_BOUNDS) = 4 x the oracle's worst per size and kind" % (FB.T_FRAME, FB.PHI_BIN))
    print("# size tile input who | spatial: " + " ".join(H.CHANNELS[c] for c in FB.SPATIAL_CHANNELS) + " | per bin (white)")
    worst = {}
    for n in sizes:
        t0 = time.time()
        names = list(FB.inputs(n)) if n < 2048 else ["white", "lines"]
        for ti in (0, 1):
            for name in names:
                kind = FB.inputs(n)[name][0]
                tile, h0, om, r = FB.cpu_case(n, ti, name)
                for who in ["oracle"] + [e for e, s in FB.EMUL_ENTRIES.items() if n in s]:
                    a = FB.oracle_channels(h0, FB.T_FRAME, tile, **FB.UNPACK) if who == "oracle" else FB.emul_channels(who, h0, om, FB.T_FRAME, tile, **FB.UNPACK)[0]
                    sp, pb = figures(a, r, n, kind)
                    note(worst, who, n, kind, sp, pb)
                    print(row(f"{n:5d} {tile[0]:g}x{tile[1]:g} {name:15s} {who:18s}", sp, pb), flush=True)
        print(f"# {n}^2: oracle and emulation {time.time() - t0:.1f} s", flush=True)
    if device:
        print("# device: size x cascades path kernels family | cascade tile input | spatial | per bin (white) | wall time of the case")
        for name, n, cascades, path, kernels, family, ticks in FB.gpu_cases():
            if n not in sizes:
                continue
            t0 = time.time()
            got_family, hits, layers = FB.run_gpu_case(name, n, cascades, path, kernels, ticks)
            kind = FB.inputs(n)[name][0]
            for i, d in enumerate(layers):
                sp, pb = figures(d["f32"], d["twin"], n, kind)
                note(worst, f"device {path} {kernels or 'default'} -> {got_family}", n, kind, sp, pb)
                foam = np.abs(d["f32"][..., 6] - d["oracle_foam"]).max()
                print(row(f"{n:5d}x{cascades} {path:10s} {kernels or 'default':22s} {got_family:22s} | {i} {d['tile'][0]:g}x{d['tile'][1]:g} {name:15s}", sp, pb) +
                      f" | foam vs oracle {foam:.1e} hits {hits}" + ("" if got_family == family else f"  FAMILY IS NOT {family}"), flush=True)
            print(f"# {n}x{cascades} {path} {kernels or 'default'} {name}: {time.time() - t0:.1f} s", flush=True)
    print("# worst per size (and its share of the bound): who size | spatial white, spatial sparse, per bin white")
    for (who, n), w in worst.items():
        b = H.FRAME_BIN_BOUNDS[n]
        print(f"# {who:60s} {n:5d} | " + ", ".join(f"{w[k]:.2e} ({w[k] / b[k]:.2f})" for k in ("spatial_white", "spatial_sparse", "bin_white")), flush=True)
    print("# teeth (256^2, non-square tile): mutant | input | worst figure over its bound | today's metric (max norm over a channel, preset 2) where the mutant is a whole-array one")
    for t in FB.teeth(256):
        print(f"# {t['mutant']:55s} | {t['input']:13s} | {t['ratio']:10.3g} ({t['what']})" + ("" if t["today"] is None else f" | {t['today']:.2e} (< 1e-4: not seen)"), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
