#!/usr/bin/env python3
"""Per-texel margins of the spectrum kernel (k_spectrum: ow_device.h spectrum_amplitude_fast) against the oracle's literal form and the FP64 twin,
for every size and every record of tests/helpers.spectrum_records (presets, range edges, fuzzed records), eight records per context -- one in every
cascade slot.  Per (size, record) it prints, in the metric of tests/helpers.spectrum_margins (floor phi = H.SPEC_PHI):
  * device vs oracle: the max-norm error, the smallest rho that holds every texel above the floor (rho_needed) with SPEC_ARG_ULPS ulps of
    theta - angle allowed on top (np_twin.direction_ulp_sensitivity), the ulps needed at the test's rho, the worst ratio at the test's
    bounds, the share of texel-channels that need the floor, and the worst texel's (x, y, |k|);
  * device vs twin with kappa |oracle - twin| allowed on top (the same columns), and the oracle's own margins against the twin;
  * omega: texels that differ from the oracle's (bitwise) and texels that differ from their mirror (bitwise).
    python scripts/spectrum_margins.py [--emul] [n ...]     > profiles/spectrum_margins.txt
--emul: the kernel's form compiled for the CPU (tests/emul, over glibc's libm) instead of the device: the same formulas, other instructions.
The bounds of tests/test_spectrum_texels.py are set from one MI355X run of this script."""
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import helpers as H  # noqa: E402

SIZES = (128, 256, 512, 1024, 2048)


def measure(n, dev_h0c, ref):
    """dev_h0c: [n][n][2] complex (h0(k), conj h0(-k)) of the kernel's form; ref: (oracle, twin, omega, direction sensitivity) -> dict of margins"""
    oracle4, twin, _, sens = ref
    _, twin = H.zero_where_reference_is_not_finite(H.h0_complex(oracle4)[..., 0], twin)
    orc, dev_h0c = H.zero_where_reference_is_not_finite(H.h0_complex(oracle4), dev_h0c)
    sens2 = np.stack([sens, H.mirror(sens)], axis=-1)
    d2 = H.spectrum_margins(dev_h0c, orc, H.SPEC_RHO_ORACLE, sens2)
    d2["relmax"] = H.relmax(dev_h0c, orc)
    tw, sens1 = twin[..., None], sens[..., None]
    lit = np.abs(orc[..., :1] - tw)
    d3 = H.spectrum_margins(dev_h0c[..., :1], tw, H.SPEC_RHO_TWIN, sens1, extra=H.SPEC_KAPPA * lit)
    lo = H.spectrum_margins(orc[..., :1], tw, H.SPEC_RHO_LITERAL, sens1)
    return dict(oracle=d2, twin=d3, literal=lo)


def where(n, pc, at):
    y, x = int(at[0]), int(at[1])
    kx, ky = (x - n / 2) * 2 * math.pi / pc.tile_length[0], (y - n / 2) * 2 * math.pi / pc.tile_length[1]
    return f"({x},{y}) |k| {math.hypot(kx, ky):.4g}"


def main(argv):
    emul = "--emul" in argv
    sizes = [int(a) for a in argv if not a.startswith("-")] or list(SIZES)
    recs = H.spectrum_records()
    E = H.emul_library() if emul else None
    print(f"# spectrum texel margins: {'the CPU build of spectrum_amplitude_fast (glibc libm)' if emul else 'k_spectrum on the device'} vs the oracle and the FP64 twin")
    print(f"# phi {H.SPEC_PHI:g}; vs oracle rho {H.SPEC_RHO_ORACLE:g}; vs twin kappa {H.SPEC_KAPPA:g} rho {H.SPEC_RHO_TWIN:g}; oracle vs twin rho {H.SPEC_RHO_LITERAL:g}; ulps of theta - angle {H.SPEC_ARG_ULPS:g}")
    print("# size record slot | vs oracle: relmax rho_needed ulps_needed worst floor% at | vs twin: rho_needed ulps_needed worst floor% at | oracle vs twin: rho_needed ulps_needed worst | omega !=oracle !=mirror")
    tot = {}
    for n in sizes:
        for b in range(0, len(recs), 8):
            batch = recs[b:b + 8]
            pcs = [H.record_pc(r) for _, r in batch]
            t0 = time.time()
            dev = None if emul else H.device_spectra(n, [r for _, r in batch])
            t1 = time.time()
            refs = H.spectrum_references(n, pcs)
            t2 = time.time()
            for s, ((name, rec), pc, ref) in enumerate(zip(batch, pcs, refs)):
                if emul:
                    f = H.emul_fast_h0(E, n, pc)
                    h0c = np.stack([f, np.conj(H.mirror(f))], axis=-1)
                    om = ref[2]
                    words_ok = True
                else:
                    h0, om, words = dev[s]
                    h0c = H.h0_complex(h0)
                    words_ok = np.array_equal(words[:12], H.pc_words(pc))
                m = measure(n, h0c, ref)
                om_diff = int((om.view(np.uint32) != ref[2].view(np.uint32)).sum())
                om_sym = int((om.view(np.uint32) != H.mirror(om).view(np.uint32)).sum())
                finite = np.array_equal(np.isfinite(h0c), np.isfinite(H.h0_complex(ref[0])))  # (the reference's own log(0): see helpers)
                o, t, lo = m["oracle"], m["twin"], m["literal"]
                print(f"{n:5d} {name:30s} {s} | {o['relmax']:.2e} {o['rho_needed']:.2e} {o['ulps_needed']:5.2f} {o['worst']:6.3f} {o['floor_share']*100:8.5f} {where(n, pc, o['at']):28s}"
                      f" | {t['rho_needed']:.2e} {t['ulps_needed']:5.2f} {t['worst']:6.3f} {t['floor_share']*100:8.5f} {where(n, pc, t['at']):28s} | {lo['rho_needed']:.2e} {lo['ulps_needed']:5.2f} {lo['worst']:6.3f}"
                      f" | {om_diff} {om_sym}" + ("" if finite else "  NON-FINITE WHERE THE ORACLE IS FINITE") + ("" if words_ok else "  PUSH-CONSTANTS DIFFER"), flush=True)
                for key, v in (("relmax", o["relmax"]), ("rho_oracle", o["rho_needed"]), ("ulps_oracle", o["ulps_needed"]), ("floor_oracle", o["floor_share"]), ("rho_twin", t["rho_needed"]), ("ulps_twin", t["ulps_needed"]),
                               ("floor_twin", t["floor_share"]), ("rho_literal", lo["rho_needed"]), ("ulps_literal", lo["ulps_needed"]), ("worst_literal", lo["worst"]), ("worst_oracle", o["worst"]), ("worst_twin", t["worst"])):
                    tot[key] = max(tot.get(key, 0.0), v)
            print(f"# {n}^2 records {b}..{b + len(batch) - 1}: device {t1 - t0:.1f} s, oracle + twin {t2 - t1:.1f} s", flush=True)
    print("# worst over all: " + ", ".join(f"{k} {v:.3g}" for k, v in tot.items()))


if __name__ == "__main__":
    main(sys.argv[1:])
