#!/usr/bin/env python3
"""Writes tests/golden/ref_digests.json: SHA-256 digests (tests/helpers.py digest) of what the REFERENCE'S OWN shaders computed
(oracle/_ref/libglsl_ref.so) in the cases of tests/test_oracle_ref.py (every pinned stage of every frame) and
tests/test_surface_sampling.py (every pinned field).  Those tests hold the oracle to these digests bit for bit, so that the pins
hold where the reference checkout is absent.  Run where it exists:   make -C oracle ref && python tests/golden/make_ref_digests.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..", "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import helpers as H  # noqa: E402
import scenes as S  # noqa: E402
from godotoceanwaves_amd.presets import UPDATE_DELTA, cascade_preset  # noqa: E402
from oracle import ref as R  # noqa: E402


def main():
    if not R.available():
        raise SystemExit("oracle/_ref/libglsl_ref.so missing: run `make -C oracle ref` where the reference checkout exists")
    out = {"cascade": {}, "edge": {}, "sampling": {}}
    for n, ci, frames in H.CASCADE_CASES:
        rc = R.RefCascade(n, cascade_preset(ci))
        e = {"butterfly": H.digest(rc.butterfly), "frames": []}
        for _ in range(frames):
            rc.update(UPDATE_DELTA)
            e["frames"].append({"time": rc.time, **H.stage_digests(rc)})
        out["cascade"][f"n{n}_c{ci}"] = e
        print(f"cascade n{n}_c{ci}", flush=True)
    for name, preset in H.edge_cases():
        rc = R.RefCascade(128, preset)
        for _ in range(H.EDGE_FRAMES):
            rc.update(UPDATE_DELTA)
        out["edge"][name] = H.stage_digests(rc)
    for case in ("random_maps", "generated_maps", "spray_active", "fine_cascades"):
        d, m, sc, xz = S.sampling_case(case)
        out["sampling"][case] = S.ref_sampling_digests(*R.sample_surface(d, m, sc, xz))
    with open(H.REF_DIGESTS, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(H.REF_DIGESTS)


if __name__ == "__main__":
    main()
