#!/usr/bin/env python3
"""Records tests/golden/schedule_counters.json: the scripted call sequence of tests/schedule_script.py on every configuration there, the
scheduler's exported counters after every call and a SHA-256 of every map at the end.  Run it on an MI355X from the commit whose schedule is
to be pinned (it uses the public wrapper only), BEFORE the scheduler is changed; tests/test_schedule_counters.py replays it.
    python scripts/record_schedule_counters.py <commit the library was built from> [output file]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import schedule_script as S  # noqa: E402

def write(record, path):
    """one call per line, so that a re-recording reads as a diff of the calls that changed"""
    one = lambda v: json.dumps(v, separators=(", ", ": "))
    configs = []
    for name, r in record["configurations"].items():
        calls = ",\n".join("   " + one(c) for c in r["calls"])
        digests = ",\n".join("   " + one(d) for d in r["digests"])
        configs.append(f'  {one(name)}: {{\n   "calls": [\n{calls}\n   ],\n   "digests": [\n{digests}\n   ]\n  }}')
    with open(path, "w") as f:
        f.write(f'{{\n "recorded_from": {one(record["recorded_from"])},\n "counters": {one(record["counters"])},\n "configurations": {{\n'
                + ",\n".join(configs) + "\n }\n}\n")


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "schedule_counters.json")
    record = {"recorded_from": sys.argv[1], "counters": list(S.COUNTERS), "configurations": {}}
    for n, count in S.CONFIGS:
        record["configurations"][S.key(n, count)] = r = S.replay(n, count)
        print(f"{n}^2 x {count}: {len(r['calls'])} calls, last {r['calls'][-1][1]}", flush=True)
    write(record, out)
    print(out)
