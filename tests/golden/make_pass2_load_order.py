#!/usr/bin/env python3
"""Record tests/golden/pass2_load_order.json: run with the package of the commit BEFORE the pass-2 load order changed first on the path
(PYTHONPATH=<checkout of that commit, built>), on a GPU:
    PYTHONPATH=<parent> python tests/golden/make_pass2_load_order.py [out.json]
The schedules are those of tests/pass2_schedules.py, which tests/test_pass2_load_order.py replays; the file holds one SHA-1 and the kernel family per schedule."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.append(os.path.dirname(HERE))  # tests/ -- after PYTHONPATH, so that the package is the recorded commit's
import pass2_schedules as T  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
rec = {}
for case in T.CASES:
    sha, family = T.replay(case)
    rec[T.case_id(case)] = {"sha1": sha, "family": family}
    print(T.case_id(case), sha, family, flush=True)
with open(out, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
