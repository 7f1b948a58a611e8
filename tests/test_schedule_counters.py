"""The frame scheduler's decisions, pinned: tests/schedule_script.py's fixed call sequence -- update_all with repeating and changing deltas, the
reference's schedule with and without a leftover, a tile-length and a whitecap edit, readbacks, runs that follow runs -- is replayed on the
smallest configuration of every launch shape, and after EVERY call the counters the library exports (look-ahead hits and speculations, split
launches, spectra generated and skipped, host synchronisations, the last kernel family, batch size and tick-group depth, cascades left armed)
must equal what tests/golden/schedule_counters.json holds, recorded by scripts/record_schedule_counters.py from the commit named in its
"recorded_from"; so must the SHA-256 of every cascade's displacement and normal map at the end.  The other tests hold the maps to the same
bits whichever way a call is scheduled; this one notices a change that quietly stops merging, speculating or splitting.

The counters are a floor, not the proof: they do not see block sizes, scratch groups, the choice of stream or any argument value.  What those
affect is covered by the map digests here, the bit-identity tests (test_lookahead.py, test_run_after_run.py, test_tick_groups.py,
test_two_chains.py) and scripts/fuzz_schedule.py."""
import json
import os

import pytest

import schedule_script as S

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(__file__), "golden", "schedule_counters.json")) as _f:
    RECORD = json.load(_f)


def test_the_fixture_covers_the_scripted_configurations():
    assert RECORD["counters"] == list(S.COUNTERS)
    assert sorted(RECORD["configurations"]) == sorted(S.key(n, count) for n, count in S.CONFIGS)


@pytest.mark.parametrize("n,count", S.CONFIGS)
def test_every_call_leaves_the_recorded_counters_and_the_run_the_recorded_maps(n, count):
    want, got = RECORD["configurations"][S.key(n, count)], S.replay(n, count)
    assert len(got["calls"]) == len(want["calls"])
    for k, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        assert g == w, (k, dict(zip(S.COUNTERS, zip(g[1], w[1]))))
    assert got["digests"] == want["digests"]
