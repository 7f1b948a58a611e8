"""Pass 2 of the compact family asks for its inputs early (ow_frame_kernels.h pass2c_item, OW_P2_EARLY): the side-row record through the scalar
cache where a wave holds one x', as three vector loads beside C1's elsewhere (on by default); pcol's eight pieces together, C0 and C2 above the
epilogue before them (behind the switch, off).  Only where and how the loads are issued
changed, so both maps of every cascade must be BITWISE what the commit before the change wrote.  tests/golden/pass2_load_order.json holds the SHA-1
over both RGBA16F maps of every cascade that a build of that commit printed for the short schedules of tests/pass2_schedules.py
(tests/golden/make_pass2_load_order.py),
one per shape at which the new order takes another path:
    1024^2 x 2, 5 ticks of ow_run    one x' per wave: the scalar path; pair kernel on one stream
    1024^2 x 4, 9 ticks              the split launches (two chains)
    512^2 x 8, 3 ticks               two x' per wave: the vector side-row path; pair kernel
    256^2 x 4, 5 ticks               tick groups walking several ticks with the foam in registers
    2048^2 x 1, 3 ticks              one x' spanning two waves (the second holds no row-0 lane)
    1024^2 x 1, 2 x ow_update_all    the layer-parallel pass 2, which does not change
A whole-map hash covers x' = 0, odd x' (the sign of pcol) and the row-0 slot of lane 0."""
import json

import pytest

from pass2_schedules import CASES, GOLDEN, case_id, replay


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_maps_are_bitwise_those_of_the_order_before(case):
    with open(GOLDEN) as f:
        want = json.load(f)[case_id(case)]
    sha, family = replay(case)
    assert family == want["family"]  # the schedule still reaches the kernel this case is about
    assert sha == want["sha1"]
