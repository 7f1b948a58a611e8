"""The short fixed schedules behind tests/golden/pass2_load_order.json: what tests/test_pass2_load_order.py replays and what
tests/golden/make_pass2_load_order.py recorded from the commit before pass 2's load order changed."""
import hashlib
import os

from godotoceanwaves_amd import WaveCascadeParameters, WaveGenerator
from godotoceanwaves_amd.presets import UPDATE_DELTA, cascade_preset

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pass2_load_order.json")
# (map size, cascades, call, how many)
CASES = [(1024, 2, "run", 5), (1024, 4, "run", 9), (512, 8, "run", 3), (256, 4, "run", 5), (2048, 1, "run", 3), (1024, 1, "update_all", 2)]


def case_id(case):
    n, count, call, k = case
    return f"{n}x{count}_{call}{k}"


def replay(case):
    """-> (SHA-1 over displacement and normal map of every cascade, kernel family of the last call)"""
    n, count, call, k = case
    gen = WaveGenerator()
    gen.map_size = n
    gen.init_gpu(max(2, count))
    params = [WaveCascadeParameters(**cascade_preset(i)) for i in range(count)]
    if call == "run":
        gen.run(UPDATE_DELTA, params, k)
    else:
        for _ in range(k):
            gen.update_all(UPDATE_DELTA, params)
    gen.sync()
    h = hashlib.sha1()
    for i in range(count):
        disp, norm = gen.get_maps(i)
        h.update(disp.tobytes())
        h.update(norm.tobytes())
    family = gen.last_kernel_family()
    gen.free()
    return h.hexdigest(), family
