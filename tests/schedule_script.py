"""One fixed, scripted call sequence per configuration, with the frame scheduler's exported counters read after every call and a SHA-256 of
every map at the end: what scripts/record_schedule_counters.py records into tests/golden/schedule_counters.json and what
tests/test_schedule_counters.py replays.  Only the public wrapper is used, so the recorder runs on any commit that has it."""
import hashlib

from godotoceanwaves_amd import WaveCascadeParameters, WaveGenerator
from godotoceanwaves_amd.presets import UPDATE_DELTA, cascade_preset

# the smallest configuration at which each launch shape exists: tick groups at depth sixteen and the four-ahead queue; the group kernel and a
# pre-arm of several cascades; the single-batch pair stream and two chains at 512^2; the headline (two chains); two batches, 3 + 2 (the
# cascade-major stream); the split pair kernel
CONFIGS = [(256, 1), (256, 4), (512, 8), (1024, 4), (1024, 5), (2048, 1)]
MULTI_BATCH = (1024, 5)   # the one whose run(70) crosses a 64-tick block of the cascade-major stream
OTHER_DELTA = 0.03
COUNTERS = ("lookahead_hits", "lookahead_speculated", "split_launches", "spectra_generated", "spectra_skipped", "host_syncs",
            "last_kernel_family", "last_batch_cascades", "tick_group_depth", "cascades_remaining")


def key(n, count):
    return f"{n}x{count}"


def counters(gen):
    """the tuple COUNTERS names, as JSON holds it"""
    return [*gen.lookahead_stats(), gen.chain_stats(), *gen.spectrum_stats(), gen.sync_stats(), gen.last_kernel_family(),
            gen.last_batch_cascades(), gen.tick_group_depth(), gen.pass_num_cascades_remaining]


def replay(n, count):
    """{"calls": [[label, counters after it], ..], "digests": [[sha256 of displacement, of normal] per cascade]}"""
    gen = WaveGenerator()
    gen.map_size = n
    gen.init_gpu(max(2, count))
    params = [WaveCascadeParameters(**cascade_preset(i)) for i in range(count)]
    calls = []

    def call(label, f):
        f()
        calls.append([label, counters(gen)])

    def update_and_process(processes):
        call("update", lambda: gen.update(UPDATE_DELTA, params))
        for _ in range(processes):
            call("process", lambda: gen._process(0.0))

    def edit_tile():
        params[-1].tile_length = (41.0, 43.0)

    def edit_whitecap():
        params[1 % count].whitecap = 0.9   # (the setter raises the dirty flag: the resident spectrum serves it)

    try:
        for _ in range(6):
            call("update_all", lambda: gen.update_all(UPDATE_DELTA, params))
        call("update_all, other delta", lambda: gen.update_all(OTHER_DELTA, params))
        for _ in range(3):
            update_and_process(count)
        update_and_process(count - 1)            # one _process too few: a leftover ...
        call("update", lambda: gen.update(UPDATE_DELTA, params))   # ... that this update flushes
        call("tile_length edit", edit_tile)
        call("update_all", lambda: gen.update_all(UPDATE_DELTA, params))
        call("whitecap edit", edit_whitecap)
        call("update_all", lambda: gen.update_all(UPDATE_DELTA, params))
        for i in range(count):
            call(f"get_maps({i})", lambda: gen.get_maps(i))
        for frames, delta in ((3, UPDATE_DELTA), (12, UPDATE_DELTA), (12, UPDATE_DELTA), (5, OTHER_DELTA)):
            call(f"run({frames})", lambda: gen.run(delta, params, frames))
        if (n, count) == MULTI_BATCH:
            call("run(70)", lambda: gen.run(OTHER_DELTA, params, 70))
        call("closing update_all", lambda: gen.update_all(UPDATE_DELTA, params))
        gen.sync()
        digests = [[hashlib.sha256(m.tobytes()).hexdigest() for m in gen.get_maps(i)] for i in range(count)]
    finally:
        gen.free()
    return {"calls": calls, "digests": digests}
