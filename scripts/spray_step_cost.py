"""The cost of ow_spray_step at 1024^2 x 3: the reference emitter (ow_spray_options_default: 32 768 particles, emitter lifetime 6 s) stepped at
the scene's update delta behind the ticks that make its maps, timed with events on the context's stream (a caller's stream, so that the
events and the launches share it); the median per step over the emitter's first cycles, and the bytes a step must move.
    python scripts/spray_step_cost.py [out.txt]          what profiles/spray_step_cost.txt holds"""
import os, sys, statistics
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from godotoceanwaves_amd.presets import UPDATE_DELTA
from scenes import make_gen, scales_of
out = open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, "w")
def say(*a):
    line = " ".join(str(x) for x in a); print(line, flush=True); out.write(line + "\n"); out.flush()
stream = torch.cuda.Stream()
gen, params = make_gen(1024, [0, 1, 2], stream=stream.cuda_stream)
sc = scales_of(params)
spray = gen.spray_create()
amount = spray.amount
STEPS = 600     # 12 s: two emitter cycles
for _ in range(4): gen.update_all(UPDATE_DELTA, params)
ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(STEPS)]
live = []
with torch.cuda.stream(stream):
    for k in range(STEPS):
        gen.update_all(UPDATE_DELTA, params)
        ev[k][0].record(stream)
        gen.spray_step(spray, UPDATE_DELTA, sc)
        ev[k][1].record(stream)
        if k % 50 == 49: live.append(gen.spray_live_count(spray))
stream.synchronize()
us = [a.elapsed_time(b) * 1e3 for a, b in ev]
st = gen.spray_stats(spray)
inst, part, draw = gen.spray_read(spray)
blocks = (amount + 255) // 256
frac = len(draw) / amount
say(f"ow_spray_step, {amount} particles, 1024^2 x 3, delta {UPDATE_DELTA:.4f} s, {STEPS} steps behind their ticks (events on the context's stream)")
say(f"per step: median {statistics.median(us):.2f} us, min {min(us):.2f}, max {max(us):.2f}; second cycle alone (steps 300..599): median {statistics.median(us[300:]):.2f} us")
say(f"live count every 50 steps: {live}; stats {st}")
say(f"bytes a step must move at the last step's live fraction {frac:.4f}:")
say(f"  state and instance, 112 B per particle each way: {amount * 112} B read + {amount * 112} B written at most (the kernel reads the 48 B state alone and writes only particles that restart or are ACTIVE)")
say(f"  taps of the live fraction: {len(draw)} particles x 3 cascades x 2 rows x 16 B = {len(draw) * 3 * 2 * 16} B of displacement (a particle at :78 reads the normal map's bilinear and bicubic taps once)")
say(f"  block counts: {blocks} x 32 B written, then read by every block after them: {blocks * (blocks - 1) // 2 * 4} B of reads that hit the L2")
say(f"  draw list: {amount * 4} B of flags read, {len(draw) * 4} B written")
gen.spray_destroy(spray)
