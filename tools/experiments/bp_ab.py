"""A/B of libft8hip.so builds on k_bp alone: per build and round, the step time, the event-timed `bp`
stage, the decode count, and k_bp's own shader-clock cycles per launch (ft8_get_bp_clock: clock-
independent) with the launch's message passes.  One subprocess per build, rounds interleaved.
Usage: python tools/experiments/bp_ab.py [--rounds N] lib1.so lib2.so ...   (JSON lines on stdout)"""
import argparse
import json
import os
import subprocess
import sys

CHILD = r'''
import os, sys, json, time
sys.path.insert(0, os.environ["REPO"])
import torch
from ft8_demodulator_amd import SlotDecoder, synth
torch.manual_seed(0)
x, _ = synth.make_slots(256, 50, seed=100000, device="cuda")
dec = SlotDecoder(12000, 2, 2, 300, 2, 20)
for _ in range(20): dec.run(x)   # k_bp settles over ~15 launches
torch.cuda.synchronize()
ctx = dec.ctx
t0 = time.perf_counter()
for _ in range(40): out, cnt = dec.run(x)
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / 40
R = 16
ctx.timing(reset=True); ctx.counters(reset=True); ctx.bp_clock(reset=True)
ctx.set_timing(True, stages=["bp"])
for _ in range(R): dec.run(x)
torch.cuda.synchronize()
ctx.set_timing(False)
tm = ctx.timing(reset=True)["bp"]
cn = ctx.counters(reset=True)
ck = ctx.bp_clock(reset=True)
print(json.dumps({"lib": os.path.basename(os.environ["FT8HIP_LIB"]), "ms_step": round(dt * 1e3, 4),
                  "bp_ms": round(tm[0] / max(tm[1], 1), 4), "decodes": int(cnt.sum()),
                  "passes_per_launch": cn["passes"] / R, "candidates_per_launch": cn["candidates"] / R,
                  "mean_wave_cycles": round(ck["wave_cycles"] / max(ck["waves"], 1), 1),
                  "max_wave_cycles": ck["max_wave_cycles"], "waves_per_launch": ck["waves"] / R}))
'''


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("libs", nargs="+")
    a = ap.parse_args()
    repo = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for rnd in range(a.rounds):
        for l in a.libs:
            env = dict(os.environ, FT8HIP_LIB=os.path.abspath(l), REPO=repo, FT8HIP_ALLOW_STALE="1")
            out = subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True, timeout=240)
            line = [x for x in out.stdout.splitlines() if x.startswith("{")]
            if out.returncode != 0 or not line:
                # a build that fails here is not run again: the caller reads the reason first
                print(json.dumps({"lib": os.path.basename(l), "round": rnd, "failed": out.returncode,
                                  "stderr": out.stderr[-1500:]}), flush=True)
                return 1
            d = json.loads(line[-1])
            d["round"] = rnd
            print(json.dumps(d), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
