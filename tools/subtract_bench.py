#!/usr/bin/env python3
"""Measurements of the n-pass subtraction on the GPU: nothing here asserts.

  crowded  bench config 4's crowded batch (334 slots of 50 signals at -24 .. -10 dB, seed 200000, top-K
           selection, K = 300, min_score 2, 50 iterations) decoded with FT8_FLAG_SUBTRACT at 2, 3 and 4
           passes -- without retries, with coherent = 8 and with coherent = 32 in every pass: distinct true
           decodes per slot after each pass, false decodes, rows with pass_index bit 2, and ms per step
           (one step at a time with a synchronise, the configurations alternating on the same batch)
  noise    256 noise-only slots, the same configurations: rows after each pass (false by construction)

Prints one JSON line and writes it to --out.  Needs a GPU; there is no CPU fallback.
"""
import argparse
import json
import os
import socket
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from ap_bench import FS, N, timed_steps  # noqa: E402

CFG4 = dict(max_candidates=300, min_score=2, max_iterations=50)
SEED4 = 200000                  # bench.py SUB_SEED0
PASSES = (2, 3, 4)
RETRIES = (("plain", None), ("coherent_8", 8), ("coherent_32", 32))


def decoders(dev):
    from ft8_demodulator_amd import SlotDecoder, _lib
    return [(f"{name}_n{n}", n, SlotDecoder(FS, 2, 2, device=dev, context=_lib.Context(dev.index),
                                            flags=_lib.FT8_FLAG_TOPK, subtract=n, coherent=m, **CFG4))
            for name, m in RETRIES for n in PASSES]


def tally(dec, n, x, truths):
    """-> rows and distinct true decodes per slot after each pass, false decodes, rows with bit 2."""
    recs = dec.records(x)
    pc = dec.pass_counts()
    true_after = np.zeros(n)
    false = drift = 0
    for s, r in enumerate(recs):
        tr = {bytes(p) for p in truths[s].payloads} if truths is not None else set()
        pay = [bytes(q["payload"]) for q in r]
        for k in range(n):
            true_after[k] += len(set(pay[:min(int(pc[s, k]), len(r))]) & tr)
        false += len(set(pay) - tr)
        drift += int(np.sum(r["pass_index"] & 4 != 0))
    n_slots = len(recs)
    return {"rows_after_pass": (pc.sum(axis=0) / n_slots).tolist(),
            "true_per_slot_after_pass": (true_after / n_slots).tolist(), "false_decodes": false,
            "rows_bit2": drift, "rescued_rows": int(sum(np.sum(r["pass_index"] & 2 != 0) for r in recs)),
            "rescued_from_residual": int(sum(np.sum(r["pass_index"] & 3 == 3) for r in recs))}


def leg_crowded(torch, dev, args):
    from ft8_demodulator_amd import synth
    x, truths = synth.make_slots(args.slots, 50, fs=FS, snr_db=(-24.0, -10.0), seed=SEED4, device=dev)
    decs = decoders(dev)
    times = timed_steps(torch, [d for _, _, d in decs], x, args.steps, args.warmup)
    out = {"slots": args.slots, "steps": args.steps, "warmup": args.warmup, "seed": SEED4}
    for (name, n, dec), t in zip(decs, times):
        out[name] = dict(t, **tally(dec, n, x, truths))
    return out


def leg_noise(torch, dev, args):
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    x = torch.randn(args.noise_slots, N, generator=g, device=dev, dtype=torch.float32)
    out = {"slots": args.noise_slots, "seed": args.seed}
    decs = decoders(dev)
    times = timed_steps(torch, [d for _, _, d in decs], x, args.steps, args.warmup)
    for (name, n, dec), t in zip(decs, times):
        out[name] = dict(t, **tally(dec, n, x, None))
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--legs", default="crowded,noise", help="comma-separated subset of crowded,noise")
    p.add_argument("--slots", type=int, default=334)
    p.add_argument("--noise-slots", type=int, default=256)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--seed", type=int, default=20261)
    p.add_argument("--out", default=os.path.join(os.environ.get("FT8_OUT", "out"), "subtract_bench.json"))
    args = p.parse_args()
    import torch
    from ft8_demodulator_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    res = {"box": socket.gethostname(), "gpu": torch.cuda.get_device_name(0),
           "build_id": _lib.lib().ft8_build_id().decode()}
    legs = {"crowded": leg_crowded, "noise": leg_noise}
    for name in args.legs.split(","):
        res[name] = legs[name](torch, dev, args)
    line = json.dumps(res)
    out = args.out if os.path.isabs(args.out) else os.path.join(ROOT, args.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
