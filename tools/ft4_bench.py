#!/usr/bin/env python3
"""Measurements of the FT4 receive path on the GPU: nothing here asserts.

  step    256 FT4 slots of 90 000 samples with 25 signals each (-16 .. -4 dB), top-K selection at K = 300,
          min_score 2, 20 iterations: slots/s, ms per stage (ft8_set_timing), decodes; and on the same box
          in the same run a 256-slot FT8 batch (180 000 samples, 50 signals, the same K) through the unchanged
          FT8 kernels, for the two comparisons
            k_score4<2,2> ns per grid point  vs  k_score2<2,2>'s   (target: not above it)
            k_llr4 ns per candidate          vs  k_llr's           (target: at most 87 / 58 = 1.5 x)
  sweep   8 separated signals per slot, 32 slots per 2 dB step from -8 to -18 dB (full-band SNR): the fraction
          of transmitted messages decoded (top-K, K = 100, min_score 1)
  noise   256 noise-only slots at K = 300: decodes (false by construction), plain and with osd=(2, 32)

Prints one JSON line and writes it to --out.  Needs a GPU; there is no CPU fallback.
"""
import argparse
import json
import os
import socket
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FS = 12000
N4, N8 = 90000, 180000


def ft4_slots(torch, dev, n_slots, n_sig, snr_db, seed, noise=True):
    """make_slots_ft4's construction with the device's transmit chain: -> (samples float32 [n_slots, N4],
    payload sets per slot)."""
    from ft8_demodulator_amd import _lib, ft8_generator as G, synth
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    acc = (torch.randn(n_slots, N4, generator=g, device=dev, dtype=torch.float32) if noise
           else torch.zeros(n_slots, N4, device=dev, dtype=torch.float32))
    rng = np.random.default_rng(seed)
    pays, rows, sets = [], [], []
    lo, hi = (snr_db, snr_db) if np.isscalar(snr_db) else snr_db
    for b in range(n_slots):
        p = synth.random_payloads(n_sig, rng)
        lane = 2400.0 / max(n_sig, 1)
        f0 = 300.0 + (rng.permutation(n_sig) + 0.3 * rng.uniform(0, 1, n_sig)) * lane
        st = rng.uniform(0.3, 1.2, n_sig)
        snr = rng.uniform(lo, hi, n_sig)
        pays.append(p)
        sets.append({r.tobytes() for r in p})
        rows += [(float(f0[i]), float(np.sqrt(2.0 * 10.0 ** (snr[i] / 10.0))), 0.0, int(st[i] * FS), b, 0)
                 for i in range(n_sig)]
    if rows:
        _, _, tones = G.ft4_encode_batch(np.concatenate(pays), device=dev)
        G.synthesize(tones, np.array(rows, dtype=_lib.TX_SIGNAL_DTYPE), n_slots, N4, FS, out=acc, device=dev,
                     protocol="ft4")
    return acc, sets


def timed(torch, dec, x, steps, warmup):
    """-> (ms per step by wall clock over back-to-back steps, ms per launch of every stage by events)."""
    for _ in range(warmup):
        dec.run(x)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        dec.run(x)
    b.record()
    torch.cuda.synchronize()
    step_ms = a.elapsed_time(b) / steps
    dec.ctx.set_timing(True)
    dec.ctx.timing(reset=True)
    for _ in range(steps):
        dec.run(x)
    t = dec.ctx.timing(reset=True)
    dec.ctx.set_timing(False)
    return step_ms, {k: ms / n for k, (ms, n) in t.items() if n}


def leg_step(torch, dev, args):
    from ft8_demodulator_amd import SlotDecoder, _lib, synth
    from ft8_demodulator_amd.ft4 import ft4_grid_shape
    from ft8_demodulator_amd._device import grid_shape
    kw = dict(max_candidates=300, min_score=2, max_iterations=20, flags=_lib.FT8_FLAG_TOPK, device=dev)
    out = {"slots": args.slots, "steps": args.steps, "warmup": args.warmup, "K": 300}
    x4, sets = ft4_slots(torch, dev, args.slots, 25, (-16.0, -4.0), args.seed)
    d4 = SlotDecoder(FS, 2, 2, context=_lib.Context(dev.index), protocol="ft4", **kw)
    ms4, st4 = timed(torch, d4, x4, args.steps, args.warmup)
    recs = d4.records(x4)
    hit = sum(len({bytes(r["payload"]) for r in s} & w) for s, w in zip(recs, sets))
    p4 = d4.plan(N4)
    _, NT4, NF4 = ft4_grid_shape(p4.T, p4.F, 2, 2)
    out["ft4"] = {"ms_per_step": ms4, "slots_per_s": 1e3 * args.slots / ms4, "stage_ms": st4,
                  "decodes": sum(len(s) for s in recs), "transmitted": 25 * args.slots, "transmitted_decoded": hit,
                  "grid": [NT4, NF4]}
    x8, _ = synth.make_slots(args.slots, 50, fs=FS, snr_db=(-24.0, -10.0),
                             seeds=[100000 + b for b in range(args.slots)], device=dev)
    d8 = SlotDecoder(FS, 2, 2, context=_lib.Context(dev.index), **kw)
    ms8, st8 = timed(torch, d8, x8, args.steps, args.warmup)
    p8 = d8.plan(N8)
    _, NT8, NF8 = grid_shape(p8.T, p8.F, 2, 2)
    out["ft8"] = {"ms_per_step": ms8, "slots_per_s": 1e3 * args.slots / ms8, "stage_ms": st8, "grid": [NT8, NF8]}
    pts4, pts8 = args.slots * NT4 * NF4, args.slots * NT8 * NF8
    s4, s8 = 1e6 * st4["score"] / pts4, 1e6 * st8["score"] / pts8
    l4, l8 = 1e6 * st4["llr"] / (args.slots * 300), 1e6 * st8["llr"] / (args.slots * 300)
    out["score_ns_per_grid_point"] = {"k_score4": s4, "k_score2": s8, "ratio": s4 / s8, "target": "<= 1"}
    out["llr_ns_per_candidate"] = {"k_llr4": l4, "k_llr": l8, "ratio": l4 / l8, "target": "<= 1.5"}
    return out


def leg_sweep(torch, dev, args):
    from ft8_demodulator_amd import SlotDecoder, _lib
    dec = SlotDecoder(FS, 2, 2, max_candidates=100, min_score=1, max_iterations=20, flags=_lib.FT8_FLAG_TOPK,
                      device=dev, protocol="ft4")
    rows = []
    for i, snr in enumerate(np.arange(-8.0, -18.5, -2.0)):
        x, sets = ft4_slots(torch, dev, args.sweep_slots, 8, float(snr), args.seed + 10 + i)
        recs = dec.records(x)
        got = [{bytes(r["payload"]) for r in s} for s in recs]
        hit = sum(len(g & w) for g, w in zip(got, sets))
        rows.append({"snr_db_full_band": float(snr), "snr_db_2500": float(snr + 10.0 * np.log10(FS / 2.0 / 2500.0)),
                     "decoded": hit, "fraction": hit / (8.0 * args.sweep_slots),
                     "false": sum(len(g - w) for g, w in zip(got, sets))})
    return {"slots_per_step": args.sweep_slots, "signals_per_slot": 8, "selection": "top-K, K = 100, min_score 1",
            "rows": rows}


def leg_noise(torch, dev, args):
    from ft8_demodulator_amd import SlotDecoder, _lib
    x, _ = ft4_slots(torch, dev, args.slots, 0, 0.0, args.seed + 99)
    out = {"slots": args.slots}
    for name, osd in (("plain", None), ("osd_2_32", (2, 32))):
        recs = SlotDecoder(FS, 2, 2, max_candidates=300, min_score=2, max_iterations=20, flags=_lib.FT8_FLAG_TOPK,
                           device=dev, osd=osd, protocol="ft4").records(x)
        out[name] = sum(len(s) for s in recs)
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--legs", default="step,sweep,noise", help="comma-separated subset of step,sweep,noise")
    p.add_argument("--slots", type=int, default=256)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--sweep-slots", type=int, default=32)
    p.add_argument("--seed", type=int, default=20264)
    p.add_argument("--out", default=os.path.join(os.environ.get("FT8_OUT", "out"), "ft4_bench.json"))
    args = p.parse_args()
    import torch
    from ft8_demodulator_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    res = {"box": socket.gethostname(), "gpu": torch.cuda.get_device_name(0),
           "build_id": _lib.lib().ft8_build_id().decode()}
    legs = {"step": leg_step, "sweep": leg_sweep, "noise": leg_noise}
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
