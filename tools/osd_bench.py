#!/usr/bin/env python3
"""Measurements of ordered-statistics decoding (OSD) on the GPU: nothing here asserts.

  step    bench config 3 (256 crowded slots, K = 300, min_score 2, 20 iterations) with the top-K selection,
          decoded without OSD and with osd=(2, 32), (1, 32) and (2, 0), the four alternating on the same
          batch: ms per step and what the pass rescued; and k_osd alone, timed by events around
          ft8_osd_decode on 8192 failed vectors at each order
  sweep   one CQ message per slot, 64 slots per 1 dB step across the threshold: the fraction of slots whose
          transmitted message is decoded -- plain, OSD at orders 0, 1 and 2, and OSD order 2 after
          coherent=32 and ap=["CQ ? ?"] (top-K selection, K = 40, min_score 2)
  noise   256 noise-only slots at K = 300: OSD decodes (false by construction) at max_hard_errors 36 and 174,
          with 32 and with all failed candidates per slot

Prints one JSON line and writes it to --out.  Needs a GPU; there is no CPU fallback.
"""
import argparse
import json
import os
import socket
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from ap_bench import AP, CFG3, FS, N, cq_slots, timed_steps  # noqa: E402

STEP_SETTINGS = (("plain", None), ("osd_2_32", (2, 32)), ("osd_1_32", (1, 32)), ("osd_2_all", (2, 0)))


def n_osd(recs):
    from ft8_demodulator_amd import osd
    return sum(int(sum(osd.osd_index(r) for r in s)) for s in recs)


def kernel_alone(torch, dev, n=8192, reps=5):
    """k_osd by itself: ft8_osd_decode on n noise vectors with failed records, events around the call."""
    from ft8_demodulator_amd import _lib
    ctx = _lib.Context(dev.index)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    llr = 4.9 * torch.randn(n, 174, generator=g, device=dev, dtype=torch.float64)
    out = {"vectors": n}
    for order in (0, 1, 2):
        ctx.set_osd(order, 0, 36)
        ms = []
        for _ in range(reps + 1):
            res = torch.zeros(n * _lib.RESULT_DTYPE.itemsize + 8, dtype=torch.uint8, device=dev)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ctx.check(_lib.lib().ft8_osd_decode(ctx.handle, _lib.ptr(llr), _lib.ptr(res), n, None, None,
                                                _lib.stream_handle(dev)), "ft8_osd_decode")
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        out[f"order_{order}"] = {"median_ms": float(np.median(ms[1:])), "min_ms": float(np.min(ms[1:])),
                                 "us_per_vector": 1e3 * float(np.median(ms[1:])) / n}
    return out


def leg_step(torch, dev, args):
    from ft8_demodulator_amd import SlotDecoder, _lib, synth
    x, _ = synth.make_slots(args.slots, 50, fs=FS, snr_db=(-24.0, -10.0),
                            seeds=[100000 + b for b in range(args.slots)], device=dev)
    decs = [SlotDecoder(FS, 2, 2, device=dev, context=_lib.Context(dev.index), flags=_lib.FT8_FLAG_TOPK, osd=o, **CFG3)
            for _, o in STEP_SETTINGS]
    times = timed_steps(torch, decs, x, args.steps, args.warmup)
    out = {"slots": args.slots, "steps": args.steps, "warmup": args.warmup, "selection": "top-K"}
    for (name, _), d, t in zip(STEP_SETTINGS, decs, times):
        recs = d.records(x)
        out[name] = dict(t, decodes=sum(len(s) for s in recs), osd_decodes=n_osd(recs),
                         distinct=sum(len({bytes(r["payload"]) for r in s}) for s in recs))
    out["k_osd_alone"] = kernel_alone(torch, dev)
    return out


def leg_sweep(torch, dev, args):
    from ft8_demodulator_amd import SlotDecoder, _lib
    kw = dict(max_candidates=40, min_score=2, max_iterations=20, flags=_lib.FT8_FLAG_TOPK)
    decs = [("plain", SlotDecoder(FS, 2, 2, device=dev, **kw))]
    decs += [(f"osd{k}", SlotDecoder(FS, 2, 2, device=dev, osd=(k, 32), **kw)) for k in (0, 1, 2)]
    decs += [("coherent_ap", SlotDecoder(FS, 2, 2, device=dev, coherent=32, ap=AP, **kw)),
             ("coherent_ap_osd2", SlotDecoder(FS, 2, 2, device=dev, coherent=32, ap=AP, osd=(2, 32), **kw))]
    rows = []
    for i, snr in enumerate(np.arange(args.snr_lo, args.snr_hi + 0.5, 1.0)):
        x, pay = cq_slots(args.sweep_slots, float(snr), args.seed + i, dev)
        row = {"snr_db_full_band": float(snr), "snr_db_2500": float(snr + 10.0 * np.log10(FS / 2.0 / 2500.0))}
        for name, dec in decs:
            recs = dec.records(x)
            hit = sum(any(bytes(r["payload"]) == bytes(pay[s]) for r in recs[s]) for s in range(len(recs)))
            false = sum(sum(bytes(r["payload"]) != bytes(pay[s]) for r in recs[s]) for s in range(len(recs)))
            row[name] = {"decoded": hit, "fraction": hit / len(recs), "false": false}
        rows.append(row)
    return {"slots_per_step": args.sweep_slots, "seed": args.seed, "selection": "top-K, K = 40, min_score 2",
            "osd_max_per_slot": 32, "rows": rows}


def leg_noise(torch, dev, args):
    from ft8_demodulator_amd import SlotDecoder, _lib
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    x = torch.randn(args.slots, N, generator=g, device=dev, dtype=torch.float32)
    out = {"slots": args.slots, "seed": args.seed}
    for cap in (32, 0):
        for limit in (36, 174):
            recs = SlotDecoder(FS, 2, 2, device=dev, flags=_lib.FT8_FLAG_TOPK, osd=(2, cap), osd_max_hard_errors=limit,
                               **CFG3).records(x)
            out[f"cap_{cap}_max_hard_errors_{limit}"] = {"osd_decodes": n_osd(recs),
                                                         "other_decodes": sum(len(s) for s in recs) - n_osd(recs)}
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--legs", default="step,sweep,noise", help="comma-separated subset of step,sweep,noise")
    p.add_argument("--slots", type=int, default=256)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--sweep-slots", type=int, default=64)
    p.add_argument("--snr-lo", type=float, default=-27.0, help="full-band SNR of the first sweep step, dB")
    p.add_argument("--snr-hi", type=float, default=-18.0)
    p.add_argument("--seed", type=int, default=20261)
    p.add_argument("--out", default=os.path.join(os.environ.get("FT8_OUT", "out"), "osd_bench.json"))
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
