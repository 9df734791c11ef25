#!/usr/bin/env python3
"""Measurements of the float32 belief propagation (k_bp32, FT8_FLAG_BP_F32) against the float64 kernel k_bp on
the GPU: nothing here asserts.  Both kernels run in the same process on the same
inputs, alternating, three runs each; every figure is a mean with its spread (max - min over the runs).

  stress  BASELINE config 4 (100 k vectors of bp_stress_llrs at sigma 0.85, normalised, 50 iterations):
          ft8_bp against ft8_bp_f32, events around the call -> candidates/s, the kernels' own wave cycles
          (ft8_get_bp_clock, a timed launch of its own) and the two kernels' work counters, which should be equal
  step    ms per 256-slot step (K = 300, 20 iterations, top-K selection) without and with the flag, plain and
          with ap=["CQ ? ?", "K1ABC ? ?"], FT8 (bench config 3's slots) and FT4; with the decode counts of both
  sweep   one CQ message per slot across the threshold (tools/osd_bench.py's construction): decode fraction per
          SNR of both precisions, FT8; tools/ft4_bench.py's construction for FT4
  noise   256 noise-only slots at K = 300: decodes (false by construction) of both precisions

Prints one JSON line and writes it to --out.  Needs a GPU; there is no CPU fallback.
"""
import argparse
import json
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from ap_bench import CFG3, FS, N, cq_slots  # noqa: E402
from ft4_bench import ft4_slots  # noqa: E402

AP2 = ["CQ ? ?", "K1ABC ? ?"]
RUNS = 3


def stat(v):
    v = [float(x) for x in v]
    return {"mean": float(np.mean(v)), "spread": float(np.max(v) - np.min(v)), "runs": v}


def leg_stress(torch, dev, args):
    from ft8_demodulator_amd import _device, _lib, synth
    llr, _ = synth.bp_stress_llrs(args.vectors, sigma=0.85, seed=7)
    x = torch.from_numpy(_device.normalize(llr)).to(dev)
    n = x.shape[0]
    ctx = _lib.Context(dev.index)
    ctx.set_timing(True, stages=[])   # allocates the work counters; they count with timing off too
    ctx.set_timing(False)
    res = torch.zeros(n * _lib.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    L, st = _lib.lib(), _lib.stream_handle(dev)
    calls = {"k_bp": L.ft8_bp, "k_bp32": L.ft8_bp_f32}

    def once(name):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ctx.check(calls[name](ctx.handle, _lib.ptr(x), n, args.stress_iters, None, _lib.ptr(res), st), name)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    for name in calls:          # warm-up: code objects, counters
        once(name)
    ms = {k: [] for k in calls}
    for _ in range(RUNS):
        for name in calls:
            ms[name].append(once(name))
    out = {"vectors": n, "iterations": args.stress_iters}
    for name in calls:
        ctx.counters(reset=True)
        once(name)
        cnt = ctx.counters(reset=True)
        ok = int(res.cpu().numpy().view(_lib.RESULT_DTYPE)["ok"].sum())
        ctx.set_timing(True, stages=["bp"])
        ctx.bp_clock(reset=True)
        once(name)
        clk = ctx.bp_clock(reset=True)
        ctx.set_timing(False)
        out[name] = {"ms": stat(ms[name]), "candidates_per_s": stat([1e3 * n / m for m in ms[name]]),
                     "counters": cnt, "ok": ok, "clock": clk}
    out["ratio_k_bp_over_k_bp32"] = out["k_bp"]["ms"]["mean"] / out["k_bp32"]["ms"]["mean"]
    out["wave_cycle_ratio"] = out["k_bp"]["clock"]["wave_cycles"] / max(out["k_bp32"]["clock"]["wave_cycles"], 1)
    return out


def timed_runs(torch, decs, x, steps, warmup):
    """decs alternate on the same batch, RUNS runs of `steps` back-to-back steps each (host clock around a
    synchronise) -> ms per step of each decoder, per run."""
    for _ in range(warmup):
        for d in decs:
            d.run(x)
    torch.cuda.synchronize()
    ms = [[] for _ in decs]
    for _ in range(RUNS):
        for k, d in enumerate(decs):
            t0 = time.perf_counter()
            for _ in range(steps):
                d.run(x)
            torch.cuda.synchronize()
            ms[k].append(1e3 * (time.perf_counter() - t0) / steps)
    return [stat(m) for m in ms]


def leg_step(torch, dev, args):
    from ft8_demodulator_amd import SlotDecoder, _lib, synth
    kw = dict(CFG3, flags=_lib.FT8_FLAG_TOPK, device=dev)
    x8, _ = synth.make_slots(args.slots, 50, fs=FS, snr_db=(-24.0, -10.0),
                             seeds=[100000 + b for b in range(args.slots)], device=dev)
    x4, _ = ft4_slots(torch, dev, args.slots, 25, (-16.0, -4.0), args.seed)
    out = {"slots": args.slots, "steps": args.steps, "warmup": args.warmup, "runs": RUNS, "K": CFG3["max_candidates"]}
    for proto, x in (("ft8", x8), ("ft4", x4)):
        for name, ap in (("plain", None), ("ap2", AP2)):
            decs = [SlotDecoder(FS, 2, 2, context=_lib.Context(dev.index), protocol=proto, ap=ap, bp32=f, **kw)
                    for f in (False, True)]
            t64, t32 = timed_runs(torch, decs, x, args.steps, args.warmup)
            recs = [d.records(x) for d in decs]
            sets = [[{bytes(r["payload"]) for r in s} for s in rr] for rr in recs]
            stage = {}
            for key, d in zip(("f64", "f32"), decs):
                d.ctx.set_timing(True)
                d.ctx.timing(reset=True)
                for _ in range(args.steps):
                    d.run(x)
                stage[key] = {k: ms / args.steps for k, (ms, cnt) in d.ctx.timing(reset=True).items() if cnt}
                d.ctx.set_timing(False)
            out[f"{proto}_{name}"] = {
                "f64_ms": t64, "f32_ms": t32, "ratio": t64["mean"] / t32["mean"],
                "stage_ms_per_step": stage,
                "decodes": {"f64": sum(len(s) for s in recs[0]), "f32": sum(len(s) for s in recs[1])},
                "distinct": {"f64": sum(len(s) for s in sets[0]), "f32": sum(len(s) for s in sets[1]),
                             "only_f64": sum(len(a - b) for a, b in zip(*sets)),
                             "only_f32": sum(len(b - a) for a, b in zip(*sets))}}
    return out


def leg_sweep(torch, dev, args):
    from ft8_demodulator_amd import SlotDecoder, _lib
    kw = dict(max_candidates=40, min_score=2, max_iterations=20, flags=_lib.FT8_FLAG_TOPK, device=dev)
    d8 = [(k, SlotDecoder(FS, 2, 2, bp32=f, **kw)) for k, f in (("f64", False), ("f32", True))]
    rows8 = []
    for i, snr in enumerate(np.arange(args.snr_lo, args.snr_hi + 0.5, 1.0)):
        x, pay = cq_slots(args.sweep_slots, float(snr), args.seed + i, dev)
        row = {"snr_db_full_band": float(snr)}
        for name, dec in d8:
            recs = dec.records(x)
            hit = sum(any(bytes(r["payload"]) == bytes(pay[s]) for r in recs[s]) for s in range(len(recs)))
            false = sum(sum(bytes(r["payload"]) != bytes(pay[s]) for r in recs[s]) for s in range(len(recs)))
            row[name] = {"decoded": hit, "fraction": hit / len(recs), "false": false}
        rows8.append(row)
    kw4 = dict(max_candidates=100, min_score=1, max_iterations=20, flags=_lib.FT8_FLAG_TOPK, device=dev, protocol="ft4")
    d4 = [(k, SlotDecoder(FS, 2, 2, bp32=f, **kw4)) for k, f in (("f64", False), ("f32", True))]
    rows4 = []
    for i, snr in enumerate(np.arange(-8.0, -18.5, -2.0)):
        x, sets = ft4_slots(torch, dev, args.sweep_slots, 8, float(snr), args.seed + 10 + i)
        row = {"snr_db_full_band": float(snr)}
        for name, dec in d4:
            got = [{bytes(r["payload"]) for r in s} for s in dec.records(x)]
            hit = sum(len(g & w) for g, w in zip(got, sets))
            row[name] = {"decoded": hit, "fraction": hit / (8.0 * args.sweep_slots),
                         "false": sum(len(g - w) for g, w in zip(got, sets))}
        rows4.append(row)
    return {"slots_per_step": args.sweep_slots, "seed": args.seed, "ft8": rows8, "ft4": rows4}


def leg_noise(torch, dev, args):
    from ft8_demodulator_amd import SlotDecoder, _lib
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    x = torch.randn(args.slots, N, generator=g, device=dev, dtype=torch.float32)
    out = {"slots": args.slots, "seed": args.seed}
    for name, f in (("f64", False), ("f32", True)):
        recs = SlotDecoder(FS, 2, 2, device=dev, flags=_lib.FT8_FLAG_TOPK, bp32=f, **CFG3).records(x)
        out[name] = {"decodes": sum(len(s) for s in recs)}
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--legs", default="stress,step,sweep,noise", help="comma-separated subset of stress,step,sweep,noise")
    p.add_argument("--vectors", type=int, default=100000)
    p.add_argument("--stress-iters", type=int, default=50)
    p.add_argument("--slots", type=int, default=256)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--sweep-slots", type=int, default=64)
    p.add_argument("--snr-lo", type=float, default=-27.0, help="full-band SNR of the first FT8 sweep step, dB")
    p.add_argument("--snr-hi", type=float, default=-18.0)
    p.add_argument("--seed", type=int, default=20261)
    p.add_argument("--out", default=os.path.join(os.environ.get("FT8_OUT", "out"), "bp32_bench.json"))
    args = p.parse_args()
    import torch
    from ft8_demodulator_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    res = {"box": socket.gethostname(), "gpu": torch.cuda.get_device_name(0),
           "build_id": _lib.lib().ft8_build_id().decode()}
    legs = {"stress": leg_stress, "step": leg_step, "sweep": leg_sweep, "noise": leg_noise}
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
