#!/usr/bin/env python3
"""Measurements of a-priori (AP) decoding on the GPU: nothing here asserts.

  step    bench config 3 (256 crowded slots, K = 300, min_score 2, 20 iterations) decoded plain and with
          ap=["CQ ? ?"], the two alternating on the same batch: ms per step, how many candidates the
          AP pass ran BP on, how many it rescued
  sweep   one CQ message per slot, 64 slots per 1 dB step across the threshold: the fraction of slots
          whose transmitted message is decoded, plain and with AP (top-K selection, K = 40, min_score 2)
  noise   256 noise-only slots at K = 300: AP decodes (false by construction) at the default
          ap_max_hard_errors and without a limit

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
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FS, N = 12000, 180000
CFG3 = dict(max_candidates=300, min_score=2, max_iterations=20)
AP = ["CQ ? ?"]


def cq_payloads(n, rng):
    """n standard messages with CQ in the first call field: n28a = 2, i3 = 1, every other field random."""
    from ft8_demodulator_amd import ap
    _, value = ap.ap_hypothesis("CQ ? ?")
    bits = rng.integers(0, 2, size=(n, 80), dtype=np.uint8)
    bits[:, 77:] = 0
    bits[:, :29] = ap.hyp_bits(value)[:29]
    bits[:, 74:77] = (0, 0, 1)
    return np.packbits(bits, axis=1)


def cq_slots(n_slots, snr_db, seed, dev):
    """One CQ signal per slot at snr_db (full-band SNR, synth's convention) in unit-variance noise."""
    import torch
    from ft8_demodulator_amd import _lib, ft8_generator as G
    rng = np.random.default_rng(seed)
    pay = cq_payloads(n_slots, rng)
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    acc = torch.randn(n_slots, N, generator=g, device=dev, dtype=torch.float64)
    sig = np.zeros(n_slots, dtype=_lib.TX_SIGNAL_DTYPE)
    sig["f0"] = rng.uniform(200.0, 2800.0, n_slots)
    sig["amplitude"] = np.sqrt(2.0 * 10.0 ** (snr_db / 10.0))
    sig["start"] = (rng.uniform(0.0, 2.0, n_slots) * FS).astype(np.int64)
    sig["slot"] = np.arange(n_slots)
    _, _, tones = G.encode_batch(pay, device=dev)
    G.synthesize(tones, sig, n_slots, N, FS, _lib.FT8_TX_PROTOCOL, out=acc, device=dev)
    return acc.to(torch.float32), pay


def timed_steps(torch, decs, x, steps, warmup):
    """decs alternate on the same batch; -> ms per step of each (host clock around a synchronise)."""
    for _ in range(warmup):
        for d in decs:
            d.run(x)
    torch.cuda.synchronize()
    ms = [[] for _ in decs]
    for _ in range(steps):
        for k, d in enumerate(decs):
            t0 = time.perf_counter()
            d.run(x)
            torch.cuda.synchronize()
            ms[k].append(1e3 * (time.perf_counter() - t0))
    return [{"median_ms": float(np.median(m)), "min_ms": float(np.min(m)), "max_ms": float(np.max(m))} for m in ms]


def bp_candidates(dec, x):
    """Candidates one step runs BP on (k_bp's own counter), all launches of the step together."""
    dec.ctx.set_timing(True, stages=[])
    dec.ctx.counters(reset=True)
    dec.run(x)
    n = dec.ctx.counters(reset=True)["candidates"]
    dec.ctx.set_timing(False)
    return int(n)


def leg_step(torch, dev, args):
    from ft8_demodulator_amd import SlotDecoder, _lib, ap, synth
    x, _ = synth.make_slots(args.slots, 50, fs=FS, snr_db=(-24.0, -10.0),
                            seeds=[100000 + b for b in range(args.slots)], device=dev)
    plain = SlotDecoder(FS, 2, 2, device=dev, context=_lib.Context(dev.index), **CFG3)
    with_ap = SlotDecoder(FS, 2, 2, device=dev, context=_lib.Context(dev.index), ap=AP, **CFG3)
    t_plain, t_ap = timed_steps(torch, [plain, with_ap], x, args.steps, args.warmup)
    n_plain, n_ap = bp_candidates(plain, x), bp_candidates(with_ap, x)
    recs = with_ap.records(x)
    rescued = sum(int(sum(ap.ap_index(r) > 0 for r in s)) for s in recs)
    return {"slots": args.slots, "steps": args.steps, "warmup": args.warmup, "plain": t_plain, "ap": t_ap,
            "bp_candidates_plain": n_plain, "bp_candidates_ap_pass": n_ap - n_plain,
            "decodes_plain": sum(len(s) for s in plain.records(x)), "decodes_ap": sum(len(s) for s in recs),
            "rescued": rescued}


def leg_sweep(torch, dev, args):
    from ft8_demodulator_amd import SlotDecoder, _lib
    kw = dict(max_candidates=40, min_score=2, max_iterations=20, flags=_lib.FT8_FLAG_TOPK)
    plain = SlotDecoder(FS, 2, 2, device=dev, **kw)
    with_ap = SlotDecoder(FS, 2, 2, device=dev, ap=AP, **kw)
    rows = []
    for i, snr in enumerate(np.arange(args.snr_lo, args.snr_hi + 0.5, 1.0)):
        x, pay = cq_slots(args.sweep_slots, float(snr), args.seed + i, dev)
        row = {"snr_db_full_band": float(snr), "snr_db_2500": float(snr + 10.0 * np.log10(FS / 2.0 / 2500.0))}
        for name, dec in (("plain", plain), ("ap", with_ap)):
            recs = dec.records(x)
            hit = sum(any(bytes(r["payload"]) == bytes(pay[s]) for r in recs[s]) for s in range(len(recs)))
            false = sum(sum(bytes(r["payload"]) != bytes(pay[s]) for r in recs[s]) for s in range(len(recs)))
            row[name] = {"decoded": hit, "fraction": hit / len(recs), "false": false}
        rows.append(row)
    return {"slots_per_step": args.sweep_slots, "seed": args.seed, "selection": "top-K, K = 40, min_score 2",
            "rows": rows}


def leg_noise(torch, dev, args):
    from ft8_demodulator_amd import SlotDecoder, ap
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    x = torch.randn(args.slots, N, generator=g, device=dev, dtype=torch.float32)
    out = {"slots": args.slots, "seed": args.seed}
    for limit in (ap.DEFAULT_MAX_HARD_ERRORS, 174):
        recs = SlotDecoder(FS, 2, 2, device=dev, ap=AP, ap_max_hard_errors=limit, **CFG3).records(x)
        out[f"max_hard_errors_{limit}"] = {
            "ap_decodes": sum(int(sum(ap.ap_index(r) > 0 for r in s)) for s in recs),
            "plain_decodes": sum(int(sum(ap.ap_index(r) == 0 for r in s)) for s in recs)}
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
    p.add_argument("--out", default=os.path.join(os.environ.get("FT8_OUT", "out"), "ap_bench.json"))
    args = p.parse_args()
    import torch
    from ft8_demodulator_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    res = {"box": socket.gethostname(), "gpu": torch.cuda.get_device_name(0),
           "build_id": _lib.lib().ft8_build_id().decode(), "ap": AP}
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
