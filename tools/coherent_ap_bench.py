#!/usr/bin/env python3
"""Measurements of the a-priori retries on the coherent LLRs (coherent_ap): nothing
here asserts.

  step    bench config 3 (256 crowded slots, K = 300, min_score 2, 20 iterations) with coherent=32 and
          ap=["CQ ? ?"], coherent_ap off and on, and the same pair at H = 2 hypotheses and S = 3 sets, all
          alternating on the same batch: ms per step, and how many more candidates k_bp ran on with the
          stage on (its attempts, less the STFT retries its rescues save)
  sweep   one CQ message per slot, 64 slots per 1 dB step across the threshold (ap_bench.py's slots and
          selection): the fraction of slots whose transmitted message is decoded -- plain, STFT-AP, coherent,
          coherent + STFT-AP, coherent-AP, and the last two at coherent_nsym = 3 -- with the interpolated
          50 % points and every payload other than the transmitted one
  noise   256 noise-only slots at K = 300, coherent=32, ap=["CQ ? ?"], coherent_ap on: rows with a
          hypothesis index and bit 1 (false by construction) at max_hard_errors 36 and 174

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

from ap_bench import AP, CFG3, FS, N, bp_candidates, cq_slots, timed_steps  # noqa: E402

AP2 = ["K1ABC ? ?", "CQ ? ?"]


def both_marks(r):
    return (int(r["pass_index"]) >> 4) > 0 and (int(r["pass_index"]) & 2) != 0


def leg_step(torch, dev, args):
    from ft8_demodulator_amd import SlotDecoder, _lib, synth
    x, _ = synth.make_slots(args.slots, 50, fs=FS, snr_db=(-24.0, -10.0),
                            seeds=[100000 + b for b in range(args.slots)], device=dev)
    confs = [("h1_s1_off", dict(ap=AP)), ("h1_s1_on", dict(ap=AP, coherent_ap=True)),
             ("h2_s3_off", dict(ap=AP2, coherent_nsym=3)), ("h2_s3_on", dict(ap=AP2, coherent_nsym=3, coherent_ap=True))]
    decs = [SlotDecoder(FS, 2, 2, device=dev, context=_lib.Context(dev.index), coherent=32, **kw, **CFG3)
            for _, kw in confs]
    times = timed_steps(torch, decs, x, args.steps, args.warmup)
    out = {"slots": args.slots, "steps": args.steps, "warmup": args.warmup}
    for (name, _), dec, t in zip(confs, decs, times):
        recs = dec.records(x)
        out[name] = dict(t, bp_candidates=bp_candidates(dec, x), decodes=sum(len(s) for s in recs),
                         both_marks=sum(int(sum(both_marks(r) for r in s)) for s in recs))
    for pair in ("h1_s1", "h2_s3"):
        out[pair + "_stage_bp_candidates_net"] = out[pair + "_on"]["bp_candidates"] - out[pair + "_off"]["bp_candidates"]
        out[pair + "_stage_ms"] = out[pair + "_on"]["median_ms"] - out[pair + "_off"]["median_ms"]
    return out


def half_point(snrs, fractions):
    """The SNR at which the fraction first reaches 0.5, by linear interpolation between the steps; None if never."""
    for i in range(1, len(snrs)):
        a, b = fractions[i - 1], fractions[i]
        if a < 0.5 <= b:
            return float(snrs[i - 1] + (0.5 - a) / (b - a) * (snrs[i] - snrs[i - 1]))
    return float(snrs[0]) if fractions and fractions[0] >= 0.5 else None


def leg_sweep(torch, dev, args):
    from ft8_demodulator_amd import SlotDecoder, _lib
    kw = dict(max_candidates=40, min_score=2, max_iterations=20, flags=_lib.FT8_FLAG_TOPK)
    confs = [("plain", {}), ("stft_ap", dict(ap=AP)), ("coherent", dict(coherent=True)),
             ("coherent_stft_ap", dict(coherent=True, ap=AP)),
             ("coherent_ap", dict(coherent=True, ap=AP, coherent_ap=True)),
             ("coherent3_stft_ap", dict(coherent=True, ap=AP, coherent_nsym=3)),
             ("coherent3_ap", dict(coherent=True, ap=AP, coherent_nsym=3, coherent_ap=True))]
    decs = [(name, SlotDecoder(FS, 2, 2, device=dev, **c, **kw)) for name, c in confs]
    rows, snrs = [], np.arange(args.snr_lo, args.snr_hi + 0.5, 1.0)
    for i, snr in enumerate(snrs):
        x, pay = cq_slots(args.sweep_slots, float(snr), args.seed + i, dev)
        row = {"snr_db_full_band": float(snr), "snr_db_2500": float(snr + 10.0 * np.log10(FS / 2.0 / 2500.0))}
        for name, dec in decs:
            recs = dec.records(x)
            hit = sum(any(bytes(r["payload"]) == bytes(pay[s]) for r in recs[s]) for s in range(len(recs)))
            false = sum(sum(bytes(r["payload"]) != bytes(pay[s]) for r in recs[s]) for s in range(len(recs)))
            row[name] = {"decoded": hit, "fraction": hit / len(recs), "false": false}
        rows.append(row)
    half = {name: half_point(snrs, [r[name]["fraction"] for r in rows]) for name, _ in confs}
    return {"slots_per_step": args.sweep_slots, "seed": args.seed, "selection": "top-K, K = 40, min_score 2",
            "rows": rows, "half_point_db_full_band": half}


def leg_noise(torch, dev, args):
    from ft8_demodulator_amd import SlotDecoder, ap
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    x = torch.randn(args.slots, N, generator=g, device=dev, dtype=torch.float32)
    out = {"slots": args.slots, "seed": args.seed}
    for limit in (ap.DEFAULT_MAX_HARD_ERRORS, 174):
        recs = SlotDecoder(FS, 2, 2, device=dev, ap=AP, ap_max_hard_errors=limit, coherent=32, coherent_ap=True,
                           **CFG3).records(x)
        out[f"max_hard_errors_{limit}"] = {
            "both_marks": sum(int(sum(both_marks(r) for r in s)) for s in recs),
            "decodes": sum(len(s) for s in recs)}
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--legs", default="step,sweep,noise", help="comma-separated subset of step,sweep,noise")
    p.add_argument("--slots", type=int, default=256)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--sweep-slots", type=int, default=64)
    p.add_argument("--snr-lo", type=float, default=-29.0, help="full-band SNR of the first sweep step, dB")
    p.add_argument("--snr-hi", type=float, default=-19.0)
    p.add_argument("--seed", type=int, default=20261)
    p.add_argument("--out", default=os.path.join(os.environ.get("FT8_OUT", "out"), "coherent_ap_bench.json"))
    args = p.parse_args()
    import torch
    from ft8_demodulator_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    res = {"box": socket.gethostname(), "gpu": torch.cuda.get_device_name(0),
           "build_id": _lib.lib().ft8_build_id().decode(), "ap": AP, "ap2": AP2}
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
