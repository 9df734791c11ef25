#!/usr/bin/env python3
"""Measurements of the coherent re-demodulation on the GPU: nothing here asserts.

  step    bench config 3 (256 crowded slots, K = 300, min_score 2, 20 iterations) decoded plain and with
          coherent = 8, 32 and 0 (every failed candidate), alternating on the same batch: ms per step,
          how many candidates the pass ran BP on, how many it rescued
  kernel  k_coherent alone through the stage call, on the batch's first M selected candidates per slot
          listed in the order of the in-batch launch (workgroup w: slot w % 8 + 8 (w / 8 / M)), so a
          slot's candidates share an XCD as they do there: ms per launch and the bytes of samples read
          per second (every candidate reads (79 Q + 2 Mg) D samples)
  sweep   one CQ message per slot, 64 slots per 1 dB step across the threshold: the fraction of slots
          whose transmitted message is decoded -- plain, coherent, coherent + AP "CQ ? ?" (top-K
          selection, K = 40, min_score 2)
  noise   256 noise-only slots at K = 300: decodes (false by construction) with coherent = 32 and 0
  drift   (--drift, or --legs drift) the drift search (ft8_set_coherent_drift): the fraction of one-signal slots
          decoded over the drift rate at two SNRs -- plain, coherent, coherent with the search (top-K,
          K = 40, min_score 2); decodes on the noise-only slots with the search on; k_coherent ms per launch
          at 1, 9, 17 and 33 rates for M = 8 and 32; the step with coherent = 8 and 32, search off and (1.0, 9)
  nsym    (--nsym, or --legs nsym) the multi-symbol sets (ft8_set_coherent_nsym): the sweep's decode fractions
          with a row per max_nsym (1 and 3), decodes on the noise-only slots at 3, k_coherent ms per launch at
          max_nsym 1 and 3 for M = 8 and 32, and the flagged step (config 3, and the same batch under top-K)
          at coherent = 32 for max_nsym 1, 2 and 3 with the rescued record counts

Prints one JSON line and writes it to --out.  Needs a GPU; there is no CPU fallback.
"""
import argparse
import ctypes
import json
import os
import socket
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

from ap_bench import AP, CFG3, FS, N, bp_candidates, cq_slots, timed_steps  # noqa: E402

CAPS = (8, 32, 0)


def crowded(args, dev):
    from ft8_demodulator_amd import synth
    return synth.make_slots(args.slots, 50, fs=FS, snr_db=(-24.0, -10.0),
                            seeds=[100000 + b for b in range(args.slots)], device=dev)[0]


def leg_step(torch, dev, args):
    from ft8_demodulator_amd import SlotDecoder, _lib, coherent
    x = crowded(args, dev)
    decs = [SlotDecoder(FS, 2, 2, device=dev, context=_lib.Context(dev.index), **CFG3)]
    decs += [SlotDecoder(FS, 2, 2, device=dev, context=_lib.Context(dev.index), coherent=m, **CFG3) for m in CAPS]
    # config 3's reference selection keeps the first 300 passing grid points in scan order: the time rows
    # before the slot starts, whose windows take k_coherent's range-checked path.  The same batch under
    # top-K selection (candidates inside the slot) for comparison
    topk = dict(CFG3, flags=_lib.FT8_FLAG_TOPK)
    decs += [SlotDecoder(FS, 2, 2, device=dev, context=_lib.Context(dev.index), coherent=m, **topk) for m in (None, 32)]
    times = timed_steps(torch, decs, x, args.steps, args.warmup)
    n_plain = bp_candidates(decs[0], x)
    out = {"slots": args.slots, "steps": args.steps, "warmup": args.warmup, "plain": times[0],
           "decodes_plain": sum(len(s) for s in decs[0].records(x)), "topk_plain": times[4],
           "topk_coherent_32": dict(times[5], rescued=sum(int(sum(coherent.coherent_index(r) for r in s))
                                                          for s in decs[5].records(x)))}
    for m, dec, t in zip(CAPS, decs[1:4], times[1:4]):
        recs = dec.records(x)
        out[f"coherent_{m or 'all'}"] = dict(
            t, bp_candidates_pass=bp_candidates(dec, x) - n_plain, decodes=sum(len(s) for s in recs),
            rescued=sum(int(sum(coherent.coherent_index(r) for r in s)) for s in recs),
            distinct_messages=sum(len({bytes(r["payload"]) for r in s}) for s in recs))
    out["distinct_messages_plain"] = sum(len({bytes(r["payload"]) for r in s}) for s in decs[0].records(x))
    return out


def leg_kernel(torch, dev, args):
    from ft8_demodulator_amd import _lib, coherent
    from ft8_demodulator_amd._pipeline import make_params, make_plan
    x = crowded(args, dev)
    S, K = args.slots, CFG3["max_candidates"]
    ctx, L, st = _lib.Context(dev.index), _lib.lib(), _lib.stream_handle(dev)
    plan = make_plan(N, FS)
    p = make_params(plan, K, CFG3["min_score"], 20, _lib.FT8_FLAG_TOPK)
    d_wf = torch.empty(S, plan.T, plan.F, dtype=torch.float32, device=dev)
    ctx.check(L.ft8_stft(ctx.handle, _lib.ptr(x), _lib.FT8_F32, N, S, N, ctypes.byref(p), _lib.ptr(d_wf), st), "stft")
    d_cand = torch.zeros(S, K, 2, dtype=torch.int32, device=dev)
    d_score = torch.zeros(S, K, dtype=torch.float64, device=dev)
    d_cnt = torch.zeros(S, dtype=torch.int32, device=dev)
    ctx.check(L.ft8_sync_select(ctx.handle, _lib.ptr(d_wf), 0, S, plan.T, plan.F, ctypes.byref(p), _lib.ptr(d_cand),
                                _lib.ptr(d_score), _lib.ptr(d_cnt), None, st), "select")
    cand, cnt = d_cand.cpu().numpy(), d_cnt.cpu().numpy()
    del d_wf
    hop, Q, D, Mt, Mg = coherent.geometry(plan.nperseg, 2)
    per_cand = (79 * Q + 2 * Mg) * D * 4
    rows = {}
    for m in CAPS:
        M = m or K
        w = np.arange(((S + 7) // 8) * 8 * M)
        slot, j = (w % 8) + 8 * ((w // 8) // M), (w // 8) % M
        keep = (slot < S) & (j < np.minimum(cnt[np.minimum(slot, S - 1)], M))
        slot, j = slot[keep], j[keep]
        n = len(slot)
        d_c = torch.from_numpy(np.ascontiguousarray(cand[slot, j])).to(dev)
        d_so = torch.from_numpy(slot.astype(np.int32)).to(dev)
        d_llr = torch.empty(n, 174, dtype=torch.float64, device=dev)
        d_fit = torch.empty(n * coherent.FIT_DTYPE.itemsize, dtype=torch.uint8, device=dev)

        def launch():
            ctx.check(L.ft8_coherent_llr(ctx.handle, _lib.ptr(x), _lib.FT8_F32, N, S, N, ctypes.byref(p), _lib.ptr(d_c),
                                         _lib.ptr(d_so), n, _lib.ptr(d_llr), _lib.ptr(d_fit), st), "coherent")
        for _ in range(args.warmup):
            launch()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
        ev[0].record()
        for i in range(args.steps):
            launch()
            ev[i + 1].record()
        torch.cuda.synchronize()
        ms = np.array([ev[i].elapsed_time(ev[i + 1]) for i in range(args.steps)])
        rows[f"M_{m or 'all'}"] = {"candidates": int(n), "median_ms": float(np.median(ms)), "min_ms": float(ms.min()),
                                   "max_ms": float(ms.max()), "sample_bytes": int(n) * per_cand,
                                   "sample_gb_per_s": float(n * per_cand / (np.median(ms) * 1e-3) / 1e9)}
    return {"slots": S, "bytes_per_candidate": per_cand, "rows": rows}


def leg_sweep(torch, dev, args):
    from ft8_demodulator_amd import SlotDecoder, _lib
    kw = dict(max_candidates=40, min_score=2, max_iterations=20, flags=_lib.FT8_FLAG_TOPK)
    decs = (("plain", SlotDecoder(FS, 2, 2, device=dev, **kw)),
            ("coherent", SlotDecoder(FS, 2, 2, device=dev, coherent=True, **kw)),
            ("coherent_ap", SlotDecoder(FS, 2, 2, device=dev, coherent=True, ap=AP, **kw)))
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
            "rows": rows}


def leg_noise(torch, dev, args):
    from ft8_demodulator_amd import SlotDecoder, coherent
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    x = torch.randn(args.slots, N, generator=g, device=dev, dtype=torch.float32)
    out = {"slots": args.slots, "seed": args.seed}
    for m in (32, 0):
        recs = SlotDecoder(FS, 2, 2, device=dev, coherent=m, **CFG3).records(x)
        out[f"coherent_{m or 'all'}"] = {
            "coherent_decodes": sum(int(sum(coherent.coherent_index(r) for r in s)) for s in recs),
            "plain_decodes": sum(int(sum(1 - coherent.coherent_index(r) for r in s)) for s in recs)}
    return out


DRIFT_RATES = (0.0, 0.25, -0.25, 0.5, -0.5, 0.75, -0.75, 1.0, -1.0, 1.5, -1.5)   # Hz/s
DRIFT_KERNEL_RATES = (1, 9, 17, 33)
DRIFT_STEP = (1.0, 9)


def _timed_launches(torch, launch, steps, warmup):
    for _ in range(warmup):
        launch()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    ev[0].record()
    for i in range(steps):
        launch()
        ev[i + 1].record()
    torch.cuda.synchronize()
    ms = np.array([ev[i].elapsed_time(ev[i + 1]) for i in range(steps)])
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max())}


def leg_drift(torch, dev, args):
    from ft8_demodulator_amd import SlotDecoder, _lib, coherent, synth
    from ft8_demodulator_amd._pipeline import make_params, make_plan
    search = (float(args.drift_search.split(":")[0]), int(args.drift_search.split(":")[1]))
    kw = dict(max_candidates=40, min_score=2, max_iterations=20, flags=_lib.FT8_FLAG_TOPK)
    decs = (("plain", SlotDecoder(FS, 2, 2, device=dev, context=_lib.Context(dev.index), **kw)),
            ("coherent", SlotDecoder(FS, 2, 2, device=dev, context=_lib.Context(dev.index), coherent=True, **kw)),
            ("coherent_drift", SlotDecoder(FS, 2, 2, device=dev, context=_lib.Context(dev.index), coherent=True,
                                           coherent_drift=search, **kw)))
    # ---- decode fractions: one signal per slot (synthesised on the CPU: the device's chain has no drift)
    table = []
    for k, snr in enumerate(args.drift_snrs):
        for r in DRIFT_RATES:
            x, truth = synth.make_slots(args.sweep_slots, 1, fs=FS, snr_db=float(snr),
                                        seeds=[args.seed + 1000 * k + s for s in range(args.sweep_slots)],
                                        drift_hz_per_s=r)
            x = x.to(dev)
            row = {"snr_db_full_band": float(snr), "snr_db_2500": float(snr + 10.0 * np.log10(FS / 2.0 / 2500.0)),
                   "rate_hz_per_s": r}
            for name, dec in decs:
                recs = dec.records(x)
                pay = [bytes(t.payloads[0]) for t in truth]
                hit = sum(any(bytes(v["payload"]) == pay[s] for v in recs[s]) for s in range(len(recs)))
                false = sum(sum(bytes(v["payload"]) != pay[s] for v in recs[s]) for s in range(len(recs)))
                row[name] = {"decoded": hit, "fraction": hit / len(recs), "false": false}
            table.append(row)
    # ---- noise-only slots, the search on
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    xn = torch.randn(args.slots, N, generator=g, device=dev, dtype=torch.float32)
    recs = SlotDecoder(FS, 2, 2, device=dev, coherent=32, coherent_drift=search, **CFG3).records(xn)
    noise = {"slots": args.slots, "search": search, "decodes": sum(len(s) for s in recs),
             "drift_decodes": sum(int(sum(coherent.drift_index(r) for r in s)) for s in recs)}
    # ---- k_coherent per launch over the number of rates, candidates listed as the in-batch launch lists them
    x = crowded(args, dev)
    S, K = args.slots, CFG3["max_candidates"]
    ctx, L, st = _lib.Context(dev.index), _lib.lib(), _lib.stream_handle(dev)
    plan = make_plan(N, FS)
    p = make_params(plan, K, CFG3["min_score"], 20, _lib.FT8_FLAG_TOPK)
    d_wf = torch.empty(S, plan.T, plan.F, dtype=torch.float32, device=dev)
    ctx.check(L.ft8_stft(ctx.handle, _lib.ptr(x), _lib.FT8_F32, N, S, N, ctypes.byref(p), _lib.ptr(d_wf), st), "stft")
    d_cand = torch.zeros(S, K, 2, dtype=torch.int32, device=dev)
    d_score = torch.zeros(S, K, dtype=torch.float64, device=dev)
    d_cnt = torch.zeros(S, dtype=torch.int32, device=dev)
    ctx.check(L.ft8_sync_select(ctx.handle, _lib.ptr(d_wf), 0, S, plan.T, plan.F, ctypes.byref(p), _lib.ptr(d_cand),
                                _lib.ptr(d_score), _lib.ptr(d_cnt), None, st), "select")
    cand, cnt = d_cand.cpu().numpy(), d_cnt.cpu().numpy()
    del d_wf
    kernel = {}
    for M in (8, 32):
        w = np.arange(((S + 7) // 8) * 8 * M)
        slot, j = (w % 8) + 8 * ((w // 8) // M), (w // 8) % M
        keep = (slot < S) & (j < np.minimum(cnt[np.minimum(slot, S - 1)], M))
        slot, j = slot[keep], j[keep]
        n = len(slot)
        d_c = torch.from_numpy(np.ascontiguousarray(cand[slot, j])).to(dev)
        d_so = torch.from_numpy(slot.astype(np.int32)).to(dev)
        d_llr = torch.empty(n, 174, dtype=torch.float64, device=dev)
        d_fit = torch.empty(n * coherent.FIT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_dr = torch.empty(n * coherent.DRIFT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        for R in DRIFT_KERNEL_RATES:
            def launch():
                ctx.check(L.ft8_coherent_drift_llr(ctx.handle, _lib.ptr(x), _lib.FT8_F32, N, S, N, ctypes.byref(p),
                                                   _lib.ptr(d_c), _lib.ptr(d_so), n, 1.0, R, _lib.ptr(d_llr),
                                                   _lib.ptr(d_fit), _lib.ptr(d_dr), st), "coherent drift")
            kernel[f"M_{M}_R_{R}"] = dict(_timed_launches(torch, launch, args.steps, args.warmup), candidates=int(n))
    # ---- the flagged step, search off and on, alternating on the crowded batch
    names, sd = [], []
    for m in (8, 32):
        for d in (None, DRIFT_STEP):
            names.append(f"coherent_{m}" + ("_drift" if d else ""))
            sd.append(SlotDecoder(FS, 2, 2, device=dev, context=_lib.Context(dev.index), coherent=m, coherent_drift=d,
                                  **CFG3))
    times = timed_steps(torch, sd, x, args.steps, args.warmup)
    step = {"search": DRIFT_STEP}
    for name, dec, t in zip(names, sd, times):
        recs = dec.records(x)
        step[name] = dict(t, decodes=sum(len(s) for s in recs),
                          rescued=sum(int(sum(coherent.coherent_index(r) for r in s)) for s in recs),
                          rescued_drifting=sum(int(sum(coherent.drift_index(r) for r in s)) for s in recs),
                          distinct_messages=sum(len({bytes(r["payload"]) for r in s}) for s in recs))
    return {"search": search, "slots_per_cell": args.sweep_slots, "selection": "top-K, K = 40, min_score 2",
            "table": table, "noise": noise, "kernel": kernel, "step": step}


def leg_nsym(torch, dev, args):
    from ft8_demodulator_amd import SlotDecoder, _lib, coherent
    from ft8_demodulator_amd._pipeline import make_params, make_plan
    kw = dict(max_candidates=40, min_score=2, max_iterations=20, flags=_lib.FT8_FLAG_TOPK)
    decs = [("plain", SlotDecoder(FS, 2, 2, device=dev, context=_lib.Context(dev.index), **kw))]
    decs += [(f"nsym_{n}", SlotDecoder(FS, 2, 2, device=dev, context=_lib.Context(dev.index), coherent=True,
                                       coherent_nsym=n, **kw)) for n in (1, 3)]
    # ---- decode fractions, the sweep's slots
    table = []
    for i, snr in enumerate(np.arange(args.snr_lo, args.snr_hi + 0.5, 1.0)):
        x, pay = cq_slots(args.sweep_slots, float(snr), args.seed + i, dev)
        row = {"snr_db_full_band": float(snr), "snr_db_2500": float(snr + 10.0 * np.log10(FS / 2.0 / 2500.0))}
        for name, dec in decs:
            recs = dec.records(x)
            hit = sum(any(bytes(r["payload"]) == bytes(pay[s]) for r in recs[s]) for s in range(len(recs)))
            false = sum(sum(bytes(r["payload"]) != bytes(pay[s]) for r in recs[s]) for s in range(len(recs)))
            row[name] = {"decoded": hit, "fraction": hit / len(recs), "false": false,
                         "multi_symbol": sum(int(sum(coherent.multisymbol_index(r) for r in s)) for s in recs)}
        table.append(row)
    # ---- noise-only slots at max_nsym 3
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    xn = torch.randn(args.slots, N, generator=g, device=dev, dtype=torch.float32)
    recs = SlotDecoder(FS, 2, 2, device=dev, coherent=32, coherent_nsym=3, **CFG3).records(xn)
    noise = {"slots": args.slots, "max_nsym": 3, "decodes": sum(len(s) for s in recs),
             "multi_symbol_decodes": sum(int(sum(coherent.multisymbol_index(r) for r in s)) for s in recs)}
    # ---- k_coherent per launch at max_nsym 1 and 3, candidates listed as the in-batch launch lists them
    x = crowded(args, dev)
    S, K = args.slots, CFG3["max_candidates"]
    ctx, L, st = _lib.Context(dev.index), _lib.lib(), _lib.stream_handle(dev)
    plan = make_plan(N, FS)
    p = make_params(plan, K, CFG3["min_score"], 20, _lib.FT8_FLAG_TOPK)
    d_wf = torch.empty(S, plan.T, plan.F, dtype=torch.float32, device=dev)
    ctx.check(L.ft8_stft(ctx.handle, _lib.ptr(x), _lib.FT8_F32, N, S, N, ctypes.byref(p), _lib.ptr(d_wf), st), "stft")
    d_cand = torch.zeros(S, K, 2, dtype=torch.int32, device=dev)
    d_score = torch.zeros(S, K, dtype=torch.float64, device=dev)
    d_cnt = torch.zeros(S, dtype=torch.int32, device=dev)
    ctx.check(L.ft8_sync_select(ctx.handle, _lib.ptr(d_wf), 0, S, plan.T, plan.F, ctypes.byref(p), _lib.ptr(d_cand),
                                _lib.ptr(d_score), _lib.ptr(d_cnt), None, st), "select")
    cand, cnt = d_cand.cpu().numpy(), d_cnt.cpu().numpy()
    del d_wf
    kernel = {}
    for M in (8, 32):
        w = np.arange(((S + 7) // 8) * 8 * M)
        slot, j = (w % 8) + 8 * ((w // 8) // M), (w // 8) % M
        keep = (slot < S) & (j < np.minimum(cnt[np.minimum(slot, S - 1)], M))
        slot, j = slot[keep], j[keep]
        n = len(slot)
        d_c = torch.from_numpy(np.ascontiguousarray(cand[slot, j])).to(dev)
        d_so = torch.from_numpy(slot.astype(np.int32)).to(dev)
        d_llr = torch.empty(n, 3, 174, dtype=torch.float64, device=dev)
        d_fit = torch.empty(n * coherent.FIT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_v = torch.empty(n, dtype=torch.uint8, device=dev)
        for ns in (1, 3):
            def launch():
                ctx.check(L.ft8_coherent_nsym_llr(ctx.handle, _lib.ptr(x), _lib.FT8_F32, N, S, N, ctypes.byref(p),
                                                  _lib.ptr(d_c), _lib.ptr(d_so), n, 0.0, 1, _lib.ptr(d_llr),
                                                  _lib.ptr(d_fit), None, ns, _lib.ptr(d_v), st), "coherent nsym")
            kernel[f"M_{M}_nsym_{ns}"] = dict(_timed_launches(torch, launch, args.steps, args.warmup), candidates=int(n))
    # ---- the flagged step at coherent = 32, alternating on the crowded batch: config 3 and top-K
    names, sd = [], []
    for sel, cfg in (("", CFG3), ("topk_", dict(CFG3, flags=_lib.FT8_FLAG_TOPK))):
        for ns in (1, 2, 3):
            names.append(f"{sel}nsym_{ns}")
            sd.append(SlotDecoder(FS, 2, 2, device=dev, context=_lib.Context(dev.index), coherent=32, coherent_nsym=ns,
                                  **cfg))
    times = timed_steps(torch, sd, x, args.steps, args.warmup)
    step = {"coherent": 32}
    for name, dec, t in zip(names, sd, times):
        recs = dec.records(x)
        step[name] = dict(t, decodes=sum(len(s) for s in recs),
                          rescued=sum(int(sum(coherent.coherent_index(r) for r in s)) for s in recs),
                          rescued_multi_symbol=sum(int(sum(coherent.multisymbol_index(r) for r in s)) for s in recs),
                          distinct_messages=sum(len({bytes(r["payload"]) for r in s}) for s in recs))
    return {"slots_per_step": args.sweep_slots, "selection": "top-K, K = 40, min_score 2", "table": table,
            "noise": noise, "kernel": kernel, "step": step}


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--legs", default="step,kernel,sweep,noise",
                   help="comma-separated subset of step,kernel,sweep,noise,drift,nsym")
    p.add_argument("--nsym", action="store_true", help="the multi-symbol sets' measurements only (--legs nsym)")
    p.add_argument("--drift", action="store_true", help="the drift search's measurements only (--legs drift)")
    p.add_argument("--drift-search", default="2.0:17", metavar="MAX:N",
                   help="the search of the drift leg's decode fractions and noise slots")
    p.add_argument("--drift-snrs", type=float, nargs=2, default=(-21.8, -13.8), metavar="DB",
                   help="the two full-band SNRs of the drift leg's table (default: -18 and -10 dB in 2500 Hz)")
    p.add_argument("--slots", type=int, default=256)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--sweep-slots", type=int, default=64)
    p.add_argument("--snr-lo", type=float, default=-27.0, help="full-band SNR of the first sweep step, dB")
    p.add_argument("--snr-hi", type=float, default=-18.0)
    p.add_argument("--seed", type=int, default=20261)
    p.add_argument("--out", default=os.path.join(os.environ.get("FT8_OUT", "out"), "coherent_bench.json"))
    args = p.parse_args()
    import torch
    from ft8_demodulator_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    res = {"box": socket.gethostname(), "gpu": torch.cuda.get_device_name(0),
           "build_id": _lib.lib().ft8_build_id().decode()}
    legs = {"step": leg_step, "kernel": leg_kernel, "sweep": leg_sweep, "noise": leg_noise, "drift": leg_drift,
            "nsym": leg_nsym}
    for name in (["drift"] if args.drift else ["nsym"] if args.nsym else args.legs.split(",")):
        res[name] = legs[name](torch, dev, args)
    line = json.dumps(res)
    out = args.out if os.path.isabs(args.out) else os.path.join(ROOT, args.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
