"""The construction that pins what the retry passes of ft8_decode_batch write into the records
(test_gpu_ap.py, test_gpu_coherent.py, test_gpu_coherent_drift.py, test_gpu_coherent_multisym.py): the device's
own stage calls give every candidate's LLRs, the oracle's BP the plain records, and the passes are applied on
the host by their restatements (coherent.retry_list, coherent.coherent_pass_restate, ap.ap_restate)."""
import ctypes

import numpy as np

import ap_cases as A
from ft8_demodulator_amd import _lib, coherent
from ft8_demodulator_amd import ap as _ap

ITERS = A.ITERS


def stage_records(x, fs, max_candidates, min_score, flags, bpt=2, sps=2):
    """The device half: samples x [n_slots, n] (float32) through ft8_stft, ft8_sync_select and ft8_llr (at bpt
    bins per tone and sps steps per symbol) on a context of its own -> (STFT LLRs [k, 174], rows [(slot, abs_time, abs_freq)] * k, the plain records [k] the
    oracle's BP decodes from the LLRs, with score, slot, cand_index, abs_time and abs_freq filled)."""
    from ft8_demodulator_amd._pipeline import make_params, make_plan
    torch = _lib.require_gpu()
    n_slots, n = x.shape
    ctx = _lib.Context(0)
    L, st = _lib.lib(), _lib.stream_handle(0)
    plan = make_plan(n, fs, bins_per_tone=bpt, steps_per_symbol=sps)
    N = max_candidates
    p = make_params(plan, N, min_score, ITERS, flags)
    d_x = torch.from_numpy(x).cuda()
    T, F = plan.T, plan.F
    d_wf = torch.empty(n_slots, T, F, dtype=torch.float32, device="cuda")
    ctx.check(L.ft8_stft(ctx.handle, _lib.ptr(d_x), _lib.FT8_F32, n, n_slots, n, ctypes.byref(p), _lib.ptr(d_wf), st),
              "ft8_stft")
    d_cand = torch.zeros(n_slots, N, 2, dtype=torch.int32, device="cuda")
    d_score = torch.zeros(n_slots, N, dtype=torch.float64, device="cuda")
    d_cnt = torch.zeros(n_slots, dtype=torch.int32, device="cuda")
    ctx.check(L.ft8_sync_select(ctx.handle, _lib.ptr(d_wf), 0, n_slots, T, F, ctypes.byref(p), _lib.ptr(d_cand),
                                _lib.ptr(d_score), _lib.ptr(d_cnt), None, st), "ft8_sync_select")
    cand, score, cnt = d_cand.cpu().numpy(), d_score.cpu().numpy(), d_cnt.cpu().numpy()
    rows = [(s, int(cand[s, i, 0]), int(cand[s, i, 1])) for s in range(n_slots) for i in range(int(cnt[s]))]
    d_c3 = torch.tensor(rows, dtype=torch.int32, device="cuda")
    d_llr = torch.empty(len(rows), 174, dtype=torch.float64, device="cuda")
    ctx.check(L.ft8_llr(ctx.handle, _lib.ptr(d_wf), 0, T, F, sps, bpt, _lib.ptr(d_c3), len(rows), 1, _lib.ptr(d_llr), st),
              "ft8_llr")
    llr = d_llr.cpu().numpy()
    rec0 = A.plain_records(llr)
    k = 0
    for s in range(n_slots):
        for i in range(int(cnt[s])):
            rec0["score"][k], rec0["slot"][k], rec0["cand_index"][k] = score[s, i], s, i
            rec0["abs_time"][k], rec0["abs_freq"][k] = cand[s, i]
            k += 1
    return llr, rows, rec0


def _bp(x, iters):
    with np.errstate(all="ignore"):
        return A.oracle_lib().bp_decode(x, iters)


def expectation(x, fs, search, cap=None, drift=None, nsym=1, ap=None, bpt=2, sps=2):
    """The records ft8_decode_batch must return for the slots x under the TOPK selection `search`
    (max_candidates, min_score), from stage_records: each slot's first `cap` (a number, or a function of the
    plain records that returns (slot, cap) as late_cap does; None: no coherent pass) failed candidates get the
    stage call's coherent LLRs -- with the drift search `drift` and up to `nsym` symbols per metric where
    given, at bpt bins per tone and sps steps per symbol -- and coherent_pass_restate applies them; with the patterns `ap`, ap_cases.restate follows on the STFT
    LLRs.  -> dict: x, the plain records, those after the coherent pass, `both` after coherent + AP (None
    without ap), the listed indices, cap and late_cap's slot; the arrays are read-only."""
    from ft8_demodulator_amd.ldpc_decoder import coherent_llr_batch
    x = np.array(x)
    llr, rows, rec0 = stage_records(x, fs, search["max_candidates"], search["min_score"], _lib.FT8_FLAG_TOPK, bpt, sps)
    slot = None
    if callable(cap):
        slot, cap = cap(rec0)
    listed, coh = np.zeros(0, dtype=np.int64), np.array(rec0, copy=True)
    if cap is not None:
        listed = coherent.retry_list(rec0, cap)
        # only the options given, so that each of the three stage calls stays the one its fixture reaches
        kw = {}
        if drift is not None:
            kw["drift"] = drift
        if nsym > 1:
            kw["nsym"] = nsym
        out = coherent_llr_batch(x, [rows[i][1:] for i in listed], [rows[i][0] for i in listed], fs,
                                 bins_per_tone=bpt, steps_per_symbol=sps, **kw)
        drifts = out[2] if drift is not None else None
        valid = out[-1] if nsym > 1 else None
        if valid is not None:
            assert np.array_equal(valid & 1, (out[1]["status"] == 0).astype(np.uint8))
        coh = coherent.coherent_pass_restate(rec0, listed, out[0], out[1], ITERS, _bp, A.oracle_lib().decode_tail,
                                             drifts, valid)
    both = None
    if ap:
        both = A.restate(llr, coh, [_ap.ap_hypothesis(t) for t in ap], _ap.DEFAULT_MAX_HARD_ERRORS)[0]
    for a in (rec0, coh, listed) + (() if both is None else (both,)):
        a.setflags(write=False)
    return {"x": x, "plain": rec0, "coherent": coh, "both": both, "listed": listed, "cap": cap, "slot": slot}


def late_cap(plain):
    """(slot, cap) from the plain records of three slots alone: the slot with the most failed candidates past
    its first 64 (what one wave scans in a round), and a cap halfway between its failed candidates among the
    first 64 and all its failed ones."""
    fails = [(int(((plain["slot"] == s) & (plain["ok"] == 0) & (plain["cand_index"] < 64)).sum()),
              int(((plain["slot"] == s) & (plain["ok"] == 0)).sum())) for s in range(3)]
    s = max(range(3), key=lambda i: fails[i][1] - fails[i][0])
    return s, (fails[s][0] + fails[s][1] + 1) // 2


def per_slot(rec, s):
    """The records a batch returns for slot s: the decoded ones."""
    return rec[(rec["slot"] == s) & (rec["ok"] == 1)]


def decoder(fs, search, bpt=2, sps=2, **kw):
    """A SlotDecoder under the TOPK selection `search` (flags= replaces the flags)."""
    from ft8_demodulator_amd._pipeline import SlotDecoder
    return SlotDecoder(fs, bins_per_tone=bpt, steps_per_symbol=sps, max_iterations=ITERS,
                       flags=kw.pop("flags", _lib.FT8_FLAG_TOPK), **search, **kw)
