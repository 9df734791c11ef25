"""Shared inputs and constructions for the tests of the a-priori retries on the coherent LLRs
(test_coherent_ap_reference.py, test_gpu_coherent_ap.py): the stage call's LLR sets, the whole path's slots and
the expectation built from the existing helpers plus coherent.coherent_ap_restate.  Everything here but
`expectation` runs on the CPU, on the oracle's bp_decode / decode_tail; nothing is modified once computed."""
import functools

import numpy as np

import ap_cases as A
import retry_cases as R
from ft8_demodulator_amd import _lib, coherent, synth
from ft8_demodulator_amd import ap as _ap
from ft8_demodulator_amd.message import pack77

ITERS = A.ITERS
FS = A.E2E_FS

# ---- the stage call -----------------------------------------------------------------------------------
# Set 1 is ap_cases.stage_case()'s 67 vectors; sets 0 and 2 are the same codewords at a larger sigma from fixed
# seeds, so that a position's earlier set fails where a later one is rescued.
SET0_SEED, SET0_SIGMA = 105, 1.0
SET2_SEED, SET2_SIGMA = 205, 0.95
# H = 8: five first-call patterns no vector carries, then the stage patterns, so the winners are h = 6 and 7
EIGHT_PATTERNS = ("W9XYZ ? ?", "G4ABC ? ?", "JA1XYZ ? ?", "VK2DEF ? ?", "DL1ABC ? ?") + A.STAGE_PATTERNS
ONE_PATTERN = ("CQ ? ?",)


def _bp(x, iters):
    with np.errstate(all="ignore"):
        return A.oracle_lib().bp_decode(x, iters)


def hyps_of(patterns):
    """Patterns (ap.ap_hypothesis) or ready (mask, value) pairs -> [(mask, value)]."""
    return [_ap.ap_hypothesis(p) if isinstance(p, str) else (bytes(p[0]), bytes(p[1])) for p in patterns]


def payload_hyps(payloads):
    """One hypothesis per payload that knows what "CQ ? ?" knows of a CQ -- bits 0 .. 28 and 74 .. 76 -- for
    signals whose payloads are random bits, which no pattern names."""
    mask = np.zeros(80, dtype=np.uint8)
    mask[:29] = mask[74:77] = 1
    m = np.packbits(mask)
    return [(m.tobytes(), (np.frombuffer(bytes(p), dtype=np.uint8) & m).tobytes()) for p in payloads]


def restate(records, listed, llr, fits, hyps, max_hard, **kw):
    """coherent.coherent_ap_restate on the oracle's BP and tail."""
    return coherent.coherent_ap_restate(records, listed, llr, fits, hyps, ITERS, max_hard, _bp,
                                        A.oracle_lib().decode_tail, **kw)


@functools.lru_cache(maxsize=None)
def stage_sets():
    """-> llr [67, 3, 174] (read-only): sets 0 and 2 as above around ap_cases.stage_case()'s vectors as set 1."""
    c = A.stage_case()
    bits = synth.codeword_bits_batch(np.array(c["payloads"]))
    sets = []
    for seed, sigma in ((SET0_SEED, SET0_SIGMA), (SET2_SEED, SET2_SIGMA)):
        rng = np.random.default_rng(seed)
        sets.append(A.normalize_rows((2.0 * bits - 1.0) + sigma * rng.standard_normal(bits.shape)))
    llr = np.stack([sets[0], np.array(c["llr"]), sets[1]], axis=1)
    llr.setflags(write=False)
    return llr


def stage_llr(S):
    """The stage tests' LLRs at S sets [67, S, 174]: set 1 alone, sets 0 and 1, all three."""
    llr = stage_sets()
    return llr[:, 1:2] if S == 1 else llr[:, :S]


def all_fits(n, status=0):
    fits = np.zeros(n, dtype=coherent.FIT_DTYPE)
    fits["status"] = status
    return fits


def stage_restate(llr, records, hyps, max_hard, valid=None):
    """The stage call's contract: the n records are one list, every fit valid, no drift -> (records, hard)."""
    n = len(records)
    return restate(records, np.arange(n), llr, all_fits(n), hyps, max_hard, valid=valid)


@functools.lru_cache(maxsize=None)
def stage_reference():
    """The CPU test's case: sets 0 and 1, the three stage hypotheses, no hard-error limit, on the records plain
    BP wrote from set 1 -> dict(llr, records, hyps, ref, hard)."""
    c = A.stage_case()
    llr = stage_llr(2)
    ref, hard = stage_restate(llr, c["plain"], list(c["hyps"]), 174)
    ref.setflags(write=False)
    hard.setflags(write=False)
    return {"llr": llr, "records": c["plain"], "hyps": c["hyps"], "ref": ref, "hard": hard}


@functools.lru_cache(maxsize=None)
def stage_order():
    """The 67 indices with the reference's rescues first (a later-set rescue, then one at h > 0), so that the
    stage tests at n = 1, 4 and 5 retry something; then a record that is ok already, then the rest."""
    r = stage_reference()
    ref, plain = r["ref"], r["records"]
    rescued = np.nonzero(ref["pass_index"] != 0)[0]
    later = [i for i in rescued if ref["pass_index"][i] & 8]
    high = [i for i in rescued if (ref["pass_index"][i] >> 4) > 2 and i not in later[:1]]
    ok = np.nonzero(plain["ok"])[0]
    failed = np.nonzero(ref["ok"] == 0)[0]
    head = later[:1] + high[:1] + [int(ok[0]), int(failed[0])]
    return tuple(head + [i for i in range(len(ref)) if i not in head])


# ---- the whole path -----------------------------------------------------------------------------------
E2E = dict(max_candidates=40, min_score=2)
AP = ["K1ABC ? ?", "CQ ? ?"]          # K1ABC first, so the CQ rescues have h = 1
CAP = 8
# Found on the CPU (the oracle's front end and BP, coherent.coherent_restate): the seed and the SNR tuple,
# ap_cases.E2E_SNR_DB shifted down, at which the expectation shows every outcome with a margin.
E2E_SEED = 6
E2E_SHIFT_DB = -1.0
E2E_SNR_DB = tuple(v + E2E_SHIFT_DB for v in A.E2E_SNR_DB)
THIRD_SEED = E2E_SEED + 1


@functools.lru_cache(maxsize=None)
def e2e_slots(seed=E2E_SEED, snr_db=E2E_SNR_DB, third_seed=THIRD_SEED):
    """ap_cases.e2e_samples(seed, snr_db) -- eight CQ signals in slot 0, noise in slot 1 -- followed by slot 0 of
    the same construction at third_seed -> float32 [3, 180000], read-only."""
    x = np.concatenate([A.e2e_samples(seed, snr_db), A.e2e_samples(third_seed, snr_db)[:1]])
    x.setflags(write=False)
    return x


def sent_payloads():
    return frozenset(bytes(p) for p in A.e2e_payloads())


def construct(llr, rows, rec0, coh_llr, cap, ap=AP, drift=None, nsym=1, coherent_ap=True,
              max_hard=_ap.DEFAULT_MAX_HARD_ERRORS):
    """Steps 2 - 6 of the construction on the plain records rec0 of every candidate (rows [(slot, abs_time,
    abs_freq)], STFT LLRs llr): coherent.retry_list, the coherent stage call coh_llr(cand, slot_of, **kw),
    coherent.coherent_pass_restate, coherent.coherent_ap_restate on the listed positions' coherent LLRs and
    ap_cases.restate on the STFT LLRs -> dict of read-only arrays: plain, coherent (after the coherent pass),
    coh_ap (after the new stage), both (after the a-priori pass), listed, hard."""
    slot = None
    if callable(cap):
        slot, cap = cap(rec0)
    listed = coherent.retry_list(rec0, cap)
    kw = {}
    if drift is not None:
        kw["drift"] = drift
    if nsym > 1:
        kw["nsym"] = nsym
    out = coh_llr([rows[i][1:] for i in listed], [rows[i][0] for i in listed], **kw)
    drifts = out[2] if drift is not None else None
    valid = out[-1] if nsym > 1 else None
    tail = A.oracle_lib().decode_tail
    hyps = hyps_of(ap)
    coh = coherent.coherent_pass_restate(rec0, listed, out[0], out[1], ITERS, _bp, tail, drifts, valid)
    hard = np.full(len(rec0), -1, dtype=np.int16)
    cap_rec = coh
    if coherent_ap:
        cap_rec, hard = restate(coh, listed, out[0], out[1], hyps, max_hard, drifts=drifts, valid=valid)
    both = A.restate(llr, cap_rec, hyps, max_hard)[0]
    res = {"plain": rec0, "coherent": coh, "coh_ap": cap_rec, "both": both, "listed": listed, "hard": hard}
    for a in res.values():
        a.setflags(write=False)
    return dict(res, cap=cap, slot=slot)


def expectation(x, search=E2E, cap=CAP, ap=AP, drift=None, nsym=1, coherent_ap=True, fs=FS):
    """The records ft8_decode_batch must return for the slots x with coherent_ap on: retry_cases.stage_records
    (the device's front end and the oracle's BP), then `construct` with the device's coherent stage call."""
    from ft8_demodulator_amd.ldpc_decoder import coherent_llr_batch
    x = np.array(x)
    llr, rows, rec0 = R.stage_records(x, fs, search["max_candidates"], search["min_score"], _lib.FT8_FLAG_TOPK)
    e = construct(llr, rows, rec0, lambda cand, so, **kw: coherent_llr_batch(x, cand, so, fs, **kw), cap, ap, drift,
                  nsym, coherent_ap)
    return dict(e, x=x)


def outcomes(e):
    """Counts over the expectation's candidates: plain decodes, coherent-only rescues, rescues by the new stage
    (bit 1 and a hypothesis index), STFT a-priori rescues (a hypothesis index without bit 1), listed candidates
    nothing rescues."""
    both = e["both"]
    pi = both["pass_index"]
    return {"plain": int(((both["ok"] == 1) & (pi == 0)).sum()),
            "coherent": int((((pi & 2) != 0) & ((pi >> 4) == 0)).sum()),
            "coherent_ap": int((((pi & 2) != 0) & ((pi >> 4) != 0)).sum()),
            "stft_ap": int((((pi & 2) == 0) & ((pi >> 4) != 0)).sum()),
            "listed_failed": int((both["ok"][e["listed"]] == 0).sum())}


# ---- the gain test's slots ----------------------------------------------------------------------------
N_WEAK = 32
WEAK_SEED0 = 9000
# tools/coherent_ap_bench.py, decode-fraction table: the 1 dB step at which coherent + STFT-AP (coherent_ap off)
# decodes between 20 % and 80 % of its slots; the row is quoted in DESIGN.md section 12d.
WEAK_SNR_DB = -24.0


def cq_slots(n, snr_db, seed0, fs=FS):
    """n one-signal slots as synth.make_slots(1, 1, snr_db=snr_db, seeds=[seed0 + s]) builds them -- the same
    draws of f0 and start, the same noise -- but with the payload pack77("CQ " + call), the calls of
    ap_cases.E2E_CALLS in turn -> (samples float32 [n, 180000], payloads)."""
    import torch
    N = int(15.0 * fs)
    nsps = int(0.16 * fs)
    xs, pays = [], []
    for s in range(n):
        sd = seed0 + s
        rng = np.random.default_rng(sd)
        synth.random_payload(rng)                      # make_slots draws the payload first
        snr = rng.uniform(snr_db, snr_db, 1)
        f0 = rng.uniform(200.0, 2800.0, 1)
        st = rng.uniform(0.0, 2.0, 1)
        g = torch.Generator(device="cpu")
        g.manual_seed(sd)
        acc = torch.randn(N, generator=g, dtype=torch.float64)
        pay = pack77("CQ " + A.E2E_CALLS[s % len(A.E2E_CALLS)])
        tones = torch.as_tensor(np.stack([synth.itones(pay)]))
        wav = synth.gfsk_waveforms(tones, fs, torch.as_tensor(f0)) * float(np.sqrt(2.0 * 10.0 ** (snr[0] / 10.0)))
        s0 = int(st[0] * fs)
        m = min(79 * nsps, N - s0)
        acc[s0:s0 + m] += wav[0, :m]
        xs.append(acc.to(torch.float32).numpy())
        pays.append(bytes(pay))
    return np.stack(xs), tuple(pays)


@functools.lru_cache(maxsize=None)
def weak_cq_slots():
    x, pays = cq_slots(N_WEAK, WEAK_SNR_DB, WEAK_SEED0)
    x.setflags(write=False)
    return x, pays
