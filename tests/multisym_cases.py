"""Shared inputs for the multi-symbol coherent tests (test_coherent_multisym_reference.py,
test_gpu_coherent_multisym.py): the weak slots, the noiseless phase-continuous slots, the noise slots and the
whole path's expectation builder, each computed once and never modified."""
import ctypes
import functools

import numpy as np

import ap_cases as A
import coherent_cases as C
from ft8_demodulator_amd import coherent, synth

ITERS = C.ITERS
FS, NSPS, NFFT, HOP = C.FS, C.NSPS, C.NFFT, C.HOP
S = 3                                  # max_nsym of every test
WEAK_SNR_DB = -23.0                    # full-band; -19.2 dB in 2500 Hz
N_WEAK = 32
WEAK_SEED0 = 9000
# set 1 fails and a later set decodes at the nearest grid point (float64 prototype)
LATER_SET_SEEDS = (9000, 9002, 9007, 9013, 9016, 9023)
CLEAN_SEEDS = (77, 78, 79, 80)
N_NOISE = 64


@functools.lru_cache(maxsize=None)
def weak_slots():
    """32 one-signal 12 kHz slots at -23 dB -> (samples float32 [32, 180000], payloads, (abs_time, abs_freq))."""
    xs, pays, cands = [], [], []
    for s in range(N_WEAK):
        x, truth = synth.make_slots(1, 1, fs=FS, snr_db=WEAK_SNR_DB, seeds=[WEAK_SEED0 + s])
        xs.append(x[0].numpy())
        pays.append(bytes(truth[0].payloads[0]))
        cands.append(C.nearest(truth[0]))
    x = np.stack(xs)
    x.setflags(write=False)
    return x, tuple(pays), tuple(cands)


@functools.lru_cache(maxsize=None)
def weak_restated():
    """The restatement at max_nsym 3 on the weak slots' nearest grid points -> (llr [32, 3, 174], fits, valid)."""
    x, _, cands = weak_slots()
    out = coherent.coherent_restate(x, np.array(cands), np.arange(N_WEAK), FS, NSPS, NFFT, 2, nsym=S)
    for v in out:
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def clean_slots():
    """4 noiseless one-signal slots (GFSK, continuous phase; df from -0.80 to +1.56 Hz)
    -> (samples [4, 180000], payloads, candidates, tones [4, 79])."""
    xs, pays, cands, tones = [], [], [], []
    for seed in CLEAN_SEEDS:
        x, truth = synth.make_slots(1, 1, fs=FS, snr_db=-10.0, seeds=[seed], noise=False)
        xs.append(x[0].numpy())
        pays.append(bytes(truth[0].payloads[0]))
        cands.append(C.nearest(truth[0]))
        tones.append(np.asarray(synth.itones(pays[-1])))
    x = np.stack(xs)
    x.setflags(write=False)
    return x, tuple(pays), tuple(cands), np.stack(tones)


@functools.lru_cache(maxsize=None)
def noise_slots(n=N_NOISE):
    """n noise-only slots (default_rng(1), unit variance) and one arbitrary candidate each."""
    rng = np.random.default_rng(1)
    x = rng.standard_normal((n, 180000)).astype(np.float32)
    cand = np.stack([rng.integers(0, 40, n), rng.integers(100, 1100, n)], axis=1).astype(np.int32)
    x.setflags(write=False)
    cand.setflags(write=False)
    return x, cand


def first_set(O, llr3, valid):
    """The first valid set (1-based) of one candidate's [S, 174] LLRs that the oracle's BP and tail decode
    -> (set or 0, payload or None)."""
    for n in range(llr3.shape[0]):
        if (int(valid) >> n) & 1:
            ok, pay = C.decode_llr(O, llr3[n])[:2]
            if ok:
                return n + 1, pay
    return 0, None


# ---- the whole path's expectation ------------------------------------------------------------------------
E2E = dict(max_candidates=20, min_score=2)
CAP = 4
AP = ["CQ ? ?"]


@functools.lru_cache(maxsize=None)
def e2e_slots():
    """The three stage_case_12k slots and the six weak slots a later set decodes -> (samples [9, 180000],
    the set of transmitted payloads)."""
    x, pays, _ = weak_slots()
    idx = [s - WEAK_SEED0 for s in LATER_SET_SEEDS]
    c = C.stage_case_12k()
    out = np.concatenate([np.array(c["x"]), x[idx]])
    out.setflags(write=False)
    return out, frozenset(c["payloads"]) | frozenset(pays[i] for i in idx)


def expectation(torch, _lib, oracle, with_ap=True):
    """test_gpu_coherent.py's construction with the sets: ft8_stft, ft8_sync_select and ft8_llr give every
    candidate's STFT LLRs, the oracle's BP the plain records; each slot's first CAP failed candidates get
    the stage call's LLRs at max_nsym 3, and the sets are decoded by the oracle in order: the first valid
    set that decodes (with a valid fit) writes the record, pass_index 2, and 10 from set 2 or 3.
    -> records after the coherent pass, after coherent + AP, the plain ones, the listed indices."""
    from ft8_demodulator_amd import ap
    from ft8_demodulator_amd._pipeline import make_params, make_plan
    from ft8_demodulator_amd.ldpc_decoder import coherent_llr_batch
    x = np.array(e2e_slots()[0])
    n_slots, n = x.shape
    ctx = _lib.Context(0)
    L, st = _lib.lib(), _lib.stream_handle(0)
    plan = make_plan(n, FS)
    N = E2E["max_candidates"]
    p = make_params(plan, N, E2E["min_score"], ITERS, _lib.FT8_FLAG_TOPK)
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
    ctx.check(L.ft8_llr(ctx.handle, _lib.ptr(d_wf), 0, T, F, 2, 2, _lib.ptr(d_c3), len(rows), 1, _lib.ptr(d_llr), st),
              "ft8_llr")
    llr = d_llr.cpu().numpy()
    rec0 = A.plain_records(llr)
    k = 0
    for s in range(n_slots):
        for i in range(int(cnt[s])):
            rec0["score"][k], rec0["slot"][k], rec0["cand_index"][k] = score[s, i], s, i
            rec0["abs_time"][k], rec0["abs_freq"][k] = cand[s, i]
            k += 1
    listed = [i for s in range(n_slots) for i in np.nonzero((rec0["slot"] == s) & (rec0["ok"] == 0))[0][:CAP]]
    cl, cf, cv = coherent_llr_batch(x, [(rows[i][1], rows[i][2]) for i in listed], [rows[i][0] for i in listed], FS,
                                    nsym=S)
    coh = np.array(rec0, copy=True)
    for i, v, f, b in zip(listed, cl, cf, cv):
        assert (int(b) & 1) == int(f["status"] == 0)
        for m in range(S):
            if f["status"] != 0 or not (int(b) >> m) & 1:
                continue
            ok, pay, ce, cc, err = C.decode_llr(oracle, v[m])
            if ok:
                coh["ok"][i], coh["pass_index"][i] = 1, 2 | (8 if m > 0 else 0)
                coh["payload"][i] = np.frombuffer(pay, dtype=np.uint8)
                coh["crc_extracted"][i], coh["crc_calculated"][i], coh["ldpc_errors"][i] = ce, cc, err
                break
    both = A.restate(llr, coh, [ap.ap_hypothesis(t) for t in AP], ap.DEFAULT_MAX_HARD_ERRORS)[0] if with_ap else None
    for a in (rec0, coh) + ((both,) if with_ap else ()):
        a.setflags(write=False)
    return {"x": x, "plain": rec0, "coherent": coh, "both": both, "listed": listed}
