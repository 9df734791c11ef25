"""Shared inputs for the multi-symbol coherent tests (test_coherent_multisym_reference.py,
test_gpu_coherent_multisym.py): the weak slots, the noiseless phase-continuous slots, the noise slots and the
whole path's slots, each computed once and never modified."""
import functools

import numpy as np

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


# ---- the whole path's inputs (retry_cases.expectation builds the expectation) --------------------------
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
