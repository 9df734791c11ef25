"""Shared inputs for the coherent drift-search tests (test_coherent_drift_reference.py,
test_gpu_coherent_drift.py): drifting synthetic slots, candidate lists and the float64 restatement's
results, each computed once on the CPU and never modified."""
import functools

import numpy as np

import coherent_cases as C
from ft8_demodulator_amd import coherent, synth

FS, NSPS, HOP, NFFT, BIN = C.FS, C.NSPS, C.HOP, C.NFFT, C.BIN
DRIFT = (1.0, 9)          # the default search: +-1 Hz/s in steps of 0.25
DRIFT_WIDE = (4.0, 33)    # the widest the library takes
GAIN_RATE = 0.5           # Hz/s: one tone over the slot
# full-band; -19.2 dB in 2500 Hz.  At coherent_cases.WEAK_SNR_DB (-22) synth's GFSK does not separate the
# two passes at this rate (float64: 8 of 16 without the search, 16 with it); one dB lower it does (0 and 14)
GAIN_SNR_DB = -23.0
N_GAIN = 16


def fsk_tones_drift(payload, fs, nsps, f0, start, n_samples, rate, amplitude=1.0):
    """coherent_cases.fsk_tones with a linear drift of `rate` Hz/s about the centre of the 79 symbols:
    the phase gains pi rate tau^2, tau = (n - 39.5 nsps) / fs."""
    tones = synth.itones(payload).astype(np.float64)
    n = np.arange(79 * nsps)
    tau = (n - 39.5 * nsps) / fs
    x = amplitude * np.cos(2.0 * np.pi * ((f0 + 6.25 * np.repeat(tones, nsps)) * (start + n) / fs + 0.5 * rate * tau * tau))
    out = np.zeros(n_samples, dtype=np.float64)
    lo, hi = max(start, 0), min(start + len(n), n_samples)
    if hi > lo:
        out[lo:hi] = x[lo - start:hi - start]
    return out.astype(np.float32)


@functools.lru_cache(maxsize=None)
def gain_slots():
    """16 one-signal 12 kHz slots at GAIN_SNR_DB drifting by GAIN_RATE
    -> (samples float32 [16, 180000], payloads, (abs_time, abs_freq) nearest the truth)."""
    xs, pays, cands = [], [], []
    for s in range(N_GAIN):
        x, truth = synth.make_slots(1, 1, fs=FS, snr_db=GAIN_SNR_DB, seeds=[5100 + s], drift_hz_per_s=GAIN_RATE)
        xs.append(x[0].numpy())
        pays.append(bytes(truth[0].payloads[0]))
        cands.append(C.nearest(truth[0]))
    x = np.stack(xs)
    x.setflags(write=False)
    return x, tuple(pays), tuple(cands)


# ---- the stage test's inputs ----------------------------------------------------------------------------
STAGE_RATES = (0.0, 1.0, -0.6)      # per slot: a static signal, two drifting ones (the last one late)


def _pcm(x):
    return np.clip(np.round(x / 8.0 * 32767.0), -32767, 32767).astype(np.int16)


@functools.lru_cache(maxsize=None)
def stage_slots_12k():
    """3 slots (not a multiple of 8) at 12 kHz: per slot a static signal, one at +1.0 Hz/s and one at
    -0.6 Hz/s that starts near 2.4 s, so that its final Costas block is incomplete; candidates: the 3 x 3
    grid points around every truth, windows that start before sample 0 and end past the slot.
    -> dict: samples x (float32) and pcm (int16), cand, slot_of, and the payloads (one per 9 candidates)."""
    xs, cand, slot_of, pays = [], [], [], []
    for s in range(3):
        x2, t2 = synth.make_slots(1, 2, fs=FS, snr_db=(-16.0, -8.0), seeds=[7400 + s], drift_hz_per_s=STAGE_RATES[:2])
        x1, t1 = synth.make_slots(1, 1, fs=FS, snr_db=(-16.0, -8.0), start_range=(2.38, 2.42), seeds=[7500 + s],
                                  noise=False, drift_hz_per_s=STAGE_RATES[2])
        xs.append((x2[0] + x1[0]).numpy())
        for t, k in ((t2[0], 0), (t2[0], 1), (t1[0], 0)):
            cand += C._grid9(*C.nearest(t, k))
            slot_of += [s] * 9
            pays.append(bytes(t.payloads[k]))
    cand += [(-12, 700), (187, 640)]          # a window that starts before the slot, one past its end
    slot_of += [0, 1]
    x = np.stack(xs).astype(np.float32)
    out = {"x": x, "pcm": _pcm(x), "cand": np.array(cand, dtype=np.int32), "slot_of": np.array(slot_of, dtype=np.int32),
           "payloads": tuple(pays)}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def stage_case_12k(key):
    """The restatement's (llr, fits, drifts, volumes) of stage_slots_12k with DRIFT, key "f32" or "i16"."""
    c = stage_slots_12k()
    return coherent.coherent_restate(c["x"] if key == "f32" else c["pcm"], c["cand"], c["slot_of"], FS, NSPS, NFFT, 2,
                                     details=True, drift=DRIFT)


@functools.lru_cache(maxsize=None)
def stage_case_wide():
    """Slot 0 of stage_slots_12k with DRIFT_WIDE (33 rates over +-4 Hz/s) -> (cand, slot_of, restatement)."""
    c = stage_slots_12k()
    keep = c["slot_of"] == 0
    cand, slot_of = c["cand"][keep], c["slot_of"][keep]
    return cand, slot_of, coherent.coherent_restate(c["x"][:1], cand, slot_of, FS, NSPS, NFFT, 2, details=True,
                                                    drift=DRIFT_WIDE)


@functools.lru_cache(maxsize=None)
def stage_case_10k():
    """One slot at fs = 10000 with 4 bins per tone and 4 steps per symbol (D = 50: the range-checked
    load path), a static signal and one at +1.0 Hz/s, with DRIFT."""
    x, t = synth.make_slots(1, 2, fs=C.FS10, snr_db=(-14.0, -8.0), f0_range=(300.0, 2500.0), seeds=[7601],
                            drift_hz_per_s=STAGE_RATES[:2])
    hop, binw = C.NSPS10 // C.SPS10, C.FS10 / C.NFFT10
    cand = []
    for k in range(2):
        cand += C._grid9(*C.nearest(t[0], k, C.FS10, hop, binw))
    cand = np.array(cand, dtype=np.int32)
    slot_of = np.zeros(len(cand), dtype=np.int32)
    x = x.numpy().astype(np.float32)
    ref = coherent.coherent_restate(x, cand, slot_of, C.FS10, C.NSPS10, C.NFFT10, C.SPS10, details=True, drift=DRIFT)
    for v in (x, cand, slot_of):
        v.setflags(write=False)
    return {"x": x, "cand": cand, "slot_of": slot_of, "ref": ref}


# ---- the device gain test's inputs -------------------------------------------------------------------------
DEVICE_DRIFT = (2.0, 17)
DEVICE_RATE = 1.25
DEVICE_SNR_DB = -11.8     # full-band: -8 dB in 2500 Hz (10 log10(6000 / 2500) = 3.8)
N_DEVICE = 8
DEVICE_SEARCH = dict(max_candidates=40, min_score=2)


@functools.lru_cache(maxsize=None)
def device_gain_slots():
    """8 one-signal slots at -8 dB in 2500 Hz drifting by +-1.25 Hz/s (alternating)
    -> (samples float32 [8, 180000], payloads, (abs_time, abs_freq) nearest the truth, rates)."""
    xs, pays, cands, rates = [], [], [], []
    for s in range(N_DEVICE):
        r = DEVICE_RATE if s % 2 == 0 else -DEVICE_RATE
        x, truth = synth.make_slots(1, 1, fs=FS, snr_db=DEVICE_SNR_DB, seeds=[5200 + s], drift_hz_per_s=r)
        xs.append(x[0].numpy())
        pays.append(bytes(truth[0].payloads[0]))
        cands.append(C.nearest(truth[0]))
        rates.append(r)
    x = np.stack(xs)
    x.setflags(write=False)
    return x, tuple(pays), tuple(cands), tuple(rates)
