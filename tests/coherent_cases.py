"""Shared inputs for the coherent re-demodulation tests (test_coherent_reference.py,
test_gpu_coherent.py): synthetic slots, candidate lists and the float64 restatement's results, each
computed once on the CPU and never modified."""
import functools

import numpy as np

from ft8_demodulator_amd import coherent, synth

ITERS = 20
FS = 12000
NSPS, HOP, NFFT = 1920, 960, 3840      # 12 kHz at 2 bins per tone, 2 steps per symbol
BIN = FS / NFFT
WEAK_SNR_DB = -22.0                    # full-band; -18.2 dB in 2500 Hz
N_WEAK = 16


def nearest(truth, i=0, fs=FS, hop=HOP, binw=BIN):
    """The grid point nearest signal i of a SlotTruth, as tests/test_snr_reference.py computes it."""
    return int(round(int(truth.start_s[i] * fs) / float(hop))), int(round(truth.f0[i] / binw))


@functools.lru_cache(maxsize=None)
def weak_slots():
    """16 one-signal 12 kHz slots at -22 dB -> (samples float32 [16, 180000], payloads, (abs_time, abs_freq))."""
    xs, pays, cands = [], [], []
    for s in range(N_WEAK):
        x, truth = synth.make_slots(1, 1, fs=FS, snr_db=WEAK_SNR_DB, seeds=[5000 + s])
        xs.append(x[0].numpy())
        pays.append(bytes(truth[0].payloads[0]))
        cands.append(nearest(truth[0]))
    x = np.stack(xs)
    x.setflags(write=False)
    return x, tuple(pays), tuple(cands)


def decode_llr(O, llr, iters=ITERS):
    """Oracle bp_decode + decode_tail -> (ok, payload bytes, crc_extracted, crc_calculated, ldpc_errors)."""
    with np.errstate(all="ignore"):
        plain, err = O.bp_decode(llr, iters)
    ok, pay, ce, cc = O.decode_tail(plain, err)
    return bool(ok), bytes(pay), ce, cc, err


def fsk_tones(payload, fs, nsps, f0, start, n_samples, amplitude=1.0):
    """A noiseless rectangular FSK tone sequence (no GFSK smoothing, no ramps): symbol k is
    amplitude cos(2 pi (f0 + 6.25 tone_k) n / fs) on samples [start + k nsps, start + (k + 1) nsps)."""
    tones = synth.itones(payload).astype(np.float64)
    n = np.arange(79 * nsps)
    x = amplitude * np.cos(2.0 * np.pi * (f0 + 6.25 * np.repeat(tones, nsps)) * (start + n) / fs)
    out = np.zeros(n_samples, dtype=np.float64)
    lo, hi = max(start, 0), min(start + len(n), n_samples)
    if hi > lo:
        out[lo:hi] = x[lo - start:hi - start]
    return out.astype(np.float32)


# ---- the stage comparison ---------------------------------------------------------------------------------
# max |LLR_device - LLR_restate| over the stage test's candidates, measured once on an MI355X against
# the float64 restatement: 1.65e-5 (12 kHz float32), 1.86e-5 (int16), 1.11e-5 (10 kHz); the LLRs are scaled
# to a variance of 24.  The bound is 8 x the largest (float32 summation order varies by a small factor
# from input to input); 1 % of sqrt(24) would be 4.9e-2.
LLR_MEASURED = 1.86e-5
LLR_BOUND = 8 * LLR_MEASURED


def check_stage(name, got, ref, fs, D, binw, bound=LLR_BOUND):
    """The device's (llr, fits) of a stage call against the restatement's (llr, fits, grids) -> the mask of
    the candidates compared (measured, and no near tie in their grid) and the largest LLR difference."""
    llr, fits = got
    rllr, rfits, grids = ref
    assert np.array_equal(fits["status"], rfits["status"])
    assert np.array_equal(fits["n_sync"], rfits["n_sync"])
    measured = fits["status"] == 0
    tie = np.array([g is not None and coherent.near_tie(g) for g in grids])
    cmp_ = measured & ~tie
    assert int((measured & tie).sum()) * 20 <= int(measured.sum())
    assert np.array_equal(fits["dt_index"][cmp_], rfits["dt_index"][cmp_])
    assert np.array_equal(fits["df_index"][cmp_], rfits["df_index"][cmp_])
    assert np.abs(fits["df_hz"][cmp_].astype(np.float64) - rfits["df_hz"][cmp_]).max() <= 0.01
    assert np.array_equal(fits["dt_s"][cmp_], (rfits["dt_index"][cmp_] * (D / fs)).astype(np.float32))
    assert np.allclose(fits["metric"][cmp_], rfits["metric"][cmp_], rtol=1e-4)
    # status 2 / 3: zeros
    assert (llr[~measured] == 0.0).all()
    err = float(np.abs(llr[cmp_] - rllr[cmp_]).max())
    print(f"{name}: {int(cmp_.sum())} candidates compared, {int((measured & tie).sum())} near ties left out, "
          f"max |LLR_device - LLR_restate| = {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    return cmp_, err


# ---- the stage test's inputs ----------------------------------------------------------------------------
def _grid9(at, af):
    return [(at + a, af + b) for a in (-1, 0, 1) for b in (-1, 0, 1)]


@functools.lru_cache(maxsize=None)
def stage_case_12k():
    """3 slots (not a multiple of 8) at 12 kHz, 3 signals each at -16 .. -8 dB, the third signal of
    every slot starting near 2.4 s so that its last symbols lie beyond the slot's end; candidates:
    the 3 x 3 grid points around every truth, one candidate with negative abs_time whose window starts
    before the slot, one past the slot's end.  -> dict with samples (float32 and int16 PCM), cand,
    slot_of and the restatement's results for both dtypes."""
    xs, cand, slot_of, pays = [], [], [], []
    for s in range(3):
        x2, t2 = synth.make_slots(1, 2, fs=FS, snr_db=(-16.0, -8.0), seeds=[7100 + s])
        x1, t1 = synth.make_slots(1, 1, fs=FS, snr_db=(-16.0, -8.0), start_range=(2.38, 2.42), seeds=[7200 + s],
                                  noise=False)
        xs.append((x2[0] + x1[0]).numpy())
        for t, k in ((t2[0], 0), (t2[0], 1), (t1[0], 0)):
            cand += _grid9(*nearest(t, k))
            slot_of += [s] * 9
            pays.append(bytes(t.payloads[k]))
    cand += [(-12, 700), (-3, 400), (160, 500), (187, 640)]   # windows that start before / end past the slot
    slot_of += [0, 1, 2, 1]
    x = np.stack(xs).astype(np.float32)
    pcm = np.clip(np.round(x / 8.0 * 32767.0), -32767, 32767).astype(np.int16)
    cand, slot_of = np.array(cand, dtype=np.int32), np.array(slot_of, dtype=np.int32)
    out = {"x": x, "pcm": pcm, "cand": cand, "slot_of": slot_of, "payloads": tuple(pays)}
    for key, data in (("f32", x), ("i16", pcm)):
        out[key] = coherent.coherent_restate(data, cand, slot_of, FS, NSPS, NFFT, 2, details=True)
    for v in (x, pcm, cand, slot_of):
        v.setflags(write=False)
    return out


FS10 = 10000
NSPS10, NFFT10, SPS10, BPT10 = 1600, 6400, 4, 4


@functools.lru_cache(maxsize=None)
def stage_case_10k():
    """One slot at fs = 10000 with 4 bins per tone and 4 steps per symbol (nsps 1600, Q 32, D 50, hop 400)."""
    x, t = synth.make_slots(1, 2, fs=FS10, snr_db=(-14.0, -8.0), f0_range=(300.0, 2500.0), seeds=[7300])
    hop, binw = NSPS10 // SPS10, FS10 / NFFT10
    cand = []
    for k in range(2):
        cand += _grid9(*nearest(t[0], k, FS10, hop, binw))
    cand = np.array(cand, dtype=np.int32)
    slot_of = np.zeros(len(cand), dtype=np.int32)
    x = x.numpy().astype(np.float32)
    ref = coherent.coherent_restate(x, cand, slot_of, FS10, NSPS10, NFFT10, SPS10, details=True)
    for v in (x, cand, slot_of):
        v.setflags(write=False)
    return {"x": x, "cand": cand, "slot_of": slot_of, "f32": ref}
