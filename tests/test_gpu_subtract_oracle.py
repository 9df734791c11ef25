"""Subtract-and-redecode pass 2 (FT8_FLAG_SUBTRACT, build-defined) pinned against its CPU
restatement, oracle/subtract.py (float64 NumPy), on crowded slots (BASELINE config 4's shape):

* pass 1 (top-k selection, K = 300) on the GPU; the oracle's own top-k decode of the same slots
  yields the same payload set;
* ft8_subtract on those records: every fit the device made (ft8_subtract_fits) equals the oracle's
  fit of the same record -- the same (start, tone-0) hypothesis of the search grid, start within
  +-1 sample, tone-0 frequency within 1e-3 Hz, the per-symbol amplitudes within 2e-3 of the largest
  where the starts agree -- and the device residual equals the oracle's residual to -40 dB of the
  subtracted energy;
* pass 2: the GPU decode of the device residual and the oracle decode of the oracle residual give
  the same new payloads (exactly), and the one-call FT8_FLAG_SUBTRACT batch reports those.

Tolerances: the device computes the fit in float32 (decimation, hypothesis metric by sliding
updates, amplitude sums) and the oracle in float64, so the fits agree to float32 rounding, except
where the parabolic refinement puts (dt + ddt) D within rounding of a half sample (start +-1)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_SLOTS, SIGNALS, SEED = 6, 50, 777
K, MIN_SCORE, ITERS = 300, 2, 20
SEED_3x2, SNR_3x2 = 780, (-24.0, -10.0)      # the batch at (3, 2): see its test


def test_subtract_pass2_matches_oracle(gpu, oracle):
    import torch
    from ft8_demodulator_amd import SlotDecoder, _lib, synth
    from ft8_demodulator_amd._pipeline import make_params
    from oracle import subtract as OS

    x, truths = synth.make_slots(N_SLOTS, SIGNALS, seed=SEED, device="cuda")
    n = x.shape[1]
    dec = SlotDecoder(12000, 2, 2, K, MIN_SCORE, ITERS, flags=_lib.FT8_FLAG_TOPK)
    out, counts = dec.run(x)
    recs = dec.records(x)
    plan = dec.plan(n)
    p = make_params(plan, K, MIN_SCORE, ITERS, _lib.FT8_FLAG_TOPK)
    ctx = dec.ctx
    L, st = _lib.lib(), _lib.stream_handle()
    resid = torch.empty_like(x)
    ctx.check(L.ft8_subtract(ctx.handle, _lib.ptr(x), _lib.FT8_F32, _lib.ptr(resid), n, N_SLOTS, n, ctypes.byref(p),
                             _lib.ptr(out), _lib.ptr(counts), dec.cap, st), "ft8_subtract")
    fits_d = torch.empty(N_SLOTS * dec.cap * _lib.SUB_FIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    ctx.check(L.ft8_subtract_fits(ctx.handle, _lib.ptr(fits_d), N_SLOTS, dec.cap, st), "ft8_subtract_fits")
    torch.cuda.synchronize()
    gfit = fits_d.cpu().numpy().view(_lib.SUB_FIT_DTYPE).reshape(N_SLOTS, dec.cap)
    xs = x.cpu().numpy()
    gres = resid.cpu().numpy()
    recs2 = SlotDecoder(12000, 2, 2, K, MIN_SCORE, ITERS, flags=_lib.FT8_FLAG_TOPK).records(resid)
    one = SlotDecoder(12000, 2, 2, K, MIN_SCORE, ITERS, flags=_lib.FT8_FLAG_TOPK | _lib.FT8_FLAG_SUBTRACT)
    one_call = one.records(x)
    # the one-call batch's raw output: every row of the buffer and the counts as k_merge wrote them
    out_m, counts_m = one.run(x)
    torch.cuda.synchronize()
    counts_m = counts_m.cpu().numpy()
    raw_m = out_m[:N_SLOTS * one.cap * _lib.RESULT_DTYPE.itemsize].cpu().numpy().view(_lib.RESULT_DTYPE)
    raw_m = raw_m.reshape(N_SLOTS, one.cap)

    n_fits = n_start_off = n_new = 0
    for s in range(N_SLOTS):
        r1 = recs[s]
        p1 = {bytes(r["payload"]) for r in r1}
        o1 = {pay for pay, _, _ in OS.decode_topk(xs[s], 12000, K, MIN_SCORE, ITERS)}
        assert p1 == o1, s                                           # pass 1: same payload set
        ofit = OS.fits(xs[s], r1, 12000, plan.nperseg, plan.hop, plan.nfft, plan.t_lo, plan.f_lo)
        for j, of in enumerate(ofit):
            g = gfit[s, j]
            assert int(g["active"]) == (of is not None), (s, j)
            if of is None:
                continue
            n_fits += 1
            D = plan.nperseg // OS.sub_q(plan.nperseg)
            assert abs(int(g["start"]) - of["start"]) <= 1, (s, j, int(g["start"]), of["start"])
            assert abs(float(g["f0"]) - of["f0"]) <= 1e-3, (s, j, float(g["f0"]), of["f0"])
            assert list(g["tones"][:79]) == list(of["tones"])
            if int(g["start"]) == of["start"]:
                ga = g["amp"][:, 0] + 1j * g["amp"][:, 1]
                assert np.max(np.abs(ga - of["amp"])) <= 2e-3 * np.max(np.abs(of["amp"])), (s, j)
            else:
                n_start_off += 1
            assert D > 0
        ores = OS.residual(xs[s], ofit, plan.nperseg, 12000)
        sub = np.sum((xs[s].astype(np.float64) - ores) ** 2)
        err = np.sum((gres[s].astype(np.float64) - ores) ** 2)
        assert err <= 1e-4 * sub, (s, err / sub)                     # residuals agree to -40 dB
        # pass 2: the new payloads decoded from the residual
        new_g = {bytes(r["payload"]) for r in recs2[s]} - p1
        new_o = {pay for pay, _, _ in OS.decode_topk(ores.astype(np.float32), 12000, K, MIN_SCORE, ITERS)} - o1
        assert new_g == new_o, s
        assert {bytes(r["payload"]) for r in one_call[s] if r["pass_index"] == 1} == new_g, s
        # the merge, row for row (oracle/subtract.py merge): the pass-1 rows byte for byte, then the ok
        # pass-2 rows decoded from the device residual whose payload no pass-1 row carries, in pass-2
        # order, byte for byte but for pass_index 1; the count is that of both
        want = OS.merge(r1, recs2[s])
        c1 = len(r1)
        assert c1 > 0 and np.all(r1["pass_index"] == 0) and np.all(recs2[s]["pass_index"] == 0)
        assert int(counts_m[s]) == len(want) <= one.cap, (s, int(counts_m[s]), len(want))
        got = raw_m[s, :len(want)]
        assert got[:c1].tobytes() == r1.tobytes(), s
        assert list(got[c1:]["pass_index"]) == [1] * (len(want) - c1), s
        assert got[c1:].tobytes() == want[c1:].tobytes(), s
        assert len(one_call[s]) == len(want) and one_call[s].tobytes() == want.tobytes(), s
        n_new += len(want) - c1
    assert n_fits >= 3 * N_SLOTS
    assert n_start_off <= max(1, n_fits // 20)
    assert n_new >= 1                                                 # the merge appended something
    print(f"subtract oracle: {n_fits} fits, {n_start_off} with start +-1, {n_new} rows appended by the merge")


def test_subtract_batch_at_3_bins_2_steps_matches_oracle(gpu, oracle):
    """One FT8_FLAG_SUBTRACT batch at bins_per_tone 3, steps_per_symbol 2 (nfft 5760, hop 960): two slots
    of eight signals, K = 40.  Pass 1 decodes the oracle's top-k payload set; the rows the batch appends
    carry the payloads the oracle decodes anew from its own residual of its own fits, as the six-slot test
    above states at (2, 2)."""
    from ft8_demodulator_amd import SlotDecoder, _lib, synth
    from oracle import subtract as OS
    BPT, SPS, K2 = 3, 2, 40
    x, _ = synth.make_slots(2, 8, snr_db=SNR_3x2, seed=SEED_3x2, device="cuda")
    xs = x.cpu().numpy()
    dec = SlotDecoder(12000, BPT, SPS, K2, MIN_SCORE, ITERS, flags=_lib.FT8_FLAG_TOPK)
    recs = dec.records(x)
    plan = dec.plan(x.shape[1])
    assert (plan.nperseg, plan.hop, plan.nfft) == (1920, 960, 5760)
    one_call = SlotDecoder(12000, BPT, SPS, K2, MIN_SCORE, ITERS,
                           flags=_lib.FT8_FLAG_TOPK | _lib.FT8_FLAG_SUBTRACT).records(x)
    n_new = 0
    for s in range(2):
        p1 = {bytes(r["payload"]) for r in recs[s]}
        o1 = {pay for pay, _, _ in OS.decode_topk(xs[s], 12000, K2, MIN_SCORE, ITERS, bpt=BPT, sps=SPS)}
        assert p1 == o1 and len(p1) >= 3, s
        ofit = OS.fits(xs[s], recs[s], 12000, plan.nperseg, plan.hop, plan.nfft, plan.t_lo, plan.f_lo)
        ores = OS.residual(xs[s], ofit, plan.nperseg, 12000)
        new_o = {pay for pay, _, _ in OS.decode_topk(ores.astype(np.float32), 12000, K2, MIN_SCORE, ITERS, bpt=BPT,
                                                     sps=SPS)} - o1
        assert {bytes(r["payload"]) for r in one_call[s] if r["pass_index"] == 0} == p1, s
        assert {bytes(r["payload"]) for r in one_call[s] if r["pass_index"] == 1} == new_o, s
        n_new += len(new_o)
    print(f"subtract batch at (3, 2): {n_new} payloads decoded anew from the residual")
    assert n_new >= 1


# ---- the paths of the baseband front end (csrc/baseband.h) that a crowded slot does not take ----------
# one slot each; the tolerances are the test's above

def _device_fits(x, fs, bpt, sps):
    """Top-k decode of the slots x (float32 or int16 PCM on the device) and ft8_subtract on its records
    -> (records per slot, plan, fits [n_slots, cap])."""
    import torch
    from ft8_demodulator_amd import SlotDecoder, _lib
    from ft8_demodulator_amd._pipeline import make_params

    n_slots, n = x.shape
    dec = SlotDecoder(fs, bpt, sps, 40, MIN_SCORE, ITERS, flags=_lib.FT8_FLAG_TOPK)
    out, counts = dec.run(x)
    recs = dec.records(x)
    plan = dec.plan(n)
    p = make_params(plan, 40, MIN_SCORE, ITERS, _lib.FT8_FLAG_TOPK)
    ctx, L, st = dec.ctx, _lib.lib(), _lib.stream_handle()
    code = _lib.FT8_I16 if x.dtype == torch.int16 else _lib.FT8_F32
    resid = torch.empty(x.shape, dtype=torch.float32, device="cuda")
    ctx.check(L.ft8_subtract(ctx.handle, _lib.ptr(x), code, _lib.ptr(resid), n, n_slots, n, ctypes.byref(p),
                             _lib.ptr(out), _lib.ptr(counts), dec.cap, st), "ft8_subtract")
    fits_d = torch.empty(n_slots * dec.cap * _lib.SUB_FIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    ctx.check(L.ft8_subtract_fits(ctx.handle, _lib.ptr(fits_d), n_slots, dec.cap, st), "ft8_subtract_fits")
    torch.cuda.synchronize()
    return recs, plan, fits_d.cpu().numpy().view(_lib.SUB_FIT_DTYPE).reshape(n_slots, dec.cap)


def _check_fits(gfit, ofit):
    """Every device fit of one slot against the oracle's fit of the same record -> the number compared
    (the comparison and its tolerances: subtract_cases.check_fits, shared with test_gpu_subtract_lists.py)."""
    from subtract_cases import check_fits
    return check_fits(gfit, ofit)[0]


def _window(plan, rec):
    """[first, last) input sample of the baseband k_sub_est decimates for a record."""
    from oracle import subtract as OS
    Q = OS.sub_q(plan.nperseg)
    assert Q >= 8 and plan.nperseg % Q == 0
    D, sps = plan.nperseg // Q, plan.nperseg // plan.hop
    Mg = (Q + 2 * sps - 1) // (2 * sps) + 1
    nb = (plan.t_lo + int(rec["abs_time"])) * plan.hop - Mg * D
    return nb, nb + (79 * Q + 2 * Mg) * D


EDGE_STARTS = (200, 12000, 27900)     # samples: within Mg D = 540 of the slot's head, inside, of its end
EDGE_F0 = (700.0, 1500.0, 2300.0)


def _edge_slot():
    """One 12 kHz slot of unit noise and three signals at -4 dB -> (float32 [1, 180000], payloads)."""
    import torch
    from ft8_demodulator_amd import synth
    noise, _ = synth.make_slots(1, 0, fs=12000, seeds=[8100])
    rng = np.random.default_rng(8100)
    pays = [synth.random_payload(rng) for _ in EDGE_STARTS]
    tones = torch.as_tensor(np.stack([synth.itones(p) for p in pays]))
    wav = synth.gfsk_waveforms(tones, 12000, torch.tensor(EDGE_F0, dtype=torch.float64))
    wav *= np.sqrt(2.0 * 10.0 ** (-4.0 / 10.0))
    x = noise[0].to(torch.float64)
    for i, s in enumerate(EDGE_STARTS):
        x[s:s + wav.shape[1]] += wav[i]
    return x.to(torch.float32).numpy()[None], pays


@pytest.mark.parametrize("key", ["f32", "i16"])
def test_fits_at_the_slot_edges_match_oracle(gpu, oracle, key):
    """A signal whose baseband window starts before the slot, one whose window ends past it (both take
    the range-checked loop of bb_mix_down) and one inside (the vector loads), as float32 and as int16 PCM."""
    import torch
    from oracle import subtract as OS
    x, pays = _edge_slot()
    if key == "i16":
        pcm = np.clip(np.round(x / 8.0 * 32767.0), -32767, 32767).astype(np.int16)
        xd, xs = torch.from_numpy(pcm).cuda(), pcm.astype(np.float64) / 32767.0
    else:
        xd, xs = torch.from_numpy(x).cuda(), x
    n = x.shape[1]
    recs, plan, gfit = _device_fits(xd, 12000, 2, 2)
    r = recs[0]
    assert {bytes(q["payload"]) for q in r} == set(pays)                  # all three decode
    ofit = OS.fits(xs[0], r, 12000, plan.nperseg, plan.hop, plan.nfft, plan.t_lo, plan.f_lo)
    where = {}
    for q, of in zip(r, ofit):
        if of is not None:
            lo, hi = _window(plan, q)
            where[pays.index(bytes(q["payload"]))] = (lo < 0, hi > n)
    assert where == {0: (True, False), 1: (False, False), 2: (False, True)}, where
    assert _check_fits(gfit[0], ofit) == 3


def test_fits_at_10k_match_oracle(gpu, oracle):
    """fs = 10000 at 4 bins per tone and 4 steps per symbol: nsps 1600, Q 32, D 50 -- no window of
    bb_mix_down takes the four-sample loads."""
    from ft8_demodulator_amd import synth
    from oracle import subtract as OS
    x, truth = synth.make_slots(1, 2, fs=10000, snr_db=-5.0, f0_range=(300.0, 2500.0), seeds=[8200])
    recs, plan, gfit = _device_fits(x.cuda(), 10000, 4, 4)
    assert plan.nperseg == 1600 and (plan.nperseg // 32) % 4 != 0
    r = recs[0]
    assert {bytes(q["payload"]) for q in r} == {bytes(p) for p in truth[0].payloads}
    ofit = OS.fits(x[0].numpy(), r, 10000, plan.nperseg, plan.hop, plan.nfft, plan.t_lo, plan.f_lo)
    assert _check_fits(gfit[0], ofit) == 2
