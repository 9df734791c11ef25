"""The signal report on the device (csrc/snr.hip: k_noise_floor, k_snr; ft8_noise_floor, ft8_snr,
ft8_snr_last) against the NumPy restatement snr_reference on the same waterfall, and the Python
surface on top of it (SlotDecoder.snr / reports, from_wave --snr)."""
import os
import re

import numpy as np
import pytest

from conftest import DATA

pytestmark = pytest.mark.gpu

FS, BPT, SPS = 12000, 2, 2
N_SLOTS, CAP = 3, 5
COUNTS = (0, 2, 7)          # the last is capped at CAP


def _L():
    from ft8_demodulator_amd import _lib
    return _lib


def _random_wf(torch, seed, T, F, f64, n_slots=N_SLOTS):
    rng = np.random.default_rng(seed)
    wf = rng.normal(-50.0, 10.0, size=(n_slots, T, F)).astype(np.float64 if f64 else np.float32)
    return wf, torch.from_numpy(wf).cuda()


def _random_records(seed, T, F, n_slots=N_SLOTS, cap=CAP, bpt=BPT, sps=SPS):
    """Random payloads; abs_time from -20 to T + 5 with both ends present, abs_freq over every
    admissible tone-0 bin with both edges present (F = 15: only 0); record [2, 1] is not ok.  Records
    [0, 0] and [2, 3] put symbol 78's row at T (in range only at dt = -1), records at the last admissible
    bin put tone 7's bin at F - 1 (df = +1 is skipped): both straddles occur at every (bpt, sps)."""
    _lib = _L()
    rng = np.random.default_rng(seed)
    r = np.zeros((n_slots, cap), dtype=_lib.RESULT_DTYPE)
    pay = rng.integers(0, 256, size=(n_slots, cap, 10), dtype=np.uint8)
    pay[..., 9] &= 0xF8
    r["payload"] = pay
    r["ok"] = 1
    r["ok"][2, 1] = 0
    f_max = F - 1 - 7 * bpt
    r["abs_time"] = rng.integers(-20, T + 6, size=(n_slots, cap))
    r["abs_freq"] = rng.integers(0, f_max + 1, size=(n_slots, cap))
    r["abs_time"][1, 0], r["abs_time"][1, 1], r["abs_time"][2, 0] = -20, T + 5, min(T - 1, 3)
    r["abs_freq"][1, 0], r["abs_freq"][1, 1], r["abs_freq"][2, 0], r["abs_freq"][2, 2] = 0, f_max, f_max, 0
    r["abs_time"][0, 0] = r["abs_time"][2, 3] = T - 78 * sps
    r["slot"] = np.arange(n_slots)[:, None]
    ok = r["ok"] != 0
    last_row, top_bin = r["abs_time"] + 78 * sps, r["abs_freq"] + 7 * bpt
    assert (ok & (last_row - 1 < T) & (last_row + 1 >= T) & (last_row - 1 >= 0)).any()      # straddles T
    assert (ok & (top_bin - 1 <= F - 1) & (top_bin + 1 > F - 1)).any()                       # straddles F - 1
    return r


def _noise_floor(torch, d_wf, q, ctx=None):
    """ft8_noise_floor with both outputs pre-filled with -1: a value the kernel leaves unwritten shows."""
    _lib = _L()
    n_slots, T, F = d_wf.shape
    ctx = ctx or _lib.context(0)
    d_n0 = torch.full((n_slots,), -1.0, dtype=torch.float64, device="cuda")
    d_A = torch.full((n_slots, F), -1.0, dtype=torch.float64, device="cuda")
    rc = _lib.lib().ft8_noise_floor(ctx.handle, _lib.ptr(d_wf), int(d_wf.dtype == torch.float64), n_slots, T, F,
                                    float(q), _lib.ptr(d_n0), _lib.ptr(d_A), _lib.stream_handle(0))
    ctx.check(rc, "ft8_noise_floor")
    torch.cuda.synchronize()
    return d_n0, d_A


def _params(n_samples=180000, bpt=BPT, sps=SPS):
    from ft8_demodulator_amd._pipeline import make_params, make_plan
    plan = make_plan(n_samples, FS, bpt, sps)
    return plan, make_params(plan, 20, 10, 20)


def _snr(torch, d_wf, recs, counts, d_n0, radius=1, ctx=None, bpt=BPT, sps=SPS):
    """ft8_snr -> ft8_snr_rec [n_slots, cap]; the output starts as 0xA5 bytes."""
    import ctypes
    _lib = _L()
    n_slots, T, F = d_wf.shape
    cap = recs.shape[1]
    ctx = ctx or _lib.context(0)
    d_rec = torch.from_numpy(recs.reshape(-1).view(np.uint8).copy()).cuda()
    d_cnt = None if counts is None else torch.as_tensor(np.asarray(counts, dtype=np.int32)).cuda()
    d_out = torch.full((n_slots * cap * 24,), 0xA5, dtype=torch.uint8, device="cuda")
    _, p = _params(bpt=bpt, sps=sps)
    assert (p.bins_per_tone, p.steps_per_symbol) == (bpt, sps)
    rc = _lib.lib().ft8_snr(ctx.handle, _lib.ptr(d_wf), int(d_wf.dtype == torch.float64), n_slots, T, F,
                            ctypes.byref(p), 180000, _lib.ptr(d_rec), None if d_cnt is None else _lib.ptr(d_cnt), cap,
                            _lib.ptr(d_n0), radius, _lib.ptr(d_out), _lib.stream_handle(0))
    ctx.check(rc, "ft8_snr")
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(_lib.SNR_DTYPE).reshape(n_slots, cap)


def _check_reports(got, want, info):
    """Device reports against the restatement's, with the tolerances of the feature's specification."""
    assert np.array_equal(got["status"], want["status"])
    assert np.array_equal(got["n_symbols"], want["n_symbols"])
    np.testing.assert_allclose(got["snr_db"], want["snr_db"], rtol=0, atol=1e-6, equal_nan=True)
    np.testing.assert_allclose(got["signal_db"], want["signal_db"], rtol=0, atol=1e-4, equal_nan=True)
    np.testing.assert_allclose(got["noise_db"], want["noise_db"], rtol=0, atol=1e-4, equal_nan=True)
    assert not got["reserved"].any()
    for s in range(got.shape[0]):
        for r in range(got.shape[1]):
            if want["status"][s, r] >= 2:      # zeros but for the status
                assert got[s, r].tobytes() == want[s, r].tobytes(), (s, r)
                continue
            m = sorted((c[2] for c in info[s][r]), reverse=True)
            if len(m) < 2 or m[0] - m[1] > 1e-9 * abs(m[0]):
                assert (got["dt"][s, r], got["df"][s, r]) == (want["dt"][s, r], want["df"][s, r]), (s, r)


# ---- the two kernels against the restatement ----------------------------------------------------------
def _kernels_equal_restatement(gpu, T, F, f64, bpt=BPT, sps=SPS):
    from ft8_demodulator_amd.snr import noise_floor_reference, snr_reference
    seed = 1000 * T + F + int(f64) + (0 if (bpt, sps) == (BPT, SPS) else 100000 * (10 * bpt + sps))
    wf, d_wf = _random_wf(gpu, seed, T, F, f64)
    n0_ref, A_ref = noise_floor_reference(wf, 0.25)
    d_n0, d_A = _noise_floor(gpu, d_wf, 0.25)
    np.testing.assert_allclose(d_A.cpu().numpy(), A_ref, rtol=1e-12, atol=0)
    np.testing.assert_allclose(d_n0.cpu().numpy(), n0_ref, rtol=1e-12, atol=0)
    recs = _random_records(seed, T, F, bpt=bpt, sps=sps)
    for counts in (COUNTS, None):
        want, info = snr_reference(wf, recs, counts, FS, bpt, sps, q=0.25, radius=1, details=True)
        got = _snr(gpu, d_wf, recs, counts, d_n0, bpt=bpt, sps=sps)
        _check_reports(got, want, info)
    live = want["status"] < 2
    print(f"T={T} F={F} bpt={bpt} sps={sps}: max |snr_db - restatement| = "
          f"{np.nanmax(np.abs(got['snr_db'][live] - want['snr_db'][live])) if live.any() else 0:.3g} dB, "
          f"max rel colmean error = {np.max(np.abs(d_A.cpu().numpy() / A_ref - 1)):.3g}")
    if T >= 7 and F > 15:
        assert (want["status"] == 0).any()
    # radius 0: the record's own grid point
    want0, info0 = snr_reference(wf, recs, COUNTS, FS, bpt, sps, q=0.25, radius=0, details=True)
    got0 = _snr(gpu, d_wf, recs, COUNTS, d_n0, radius=0, bpt=bpt, sps=sps)
    _check_reports(got0, want0, info0)
    assert not got0["dt"].any() and not got0["df"].any()


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("F", [15, 63, 65, 1920, 3840])
@pytest.mark.parametrize("T", [1, 7, 100])
def test_kernels_equal_restatement(gpu, T, F, f64):
    _kernels_equal_restatement(gpu, T, F, f64)


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("F", [65, 1920])
@pytest.mark.parametrize("T", [7, 100])
@pytest.mark.parametrize("bpt,sps", [(3, 2), (1, 2), (2, 1), (2, 4), (5, 5)])
def test_kernels_equal_restatement_other_factors(gpu, bpt, sps, T, F, f64):
    """bins_per_tone != steps_per_symbol (a transposed pair between ft8_params and launch_snr reads other
    rows and bins: tests/test_baseband_geometry_cases.py) and a pair the decode chain does not use."""
    _kernels_equal_restatement(gpu, T, F, f64, bpt, sps)


def test_counts_ok_and_status(gpu):
    from ft8_demodulator_amd.snr import snr_reference
    T, F = 100, 65
    wf, d_wf = _random_wf(gpu, 5, T, F, False)
    recs = _random_records(5, T, F)
    d_n0, _ = _noise_floor(gpu, d_wf, 0.25)
    got = _snr(gpu, d_wf, recs, COUNTS, d_n0)
    assert (got["status"][0] == 3).all() and (got["status"][1, 2:] == 3).all() and got["status"][2, 1] == 3
    blank = np.zeros((), dtype=got.dtype)
    blank["status"] = 3
    assert all(g.tobytes() == blank.tobytes() for g in got.reshape(-1)[got.reshape(-1)["status"] == 3])
    assert got["status"][1, 1] == 2                 # abs_time = T + 5: every row out of range
    assert got["status"][1, 0] < 2 and got["n_symbols"][1, 0] == 50           # abs_time = -20: symbols 10 .. 59
    want = snr_reference(wf, recs, COUNTS, FS, BPT, SPS)
    assert np.array_equal(got["n_symbols"], want["n_symbols"])
    # negative counts read as 0
    got = _snr(gpu, d_wf, recs, [-4, 5, 1], d_n0)
    assert (got["status"][0] == 3).all() and (got["status"][2, 1:] == 3).all() and got["status"][2, 0] < 2


# ---- the quantile ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [0.0, 0.25, 1.0])
@pytest.mark.parametrize("F", [65, 1920, 2048, 2049, 8192, 8193])
def test_quantile_ranks_ties_and_nan(gpu, q, F):
    """Ranks 0, floor((F - 1) / 4) and F - 1; waterfalls quantised to a few levels with T = 1, so
    nearly every column has exact equals; a NaN column orders after every number.  Up to F = 8192 the
    keys are sorted in LDS, padded to a power of two (2048: no padding, 2049: nearly half of it);
    8193 counts ranks on the means read back from memory, where the index tie-break decides which
    lane reports, and exactly one must."""
    from ft8_demodulator_amd.snr import noise_floor_reference
    rng = np.random.default_rng(F)
    wf = np.round(rng.normal(-50.0, 3.0, size=(3, 1, F))).astype(np.float32)
    wf[1, 0, 7] = wf[1, 0, 40]                       # two exactly equal columns, whatever the rounding did
    wf[2, 0, F // 2] = np.nan
    d_n0, d_A = _noise_floor(gpu, gpu.from_numpy(wf).cuda(), q)
    n0_ref, A_ref = noise_floor_reference(wf, q)
    np.testing.assert_allclose(d_A.cpu().numpy(), A_ref, rtol=1e-12, atol=0, equal_nan=True)
    np.testing.assert_allclose(d_n0.cpu().numpy(), n0_ref, rtol=1e-12, atol=0, equal_nan=True)
    assert np.isnan(n0_ref[2]) == (q == 1.0) and not np.isnan(n0_ref[:2]).any()
    # continuous values, T = 7: the rank picks exactly the restatement's column
    wf, d_wf = _random_wf(gpu, F + 1, 7, F, True)
    d_n0, d_A = _noise_floor(gpu, d_wf, q)
    n0_ref, A_ref = noise_floor_reference(wf, q)
    A = d_A.cpu().numpy()
    np.testing.assert_allclose(A, A_ref, rtol=1e-12, atol=0)
    assert np.array_equal(d_n0.cpu().numpy(), np.sort(A, axis=1)[:, int(np.floor(q * (F - 1)))])


def test_nan_slot_between_clean_ones(gpu):
    """Slot 1 all NaN: the neighbours' results do not change; its N0 is NaN and every offset's mean
    is NaN, so (as in the restatement) its records get status 2.  Slot 1 NaN only where no record
    reads: a NaN floor under finite means gives status 0 and a NaN report."""
    from ft8_demodulator_amd.snr import snr_reference
    T, F = 100, 129
    wf, d_wf = _random_wf(gpu, 77, T, F, False)
    recs = _random_records(77, T, F)
    recs["abs_time"] = np.minimum(recs["abs_time"], T - 1)       # every record has rows in range
    recs["abs_time"][1], recs["abs_freq"][1] = [0, 1, 2, 3, 4], [111, 112, 113, 112, 111]
    recs["ok"][2, 1] = 1
    d_n0, _ = _noise_floor(gpu, d_wf, 0.25)
    clean = _snr(gpu, d_wf, recs, None, d_n0)
    assert (clean["status"] < 2).all()

    wf_nan = wf.copy()
    wf_nan[1] = np.nan
    d_nan = gpu.from_numpy(wf_nan).cuda()
    d_n0b, d_Ab = _noise_floor(gpu, d_nan, 0.25)
    n0b = d_n0b.cpu().numpy()
    assert np.isnan(n0b[1]) and np.isnan(d_Ab.cpu().numpy()[1]).all()
    assert np.array_equal(n0b[[0, 2]], d_n0.cpu().numpy()[[0, 2]])
    got = _snr(gpu, d_nan, recs, None, d_n0b)
    assert got[[0, 2]].tobytes() == clean[[0, 2]].tobytes()
    want = snr_reference(wf_nan, recs, None, FS, BPT, SPS)
    assert (got["status"][1] == 2).all() and np.array_equal(got["status"], want["status"])

    wf_part = wf.copy()
    wf_part[1, :, :110] = np.nan                     # the bins the records read, 110 .. 128, stay finite;
                                                     # rank floor(128 / 4) = 32 of A is a NaN
    d_part = gpu.from_numpy(wf_part).cuda()
    d_n0c, _ = _noise_floor(gpu, d_part, 0.25)
    assert np.isnan(d_n0c.cpu().numpy()[1])
    got = _snr(gpu, d_part, recs, None, d_n0c)
    want = snr_reference(wf_part, recs, None, FS, BPT, SPS)
    assert got[[0, 2]].tobytes() == clean[[0, 2]].tobytes()
    assert (got["status"][1] == 0).all() and np.isnan(got["snr_db"][1]).all() and np.isnan(got["noise_db"][1]).all()
    assert np.array_equal(got["status"], want["status"]) and np.array_equal(got["n_symbols"], want["n_symbols"])
    assert np.array_equal(got["dt"], want["dt"]) and np.array_equal(got["df"], want["df"])


def test_wrappers_and_arguments(gpu):
    import ctypes
    from ft8_demodulator_amd import snr as S
    _lib = _L()
    wf, d_wf = _random_wf(gpu, 9, 7, 63, True)
    recs = _random_records(9, 7, 63)
    n0, A = S.noise_floor(d_wf, 0.25)
    n0_ref, A_ref = S.noise_floor_reference(wf, 0.25)
    np.testing.assert_allclose(A.cpu().numpy(), A_ref, rtol=1e-12)
    np.testing.assert_allclose(n0.cpu().numpy(), n0_ref, rtol=1e-12)
    got = S.snr(d_wf, recs, COUNTS, sample_rate=FS)
    want, info = S.snr_reference(wf, recs, COUNTS, FS, details=True)
    _check_reports(got, want, info)
    with pytest.raises(TypeError):
        S.noise_floor(wf)

    ctx, L, sh = _lib.context(0), _lib.lib(), _lib.stream_handle(0)
    _, p = _params()
    buf = gpu.zeros(4096, dtype=gpu.float64, device="cuda")
    b = _lib.ptr(buf)
    nf = lambda *a: L.ft8_noise_floor(ctx.handle, *a, sh)                                 # noqa: E731
    assert nf(None, 0, 0, 7, 63, 0.25, None, None) == _lib.FT8_OK                        # nothing to do
    assert nf(b, 0, 1, 7, 63, 1.5, b, b) == _lib.FT8_E_ARG
    assert nf(b, 0, 1, 7, 63, float("nan"), b, b) == _lib.FT8_E_ARG
    assert nf(b, 0, 1, 0, 63, 0.25, b, b) == _lib.FT8_E_ARG
    assert nf(b, 0, 1, 7, 0, 0.25, b, b) == _lib.FT8_E_ARG
    assert nf(b, 0, 1, 7, 63, 0.25, b, None) == _lib.FT8_E_ARG                           # colmean is required
    assert nf(b, 0, -1, 7, 63, 0.25, b, b) == _lib.FT8_E_ARG
    assert L.ft8_noise_floor(None, b, 0, 1, 7, 63, 0.25, b, b, sh) == _lib.FT8_E_ARG
    sn = lambda *a: L.ft8_snr(ctx.handle, *a, sh)                                        # noqa: E731
    pp = ctypes.byref(p)
    assert sn(None, 0, 0, 7, 63, pp, 180000, None, None, 5, None, 1, None) == _lib.FT8_OK
    assert sn(b, 0, 1, 7, 63, pp, 180000, b, None, 0, b, 1, b) == _lib.FT8_OK
    assert sn(b, 0, 1, 7, 63, pp, 180000, b, None, 1, b, 2, b) == _lib.FT8_E_ARG         # radius
    assert sn(b, 0, 1, 7, 63, pp, 180000, b, None, 1, None, 1, b) == _lib.FT8_E_ARG      # no floor
    assert sn(b, 0, 1, 7, 63, pp, 180000, None, None, 1, b, 1, b) == _lib.FT8_E_ARG
    assert sn(b, 0, 1, 0, 63, pp, 180000, b, None, 1, b, 1, b) == _lib.FT8_E_ARG
    assert sn(b, 0, 1, 7, 63, None, 180000, b, None, 1, b, 1, b) == _lib.FT8_E_ARG
    gpu.cuda.synchronize()


# ---- ft8_snr_last -----------------------------------------------------------------------------------------
K = 20


@pytest.fixture(scope="module")
def decoded(gpu):
    """Two one-signal slots, their truth, and a TOPK decoder factory (the K highest sync scores: the
    signal's own grid points come first)."""
    from ft8_demodulator_amd import SlotDecoder, synth
    _lib = _L()
    x, truth = synth.make_slots(2, 1, fs=FS, snr_db=(-10.0, 0.0), seed=31, device="cpu")
    x = x.cuda()

    def decoder(flags=0, ctx=None):
        return SlotDecoder(FS, BPT, SPS, max_candidates=K, flags=_lib.FT8_FLAG_TOPK | flags,
                           context=ctx if ctx is not None else _lib.Context(0))
    return x, truth, decoder


def _snr_last(gpu, dec, out, counts, n_slots=None, cap=None):
    _lib = _L()
    n_slots = int(counts.shape[0]) if n_slots is None else n_slots
    cap = dec.cap if cap is None else cap
    d_out = gpu.full((max(n_slots * cap, 1) * 24,), 0xA5, dtype=gpu.uint8, device="cuda")
    rc = _lib.lib().ft8_snr_last(dec.ctx.handle, _lib.ptr(out), _lib.ptr(counts), n_slots, cap, _lib.ptr(d_out),
                                 _lib.stream_handle(0))
    return rc, d_out


def _stage_reports(gpu, dec, x, out, counts):
    """ft8_stft into a tensor, then ft8_noise_floor (q 0.25) and ft8_snr (radius 1) on it, on a
    context of their own."""
    import ctypes
    from ft8_demodulator_amd._pipeline import make_params
    _lib = _L()
    ctx = _lib.Context(0)
    n_slots, n = x.shape
    plan = dec.plan(n)
    p = make_params(plan, dec.max_candidates, dec.min_score, dec.max_iterations, dec.flags)
    d_wf = gpu.empty((n_slots, plan.T, plan.F), dtype=gpu.float32, device="cuda")
    rc = _lib.lib().ft8_stft(ctx.handle, _lib.ptr(x), _lib.FT8_F32, n, n_slots, n, ctypes.byref(p), _lib.ptr(d_wf),
                             _lib.stream_handle(0))
    ctx.check(rc, "ft8_stft")
    d_n0, _ = _noise_floor(gpu, d_wf, 0.25, ctx)
    d_out = gpu.full((n_slots * dec.cap * 24,), 0xA5, dtype=gpu.uint8, device="cuda")
    rc = _lib.lib().ft8_snr(ctx.handle, _lib.ptr(d_wf), 0, n_slots, plan.T, plan.F, ctypes.byref(p), n, _lib.ptr(out),
                            _lib.ptr(counts), dec.cap, _lib.ptr(d_n0), 1, _lib.ptr(d_out), _lib.stream_handle(0))
    ctx.check(rc, "ft8_snr")
    gpu.cuda.synchronize()
    return d_out


@pytest.mark.parametrize("pipeline", [None, (1, 2, 4)], ids=["one-chain", "chunked"])
def test_snr_last_equals_stage_calls_and_truth(gpu, decoded, pipeline):
    _lib = _L()
    x, truth, decoder = decoded
    dec = decoder()
    if pipeline:
        dec.ctx.set_pipeline(*pipeline)
    out, counts = dec.run(x)
    rc, d_last = _snr_last(gpu, dec, out, counts)
    dec.ctx.check(rc, "ft8_snr_last")
    gpu.cuda.synchronize()
    d_stage = _stage_reports(gpu, dec, x, out, counts)
    assert d_last.cpu().numpy().tobytes() == d_stage.cpu().numpy().tobytes()          # bit for bit
    reps = d_last.cpu().numpy().view(_lib.SNR_DTYPE).reshape(2, dec.cap)
    recs = out[: 2 * dec.cap * 40].cpu().numpy().view(_lib.RESULT_DTYPE).reshape(2, dec.cap)
    c = counts.cpu().numpy()
    for s in range(2):
        n = min(int(c[s]), dec.cap)
        assert n >= 1 and (reps["status"][s, :n] < 2).all() and (reps["status"][s, n:] == 3).all()
        want = truth[s].snr_db[0] + 10.0 * np.log10(FS / 2 / 2500.0)
        mine = [r for r in range(n) if bytes(recs[s, r]["payload"]) == truth[s].payloads[0]]
        print(f"slot {s}: truth {want:.2f} dB in 2500 Hz; decodes of it (score order):",
              [(round(float(reps['snr_db'][s, r]), 2), int(reps['dt'][s, r]), int(reps['df'][s, r])) for r in mine])
        assert mine, "the slot's signal was not decoded"
        assert abs(reps["snr_db"][s, mine[0]] - want) <= 1.0          # the decode with the highest sync score


def test_snr_last_state(gpu, decoded):
    """FT8_E_ARG before any batch, after an intervening ft8_bp and for another shape;
    FT8_E_UNSUPPORTED after a subtract batch; valid again after the next plain batch."""
    _lib = _L()
    x, _, decoder = decoded
    dec = decoder()
    out, counts = dec._buffers(2)
    counts.zero_()
    assert _snr_last(gpu, dec, out, counts, 2)[0] == _lib.FT8_E_ARG
    assert _snr_last(gpu, dec, out, counts, 0)[0] == _lib.FT8_OK                      # nothing to do
    out, counts = dec.run(x)
    assert _snr_last(gpu, dec, out, counts)[0] == _lib.FT8_OK
    assert _snr_last(gpu, dec, out, counts)[0] == _lib.FT8_OK                         # it does not invalidate itself
    assert _snr_last(gpu, dec, out, counts, cap=dec.cap + 1)[0] == _lib.FT8_E_ARG
    assert _snr_last(gpu, dec, out, counts, n_slots=1)[0] == _lib.FT8_E_ARG
    assert b"differ" in _lib.lib().ft8_last_error(dec.ctx.handle)
    assert _snr_last(gpu, dec, out, counts)[0] == _lib.FT8_OK
    llr = gpu.zeros((1, 174), dtype=gpu.float64, device="cuda")
    rc = _lib.lib().ft8_bp(dec.ctx.handle, _lib.ptr(llr), 1, 5, None, None, _lib.stream_handle(0))
    dec.ctx.check(rc, "ft8_bp")
    assert _snr_last(gpu, dec, out, counts)[0] == _lib.FT8_E_ARG
    out, counts = dec.run(x)
    assert _snr_last(gpu, dec, out, counts)[0] == _lib.FT8_OK
    gpu.cuda.synchronize()

    sub = decoder(_lib.FT8_FLAG_SUBTRACT, dec.ctx)
    out, counts = sub.run(x)
    assert _snr_last(gpu, sub, out, counts)[0] == _lib.FT8_E_UNSUPPORTED
    with pytest.raises(NotImplementedError, match="FT8_FLAG_SUBTRACT"):
        sub.snr(x)
    with pytest.raises(NotImplementedError, match="FT8_FLAG_SUBTRACT"):
        sub.reports(x)
    gpu.cuda.synchronize()


# ---- the Python layer ---------------------------------------------------------------------------------------
SLOT_TEXTS = [["CQ K1ABC FN42", "K1ABC W9XYZ -12"], ["W9XYZ K1ABC R-09"]]


@pytest.fixture(scope="module")
def text_slots(gpu):
    """Two 12 kHz slots of unit-variance noise carrying SLOT_TEXTS at 600 / 1500 Hz, each signal 5 dB
    below the noise in the sampled band."""
    from ft8_demodulator_amd import ft8_generator as G
    from ft8_demodulator_amd import pack77
    _lib = _L()
    N = 180000
    pays = [pack77(t) for slot in SLOT_TEXTS for t in slot]
    _, _, tones = G.encode_batch(np.frombuffer(b"".join(pays), dtype=np.uint8).reshape(-1, 10))
    sig = np.zeros(len(pays), dtype=_lib.TX_SIGNAL_DTYPE)
    sig["slot"] = [s for s, slot in enumerate(SLOT_TEXTS) for _ in slot]
    sig["f0"] = [600.0 + 900.0 * k for slot in SLOT_TEXTS for k in range(len(slot))]
    sig["amplitude"], sig["start"] = float(np.sqrt(2.0 * 10.0 ** -0.5)), 5760
    g = gpu.Generator(device="cuda")
    g.manual_seed(12)
    x = gpu.randn((2, N), generator=g, device="cuda", dtype=gpu.float32)
    G.synthesize(tones, sig, 2, N, FS, out=x)
    return x


def test_reports_are_messages_with_snr(gpu, decoded, text_slots):
    _, _, decoder = decoded
    x = text_slots
    dec = decoder()
    for unique in (True, False):
        msgs, reps = dec.messages(x, unique=unique), dec.reports(x, unique=unique)
        assert [len(m) for m in msgs] == [len(r) for r in reps] and all(len(m) >= 1 for m in msgs)
        for m_rows, r_rows in zip(msgs, reps):
            for m, r in zip(m_rows, r_rows):
                assert len(r) == 6 and isinstance(r[1], float)
                assert (r[0], r[2], r[3], r[4]) == (m[0], m[1], m[2], m[3]) and r[5].tobytes() == m[4].tobytes()
    recs, snr = dec.records(x), dec.snr(x)
    every = dec.reports(x, unique=False)
    for s in range(2):
        assert len(snr[s]) == len(recs[s]) == len(every[s]) and snr[s].dtype == _L().SNR_DTYPE
        assert [r[1] for r in every[s]] == [float(v) for v in snr[s]["snr_db"]]
        assert sorted({r[0] for r in every[s]}) == sorted(SLOT_TEXTS[s])
    # an empty plan (input shorter than one symbol) decodes nothing and reports nothing
    short = gpu.zeros((2, 100), dtype=gpu.float32, device="cuda")
    assert dec.reports(short) == [[], []] and [len(v) for v in dec.snr(short)] == [0, 0]


@pytest.mark.parametrize("method", ["records", "decode", "texts", "snr", "messages", "reports"])
def test_every_surface_decodes_once(gpu, decoded, text_slots, method):
    """Each public call is one ft8_decode_batch, whatever side outputs it fetches."""
    _, _, decoder = decoded
    dec = decoder()                      # on a context of its own
    dec.ctx.set_timing(True, stages=["decode_batch"])
    try:
        dec.timing(reset=True)
        got = getattr(dec, method)(text_slots)
        assert dec.timing()["decode_batch"][1] == 1
        assert len(got) == 2 and all(len(v) >= 1 for v in got)
    finally:
        dec.ctx.set_timing(False)


def test_from_wave_snr_flag(gpu, capsys):
    from ft8_demodulator_amd.from_wave import _print_results, decode_ft8_from_wave, main
    wav = os.path.join(DATA, "synth_cfg1.wav")
    res_plain = main([wav])
    plain = capsys.readouterr().out
    _print_results(decode_ft8_from_wave(wav))
    assert plain == capsys.readouterr().out          # without the flag: the output as it always was
    res = main([wav, "--snr"])
    with_snr = capsys.readouterr().out
    lines = with_snr.splitlines()
    extra = [ln for ln in lines if ln.startswith("SNR: ")]
    assert len(res) == len(res_plain) >= 1 and len(extra) == len(res)
    assert all(re.fullmatch(r"SNR: -?\d+\.\d dB", ln) for ln in extra), extra
    assert [ln for ln in lines if not ln.startswith("SNR: ")] == plain.splitlines()
    assert all(lines[i - 1].startswith("Score: ") for i, ln in enumerate(lines) if ln.startswith("SNR: "))
    assert [(bytes(m.payload), t, f, float(sc)) for m, _, t, f, sc in res] == \
           [(bytes(m.payload), t, f, float(sc)) for m, _, t, f, sc in res_plain]
