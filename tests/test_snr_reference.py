"""snr_reference, the NumPy restatement of the signal report (ft8_demodulator_amd/snr.py): against
the truth of synthetic slots, and on hand-computed waterfalls (CPU only, no library)."""
import numpy as np
import pytest

from ft8_demodulator_amd import _lib
from ft8_demodulator_amd.snr import bandwidth_db, noise_floor_reference, snr_reference

FS = 12000
BW_DB = 10.0 * np.log10(1.5 * FS / 1920 / 2500.0)   # -24.26 dB


def _records(n_slots, cap, abs_time=0, abs_freq=0, ok=1, payload=None):
    r = np.zeros((n_slots, cap), dtype=_lib.RESULT_DTYPE)
    r["abs_time"], r["abs_freq"], r["ok"] = abs_time, abs_freq, ok
    r["payload"] = np.arange(10, dtype=np.uint8) * 23 & 0xF8 if payload is None else payload
    return r


def test_bandwidth_constant():
    assert abs(bandwidth_db(FS) - BW_DB) < 1e-12 and abs(BW_DB + 24.26) < 0.005
    assert bandwidth_db(12006.3) == 10.0 * np.log10(1.5 * 12006.3 / 1921 / 2500.0)


# ---- against truth ---------------------------------------------------------------------------------------
TRUTH_SNRS = (-18.0, -10.0, 0.0, 8.0)


@pytest.fixture(scope="module")
def truth_slots():
    """Four one-signal 12 kHz slots at fixed SNRs (power over unit-variance white noise in the whole
    sampled band, synth.make_slots), their scipy waterfalls as calculate_spectrogram builds them
    (f >= 0 kept) and one record per slot at the grid point nearest the truth."""
    from oracle import oracle as O
    from ft8_demodulator_amd import synth
    wfs, recs = [], _records(4, 1)
    for s, snr in enumerate(TRUTH_SNRS):
        x, truth = synth.make_slots(1, 1, fs=FS, snr_db=snr, seeds=[100 + s])
        wfs.append(O.waterfall(x[0].numpy(), FS, 2, 2).T)       # [T, F]
        recs[s, 0]["payload"] = np.frombuffer(truth[0].payloads[0], dtype=np.uint8)
        recs[s, 0]["abs_time"] = int(round(int(truth[0].start_s[0] * FS) / 960.0))   # hop = nperseg / 2
        recs[s, 0]["abs_freq"] = int(round(truth[0].f0[0] / 3.125))                  # 6.25 Hz / bins_per_tone
    wf = np.stack(wfs)
    assert wf.shape == (4, 186, 1920) and wf.dtype == np.float32
    return wf, recs


def test_estimate_against_truth(truth_slots):
    """|estimate - truth in 2500 Hz| <= 1.0 dB at radius 1.  The truth is the power ratio in the
    sampled band fs / 2: in 2500 Hz it is 10 log10(fs / 2 / 2500) = 3.80 dB higher."""
    wf, recs = truth_slots
    got = snr_reference(wf, recs, None, FS, 2, 2, q=0.25, radius=1)
    want = np.array(TRUTH_SNRS) + 10.0 * np.log10(FS / 2 / 2500.0)
    err = got["snr_db"][:, 0] - want
    print("snr_db", got["snr_db"][:, 0], "error", err, "offsets", got["dt"][:, 0], got["df"][:, 0])
    assert (got["status"] == 0).all() and (got["n_symbols"] == 79).all()
    assert np.abs(err).max() <= 1.0
    # radius 0 measures at the record's own grid point
    got0 = snr_reference(wf, recs, None, FS, 2, 2, q=0.25, radius=0)
    err0 = got0["snr_db"][:, 0] - want
    print("radius 0 error", err0)
    assert (got0["dt"] == 0).all() and (got0["df"] == 0).all()
    assert (got0["snr_db"] <= got["snr_db"]).all() and np.abs(err0).max() <= 1.0


# ---- hand-computed ------------------------------------------------------------------------------------------
def test_noise_floor_quantile():
    row = np.array([20.0, 0.0, np.nan, 30.0, 10.0])
    wf = np.stack([np.stack([row, row]), np.stack([row + 10.0, row + 10.0])])          # [2, 2, 5]
    for q, want in [(0.0, 1.0), (0.25, 10.0), (0.74, 100.0), (0.75, 1000.0)]:
        n0, A = noise_floor_reference(wf, q)
        assert np.allclose(n0, [want, 10.0 * want], rtol=1e-15), q
    n0, A = noise_floor_reference(wf, 1.0)
    assert np.isnan(n0).all()                                                           # NaNs order last
    assert np.allclose(A[0, [0, 1, 3, 4]], [100.0, 1.0, 1000.0, 10.0], rtol=1e-15) and np.isnan(A[:, 2]).all()
    # the mean is taken over time, in linear power
    wf2 = np.array([[[0.0], [10.0], [20.0]]])
    assert np.allclose(noise_floor_reference(wf2, 0.5)[1], [[37.0]], rtol=1e-15)


def test_constant_waterfall_clamps():
    """Every column ties, M = N0 at every offset: S is raised to 1e-3 N0, status 1, the first offset
    in scan order is reported."""
    wf = np.full((1, 170, 40), -37.5, dtype=np.float32)
    got = snr_reference(wf, _records(1, 1, abs_time=5, abs_freq=5), None, FS)[0, 0]
    p = 10.0 ** (-3.75)
    assert got["status"] == 1 and (got["dt"], got["df"], got["n_symbols"]) == (-1, -1, 79)
    assert abs(got["snr_db"] - (-30.0 + BW_DB)) < 1e-9
    assert abs(got["noise_db"] - (-37.5)) < 1e-5 and abs(got["signal_db"] - 10 * np.log10(1e-3 * p)) < 1e-5


def _painted(T, F, rec, dt=0, df=0, level=0.0, back=-100.0):
    """A waterfall of `back` dB with the record's 79 tone cells at offset (dt, df) at `level` dB."""
    from ft8_demodulator_amd.synth import itones
    wf = np.full((1, T, F), back, dtype=np.float64)
    tone = itones(bytes(rec["payload"]))
    for k in range(79):
        row = int(rec["abs_time"]) + dt + 2 * k
        if 0 <= row < T:
            wf[0, row, int(rec["abs_freq"]) + df + 2 * int(tone[k])] = level
    return wf


def test_partly_out_of_range_in_time():
    """abs_time = -20 at 2 steps per symbol: symbols 10 .. 78 of offset dt = 0 lie in the waterfall
    (69), symbols 11 .. 78 of dt = -1 (68)."""
    recs = _records(1, 1, abs_time=-20, abs_freq=9)
    got, info = snr_reference(_painted(200, 64, recs[0, 0]), recs, None, FS, details=True)
    g = got[0, 0]
    assert g["status"] == 0 and (g["dt"], g["df"], g["n_symbols"]) == (0, 0, 69)
    # M = 1, N0 = 1e-10 (the 8 tone columns are far fewer than three quarters of the 64)
    assert abs(g["snr_db"] - (10 * np.log10((1.0 - 1e-10) / 1e-10) + BW_DB)) < 1e-9
    assert [(dt, df) for dt, df, _ in info[0][0]] == [(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1)]
    got = snr_reference(_painted(200, 64, recs[0, 0], dt=-1, df=1), recs, None, FS)[0, 0]
    assert (got["dt"], got["df"], got["n_symbols"]) == (-1, 1, 68)
    # the far end: abs_time + 2 k < T only for the first symbols
    recs = _records(1, 1, abs_time=190, abs_freq=9)
    got = snr_reference(_painted(200, 64, recs[0, 0]), recs, None, FS)[0, 0]
    assert (got["dt"], got["df"], got["n_symbols"]) == (0, 0, 5)


def test_frequency_edges():
    """abs_freq = 0 leaves no df = -1, abs_freq = F - 1 - 7 bpt no df = +1; one bin further in, all
    nine offsets are admissible."""
    F = 40
    wf = np.full((1, 170, F), -20.0)
    for af, missing in [(0, -1), (F - 1 - 14, 1)]:
        got, info = snr_reference(wf, _records(1, 1, abs_time=3, abs_freq=af), None, FS, details=True)
        offs = [(dt, df) for dt, df, _ in info[0][0]]
        assert offs == [(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1) if b != missing], af
        assert got[0, 0]["status"] == 1 and got[0, 0]["df"] == (0 if missing == -1 else -1)
    # the best offset is found among the admissible ones only
    recs = _records(1, 1, abs_time=3, abs_freq=F - 1 - 14)
    got = snr_reference(_painted(170, F, recs[0, 0], dt=1, df=0), recs, None, FS)[0, 0]
    assert got["status"] == 0 and (got["dt"], got["df"]) == (1, 0)
    # beyond the edge nothing is admissible: status 2
    got = snr_reference(wf, _records(1, 2, abs_time=3, abs_freq=[[F - 13, -2]]), None, FS)
    assert got["status"].tolist() == [[2, 2]]
    # F = 15 holds the 8 tones at abs_freq = 0 only
    got, info = snr_reference(np.full((1, 170, 15), -20.0), _records(1, 1, abs_time=3), None, FS, details=True)
    assert [(dt, df) for dt, df, _ in info[0][0]] == [(-1, 0), (0, 0), (1, 0)]


def test_status_2_and_3():
    wf = np.full((2, 50, 40), -20.0)
    recs = _records(2, 3, abs_time=[[55, -200, 0], [0, 0, 0]], abs_freq=4, ok=[[1, 1, 1], [1, 0, 1]])
    got = snr_reference(wf, recs, [3, 2], FS)
    assert got["status"].tolist() == [[2, 2, 1], [1, 3, 3]]
    blank = np.zeros((), dtype=_lib.SNR_DTYPE)
    for s, r, st in [(0, 0, 2), (0, 1, 2), (1, 1, 3), (1, 2, 3)]:
        blank["status"] = st
        assert got[s, r].tobytes() == blank.tobytes()
    # radius 0 at abs_time = T: the one offset has no row
    assert snr_reference(wf, _records(2, 1, abs_time=50, abs_freq=4), None, FS, radius=0)["status"].tolist() == [[2], [2]]
    # a NaN mean is skipped; with every mean NaN there is nothing left
    wfn = np.full((1, 50, 40), np.nan)
    assert snr_reference(wfn, _records(1, 1, abs_freq=4), None, FS)["status"][0, 0] == 2
    # a NaN floor with finite means: status 0, NaN report
    wfn = np.full((1, 50, 60), -20.0)
    wfn[0, :, :40] = np.nan
    recs = _records(1, 1, abs_time=0, abs_freq=44)
    got = snr_reference(wfn, recs, None, FS, q=0.5, radius=0)[0, 0]
    assert got["status"] == 0 and got["n_symbols"] == 25 and np.isnan(got["snr_db"]) and np.isnan(got["noise_db"])
