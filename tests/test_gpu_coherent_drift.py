"""The drift search of the coherent re-demodulation on the device (csrc/coherent.hip: ft8_coherent_drift_llr,
ft8_set_coherent_drift) against the float64 restatement coherent.coherent_restate(drift=...), and the whole
path against a construction from the stage call's own LLRs and the oracle's BP: exact, every field."""
import ctypes

import numpy as np
import pytest

import ap_cases as A
import coherent_cases as C
import drift_cases as Dc
import retry_cases as R

pytestmark = pytest.mark.gpu

ITERS = C.ITERS
# max |LLR_device - LLR_restate| over the stage tests' candidates, measured once on an MI355X against the
# float64 restatement: 2.69e-5 (12 kHz float32, 9 rates), 2.42e-5 (int16), 1.68e-5 (10 kHz), 1.01e-4 (33 rates
# over +-4 Hz/s); the LLRs are scaled to a variance of 24.  The plain pass has 1.86e-5: z is rotated in place
# from one rate to the next, one float32 complex multiply per element and rate, so the error grows with the
# number of rates.  The bound is 8 x the largest, the margin the plain stage test takes; 1 % of sqrt(24)
# would be 4.9e-2, sixty times the bound.
LLR_MEASURED = 1.01e-4
LLR_BOUND = 8 * LLR_MEASURED


def _L():
    from ft8_demodulator_amd import _lib
    return _lib


def _check_stage(name, got, ref, fs, D):
    from ft8_demodulator_amd import coherent
    llr, fits, drifts = got
    rllr, rfits, rdrifts, vols = ref
    assert np.array_equal(fits["status"], rfits["status"])
    assert np.array_equal(fits["n_sync"], rfits["n_sync"])
    measured = fits["status"] == 0
    # test_coherent_drift_reference.py: no input has a near tie, so no candidate is left out
    assert not any(coherent.near_tie(v, 1e-5) for v in vols if v is not None)
    assert np.array_equal(drifts["rate_index"], rdrifts["rate_index"])
    assert np.array_equal(drifts["rate_hz_per_s"], rdrifts["rate_hz_per_s"])
    assert np.array_equal(fits["dt_index"], rfits["dt_index"])
    assert np.array_equal(fits["df_index"], rfits["df_index"])
    assert np.abs(fits["df_hz"][measured].astype(np.float64) - rfits["df_hz"][measured]).max() <= 0.01
    assert np.array_equal(fits["dt_s"], (rfits["dt_index"] * (D / fs)).astype(np.float32))
    assert np.allclose(fits["metric"][measured], rfits["metric"][measured], rtol=1e-4)
    assert (llr[~measured] == 0.0).all()           # status 2 / 3: zeros
    err = float(np.abs(llr[measured] - rllr[measured]).max())
    print(f"{name}: {int(measured.sum())} candidates compared, max |LLR_device - LLR_restate| = {err:.3e} "
          f"(bound {LLR_BOUND:.3e})")
    assert err <= LLR_BOUND


@pytest.mark.parametrize("key", ["f32", "i16"])
def test_stage_equals_restatement_12k(gpu, key):
    """3 slots at 12 kHz, 83 candidates: the 3 x 3 grid points around a static signal, one at +1.0 Hz/s and
    a late one at -0.6 Hz/s per slot, a window that starts before the slot and one past its end; 9 rates."""
    from ft8_demodulator_amd.ldpc_decoder import coherent_llr_batch
    c = Dc.stage_slots_12k()
    ref = Dc.stage_case_12k(key)
    got = coherent_llr_batch(np.array(c["x"] if key == "f32" else c["pcm"]), c["cand"], c["slot_of"], C.FS, 2, 2,
                             drift=Dc.DRIFT)
    assert (ref[1]["status"] == 2).any() and ((ref[1]["n_sync"] % 21) != 0).any()
    assert len(set(ref[2]["rate_index"].tolist())) >= 5
    _check_stage(key, got, ref, C.FS, C.NSPS // 32)


def test_stage_equals_restatement_33_rates(gpu):
    """One slot with the widest search: 33 rates over +-4 Hz/s."""
    from ft8_demodulator_amd.ldpc_decoder import coherent_llr_batch
    cand, slot_of, ref = Dc.stage_case_wide()
    got = coherent_llr_batch(np.array(Dc.stage_slots_12k()["x"][:1]), cand, slot_of, C.FS, 2, 2, drift=Dc.DRIFT_WIDE)
    _check_stage("33 rates", got, ref, C.FS, C.NSPS // 32)


def test_stage_equals_restatement_10k(gpu):
    """fs = 10000 at 4 bins per tone and 4 steps per symbol: nsps 1600, D 50 (the range-checked loads), Mt 4."""
    from ft8_demodulator_amd.ldpc_decoder import coherent_llr_batch
    c = Dc.stage_case_10k()
    got = coherent_llr_batch(np.array(c["x"]), c["cand"], c["slot_of"], C.FS10, C.BPT10, C.SPS10, drift=Dc.DRIFT)
    _check_stage("10k", got, c["ref"], C.FS10, C.NSPS10 // 32)


def test_stage_off_writes_the_plain_bytes(gpu):
    """ft8_coherent_drift_llr with one rate, or with max_rate 0, writes the bytes of ft8_coherent_llr and
    zeros in the drift records; a NULL d_drift_out is accepted with the search on."""
    from ft8_demodulator_amd import coherent
    from ft8_demodulator_amd.ldpc_decoder import coherent_llr_batch
    _lib, torch = _L(), gpu
    c = Dc.stage_slots_12k()
    x = np.array(c["x"])
    llr, fits = coherent_llr_batch(x, c["cand"], c["slot_of"], C.FS, 2, 2)
    for off in ((2.0, 1), (0.0, 9)):
        l1, f1, d1 = coherent_llr_batch(x, c["cand"], c["slot_of"], C.FS, 2, 2, drift=off)
        assert l1.tobytes() == llr.tobytes() and f1.tobytes() == fits.tobytes()
        assert d1.tobytes() == bytes(8 * len(d1))
    on = coherent_llr_batch(x, c["cand"], c["slot_of"], C.FS, 2, 2, drift=Dc.DRIFT)
    ctx = _lib.context()
    n = len(c["cand"])
    p = _lib.Ft8Params()
    p.sample_rate, p.sample_rate_hz, p.bins_per_tone, p.steps_per_symbol = C.FS, float(C.FS), 2, 2
    d_x = torch.from_numpy(x).cuda()
    d_c = torch.from_numpy(np.array(c["cand"])).cuda()
    d_so = torch.from_numpy(np.array(c["slot_of"])).cuda()
    d_llr = torch.zeros(n, 174, dtype=torch.float64, device="cuda")
    d_fit = torch.zeros(n * coherent.FIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    ctx.check(_lib.lib().ft8_coherent_drift_llr(ctx.handle, _lib.ptr(d_x), _lib.FT8_F32, x.shape[1], 3, x.shape[1],
                                                ctypes.byref(p), _lib.ptr(d_c), _lib.ptr(d_so), n, 1.0, 9,
                                                _lib.ptr(d_llr), _lib.ptr(d_fit), None, _lib.stream_handle()),
              "ft8_coherent_drift_llr")
    assert d_llr.cpu().numpy().tobytes() == on[0].tobytes() and d_fit.cpu().numpy().tobytes() == on[1].tobytes()


# ---- ft8_set_coherent_drift inside ft8_decode_batch ------------------------------------------------------
E2E = dict(max_candidates=20, min_score=2)
CAP = 6
E2E_LATE = dict(max_candidates=80, min_score=2)


def _decoder(search=E2E, **kw):
    return R.decoder(C.FS, search, **kw)


@pytest.fixture(scope="module")
def e2e(gpu, oracle):
    return R.expectation(Dc.stage_slots_12k()["x"], C.FS, E2E, CAP, drift=Dc.DRIFT)


@pytest.fixture(scope="module")
def e2e_late(gpu, oracle):
    return R.expectation(Dc.stage_slots_12k()["x"], C.FS, E2E_LATE, R.late_cap, drift=Dc.DRIFT)


_per_slot = R.per_slot


def test_e2e_expectation_shows_every_outcome(e2e, e2e_late):
    """On the expectations alone: rescues at rate 0 (pass_index 2) and at another rate (6), listed candidates
    that stay failed, failed candidates beyond the cap; the late cap fills its list past candidate 64."""
    sent = set(Dc.stage_slots_12k()["payloads"])
    for e in (e2e, e2e_late):
        coh = e["coherent"]
        rescued = coh[coh["pass_index"] != 0]
        assert set(rescued["pass_index"].tolist()) <= {2, 6} and (rescued["pass_index"] == 6).any()
        assert all(bytes(r["payload"]) in sent for r in rescued)
        assert len(rescued) < len(e["listed"]) < int((e["plain"]["ok"] == 0).sum())
    assert (e2e["coherent"]["pass_index"] == 2).any() or (e2e_late["coherent"]["pass_index"] == 2).any()
    plain, s, cap = e2e_late["plain"], e2e_late["slot"], e2e_late["cap"]
    mine = plain[plain["slot"] == s]
    failed = mine["cand_index"][mine["ok"] == 0]
    assert len(mine) > 64 and int((failed < 64).sum()) < cap < len(failed)


def test_e2e_records_equal_construction(gpu, e2e):
    x = gpu.from_numpy(e2e["x"]).cuda()
    one = _decoder(coherent=CAP, coherent_drift=Dc.DRIFT)
    piped = _decoder(coherent=CAP, coherent_drift=Dc.DRIFT, context=_L().Context(0))
    piped.ctx.set_pipeline(1, 2, 4)
    for dec in (one, piped):
        got = dec.records(x)
        assert len(got) == 3
        for s in range(3):
            A.records_equal(got[s], _per_slot(e2e["coherent"], s))
    plain = _decoder().records(x)
    for s in range(3):
        A.records_equal(plain[s], _per_slot(e2e["plain"], s))


def test_late_cap_records_equal_construction(gpu, e2e_late):
    """max_candidates 80: the list kernel reaches the cap in its second round of 64, as one chain and as
    one slot per chunk over two internal streams."""
    x = gpu.from_numpy(e2e_late["x"]).cuda()
    one = _decoder(E2E_LATE, coherent=e2e_late["cap"], coherent_drift=Dc.DRIFT)
    piped = _decoder(E2E_LATE, coherent=e2e_late["cap"], coherent_drift=Dc.DRIFT, context=_L().Context(0))
    piped.ctx.set_pipeline(1, 2, 4)
    for dec in (one, piped):
        got = dec.records(x)
        assert len(got) == 3
        for s in range(3):
            A.records_equal(got[s], _per_slot(e2e_late["coherent"], s))


def test_off_means_off_in_the_whole_path(gpu):
    """On the plain coherent test's slots: ft8_set_coherent_drift(ctx, 0, 1), a context whose setter was
    never called, and a context that ran a drift batch before and was switched off again all give the
    same records and counts."""
    _lib = _L()
    x = gpu.from_numpy(np.array(C.stage_case_12k()["x"])).cuda()
    never = _decoder(coherent=4, context=_lib.Context(0))
    never.ctx.set_coherent_drift = lambda *a: None          # SlotDecoder.run sets it before every batch
    want = never.records(x)
    assert sum(int((r["pass_index"] == 2).sum()) for r in want) >= 2
    off = _decoder(coherent=4, context=_lib.Context(0))
    assert _lib.lib().ft8_set_coherent_drift(off.ctx.handle, 0.0, 1) == _lib.FT8_OK
    shared = _lib.Context(0)
    on = _decoder(coherent=4, coherent_drift=Dc.DRIFT, context=shared).records(x)
    assert len(on) == 3
    for got in (off.records(x), _decoder(coherent=4, context=shared).records(x)):
        assert len(got) == 3
        for s in range(3):
            assert got[s].tobytes() == want[s].tobytes()


def test_gain_on_the_device(gpu, oracle):
    """8 one-signal slots at -8 dB in 2500 Hz drifting by +-1.25 Hz/s, top-K 40, every failed candidate
    listed.  With coherent_drift=(2.0, 17) every slot whose signal the oracle's selection lists within one
    grid step of the truth yields the transmitted payload on a record with drift_index 1; with coherent
    alone at most 2 of them decode (float64 restatement and the oracle's BP: none from the coherent LLRs,
    2 by plain BP); no payload other than a transmitted one comes out."""
    from ft8_demodulator_amd import coherent
    x, pays, cands, rates = Dc.device_gain_slots()
    K = Dc.DEVICE_SEARCH
    listed = []
    for s in range(Dc.N_DEVICE):
        mag = oracle.waterfall(x[s], C.FS, 2, 2)
        t_lo = oracle.grid_bounds(mag.shape[0], mag.shape[1], 2, 2)[0]
        sc = oracle.score_grid(mag, 2, 2)
        idx, _ = oracle.select_topk(sc, K["max_candidates"], K["min_score"])
        near = [i for i in idx if abs(int(i // sc.shape[1]) + t_lo - cands[s][0]) <= 1
                and abs(int(i % sc.shape[1]) - cands[s][1]) <= 1]
        if near:
            listed.append(s)
    assert len(listed) >= 6
    d_x = gpu.from_numpy(np.array(x)).cuda()
    got = _decoder(K, coherent=0, coherent_drift=Dc.DEVICE_DRIFT).records(d_x)
    alone = _decoder(K, coherent=0).records(d_x)
    for s in range(Dc.N_DEVICE):
        for r in list(got[s]) + list(alone[s]):
            assert bytes(r["payload"]) == pays[s], (s, "a payload that was not transmitted")
    for s in listed:
        assert any(bytes(r["payload"]) == pays[s] and coherent.drift_index(r) == 1 and coherent.coherent_index(r) == 1
                   for r in got[s]), s
    n_alone = sum(len(alone[s]) > 0 for s in listed)
    print("slots listed", len(listed), "decoded with the drift search", len(listed), "with coherent alone", n_alone)
    assert n_alone <= 2


def test_errors_and_abi(gpu):
    _lib = _L()
    from ft8_demodulator_amd._pipeline import SlotDecoder
    from ft8_demodulator_amd.ldpc_decoder import coherent_llr_batch
    assert _lib.lib().ft8_abi_version() == 2
    ctx = _lib.Context(0)
    for a, r in ((1.0, 8), (1.0, 0), (1.0, 35), (1.0, -3), (-0.5, 9), (4.5, 9), (float("nan"), 9)):
        assert _lib.lib().ft8_set_coherent_drift(ctx.handle, a, r) == _lib.FT8_E_ARG
    for a, r in ((4.0, 33), (0.0, 1), (0.0, 33), (1.0, 1)):
        assert _lib.lib().ft8_set_coherent_drift(ctx.handle, a, r) == _lib.FT8_OK
    x = np.array(C.stage_case_12k()["x"][:1, :40000])
    for bad in ((1.0, 8), (1.0, 35), (-0.5, 9), (4.5, 9)):
        with pytest.raises(ValueError, match="coherent drift"):
            coherent_llr_batch(x, [(4, 400)], [0], C.FS, drift=bad)
    d_x = gpu.from_numpy(x).cuda()
    with pytest.raises(NotImplementedError, match="FT8_FLAG_SUBTRACT"):
        SlotDecoder(C.FS, flags=_lib.FT8_FLAG_TOPK | _lib.FT8_FLAG_SUBTRACT, coherent=4, coherent_drift=True,
                    **E2E).records(d_x)
    # a drift batch cannot be replayed either
    dec = _decoder(coherent=CAP, coherent_drift=True, context=ctx)
    dec.records(d_x)
    with pytest.raises(ValueError):
        ctx.replay("bp")


def test_from_wave_prints_the_drift(gpu, tmp_path, capsys):
    """from_wave --coherent --coherent-drift on one drifting slot as 16-bit PCM: the decode's `Coherent:`
    line ends with the rate, within one step of the transmitted -1.25 Hz/s."""
    import re
    import wave
    from ft8_demodulator_amd import from_wave
    x, pays, _, rates = Dc.device_gain_slots()
    pcm = np.clip(np.round(x[1] / 8.0 * 32767.0), -32767, 32767).astype(np.int16)
    path = str(tmp_path / "drifting.wav")
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(C.FS)
        w.writeframes(pcm.tobytes())
    opts = ["--max-candidates", "40", "--min-score", "2"]
    res = from_wave.main([path, "--coherent", "0", "--coherent-drift", "2:17"] + opts)
    out = capsys.readouterr().out
    assert len(res) >= 1 and all(bytes(r[0].payload) == pays[1] for r in res)
    found = re.findall(r"Coherent: dt [-+][0-9.]+ ms, df [-+][0-9.]+ Hz, drift ([-+][0-9.]+) Hz/s\n", out)
    assert len(found) >= 1 and all(abs(float(v) - rates[1]) <= 0.25 for v in found)
    res = from_wave.main([path, "--coherent", "0"] + opts)
    out = capsys.readouterr().out
    assert "drift" not in out
