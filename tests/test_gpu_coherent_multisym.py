"""The coherent pass's joint LLRs over 2 and 3 symbols on the device (csrc/coherent.hip:
ft8_coherent_nsym_llr, ft8_set_coherent_nsym) against the float64 restatement
coherent.coherent_restate(nsym=3), and the whole path against a construction from the stage call's own
LLRs and the oracle's BP: exact, every field."""
import ctypes

import numpy as np
import pytest

import ap_cases as A
import coherent_cases as C
import drift_cases as Dc
import multisym_cases as M
import retry_cases as R

pytestmark = pytest.mark.gpu

ITERS = C.ITERS
# Set 1 keeps the plain stage test's bound (test_gpu_coherent.py: 8 x 1.86e-5), under the drift search the
# drift stage test's (test_gpu_coherent_drift.py: 8 x 1.01e-4).
SET1_BOUND = 8 * 1.86e-5
SET1_DRIFT_BOUND = 8 * 1.01e-4
# max |LLR_device - LLR_restate| over sets 2 and 3 of the stage tests' candidates, measured once on an MI355X
# against the float64 restatement: 8.12e-5 (12 kHz float32; set 2 alone 3.68e-5), 5.94e-5 (int16; 3.89e-5),
# 3.59e-5 (10 kHz; 1.85e-5); the LLRs are scaled to a variance of 24.  Set 1 of the same runs: 1.65e-5,
# 1.86e-5, 1.11e-5, as in the plain stage test.  A joint metric adds up to three float32 correlations, each
# rotated by a float32 phase factor, before the power is taken, so its error is a small multiple of set 1's.
# The bound is 8 x the largest (float32 summation order varies by a small factor from input to input); 1 % of
# sqrt(24) would be 4.9e-2, 75 times the bound.
LLR_MEASURED = 8.12e-5
LLR_BOUND = 8 * LLR_MEASURED
# With the drift search (9 rates) sets 2 and 3 measured 2.84e-5 on the 19 candidates of that test, set 1
# 2.69e-5; they take the same bound as without the search, the largest figure measured on any input.
DRIFT_BOUND = LLR_BOUND


def _L():
    from ft8_demodulator_amd import _lib
    return _lib


def _check_stage(name, got, ref, fs, D, set1_bound=SET1_BOUND, bound=LLR_BOUND, drift=False):
    """test_gpu_coherent.py's _check_stage with the sets: status, n_sync, validity bytes and fit fields exactly
    (near ties in the sync grid left out under its cap of 1 in 20), set 1 within today's bound, sets 2 and 3
    within `bound`."""
    from ft8_demodulator_amd import coherent
    llr, fits = got[:2]
    valid = got[-1]
    rllr, rfits = ref[:2]
    rvalid, grids = (ref[3], ref[4]) if drift else (ref[2], ref[3])
    assert llr.shape == rllr.shape == (len(fits), 3, 174)
    assert np.array_equal(fits["status"], rfits["status"])
    assert np.array_equal(fits["n_sync"], rfits["n_sync"])
    assert np.array_equal(valid, rvalid) and valid.dtype == np.uint8
    assert np.array_equal(valid & 1, (fits["status"] == 0).astype(np.uint8))
    measured = fits["status"] == 0
    tie = np.array([g is not None and coherent.near_tie(g) for g in grids])
    cmp_ = measured & ~tie
    assert int((measured & tie).sum()) * 20 <= int(measured.sum())
    if drift:
        assert np.array_equal(got[2]["rate_index"][cmp_], ref[2]["rate_index"][cmp_])
    assert np.array_equal(fits["dt_index"][cmp_], rfits["dt_index"][cmp_])
    assert np.array_equal(fits["df_index"][cmp_], rfits["df_index"][cmp_])
    assert np.abs(fits["df_hz"][cmp_].astype(np.float64) - rfits["df_hz"][cmp_]).max() <= 0.01
    assert np.array_equal(fits["dt_s"][cmp_], (rfits["dt_index"][cmp_] * (D / fs)).astype(np.float32))
    assert np.allclose(fits["metric"][cmp_], rfits["metric"][cmp_], rtol=1e-4)
    assert (llr[~measured] == 0.0).all()           # status 2 / 3: zeros in every set
    err = [float(np.abs(llr[cmp_, n] - rllr[cmp_, n]).max()) for n in range(3)]
    print(f"{name}: {int(cmp_.sum())} candidates compared, {int((measured & tie).sum())} near ties left out, "
          f"max |LLR_device - LLR_restate| = {err[0]:.3e} (set 1, bound {set1_bound:.3e}), {err[1]:.3e} (set 2), "
          f"{err[2]:.3e} (set 3, bound {bound:.3e})")
    assert err[0] <= set1_bound
    assert max(err[1:]) <= bound


@pytest.fixture(scope="module")
def ref_12k():
    """The restatement at max_nsym 3 of stage_case_12k, float32 and int16."""
    from ft8_demodulator_amd import coherent
    c = C.stage_case_12k()
    return {key: coherent.coherent_restate(c["x"] if key == "f32" else c["pcm"], c["cand"], c["slot_of"], C.FS, C.NSPS,
                                           C.NFFT, 2, details=True, nsym=3) for key in ("f32", "i16")}


@pytest.mark.parametrize("key", ["f32", "i16"])
def test_stage_equals_restatement_12k(gpu, ref_12k, key):
    """3 slots at 12 kHz, 85 candidates (absent symbols, windows off both slot edges) at max_nsym 3."""
    from ft8_demodulator_amd.ldpc_decoder import coherent_llr_batch
    c = C.stage_case_12k()
    x = np.array(c["x"] if key == "f32" else c["pcm"])
    got = coherent_llr_batch(x, c["cand"], c["slot_of"], C.FS, 2, 2, nsym=3)
    ref = ref_12k[key]
    assert (ref[1]["status"] == 2).any() and ((ref[1]["n_sync"] % 21) != 0).any() and (ref[2] == 7).any()
    _check_stage(key, got, ref, C.FS, C.NSPS // 32)


def test_stage_equals_restatement_10k(gpu):
    """fs = 10000 at 4 bins per tone and 4 steps per symbol: nsps 1600, D 50, Mt 4."""
    from ft8_demodulator_amd import coherent
    from ft8_demodulator_amd.ldpc_decoder import coherent_llr_batch
    c = C.stage_case_10k()
    ref = coherent.coherent_restate(c["x"], c["cand"], c["slot_of"], C.FS10, C.NSPS10, C.NFFT10, C.SPS10, details=True,
                                    nsym=3)
    got = coherent_llr_batch(np.array(c["x"]), c["cand"], c["slot_of"], C.FS10, C.BPT10, C.SPS10, nsym=3)
    _check_stage("10k", got, ref, C.FS10, C.NSPS10 // 32)


def test_stage_with_the_drift_search(gpu):
    """9 rates on the drifting signals of drift_cases' first slot (+1.0 Hz/s, and -0.6 Hz/s running past the
    slot's end) plus the two windows off the slot: sets 2 and 3 come from z at the winning rate."""
    from ft8_demodulator_amd import coherent
    from ft8_demodulator_amd.ldpc_decoder import coherent_llr_batch
    c = Dc.stage_slots_12k()
    sel = np.r_[9:27, 81, 82]
    x, cand, so = np.array(c["x"]), c["cand"][sel], c["slot_of"][sel]
    ref = coherent.coherent_restate(x, cand, so, C.FS, C.NSPS, C.NFFT, 2, details=True, drift=Dc.DRIFT, nsym=3)
    assert len(set(ref[2]["rate_index"].tolist())) >= 3 and (ref[3] == 7).sum() >= 18
    got = coherent_llr_batch(x, cand, so, C.FS, 2, 2, drift=Dc.DRIFT, nsym=3)
    assert np.array_equal(got[2]["rate_hz_per_s"], ref[2]["rate_hz_per_s"])
    _check_stage("drift", got, ref, C.FS, C.NSPS // 32, SET1_DRIFT_BOUND, DRIFT_BOUND, drift=True)


def test_stage_slot_out_of_range_and_empty(gpu):
    from ft8_demodulator_amd.ldpc_decoder import coherent_llr_batch
    c = C.stage_case_12k()
    llr, fits, valid = coherent_llr_batch(np.array(c["x"]), c["cand"][:3], [0, 3, -1], C.FS, nsym=3)
    assert fits["status"].tolist() == [0, 3, 3] and valid.tolist() == [7, 0, 0]
    assert (llr[1:] == 0.0).all() and llr[0].any(axis=1).all()
    llr, fits, valid = coherent_llr_batch(np.array(c["x"]), np.zeros((0, 2), np.int32), [], C.FS, nsym=2)
    assert llr.shape == (0, 2, 174) and len(fits) == 0 and len(valid) == 0


def _nsym_call(x, cand, slot_of, drift, nsym, with_valid=True):
    """ft8_coherent_nsym_llr itself -> the raw bytes of (LLRs, fits, drift records, validity bytes)."""
    from ft8_demodulator_amd import coherent
    _lib, torch = _L(), __import__("torch")
    ctx = _lib.context()
    n = len(cand)
    p = _lib.Ft8Params()
    p.sample_rate, p.sample_rate_hz, p.bins_per_tone, p.steps_per_symbol = C.FS, float(C.FS), 2, 2
    d_x = torch.from_numpy(x).cuda()
    d_c = torch.from_numpy(np.array(cand)).cuda()
    d_so = torch.from_numpy(np.array(slot_of)).cuda()
    d_llr = torch.full((n, max(nsym, 1), 174), 7.0, dtype=torch.float64, device="cuda")
    d_fit = torch.full((n * coherent.FIT_DTYPE.itemsize,), 7, dtype=torch.uint8, device="cuda")
    d_dr = torch.full((n * coherent.DRIFT_DTYPE.itemsize,), 7, dtype=torch.uint8, device="cuda")
    d_v = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    rc = _lib.lib().ft8_coherent_nsym_llr(ctx.handle, _lib.ptr(d_x), _lib.FT8_F32, x.shape[1], x.shape[0], x.shape[1],
                                          ctypes.byref(p), _lib.ptr(d_c), _lib.ptr(d_so), n, drift[0], drift[1],
                                          _lib.ptr(d_llr), _lib.ptr(d_fit), _lib.ptr(d_dr), nsym,
                                          _lib.ptr(d_v) if with_valid else None, _lib.stream_handle())
    ctx.check(rc, "ft8_coherent_nsym_llr")
    return tuple(t.cpu().numpy().tobytes() for t in (d_llr, d_fit, d_dr, d_v))


def test_stage_off_writes_todays_bytes(gpu):
    """max_nsym = 1 gives the bytes of ft8_coherent_drift_llr -- LLRs, fits, drift records -- with the search
    off and at (1.0, 9), and validity bytes of 1 for a valid fit; a NULL d_valid_out is accepted at 3."""
    from ft8_demodulator_amd.ldpc_decoder import coherent_llr_batch
    c = Dc.stage_slots_12k()
    x = np.array(c["x"])
    for drift in ((0.0, 1), Dc.DRIFT):
        llr, fits, dr = coherent_llr_batch(x, c["cand"], c["slot_of"], C.FS, 2, 2, drift=drift)
        got = _nsym_call(x, c["cand"], c["slot_of"], drift, 1)
        assert got[0] == llr.tobytes() and got[1] == fits.tobytes() and got[2] == dr.tobytes()
        assert got[3] == (fits["status"] == 0).astype(np.uint8).tobytes()
        assert (fits["status"] == 2).any()
    with3 = _nsym_call(x, c["cand"], c["slot_of"], Dc.DRIFT, 3)
    null3 = _nsym_call(x, c["cand"], c["slot_of"], Dc.DRIFT, 3, with_valid=False)
    assert with3[:3] == null3[:3] and null3[3] == bytes([7]) * len(c["cand"])


# ---- ft8_set_coherent_nsym inside ft8_decode_batch ---------------------------------------------------------
E2E, CAP, AP = M.E2E, M.CAP, M.AP


def _decoder(search=E2E, **kw):
    return R.decoder(C.FS, search, **kw)


@pytest.fixture(scope="module")
def e2e(gpu, oracle):
    return R.expectation(M.e2e_slots()[0], C.FS, E2E, CAP, nsym=M.S, ap=AP)


_per_slot = R.per_slot


def test_e2e_expectation_shows_every_outcome(e2e):
    """On the expectation alone: plain decodes, set-1 rescues (pass_index 2), at least one record from a later
    set (10), listed candidates that stay failed; every rescued payload was transmitted."""
    plain, coh = e2e["plain"], e2e["coherent"]
    sent = M.e2e_slots()[1]
    assert int(plain["ok"].sum()) >= 3
    rescued = coh[coh["pass_index"] != 0]
    assert set(rescued["pass_index"].tolist()) <= {2, 10}
    n1, n23 = int((rescued["pass_index"] == 2).sum()), int((rescued["pass_index"] == 10).sum())
    print("plain decodes", int(plain["ok"].sum()), "set-1 rescues", n1, "later-set rescues", n23, "listed",
          len(e2e["listed"]))
    assert n1 >= 2 and n23 >= 1
    assert all(bytes(r["payload"]) in sent for r in rescued)
    assert len(rescued) < len(e2e["listed"]) <= 9 * CAP


def test_e2e_records_equal_construction(gpu, e2e):
    """As one chain and as one slot per chunk over two internal streams."""
    x = gpu.from_numpy(e2e["x"]).cuda()
    one = _decoder(coherent=CAP, coherent_nsym=3)
    piped = _decoder(coherent=CAP, coherent_nsym=3, context=_L().Context(0))
    piped.ctx.set_pipeline(1, 2, 4)
    for dec in (one, piped):
        got = dec.records(x)
        assert len(got) == 9
        for s in range(9):
            A.records_equal(got[s], _per_slot(e2e["coherent"], s))


def test_e2e_with_ap(gpu, e2e):
    """The a-priori pass that follows sees the STFT LLRs of the candidates still failed; rescued records
    carry no AP index."""
    from ft8_demodulator_amd import ap, coherent
    x = gpu.from_numpy(e2e["x"]).cuda()
    got = _decoder(coherent=CAP, coherent_nsym=3, ap=AP).records(x)
    for s in range(9):
        A.records_equal(got[s], _per_slot(e2e["both"], s))
        assert all(ap.ap_index(r) == 0 for r in got[s] if coherent.coherent_index(r))
    assert any(coherent.multisymbol_index(r) for s in range(9) for r in got[s])


DRIFT_CAP = 6


@pytest.fixture(scope="module")
def e2e_drift(gpu, oracle):
    return R.expectation(Dc.stage_slots_12k()["x"], C.FS, E2E, DRIFT_CAP, drift=Dc.DRIFT, nsym=2, ap=AP)


def test_e2e_drift_search_and_sets_together(gpu, e2e_drift):
    """The drifting slots of the drift tests with the drift search, two sets and the a-priori pass at once
    (k_coherent<.., CohDrift, CohMulti>; k_coh_merge ORs 4 and 8 into the 2): the batch's records equal the
    construction's with and without AP.  On the expectation alone: a rescue at a rate other than 0."""
    coh = e2e_drift["coherent"]
    rescued = coh[(coh["pass_index"] & 2) != 0]
    print("rescues", len(rescued), "at a rate other than 0", int(((rescued["pass_index"] & 4) != 0).sum()),
          "from set 2", int(((rescued["pass_index"] & 8) != 0).sum()), "listed", len(e2e_drift["listed"]))
    assert ((rescued["pass_index"] & 4) != 0).any()
    x = gpu.from_numpy(e2e_drift["x"]).cuda()
    for ap_kw, key in ((dict(ap=AP), "both"), ({}, "coherent")):
        got = _decoder(coherent=DRIFT_CAP, coherent_drift=Dc.DRIFT, coherent_nsym=2, **ap_kw).records(x)
        assert len(got) == 3
        for s in range(3):
            A.records_equal(got[s], _per_slot(e2e_drift[key], s))


def test_off_means_off_in_the_whole_path(gpu):
    """coherent_nsym=1, a context whose setter was never called, and a context that ran a batch at 3 before
    and was switched back all give the same record bytes."""
    _lib = _L()
    x = gpu.from_numpy(np.array(C.stage_case_12k()["x"])).cuda()
    never = _decoder(coherent=4, context=_lib.Context(0))
    never.ctx.set_coherent_nsym = lambda *a: None          # SlotDecoder.run sets it before every batch
    want = never.records(x)
    assert sum(int((r["pass_index"] == 2).sum()) for r in want) >= 2
    off = _decoder(coherent=4, coherent_nsym=1, context=_lib.Context(0))
    shared = _lib.Context(0)
    on = _decoder(coherent=4, coherent_nsym=3, context=shared).records(x)
    assert len(on) == 3
    for got in (off.records(x), _decoder(coherent=4, context=shared).records(x)):
        assert len(got) == 3
        for s in range(3):
            assert got[s].tobytes() == want[s].tobytes()


def test_superset_on_the_weak_slots(gpu):
    """The 32 slots at -23 dB with coherent=True: what coherent_nsym=3 decodes includes all that 1 decodes,
    nothing decoded was not transmitted, and 3 decodes at least one more slot."""
    from ft8_demodulator_amd import coherent
    x, pays, _ = M.weak_slots()
    d_x = gpu.from_numpy(np.array(x)).cuda()
    r1 = _decoder(coherent=True).records(d_x)
    r3 = _decoder(coherent=True, coherent_nsym=3).records(d_x)
    n1 = n3 = 0
    for s in range(M.N_WEAK):
        p1, p3 = {bytes(v["payload"]) for v in r1[s]}, {bytes(v["payload"]) for v in r3[s]}
        assert p1 <= {pays[s]} and p3 <= {pays[s]}, (s, "a payload that was not transmitted")
        assert p1 <= p3, s
        assert all(coherent.multisymbol_index(v) == 0 for v in r1[s])
        n1 += len(p1)
        n3 += len(p3)
    print("slots decoded at coherent_nsym 1:", n1, "at 3:", n3, "of", M.N_WEAK)
    assert n3 >= n1 + 1


def test_noise_decodes_nothing(gpu):
    """8 noise-only slots, max_candidates 300, min_score 2, coherent=32, coherent_nsym=3: 0 decodes."""
    x, _ = M.noise_slots()
    d_x = gpu.from_numpy(np.array(x[:8])).cuda()
    got = _decoder(dict(max_candidates=300, min_score=2), coherent=32, coherent_nsym=3).records(d_x)
    assert len(got) == 8 and sum(len(r) for r in got) == 0


def test_errors_and_abi(gpu):
    """max_nsym 0 and 4 give FT8_E_ARG from the setter and the stage call, and the context stays usable."""
    _lib = _L()
    from ft8_demodulator_amd.ldpc_decoder import coherent_llr_batch
    assert _lib.lib().ft8_abi_version() == 2
    ctx = _lib.Context(0)
    for bad in (0, 4, -1):
        assert _lib.lib().ft8_set_coherent_nsym(ctx.handle, bad) == _lib.FT8_E_ARG
    for good in (3, 2, 1):
        assert _lib.lib().ft8_set_coherent_nsym(ctx.handle, good) == _lib.FT8_OK
    c = C.stage_case_12k()
    x = np.array(c["x"][:1])
    for bad in (0, 4):
        with pytest.raises(ValueError, match="max_nsym"):
            _nsym_call(x, c["cand"][:2], [0, 0], (0.0, 1), bad)
        with pytest.raises(ValueError, match="nsym"):
            coherent_llr_batch(x, c["cand"][:2], [0, 0], C.FS, nsym=bad)
    llr, fits, valid = coherent_llr_batch(x, c["cand"][:2], [0, 0], C.FS, nsym=3)     # the thread's context again
    assert valid.tolist() == [7, 7]
    d_x = gpu.from_numpy(np.array(c["x"])).cuda()
    dec = _decoder(coherent=CAP, coherent_nsym=3, context=ctx)
    assert len(dec.records(d_x)) == 3
    with pytest.raises(ValueError):           # a multi-symbol batch cannot be replayed either
        ctx.replay("bp")


def test_messages_reports_and_pack_take_multisymbol_records(gpu, e2e):
    """ft8_unpack77, ft8_snr_last and ft8_pack_decodes carry a record with bit 3 unchanged."""
    from ft8_demodulator_amd import coherent, message
    _lib = _L()
    d_x = gpu.from_numpy(e2e["x"]).cuda()
    dec = _decoder(coherent=CAP, coherent_nsym=3)
    recs, texts, reps = dec._fetch(d_x, text=True, snr=True)
    multi = [(s, i) for s in range(9) for i, r in enumerate(recs[s]) if coherent.multisymbol_index(r)]
    assert multi
    for s, i in multi:
        want = message.unpack77([bytes(recs[s][i]["payload"])])[0]
        assert texts[s][i]["status"] == want["status"] and texts[s][i]["text"] == want["text"]
        assert reps[s][i]["status"] in (0, 1) and np.isfinite(reps[s][i]["snr_db"])
    out, counts = dec.run(d_x)
    nbytes = int(_lib.lib().ft8_pack_bytes(9, 64))
    send = gpu.zeros(nbytes, dtype=gpu.uint8, device="cuda")
    dec.ctx.check(_lib.lib().ft8_pack_decodes(dec.ctx.handle, _lib.ptr(out), _lib.ptr(counts), 9, dec.cap, 64, 0,
                                              _lib.ptr(send), None, _lib.stream_handle(0)), "ft8_pack_decodes")
    raw = send.cpu().numpy()
    total = int(raw[:8].view(np.int64)[0])
    packed = raw[nbytes - 64 * 40:].view(_lib.RESULT_DTYPE)[:total]
    want = np.concatenate([recs[s] for s in range(9)])
    assert total == int(counts.sum()) == len(want)
    packed = packed[np.lexsort((packed["cand_index"], packed["slot"]))]
    assert packed.tobytes() == want[np.lexsort((want["cand_index"], want["slot"]))].tobytes()
    assert int(((packed["pass_index"] & 8) != 0).sum()) == len(multi)
