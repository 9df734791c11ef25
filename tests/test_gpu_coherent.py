"""Coherent re-demodulation on the device (csrc/coherent.hip: ft8_coherent_llr, ft8_set_coherent,
FT8_FLAG_COHERENT) against the float64 restatement coherent.coherent_restate, and the whole path against
a construction from the stage call's own LLRs and the oracle's BP: exact, every field."""
import numpy as np
import pytest

import ap_cases as A
import coherent_cases as C
import retry_cases as R

pytestmark = pytest.mark.gpu

ITERS = C.ITERS
# the stage comparison and its bound live beside the cases (coherent_cases.check_stage), shared with
# test_gpu_baseband_geometry.py
LLR_MEASURED = C.LLR_MEASURED
LLR_BOUND = C.LLR_BOUND
_check_stage = C.check_stage


def _L():
    from ft8_demodulator_amd import _lib
    return _lib


@pytest.mark.parametrize("key", ["f32", "i16"])
def test_stage_equals_restatement_12k(gpu, key):
    """3 slots at 12 kHz, 85 candidates: the 3 x 3 grid points around 9 signals (three of them running past
    the slot's end), two candidates whose window starts before the slot and two past its end."""
    from ft8_demodulator_amd.ldpc_decoder import coherent_llr_batch
    c = C.stage_case_12k()
    x = np.array(c["x"] if key == "f32" else c["pcm"])
    got = coherent_llr_batch(x, c["cand"], c["slot_of"], C.FS, 2, 2)
    assert (c[key][1]["status"] == 2).any() and ((c[key][1]["n_sync"] % 21) != 0).any()
    _check_stage(key, got, c[key], C.FS, C.NSPS // 32, C.BIN)


def test_stage_equals_restatement_10k(gpu):
    """fs = 10000 at 4 bins per tone and 4 steps per symbol: nsps 1600, D 50 (no float4 path), Mt 4."""
    from ft8_demodulator_amd.ldpc_decoder import coherent_llr_batch
    c = C.stage_case_10k()
    got = coherent_llr_batch(np.array(c["x"]), c["cand"], c["slot_of"], C.FS10, C.BPT10, C.SPS10)
    _check_stage("10k", got, c["f32"], C.FS10, C.NSPS10 // 32, C.FS10 / C.NFFT10)


@pytest.mark.parametrize("key", ["f32", "i16"])
def test_stage_at_the_slot_edges(gpu, key):
    """The stage case's measured candidates whose baseband window starts before the slot or ends past it
    (the range-checked loop of bb_mix_down; csrc/baseband.h), alone, against the restatement."""
    from ft8_demodulator_amd.ldpc_decoder import coherent_llr_batch
    c = C.stage_case_12k()
    x = np.array(c["x"] if key == "f32" else c["pcm"])
    Q, sps = 32, C.NSPS // C.HOP
    D, Mg = C.NSPS // Q, (Q + 2 * sps - 1) // (2 * sps) + 1
    nb = c["cand"][:, 0].astype(np.int64) * C.HOP - Mg * D
    rllr, rfits, grids = c[key]
    measured = rfits["status"] == 0
    head, tail = measured & (nb < 0), measured & (nb + (79 * Q + 2 * Mg) * D > x.shape[1])
    assert head.any() and tail.any() and (measured & ~head & ~tail).any()
    sel = np.flatnonzero(head | tail)
    got = coherent_llr_batch(x, c["cand"][sel], c["slot_of"][sel], C.FS, 2, 2)
    _check_stage(key + " edges", got, (rllr[sel], rfits[sel], [grids[i] for i in sel]), C.FS, D, C.BIN)


def test_stage_slot_out_of_range_and_empty(gpu):
    from ft8_demodulator_amd.ldpc_decoder import coherent_llr_batch
    c = C.stage_case_12k()
    llr, fits = coherent_llr_batch(np.array(c["x"]), c["cand"][:3], [0, 3, -1], C.FS)
    assert fits["status"].tolist() == [0, 3, 3] and (llr[1:] == 0.0).all() and llr[0].any()
    llr, fits = coherent_llr_batch(np.array(c["x"]), np.zeros((0, 2), np.int32), [], C.FS)
    assert llr.shape == (0, 174) and len(fits) == 0


# ---- FT8_FLAG_COHERENT inside ft8_decode_batch -----------------------------------------------------------
E2E = dict(max_candidates=20, min_score=2)
CAP = 4
AP = ["CQ ? ?"]
# more candidates than one wave scans in a round (64): with the cap chosen by late_cap the list of one
# slot fills up in the second round
E2E_LATE = dict(max_candidates=80, min_score=2)


def _decoder(search=E2E, **kw):
    return R.decoder(C.FS, search, **kw)


@pytest.fixture(scope="module")
def e2e(gpu, oracle):
    return R.expectation(C.stage_case_12k()["x"], C.FS, E2E, CAP, ap=AP)


@pytest.fixture(scope="module")
def e2e_late(gpu, oracle):
    return R.expectation(C.stage_case_12k()["x"], C.FS, E2E_LATE, R.late_cap)


_per_slot = R.per_slot


def test_e2e_expectation_shows_every_outcome(e2e):
    """What the slots were built for, on the expectation alone: plain decodes, rescues, listed candidates
    that stay failed, and failed candidates beyond the cap."""
    plain, coh = e2e["plain"], e2e["coherent"]
    sent = set(C.stage_case_12k()["payloads"])
    assert int(plain["ok"].sum()) >= 3
    rescued = coh[coh["pass_index"] == 2]
    assert len(rescued) >= 2 and all(bytes(r["payload"]) in sent for r in rescued)
    assert len(e2e["listed"]) == 3 * CAP and len(rescued) < len(e2e["listed"])
    assert int((plain["ok"] == 0).sum()) > len(e2e["listed"])


def test_e2e_records_equal_construction(gpu, e2e):
    x = gpu.from_numpy(e2e["x"]).cuda()
    got = _decoder(coherent=CAP).records(x)
    plain = _decoder().records(x)
    assert len(got) == len(plain) == 3
    for s in range(3):
        A.records_equal(got[s], _per_slot(e2e["coherent"], s))
        A.records_equal(plain[s], _per_slot(e2e["plain"], s))      # the unflagged decoder: today's path
        assert (plain[s]["pass_index"] == 0).all()


def test_e2e_with_ap(gpu, e2e):
    """The a-priori pass that follows sees the STFT LLRs of the candidates still failed; rescued records
    carry no AP index."""
    from ft8_demodulator_amd import ap, coherent
    x = gpu.from_numpy(e2e["x"]).cuda()
    got = _decoder(coherent=CAP, ap=AP).records(x)
    for s in range(3):
        A.records_equal(got[s], _per_slot(e2e["both"], s))
        assert all(ap.ap_index(r) == 0 for r in got[s] if coherent.coherent_index(r))


def test_e2e_pipelined_chunks_and_int16(gpu, e2e):
    """One slot per chunk over two internal streams gives the single chain's records; int16 PCM of the
    same slots decodes the same payloads at the same candidates."""
    x = gpu.from_numpy(e2e["x"]).cuda()
    dec = _decoder(coherent=CAP, context=_L().Context(0))
    dec.ctx.set_pipeline(1, 2, 4)
    got = dec.records(x)
    for s in range(3):
        A.records_equal(got[s], _per_slot(e2e["coherent"], s))
    pcm = gpu.from_numpy(np.array(C.stage_case_12k()["pcm"])).cuda()
    got16 = _decoder(coherent=CAP).records(pcm, code=_L().FT8_I16)
    assert sum(int((r["pass_index"] == 2).sum()) for r in got16) >= 2


# ---- the construction at bins_per_tone != steps_per_symbol ----------------------------------------------
FACTORS = [(3, 2), (2, 4)]


@pytest.fixture(scope="module", params=FACTORS, ids=["3x2", "2x4"])
def e2e_factors(request, gpu, oracle):
    """The e2e fixture's construction (three slots, coherent=4, ap=["CQ ? ?"]) with every stage call, the
    restatements and the decoder at (bpt, sps) -> (bpt, sps, expectation)."""
    bpt, sps = request.param
    return bpt, sps, R.expectation(C.stage_case_12k()["x"], C.FS, E2E, CAP, ap=AP, bpt=bpt, sps=sps)


def test_e2e_factors_expectation_shows_every_outcome(e2e_factors):
    """On the expectation alone, at each pair: a plain decode, a rescue of a transmitted payload, a listed
    candidate that stays failed."""
    bpt, sps, e = e2e_factors
    plain, coh = e["plain"], e["coherent"]
    sent = set(C.stage_case_12k()["payloads"])
    rescued = coh[coh["pass_index"] == 2]
    print(f"({bpt}, {sps}): plain decodes {int(plain['ok'].sum())}, rescues {len(rescued)}, listed {len(e['listed'])}")
    assert int(plain["ok"].sum()) >= 1
    assert len(rescued) >= 1 and all(bytes(r["payload"]) in sent for r in rescued)
    assert len(rescued) < len(e["listed"]) <= 3 * CAP


def test_e2e_factors_records_equal_construction(gpu, e2e_factors):
    """Coherent alone and coherent + AP: the batch's records equal the construction's field for field."""
    bpt, sps, e = e2e_factors
    x = gpu.from_numpy(e["x"]).cuda()
    for kw, key in ((dict(coherent=CAP), "coherent"), (dict(coherent=CAP, ap=AP), "both")):
        got = R.decoder(C.FS, E2E, bpt, sps, **kw).records(x)
        assert len(got) == 3
        for s in range(3):
            A.records_equal(got[s], _per_slot(e[key], s))


def test_late_cap_expectation_fills_the_list_in_the_second_round(e2e_late):
    """On the expectation alone: one slot selects more than 64 candidates, fewer of its first 64 failed
    than the cap lists, and more of them all failed than the cap lists."""
    plain, s, cap = e2e_late["plain"], e2e_late["slot"], e2e_late["cap"]
    mine = plain[plain["slot"] == s]
    assert len(mine) > 64 and (mine["cand_index"] == np.arange(len(mine))).all()
    failed = mine["cand_index"][mine["ok"] == 0]
    assert int((failed < 64).sum()) < cap < len(failed)
    listed = [i for i in e2e_late["listed"] if plain["slot"][i] == s]
    assert len(listed) == cap and plain["cand_index"][listed[-1]] >= 64
    assert int(plain["ok"].sum()) >= 3 and int((e2e_late["coherent"]["pass_index"] == 2).sum()) >= 1


def test_late_cap_records_equal_construction(gpu, e2e_late):
    """max_candidates 80: the list kernel reaches the cap in its second round of 64, as one chain and as
    one slot per chunk over two internal streams."""
    x = gpu.from_numpy(e2e_late["x"]).cuda()
    one = _decoder(E2E_LATE, coherent=e2e_late["cap"])
    piped = _decoder(E2E_LATE, coherent=e2e_late["cap"], context=_L().Context(0))
    piped.ctx.set_pipeline(1, 2, 4)
    for dec in (one, piped):
        got = dec.records(x)
        assert len(got) == 3
        for s in range(3):
            A.records_equal(got[s], _per_slot(e2e_late["coherent"], s))


def test_gain_on_the_device(gpu):
    """The 16 slots at -22 dB of the CPU test: with the flag at least 12 transmitted payloads, nothing
    that was not transmitted; without it none."""
    x, pays, _ = C.weak_slots()
    d_x = gpu.from_numpy(np.array(x)).cuda()
    got = _decoder(coherent=True).records(d_x)
    found = 0
    for s, r in enumerate(got):
        dec = {bytes(v["payload"]) for v in r}
        assert dec <= {pays[s]}, (s, "a payload that was not transmitted")
        found += pays[s] in dec
    print("coherent decodes", found, "of", C.N_WEAK)
    assert found >= 12
    assert sum(len(r) for r in _decoder().records(d_x)) == 0


def test_messages_reports_and_pack_take_rescued_records(gpu):
    """ft8_unpack77, ft8_snr_last and ft8_pack_decodes run on a coherent batch unchanged: four weak slots'
    rescued rows carry a text, a finite report near the transmitted SNR (-18.2 dB in 2500 Hz), and are
    packed with their pass_index."""
    from ft8_demodulator_amd import coherent, message
    _lib = _L()
    x, pays, _ = C.weak_slots()
    d_x = gpu.from_numpy(np.array(x[:4])).cuda()
    dec = _decoder(coherent=True)
    recs, texts, reps = dec._fetch(d_x, text=True, snr=True)
    n = 0
    for s in range(4):
        want = message.unpack77([pays[s]])[0]
        for rec, t, r in zip(recs[s], texts[s], reps[s]):
            assert coherent.coherent_index(rec) == 1 and bytes(rec["payload"]) == pays[s]
            assert t["status"] == want["status"] and t["text"] == want["text"]
            assert r["status"] in (0, 1) and -24.0 < r["snr_db"] < -12.0
            n += 1
    assert n >= 3
    out, counts = dec.run(d_x)
    nbytes = int(_lib.lib().ft8_pack_bytes(4, 16))
    send = gpu.zeros(nbytes, dtype=gpu.uint8, device="cuda")
    dec.ctx.check(_lib.lib().ft8_pack_decodes(dec.ctx.handle, _lib.ptr(out), _lib.ptr(counts), 4, dec.cap, 16, 0,
                                              _lib.ptr(send), None, _lib.stream_handle(0)), "ft8_pack_decodes")
    raw = send.cpu().numpy()
    total = int(raw[:8].view(np.int64)[0])
    packed = raw[nbytes - 16 * 40:].view(_lib.RESULT_DTYPE)[:total]
    assert total == int(counts.sum()) >= 3 and (packed["pass_index"] == 2).all() and (packed["ok"] == 1).all()


def test_errors_and_abi(gpu):
    _lib = _L()
    from ft8_demodulator_amd.ldpc_decoder import coherent_llr_batch
    assert _lib.lib().ft8_abi_version() == 2
    assert _lib.FT8_FLAG_COHERENT == 8
    x = np.array(C.stage_case_12k()["x"][:1, :40000])
    cand, so = [(4, 400)], [0]
    for bad in (x.astype(np.float64), x.astype(np.complex64), x.astype(np.complex128)):
        with pytest.raises(NotImplementedError, match="float32 or int16"):
            coherent_llr_batch(bad, cand, so, C.FS)
    with pytest.raises(NotImplementedError, match="hop"):
        coherent_llr_batch(x, cand, so, 12006.3)
    d_x = gpu.from_numpy(x).cuda()
    from ft8_demodulator_amd._pipeline import SlotDecoder
    with pytest.raises(NotImplementedError, match="FT8_FLAG_SUBTRACT"):
        SlotDecoder(C.FS, flags=_lib.FT8_FLAG_TOPK | _lib.FT8_FLAG_SUBTRACT, coherent=4, **E2E).records(d_x)
    with pytest.raises(NotImplementedError, match="hop"):
        SlotDecoder(12006.3, flags=_lib.FT8_FLAG_TOPK, coherent=4, **E2E).records(d_x)
    with pytest.raises(NotImplementedError, match="float32 or int16"):
        SlotDecoder(C.FS, flags=_lib.FT8_FLAG_TOPK, coherent=4, **E2E).records(d_x.to(gpu.float64))
    with pytest.raises(ValueError):
        SlotDecoder(C.FS, coherent=-1)
    ctx = _lib.Context(0)
    assert _lib.lib().ft8_set_coherent(ctx.handle, -1) == _lib.FT8_E_ARG
    # a coherent batch cannot be replayed
    dec = _decoder(coherent=CAP, context=ctx)
    dec.records(d_x)
    with pytest.raises(ValueError):
        ctx.replay("bp")


def test_from_wave_marks_coherent_decodes(gpu, tmp_path, capsys):
    """from_wave --coherent on a weak slot as 16-bit PCM: the decode's block carries a `Coherent:` line with
    the fit's offsets; without the flag the file decodes nothing."""
    import wave
    from ft8_demodulator_amd import from_wave
    x, pays, _ = C.weak_slots()
    pcm = np.clip(np.round(x[0] / 8.0 * 32767.0), -32767, 32767).astype(np.int16)
    path = str(tmp_path / "weak.wav")
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(C.FS)
        w.writeframes(pcm.tobytes())
    opts = ["--max-candidates", "20", "--min-score", "5"]
    res = from_wave.main([path, "--coherent"] + opts)
    out = capsys.readouterr().out
    assert [bytes(r[0].payload) for r in res] == [pays[0]] * len(res) and len(res) >= 1
    assert out.count("Coherent: dt ") == len(res) and " ms, df " in out
    res = from_wave.main([path] + opts)
    out = capsys.readouterr().out
    assert res == [] and "Coherent:" not in out
    res = from_wave.main([path, "--coherent", "1"] + opts)
    assert len(res) <= 1
    capsys.readouterr()
