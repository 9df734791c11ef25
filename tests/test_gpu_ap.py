"""A-priori decoding on the device (csrc/ap.hip around the unchanged k_bp: ft8_set_ap, ft8_ap_decode,
FT8_FLAG_AP) against the CPU restatement ap.ap_restate on the oracle's BP: exact, every field."""
import ctypes

import numpy as np
import pytest

import ap_cases as C
import retry_cases as R

pytestmark = pytest.mark.gpu

ITERS = C.ITERS


def _L():
    from ft8_demodulator_amd import _lib
    return _lib


@pytest.fixture()
def ctx(gpu):
    """The thread's context; its hypotheses are cleared again after the test."""
    c = _L().context(0)
    yield c
    c.set_ap([])


def _stage(ctx, llr, hyps, max_hard, records=None):
    """ft8_bp, then ft8_ap_decode with hyps -> (plain-BP records, AP records, hard)."""
    from ft8_demodulator_amd import _device
    from ft8_demodulator_amd.ldpc_decoder import ap_decode_batch
    ctx.set_ap(hyps, max_hard)
    llr = np.array(llr, copy=True)   # the shared cases are read-only
    rec0 = _device.bp(llr, ITERS)[1] if records is None else records
    out, hard = ap_decode_batch(llr, rec0, ITERS)
    assert hard.dtype == np.int16
    return rec0, out, hard


def test_stage_equals_restatement(ctx, oracle):
    """67 vectors in three groups, three hypotheses of which the first matches nothing: every field of
    every record and d_hard equal the restatement's, without a hard-error limit and at the median
    hard-error count of the reference's rescues."""
    c = C.stage_case()
    idx = c["ref"]["pass_index"] >> 4
    rescued = np.nonzero(idx > 0)[0]
    # what the seed was picked for, on the reference alone
    assert int(c["plain"]["ok"].sum()) >= 5 and len(rescued) >= 5 and int((idx == 3).sum()) >= 3
    assert int((c["ref"]["ok"] == 0).sum()) >= 5
    rec0, out, hard = _stage(ctx, c["llr"], c["hyps"], 174)
    C.records_equal(rec0, c["plain"])
    C.records_equal(out, c["ref"])
    assert np.array_equal(hard, c["hard"])
    med = int(np.median(c["hard"][rescued]))
    want, want_hard = C.restate(c["llr"], c["plain"], c["hyps"], med)
    assert 1 <= int((want_hard >= 0).sum()) < len(rescued)      # the limit accepts some and rejects some
    _, out, hard = _stage(ctx, c["llr"], c["hyps"], med)
    C.records_equal(out, want)
    assert np.array_equal(hard, want_hard)


def test_stage_keeps_record_metadata(ctx, oracle):
    """score, slot, abs_time, abs_freq, cand_index and the low nibble of pass_index of a rescued record
    are the caller's."""
    c = C.stage_case()
    rec = np.array(c["plain"], copy=True)
    n = len(rec)
    rec["score"], rec["slot"], rec["abs_time"] = np.arange(n) + 0.5, 7, np.arange(n) - 20
    rec["abs_freq"], rec["cand_index"], rec["pass_index"] = 3 * np.arange(n), np.arange(n), 1
    want, want_hard = C.restate(c["llr"], rec, c["hyps"], 174)
    assert set(want["pass_index"].tolist()) == {1, 0x21, 0x31}
    _, out, hard = _stage(ctx, c["llr"], c["hyps"], 174, records=rec)
    C.records_equal(out, want)
    assert np.array_equal(hard, want_hard)


def test_stage_single_hypothesis(ctx, oracle):
    c = C.stage_case()
    hyps = c["hyps"][2:]
    want, want_hard = C.restate(c["llr"], c["plain"], hyps, 174)
    assert set(want["pass_index"].tolist()) == {0, 0x10}
    _, out, hard = _stage(ctx, c["llr"], hyps, 174)
    C.records_equal(out, want)
    assert np.array_equal(hard, want_hard)


def test_stage_nothing_to_do(ctx, oracle):
    """n = 0, and a batch whose records are all ok already."""
    c = C.stage_case()
    _, out, hard = _stage(ctx, np.zeros((0, 174)), c["hyps"], 174)
    assert len(out) == 0 and len(hard) == 0
    ok = np.nonzero(c["plain"]["ok"])[0]
    rec0, out, hard = _stage(ctx, c["llr"][ok], c["hyps"], 174)
    assert rec0["ok"].all()
    C.records_equal(out, c["plain"][ok])
    assert np.all(hard == -1)


def test_stage_nan_and_zero_vectors(ctx, oracle):
    """An all-NaN vector, a vector with one NaN and an all-zero vector (a = NaN, NaN, 0) keep the
    records plain BP wrote, also when those say ok = 0; their neighbours are decoded as ever."""
    c = C.stage_case()
    failed = np.nonzero(c["plain"]["ok"] == 0)[0][:6]
    llr = np.array(c["llr"][failed], copy=True)
    llr[1] = np.nan
    llr[3, 100] = np.nan
    llr[4] = 0.0
    rec0 = C.plain_records(llr)
    rec0["ok"][4] = 0      # the zero vector is the zero codeword, which plain BP decodes: force the retry
    want, want_hard = C.restate(llr, rec0, c["hyps"], 174)
    assert np.all(want_hard[[1, 3, 4]] == -1) and np.any(want_hard >= 0)
    for i in (1, 3, 4):
        assert want[i].tobytes() == rec0[i].tobytes()
    gpu_rec0, out, hard = _stage(ctx, llr, c["hyps"], 174, records=rec0)
    C.records_equal(out, want)
    assert np.array_equal(hard, want_hard)


def test_set_ap_argument_checks(ctx):
    _lib = _L()
    L, h = _lib.lib(), ctx.handle
    good = np.zeros(9, dtype=_lib.AP_HYP_DTYPE)
    p = good.ctypes.data_as(ctypes.c_void_p)
    assert L.ft8_set_ap(h, p, 9, 174) == _lib.FT8_E_RANGE
    assert L.ft8_set_ap(h, p, 8, 174) == _lib.FT8_OK
    assert L.ft8_set_ap(h, p, 1, 175) == _lib.FT8_E_ARG and L.ft8_set_ap(h, p, 1, -1) == _lib.FT8_E_ARG
    assert L.ft8_set_ap(h, None, 1, 174) == _lib.FT8_E_ARG and L.ft8_set_ap(h, p, -1, 174) == _lib.FT8_E_ARG
    for field in ("mask", "value"):
        bad = np.zeros(2, dtype=_lib.AP_HYP_DTYPE)
        bad[field][1, 9] = 0x04          # bit 77
        assert L.ft8_set_ap(h, bad.ctypes.data_as(ctypes.c_void_p), 2, 174) == _lib.FT8_E_ARG
    # no hypotheses set: the stage call refuses
    assert L.ft8_set_ap(h, None, 0, 174) == _lib.FT8_OK
    torch = _lib.require_gpu()
    d_llr = torch.zeros(174, dtype=torch.float64, device="cuda")
    d_res = torch.zeros(40, dtype=torch.uint8, device="cuda")
    assert L.ft8_ap_decode(h, _lib.ptr(d_llr), _lib.ptr(d_res), 1, ITERS, None, _lib.stream_handle(0)) == _lib.FT8_E_ARG
    assert L.ft8_abi_version() == 2


# ---- FT8_FLAG_AP inside ft8_decode_batch ---------------------------------------------------------------
E2E = dict(max_candidates=40, min_score=2)
AP = ["CQ ? ?"]


def _flags():
    # min_score = 2 lets thousands of noise points pass, and the reference selection keeps the first 40
    # of them in scan order (the time rows before the slot starts) plus one running maximum, so no
    # slot with several weak signals reaches BP through it: the candidates are the 40 highest scores
    return _L().FT8_FLAG_TOPK


@pytest.fixture(scope="module")
def e2e(gpu, oracle):
    """The expectation, from the device's own LLRs (retry_cases.expectation without a coherent pass) -> per
    slot the records the AP batch must return (read-only), and all records of every candidate."""
    e = R.expectation(C.e2e_samples(), C.E2E_FS, E2E, ap=AP)
    return {"all": e["both"], "plain": e["plain"], "per_slot": [R.per_slot(e["both"], s) for s in range(2)]}


def _decoder(**kw):
    return R.decoder(C.E2E_FS, E2E, **kw)


def test_e2e_expectation_shows_every_outcome(e2e):
    from ft8_demodulator_amd import ap
    sent = {bytes(p) for p in C.e2e_payloads()}
    recs = e2e["per_slot"][0]
    idx = np.array([ap.ap_index(r) for r in recs])
    assert int((idx == 0).sum()) >= 1
    assert sum(bytes(r["payload"]) in sent for r in recs[idx == 1]) >= 2
    assert int((e2e["all"]["ok"] == 0).sum()) >= 1
    # the AP decodes bring messages no plain decode of the slot carries
    assert {bytes(r["payload"]) for r in recs[idx == 1]} - {bytes(r["payload"]) for r in recs[idx == 0]}


def test_e2e_records_equal_expectation(gpu, e2e):
    from ft8_demodulator_amd import ap
    x = gpu.from_numpy(np.array(C.e2e_samples())).cuda()
    got = _decoder(ap=AP).records(x)
    assert len(got) == 2
    for s in range(2):
        C.records_equal(got[s], e2e["per_slot"][s])
    # the same decoder without ap: exactly the records plain BP decoded
    plain = _decoder().records(x)
    for s in range(2):
        keep = np.array([ap.ap_index(r) == 0 for r in got[s]], dtype=bool)
        C.records_equal(plain[s], got[s][keep])
        C.records_equal(plain[s], e2e["plain"][(e2e["plain"]["slot"] == s) & (e2e["plain"]["ok"] == 1)])


def test_e2e_pipelined_chunks(gpu, e2e):
    """One slot per chunk over two internal streams, the signals in the second chunk: each chunk's AP
    pass works on its own part of the scratch and gives the single chain's records."""
    x = gpu.from_numpy(np.array(C.e2e_samples()[::-1])).cuda()
    dec = _decoder(ap=AP, context=_L().Context(0))
    dec.ctx.set_pipeline(1, 2, 4)
    got = dec.records(x)
    want = np.array(e2e["per_slot"][0], copy=True)
    want["slot"] = 1
    C.records_equal(got[1], want)
    assert len(got[0]) == len(e2e["per_slot"][1])


def test_e2e_messages_and_reports(gpu, e2e):
    """unpack77 and the signal report run on an AP batch unchanged: the AP rows carry the transmitted text."""
    from ft8_demodulator_amd import ap
    x = gpu.from_numpy(np.array(C.e2e_samples())).cuda()
    dec = _decoder(ap=AP)
    sent = {"CQ " + c for c in C.E2E_CALLS}
    rows = dec.messages(x, unique=False)[0]
    assert len(rows) == len(e2e["per_slot"][0])
    ap_rows = [r for r in rows if ap.ap_index(r[4]) == 1]
    assert len(ap_rows) >= 2 and all(r[0] in sent for r in ap_rows)
    reps = dec.reports(x, unique=False)[0]
    assert [r[0] for r in reps] == [r[0] for r in rows]
    assert all(np.isfinite(r[1]) and -30.0 < r[1] < 0.0 for r in reps if ap.ap_index(r[5]) == 1)


def test_e2e_flag_errors(gpu):
    _lib = _L()
    x = gpu.from_numpy(np.array(C.e2e_samples())).cuda()
    with pytest.raises(NotImplementedError, match="FT8_FLAG_SUBTRACT"):
        _decoder(ap=AP, flags=_flags() | _lib.FT8_FLAG_SUBTRACT).records(x)
    # the flag without hypotheses on the context
    bare = _decoder(flags=_flags() | _lib.FT8_FLAG_AP, context=_lib.Context(0))
    with pytest.raises(ValueError, match="ft8_set_ap"):
        bare.records(x)
    # an AP batch cannot be replayed
    dec = _decoder(ap=AP, context=_lib.Context(0))
    dec.records(x)
    with pytest.raises(ValueError):
        dec.ctx.replay("bp")
    with pytest.raises(ValueError):
        _decoder(ap=["CQ ? ?"] * 9)


def test_from_wave_marks_ap_decodes(gpu, tmp_path, capsys):
    """from_wave --ap on slot 0 as 16-bit PCM: every a-priori decode's block carries `AP: <pattern>`,
    the blocks are the decoder's records, and without --ap the same file gives the plain decodes only."""
    import wave
    from ft8_demodulator_amd import _lib, ap, from_wave
    from ft8_demodulator_amd._pipeline import SlotDecoder
    pcm = np.clip(np.round(C.e2e_samples()[0] / 8.0 * 32767.0), -32767, 32767).astype(np.int16)
    path = str(tmp_path / "slot.wav")
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(C.E2E_FS)
        w.writeframes(pcm.tobytes())
    # min_score 5 keeps fewer than 40 candidates, so the reference selection drops none of them
    opts = ["--max-candidates", "40", "--min-score", "5", "--text"]
    recs = SlotDecoder(C.E2E_FS, max_candidates=40, min_score=5.0, ap=AP).records(
        gpu.from_numpy(pcm).cuda().unsqueeze(0), code=_lib.FT8_I16)[0]
    n_ap = sum(ap.ap_index(r) > 0 for r in recs)
    assert n_ap >= 2 and n_ap < len(recs)
    res = from_wave.main([path, "--ap", AP[0]] + opts)
    out = capsys.readouterr().out
    assert [bytes(r[0].payload) for r in res] == [bytes(r["payload"]) for r in recs]
    assert out.count("AP: CQ ? ?") == n_ap and out.count("Message: CQ ") >= n_ap
    blocks = [b for b in out.split("-" * 50) if "AP: " in b]
    sent = {"CQ " + c for c in C.E2E_CALLS}
    assert len(blocks) == n_ap and all(b.split("Message: ")[1].split("\n")[0] in sent for b in blocks)
    res = from_wave.main([path] + opts)
    out = capsys.readouterr().out
    assert "AP: " not in out and len(res) == len(recs) - n_ap
