"""Ordered-statistics decoding on the device (csrc/osd.hip: ft8_set_osd, ft8_osd_decode, FT8_FLAG_OSD) against
the CPU restatement osd.osd_pass_restate on the oracle's decode tail: exact, every field, no tolerance."""
import ctypes

import numpy as np
import pytest

import ap_cases as A
import osd_cases as C
import retry_cases as R

pytestmark = pytest.mark.gpu

FS = A.E2E_FS
E2E = dict(max_candidates=40, min_score=2)
E2E_LATE = dict(max_candidates=80, min_score=2)   # more candidates than the list kernel scans in a round
OSD = (2, 32)
AP = ["CQ ? ?"]
COHERENT = 8


def _L():
    from ft8_demodulator_amd import _lib
    return _lib


@pytest.fixture()
def ctx(gpu):
    """The thread's context; its OSD setting is the default again after the test."""
    c = _L().context(0)
    yield c
    c.set_osd(2, 0, 36)


# ---- ft8_osd_decode ------------------------------------------------------------------------------------
def _stage(ctx, order, max_hard=174):
    from ft8_demodulator_amd.ldpc_decoder import osd_decode_batch
    llr, rec = C.all_vectors()
    ctx.set_osd(order, 0, max_hard)
    return osd_decode_batch(np.array(llr, copy=True), np.array(rec, copy=True))


@pytest.mark.parametrize("order", C.ORDERS)
def test_stage_equals_restatement(ctx, oracle, order):
    """The 67 stage vectors (one more than a wave) and the 9 edge vectors: records, ft8_osd_rec and codewords."""
    want, want_info, want_cw = C.expected(order)
    out, info, cw = _stage(ctx, order)
    assert info.dtype == _L().OSD_DTYPE and cw.shape == (len(want), 22)
    for f in info.dtype.names:
        bad = np.nonzero((info[f] != want_info[f]).reshape(len(info), -1).any(axis=1))[0]
        assert bad.size == 0, (f, bad.tolist(), info[f][bad].tolist(), want_info[f][bad].tolist())
    assert np.array_equal(cw, want_cw)
    A.records_equal(out, want)
    assert len(C.rescued(out[:C.STAGE_N], C.stage_vectors()["plain"])) == {0: 2, 1: 7, 2: 26}[order]


def test_stage_hard_error_limit(ctx, oracle):
    want, want_info, want_cw = C.expected(2, 20)
    assert 0 < int((want_info["status"] == 0).sum()) < int((C.expected(2)[1]["status"] == 0).sum())
    out, info, cw = _stage(ctx, 2, 20)
    assert info.tobytes() == want_info.tobytes() and np.array_equal(cw, want_cw)
    A.records_equal(out, want)


def test_stage_nothing_to_do_and_null_outputs(ctx, oracle):
    _lib = _L()
    from ft8_demodulator_amd.ldpc_decoder import osd_decode_batch
    out, info, cw = osd_decode_batch(np.zeros((0, 174)), np.zeros(0, dtype=_lib.RESULT_DTYPE))
    assert len(out) == 0 and len(info) == 0 and len(cw) == 0
    # d_info and d_codeword are optional
    torch = _lib.require_gpu()
    llr, rec = C.all_vectors()
    ctx.set_osd(1, 0, 174)
    d_llr = torch.from_numpy(np.array(llr, copy=True)).cuda()
    d_res = torch.from_numpy(np.array(rec, copy=True).view(np.uint8)).cuda()
    rc = _lib.lib().ft8_osd_decode(ctx.handle, _lib.ptr(d_llr), _lib.ptr(d_res), len(rec), None, None,
                                   _lib.stream_handle(0))
    assert rc == _lib.FT8_OK
    A.records_equal(d_res.cpu().numpy().view(_lib.RESULT_DTYPE), C.expected(1)[0])


def test_set_osd_argument_checks(ctx):
    _lib = _L()
    L, h = _lib.lib(), ctx.handle
    for bad in ((-1, 0, 36), (3, 0, 36), (2, -1, 36), (2, 0, -1), (2, 0, 175)):
        assert L.ft8_set_osd(h, *bad) == _lib.FT8_E_ARG
    for good in ((0, 0, 0), (2, 4096, 174), (1, 7, 36)):
        assert L.ft8_set_osd(h, *good) == _lib.FT8_OK
    torch = _lib.require_gpu()
    d = torch.zeros(174, dtype=torch.float64, device="cuda")
    assert L.ft8_osd_decode(h, _lib.ptr(d), None, 1, None, None, _lib.stream_handle(0)) == _lib.FT8_E_ARG
    assert L.ft8_osd_decode(h, _lib.ptr(d), _lib.ptr(d), -1, None, None, _lib.stream_handle(0)) == _lib.FT8_E_ARG
    assert L.ft8_abi_version() == 2


# ---- FT8_FLAG_OSD inside ft8_decode_batch ---------------------------------------------------------------
def _osd_pass(llr, rec, order, cap, max_hard=36):
    """The pass on the host: osd_pass_restate on each slot's first `cap` (0: all) records still failed."""
    from ft8_demodulator_amd import osd
    listed = osd.retry_list(rec, cap or None)
    out = np.array(rec, copy=True)
    out[listed] = osd.osd_pass_restate(llr[listed], rec[listed], order, max_hard, A.oracle_lib().decode_tail)[0]
    out.setflags(write=False)
    return out, listed


def _expectation(x, search, osd_opt, **retries):
    """As retry_cases.expectation builds it: the device's stage calls give the LLRs, the oracle's BP the plain
    records, the other retries' restatements what they leave (retries: cap= / ap= of R.expectation), and
    osd_pass_restate is applied last.  osd_opt: (order, cap) or a function of the plain records -> (slot, cap)."""
    x = np.array(x)
    llr, rows, plain = R.stage_records(x, FS, search["max_candidates"], search["min_score"], _L().FT8_FLAG_TOPK)
    before, slot = plain, None
    if retries:
        e = R.expectation(x, FS, search, **retries)
        A.records_equal(e["plain"], plain)
        before = e["both"] if retries.get("ap") else e["coherent"]
    if callable(osd_opt):
        slot, cap = osd_opt(plain)
        osd_opt = (OSD[0], cap)
    after, listed = _osd_pass(llr, before, *osd_opt)
    return {"x": x, "plain": plain, "before": before, "after": after, "listed": listed, "osd": osd_opt, "slot": slot}


def _three_slots():
    x = A.e2e_samples()
    return np.stack([x[0], x[1], x[0]])


@pytest.fixture(scope="module")
def e2e(gpu, oracle):
    return _expectation(A.e2e_samples(), E2E, OSD)


@pytest.fixture(scope="module")
def e2e_late(gpu, oracle):
    return _expectation(_three_slots(), E2E_LATE, R.late_cap)


def _decoder(search=E2E, **kw):
    return R.decoder(FS, search, **kw)


def _check(got, e, n_slots):
    assert len(got) == n_slots
    for s in range(n_slots):
        A.records_equal(got[s], R.per_slot(e["after"], s))


def test_e2e_expectation_shows_every_outcome(e2e):
    """On the expectation alone: at least three OSD records, true payloads only, one of them a message plain
    decoding did not produce; the noise slot returns nothing."""
    from ft8_demodulator_amd import osd
    sent = {bytes(p) for p in A.e2e_payloads()}
    recs = R.per_slot(e2e["after"], 0)
    by_osd = [r for r in recs if osd.osd_index(r)]
    assert len(by_osd) >= 3 and all(bytes(r["payload"]) in sent for r in by_osd)
    assert {bytes(r["payload"]) for r in by_osd} - {bytes(r["payload"]) for r in R.per_slot(e2e["plain"], 0)}
    assert len(R.per_slot(e2e["plain"], 0)) >= 1 and len(R.per_slot(e2e["after"], 1)) == 0
    assert int((e2e["after"]["ok"] == 0).sum()) >= 1


def test_e2e_records_equal_expectation(gpu, e2e):
    from ft8_demodulator_amd import osd
    x = gpu.from_numpy(e2e["x"]).cuda()
    got = _decoder(osd=OSD).records(x)
    _check(got, e2e, 2)
    assert len(got[1]) == 0 and sum(osd.osd_index(r) for r in got[0]) >= 3
    # the same decoder without osd: exactly the records plain BP decoded
    plain = _decoder().records(x)
    for s in range(2):
        A.records_equal(plain[s], R.per_slot(e2e["plain"], s))


def test_late_cap_expectation_fills_the_list_in_the_second_round(e2e_late):
    plain, s, cap = e2e_late["plain"], e2e_late["slot"], e2e_late["osd"][1]
    mine = plain[plain["slot"] == s]
    failed = mine["cand_index"][mine["ok"] == 0]
    assert len(mine) > 64 and int((failed < 64).sum()) < cap < len(failed)
    listed = [i for i in e2e_late["listed"] if plain["slot"][i] == s]
    assert len(listed) == cap and plain["cand_index"][listed[-1]] >= 64


def test_late_cap_and_pipelined_chunks(gpu, e2e_late):
    """max_candidates 80 and the cap past the list kernel's first round of 64; then one slot per chunk over two
    internal streams on three slots (signals, noise, signals), where a wrong chunk offset would show."""
    x = gpu.from_numpy(e2e_late["x"]).cuda()
    one = _decoder(E2E_LATE, osd=e2e_late["osd"])
    piped = _decoder(E2E_LATE, osd=e2e_late["osd"], context=_L().Context(0))
    piped.ctx.set_pipeline(1, 2, 4)
    for dec in (one, piped):
        got = dec.records(x)
        _check(got, e2e_late, 3)
        assert len(got[1]) == 0 and len(got[0]) == len(got[2]) >= 3


def test_e2e_after_ap_and_coherent(gpu, oracle):
    """With the a-priori and the coherent pass both on, OSD sees only what they left."""
    from ft8_demodulator_amd import ap, coherent, osd
    e = _expectation(A.e2e_samples(), E2E, OSD, cap=COHERENT, ap=AP)
    assert int((e["before"]["ok"] == 1).sum()) > int((e["plain"]["ok"] == 1).sum())
    assert all(e["before"]["ok"][i] == 0 for i in e["listed"])
    x = gpu.from_numpy(e["x"]).cuda()
    got = _decoder(osd=OSD, ap=AP, coherent=COHERENT).records(x)
    _check(got, e, 2)
    assert all(ap.ap_index(r) == 0 and not coherent.coherent_index(r) for r in got[0] if osd.osd_index(r))


def test_with_subtraction(gpu, e2e):
    """FT8_FLAG_SUBTRACT | FT8_FLAG_OSD is refused unless the subtraction runs the retries; then pass 1's rows
    are the batch's without subtraction."""
    _lib = _L()
    x = gpu.from_numpy(e2e["x"]).cuda()
    with pytest.raises(NotImplementedError, match="FT8_FLAG_OSD with FT8_FLAG_SUBTRACT"):
        _decoder(osd=OSD, flags=_lib.FT8_FLAG_TOPK | _lib.FT8_FLAG_SUBTRACT).records(x)
    got = _decoder(osd=OSD, subtract=2).records(x)
    for s in range(2):
        A.records_equal(got[s][(got[s]["pass_index"] & 1) == 0], R.per_slot(e2e["after"], s))
    assert len(got[1]) == 0


def test_flag_clear_ignores_the_setting(gpu, e2e):
    """A context on which ft8_set_osd was called, in a batch without the flag: the fresh context's bytes."""
    x = gpu.from_numpy(e2e["x"]).cuda()
    fresh, touched = _decoder(context=_L().Context(0)), _decoder(context=_L().Context(0))
    touched.ctx.set_osd(1, 5, 20)
    a, ca = fresh.run(x)
    a, ca = a.cpu().numpy().copy(), ca.cpu().numpy().copy()
    b, cb = touched.run(x)
    assert np.array_equal(ca, cb.cpu().numpy())
    n = 2 * fresh.cap * _L().RESULT_DTYPE.itemsize
    rows = [slice(s * fresh.cap * 40, (s * fresh.cap + int(ca[s])) * 40) for s in range(2)]
    b = b.cpu().numpy()
    assert all(a[:n][r].tobytes() == b[:n][r].tobytes() for r in rows)
    touched.ctx.replay("bp")      # and such a batch can still be replayed


def test_replay_refuses_after_an_osd_batch(gpu, e2e):
    x = gpu.from_numpy(e2e["x"]).cuda()
    dec = _decoder(osd=OSD, context=_L().Context(0))
    dec.records(x)
    with pytest.raises(ValueError):
        dec.ctx.replay("bp")


def test_from_wave_marks_osd_decodes(gpu, tmp_path, capsys):
    """from_wave --osd on slot 0 as 16-bit PCM: every block of an OSD decode carries `OSD: order 2` and no
    `AP:` line, and the blocks are the decoder's records."""
    import wave
    from ft8_demodulator_amd import _lib, from_wave, osd
    from ft8_demodulator_amd._pipeline import SlotDecoder
    pcm = np.clip(np.round(A.e2e_samples()[0] / 8.0 * 32767.0), -32767, 32767).astype(np.int16)
    path = str(tmp_path / "slot.wav")
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(FS)
        w.writeframes(pcm.tobytes())
    opts = ["--max-candidates", "40", "--min-score", "5"]
    recs = SlotDecoder(FS, max_candidates=40, min_score=5.0, osd=True, ap=AP).records(
        gpu.from_numpy(pcm).cuda().unsqueeze(0), code=_lib.FT8_I16)[0]
    n_osd = sum(osd.osd_index(r) for r in recs)
    assert 1 <= n_osd < len(recs)
    res = from_wave.main([path, "--osd", "--ap", AP[0]] + opts)
    out = capsys.readouterr().out
    assert [bytes(r[0].payload) for r in res] == [bytes(r["payload"]) for r in recs]
    assert out.count("OSD: order 2") == n_osd
    assert all("AP: " not in b for b in out.split("-" * 50) if "OSD: " in b)
