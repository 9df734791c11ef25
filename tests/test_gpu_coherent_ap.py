"""The a-priori retries on the coherent LLRs on the device (csrc/ap.hip: k_cohap_*, ft8_set_coherent_ap,
ft8_coherent_ap_decode) against the CPU restatement coherent.coherent_ap_restate on the oracle's BP, and the
whole path against a construction from the stage calls' own LLRs: exact, every field."""
import numpy as np
import pytest

import ap_cases as A
import coherent_ap_cases as K
import drift_cases as Dc
import retry_cases as R

pytestmark = pytest.mark.gpu

ITERS = K.ITERS
FS = K.FS


def _L():
    from ft8_demodulator_amd import _lib
    return _lib


@pytest.fixture()
def ctx(gpu):
    """The thread's context; its hypotheses are cleared again after the test."""
    c = _L().context(0)
    yield c
    c.set_ap([])


# ---- the stage call ---------------------------------------------------------------------------------------
PATTERNS = {1: K.ONE_PATTERN, 3: A.STAGE_PATTERNS, 8: K.EIGHT_PATTERNS}
# (n, S, H, limit): n = 1 one wave, 4 a full workgroup, 5 one wave past it, 67 more than a wave of positions;
# "median": the median hard-error count of the same case's rescues without a limit
STAGE = [(1, 1, 3, 174), (1, 3, 8, 174), (4, 2, 3, 174), (4, 3, 1, 174), (5, 2, 1, 174), (5, 3, 8, 174),
         (67, 1, 1, 174), (67, 1, 8, 174), (67, 2, 3, 174), (67, 2, 3, "median"), (67, 3, 3, 174), (67, 3, 8, 174),
         (67, 3, 8, "median")]


def _stage_inputs(n, S):
    """The first n of stage_order(): LLRs [n, S, 174], the records plain BP wrote from set 1 (some ok already),
    and for S > 1 validity bytes cycling through 7 .. 0; at n = 67 one vector with a NaN and one all-zero
    vector among the failed records."""
    idx = list(K.stage_order()[:n])
    llr = np.array(K.stage_llr(S)[idx], copy=True)
    rec = np.array(A.stage_case()["plain"][idx], copy=True)
    valid = None if S == 1 else ((7 - np.arange(n)) % 8).astype(np.uint8)
    if n == 67:
        failed = [i for i in np.nonzero(rec["ok"] == 0)[0] if valid is None or valid[i] == 7]
        llr[failed[0], 0, 100] = np.nan
        llr[failed[1], S - 1] = 0.0
    return llr, rec, valid


def _device_stage(ctx, llr, rec, valid, hyps, limit):
    from ft8_demodulator_amd.ldpc_decoder import coherent_ap_decode_batch
    ctx.set_ap(hyps, limit)
    out, hard = coherent_ap_decode_batch(llr, rec, ITERS, valid)
    assert hard.dtype == np.int16 and len(hard) == len(out) == len(rec)
    return out, hard


@pytest.mark.parametrize("n, S, H, limit", STAGE)
def test_stage_equals_restatement(ctx, oracle, n, S, H, limit):
    llr, rec, valid = _stage_inputs(n, S)
    hyps = K.hyps_of(PATTERNS[H])
    want, want_hard = K.stage_restate(llr, rec, hyps, 174, valid)
    if limit == "median":
        limit = int(np.median(want_hard[want_hard >= 0]))
        free = int((want_hard >= 0).sum())
        want, want_hard = K.stage_restate(llr, rec, hyps, limit, valid)
        assert int((want_hard >= 0).sum()) < free            # the limit rejects what no limit accepts
    pi = want["pass_index"]
    print(f"n {n} S {S} H {H} limit {limit}: ok before {int(rec['ok'].sum())}, rescues {int((pi != 0).sum())}, "
          f"from a later set {int(((pi & 8) != 0).sum())}, hypothesis indices {sorted(set((pi >> 4).tolist()))}")
    if n == 67:
        assert int(rec["ok"].sum()) >= 5 and int((pi != 0).sum()) >= 3 and int((want["ok"] == 0).sum()) >= 5
        assert S == 1 or ((pi & 8) != 0).any()
        assert H < 3 or len(set((pi >> 4).tolist())) >= 3     # no rescue and two hypotheses at least
    out, hard = _device_stage(ctx, llr, rec, valid, hyps, limit)
    A.records_equal(out, want)
    assert np.array_equal(hard, want_hard)


def test_stage_small_cases_retry_something(oracle):
    """On the construction alone: the first records of stage_order() hold a later-set rescue, a rescue at h > 0,
    a record that is ok already and one that nothing rescues."""
    r = K.stage_reference()
    head = list(K.stage_order()[:4])
    pi = r["ref"]["pass_index"][head]
    assert pi[0] & 8 and (pi[1] >> 4) > 1 and r["records"]["ok"][head[2]] == 1 and r["ref"]["ok"][head[3]] == 0


def test_stage_keeps_record_metadata(ctx, oracle):
    """score, slot, abs_time, abs_freq, cand_index and the low bit of pass_index of a rescued record are the
    caller's; d_valid NULL means every set."""
    llr, rec, _ = _stage_inputs(67, 2)
    n = len(rec)
    rec["score"], rec["slot"], rec["abs_time"] = np.arange(n) + 0.5, 7, np.arange(n) - 20
    rec["abs_freq"], rec["cand_index"], rec["pass_index"] = 3 * np.arange(n), np.arange(n), 1
    hyps = K.hyps_of(A.STAGE_PATTERNS)
    want, want_hard = K.stage_restate(llr, rec, hyps, 174)
    assert {0x23, 0x2B} <= set(want["pass_index"].tolist())
    out, hard = _device_stage(ctx, llr, rec, None, hyps, 174)
    A.records_equal(out, want)
    assert np.array_equal(hard, want_hard)


def test_stage_nothing_to_do_and_errors(ctx):
    _lib = _L()
    from ft8_demodulator_amd.ldpc_decoder import coherent_ap_decode_batch
    torch = _lib.require_gpu()
    L, h, st = _lib.lib(), ctx.handle, _lib.stream_handle(0)
    hyps = K.hyps_of(A.STAGE_PATTERNS)
    out, hard = _device_stage(ctx, np.zeros((0, 2, 174)), np.zeros(0, _lib.RESULT_DTYPE), None, hyps, 174)
    assert len(out) == 0 and len(hard) == 0
    ok = np.nonzero(A.stage_case()["plain"]["ok"])[0]
    rec = np.array(A.stage_case()["plain"][ok])
    out, hard = _device_stage(ctx, np.array(K.stage_llr(3)[ok]), rec, None, hyps, 174)
    assert out.tobytes() == rec.tobytes() and (hard == -1).all()
    d_llr = torch.zeros(3 * 174, dtype=torch.float64, device="cuda")
    d_res = torch.zeros(40, dtype=torch.uint8, device="cuda")
    for bad in (0, 4, -1):
        assert L.ft8_coherent_ap_decode(h, _lib.ptr(d_llr), bad, None, _lib.ptr(d_res), 1, ITERS, None, st) == _lib.FT8_E_ARG
    assert L.ft8_coherent_ap_decode(h, None, 1, None, _lib.ptr(d_res), 1, ITERS, None, st) == _lib.FT8_E_ARG
    assert L.ft8_coherent_ap_decode(h, _lib.ptr(d_llr), 3, None, _lib.ptr(d_res), 1, ITERS, None, st) == _lib.FT8_OK
    ctx.set_ap([])                                    # no hypotheses set: refused, also at n = 0
    for n in (1, 0):
        assert L.ft8_coherent_ap_decode(h, _lib.ptr(d_llr), 1, None, _lib.ptr(d_res), n, ITERS, None, st) == _lib.FT8_E_ARG
    with pytest.raises(ValueError, match="ft8_set_ap"):
        coherent_ap_decode_batch(np.zeros((1, 174)), np.zeros(1, _lib.RESULT_DTYPE), ITERS)
    assert L.ft8_abi_version() == 2


# ---- ft8_set_coherent_ap inside ft8_decode_batch ----------------------------------------------------------
E2E, AP, CAP = K.E2E, K.AP, K.CAP


def _decoder(search=E2E, **kw):
    return R.decoder(FS, search, **kw)


def _equal_per_slot(got, want, n_slots=3):
    assert len(got) == n_slots
    for s in range(n_slots):
        A.records_equal(got[s], R.per_slot(want, s))


@pytest.fixture(scope="module")
def e2e(gpu, oracle):
    return K.expectation(K.e2e_slots())


def test_e2e_expectation_shows_every_outcome(e2e):
    """On the expectation alone: a plain decode, a coherent-only rescue, a rescue with bit 1 and a hypothesis index,
    an STFT-AP-only rescue and a listed candidate that nothing rescues; every decode was transmitted, and the CQ
    rescues carry h = 1."""
    o = K.outcomes(e2e)
    print("outcomes", o, "pass_index values", sorted(set(e2e["both"]["pass_index"].tolist())))
    assert all(v >= 1 for v in o.values()), o
    both = e2e["both"]
    sent = K.sent_payloads()
    assert all(bytes(r["payload"]) in sent for r in both[both["ok"] == 1])
    new = both[((both["pass_index"] & 2) != 0) & ((both["pass_index"] >> 4) != 0)]
    assert set((new["pass_index"] >> 4).tolist()) == {2}
    # the stage adds decodes: without it the same candidates stay failed or fall to the STFT retry
    assert int(e2e["both"]["ok"].sum()) >= int(e2e["coherent"]["ok"].sum()) + o["coherent_ap"]


def test_e2e_records_equal_construction(gpu, e2e):
    x = gpu.from_numpy(e2e["x"]).cuda()
    _equal_per_slot(_decoder(coherent=CAP, ap=AP, coherent_ap=True).records(x), e2e["both"])


def test_e2e_pipelined_chunks(gpu, e2e):
    """chunk_slots = 2 over two internal streams splits the three slots: the second chunk's scratch starts at
    slot 2 of every buffer."""
    x = gpu.from_numpy(e2e["x"]).cuda()
    dec = _decoder(coherent=CAP, ap=AP, coherent_ap=True, context=_L().Context(0))
    dec.ctx.set_pipeline(2, 2, 4)
    _equal_per_slot(dec.records(x), e2e["both"])
    dec.ctx.set_pipeline(1, 2, 4)
    _equal_per_slot(dec.records(x), e2e["both"])


def test_e2e_three_sets(gpu, oracle):
    e = K.expectation(K.e2e_slots(), nsym=3)
    o = K.outcomes(e)
    print("outcomes at coherent_nsym 3", o, "pass_index values", sorted(set(e["both"]["pass_index"].tolist())))
    assert o["coherent_ap"] >= 1 and ((e["coherent"]["pass_index"] & 8) != 0).any()
    x = gpu.from_numpy(e["x"]).cuda()
    _equal_per_slot(_decoder(coherent=CAP, ap=AP, coherent_ap=True, coherent_nsym=3).records(x), e["both"])


DRIFT_SEARCH = dict(max_candidates=20, min_score=2)
DRIFT_CAP = 6


def test_e2e_three_sets_and_the_drift_search(gpu, oracle):
    """The drifting slots of the drift tests.  Their payloads are random bits, which no pattern names, so the
    hypotheses know of each drifting signal what "CQ ? ?" knows of a CQ (coherent_ap_cases.payload_hyps).  On the
    expectation: a record with bits 1 and 2 and a hypothesis index."""
    c = Dc.stage_slots_12k()
    hyps = K.payload_hyps([c["payloads"][i] for i in (1, 2, 4, 5, 7, 8)])
    e = K.expectation(c["x"], DRIFT_SEARCH, DRIFT_CAP, hyps, drift=Dc.DRIFT, nsym=3)
    pi = e["both"]["pass_index"]
    print("outcomes with the drift search", K.outcomes(e), "pass_index values", sorted(set(pi.tolist())))
    assert (((pi & 6) == 6) & ((pi >> 4) != 0)).any()
    dec = _decoder(DRIFT_SEARCH, coherent=DRIFT_CAP, ap=["CQ ? ?"] * len(hyps), coherent_ap=True, coherent_nsym=3,
                   coherent_drift=Dc.DRIFT)
    dec.ap_hyps = hyps                                # SlotDecoder takes patterns; these are bits
    _equal_per_slot(dec.records(gpu.from_numpy(e["x"]).cuda()), e["both"])


LATE = dict(max_candidates=100, min_score=2)


def test_e2e_list_fills_in_a_second_round(gpu, oracle):
    """max_candidates 100 and retry_cases.late_cap: the coherent list of one slot fills past its first 64
    candidates, and its attempts take more than one round of the attempt list's scan."""
    e = K.expectation(K.e2e_slots(), LATE, R.late_cap)
    plain = e["plain"]
    s, cap = e["slot"], e["cap"]
    early = int(((plain["slot"] == s) & (plain["ok"] == 0) & (plain["cand_index"] < 64)).sum())
    print("slot", s, "cap", cap, "failed among the first 64", early, "outcomes", K.outcomes(e))
    assert early < cap and cap * len(AP) > 64 and K.outcomes(e)["coherent_ap"] >= 1
    x = gpu.from_numpy(e["x"]).cuda()
    _equal_per_slot(_decoder(LATE, coherent=cap, ap=AP, coherent_ap=True).records(x), e["both"])


def test_setting_argument_checks(gpu, e2e):
    """2 and -1 are FT8_E_ARG and leave the setting as it was, on and off: the next batch's bytes show it."""
    _lib = _L()
    x = gpu.from_numpy(e2e["x"]).cuda()
    off = K.expectation(e2e["x"], coherent_ap=False)["both"]
    assert off.tobytes() != e2e["both"].tobytes()
    for on, want in ((1, e2e["both"]), (0, off)):
        dec = _decoder(coherent=CAP, ap=AP, context=_lib.Context(0))
        assert _lib.lib().ft8_set_coherent_ap(dec.ctx.handle, on) == _lib.FT8_OK
        for bad in (2, -1):
            assert _lib.lib().ft8_set_coherent_ap(dec.ctx.handle, bad) == _lib.FT8_E_ARG
        dec.ctx.set_coherent_ap = lambda *a: None     # SlotDecoder.run sets it before every batch
        _equal_per_slot(dec.records(x), want)
    assert _lib.lib().ft8_set_coherent_ap(None, 1) == _lib.FT8_E_ARG


def test_off_means_off(gpu, e2e):
    """coherent_ap=False, a context whose setter was never called and a context that ran a batch with it on and
    was switched back give the same bytes; on with only one of the two flags gives that flag's bytes."""
    _lib = _L()
    x = gpu.from_numpy(e2e["x"]).cuda()
    never = _decoder(coherent=CAP, ap=AP, context=_lib.Context(0))
    never.ctx.set_coherent_ap = lambda *a: None
    want = never.records(x)
    assert sum(len(r) for r in want) >= 3
    shared = _lib.Context(0)
    on = _decoder(coherent=CAP, ap=AP, coherent_ap=True, context=shared).records(x)
    assert b"".join(r.tobytes() for r in on) != b"".join(r.tobytes() for r in want)
    for got in (_decoder(coherent=CAP, ap=AP, coherent_ap=False, context=_lib.Context(0)).records(x),
                _decoder(coherent=CAP, ap=AP, context=shared).records(x)):
        assert len(got) == 3
        for s in range(3):
            assert got[s].tobytes() == want[s].tobytes()
    for kw in (dict(coherent=CAP), dict(ap=AP)):
        plain_ctx = _decoder(context=_lib.Context(0), **kw).records(x)
        dec = _decoder(context=_lib.Context(0), **kw)
        dec.ctx.set_ap(K.hyps_of(AP), 36)
        dec.ctx.set_coherent_ap(True)
        dec.ctx.set_coherent_ap = lambda *a: None
        got = dec.records(x)
        for s in range(3):
            assert got[s].tobytes() == plain_ctx[s].tobytes()


def _both_marks(r):
    from ft8_demodulator_amd import ap, coherent
    return ap.ap_index(r) > 0 and coherent.coherent_index(r) == 1


def test_messages_and_reports(gpu, e2e):
    x = gpu.from_numpy(e2e["x"]).cuda()
    dec = _decoder(coherent=CAP, ap=AP, coherent_ap=True)
    sent = {"CQ " + c for c in A.E2E_CALLS}
    rows = [r for slot in dec.messages(x, unique=False) for r in slot]
    marked = [r for r in rows if _both_marks(r[4])]
    assert marked and all(r[0] in sent for r in marked)
    reps = [r for slot in dec.reports(x, unique=False) for r in slot]
    assert [r[0] for r in reps] == [r[0] for r in rows]
    assert all(np.isfinite(r[1]) for r in reps if _both_marks(r[5]))


def test_from_wave_prints_both_marks(gpu, tmp_path, capsys):
    """from_wave --ap ... --coherent 8 --coherent-ap on slot 0 as 16-bit PCM: a record with both marks prints its
    `AP:` line and its `Coherent:` line, and the blocks are the decoder's records."""
    import wave
    from ft8_demodulator_amd import _lib, from_wave
    pcm = np.clip(np.round(K.e2e_slots()[0] / 8.0 * 32767.0), -32767, 32767).astype(np.int16)
    path = str(tmp_path / "slot.wav")
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(FS)
        w.writeframes(pcm.tobytes())
    recs = _decoder(coherent=CAP, ap=AP, coherent_ap=True).records(gpu.from_numpy(pcm).cuda().unsqueeze(0),
                                                                   code=_lib.FT8_I16)[0]
    n_both = sum(_both_marks(r) for r in recs)
    assert 1 <= n_both < len(recs)
    argv = [path, "--selection", "topk", "--max-candidates", "40", "--min-score", "2", "--text", "--coherent", str(CAP)]
    for p in AP:
        argv += ["--ap", p]
    res = from_wave.main(argv + ["--coherent-ap"])
    out = capsys.readouterr().out
    assert [bytes(r[0].payload) for r in res] == [bytes(r["payload"]) for r in recs]
    blocks = [b for b in out.split("-" * 50) if "AP: " in b and "Coherent: " in b]
    assert len(blocks) == n_both
    sent = {"CQ " + c for c in A.E2E_CALLS}
    assert all("AP: CQ ? ?\n" in b and b.split("Message: ")[1].split("\n")[0] in sent for b in blocks)
    from_wave.main(argv)
    out = capsys.readouterr().out
    assert not [b for b in out.split("-" * 50) if "AP: " in b and "Coherent: " in b]


def test_under_subtraction(gpu, e2e):
    """subtract=2: per slot the first pass_counts()[:, 0] rows are the rows of the same decoder without subtract
    (acc_1 = R_1), and every row of the batch carries a transmitted payload."""
    x = gpu.from_numpy(e2e["x"]).cuda()
    kw = dict(coherent=CAP, ap=AP, coherent_ap=True)
    one = _decoder(**kw).records(x)
    dec = _decoder(subtract=2, **kw)
    rows = dec.records(x)
    pc = dec.pass_counts()
    sent = K.sent_payloads()
    for s in range(3):
        n1 = int(pc[s, 0])
        assert n1 == len(one[s]) and rows[s][:n1].tobytes() == one[s].tobytes()
        assert all(bytes(r["payload"]) in sent for r in rows[s])
    assert any(_both_marks(r) for s in range(3) for r in rows[s])
    print("rows after pass 1 and 2 per slot", pc.tolist())


def test_gain_on_the_weak_cq_slots(gpu):
    """32 one-signal CQ slots at coherent_ap_cases.WEAK_SNR_DB with coherent=True, ap "CQ ? ?" and coherent_nsym=3:
    what coherent_ap=True decodes includes all that False decodes, nothing decoded was not transmitted, and True
    decodes at least one more slot."""
    x, pays = K.weak_cq_slots()
    d_x = gpu.from_numpy(np.array(x)).cuda()
    kw = dict(coherent=True, ap=["CQ ? ?"], coherent_nsym=3)
    r0 = R.decoder(FS, dict(max_candidates=20, min_score=2), **kw).records(d_x)
    r1 = R.decoder(FS, dict(max_candidates=20, min_score=2), coherent_ap=True, **kw).records(d_x)
    n0 = n1 = 0
    for s in range(K.N_WEAK):
        p0, p1 = {bytes(v["payload"]) for v in r0[s]}, {bytes(v["payload"]) for v in r1[s]}
        assert p0 <= {pays[s]} and p1 <= {pays[s]}, (s, "a payload that was not transmitted")
        assert p0 <= p1, s
        n0 += len(p0)
        n1 += len(p1)
    print("slots decoded with coherent_ap off:", n0, "on:", n1, "of", K.N_WEAK)
    assert n1 >= n0 + 1
