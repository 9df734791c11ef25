"""The float32 decoder on the device (csrc/bp32.hip: ft8_bp_f32, FT8_FLAG_BP_F32) against its NumPy
restatement bp32.bp32_restate: bit for bit, every field, as a stage call and through every BP launch of a
batch (main pass, a-priori, coherent, FT4, subtraction)."""
import numpy as np
import pytest

import ap_cases as A
import bp32_cases as C
import coherent_cases as CC
import ft4_cases as F4
import retry_cases as R

pytestmark = pytest.mark.gpu

ITERS = A.ITERS


def _L():
    from ft8_demodulator_amd import _lib
    return _lib


def _bp(ctx, llr, iters, f32=True):
    """ft8_bp_f32 (or ft8_bp) on the context ctx -> (plain, records)."""
    _lib = _L()
    torch = _lib.require_gpu()
    a = torch.from_numpy(np.array(llr, dtype=np.float64).reshape(-1, 174)).cuda()   # a copy: the cases are read-only
    n = a.shape[0]
    plain = torch.zeros(n, 174, dtype=torch.uint8, device="cuda")
    res = torch.zeros(n * _lib.RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    call = _lib.lib().ft8_bp_f32 if f32 else _lib.lib().ft8_bp
    ctx.check(call(ctx.handle, _lib.ptr(a), n, int(iters), _lib.ptr(plain), _lib.ptr(res), _lib.stream_handle(0)), "bp")
    return plain.cpu().numpy(), res.cpu().numpy().view(_lib.RESULT_DTYPE)


def _records32(plain, err, base=None):
    """The records k_bp32 writes for the restatement's (plain, errors): the oracle's tail on them; score, slot,
    abs_time, abs_freq and cand_index are `base`'s (0 without)."""
    O = A.oracle_lib()
    rec = np.zeros(len(plain), dtype=_L().RESULT_DTYPE) if base is None else np.array(base, copy=True)
    for i in range(len(plain)):
        ok, pay, ce, cc = O.decode_tail(plain[i], int(err[i]))
        rec["ldpc_errors"][i], rec["crc_extracted"][i], rec["crc_calculated"][i], rec["ok"][i] = err[i], ce, cc, ok
        rec["payload"][i] = np.frombuffer(pay, dtype=np.uint8)
        rec["pass_index"][i] = 0
    return rec


def _bp32(x, iters):
    from ft8_demodulator_amd import bp32
    return bp32.bp_decode_f32(x, iters)


# ---- the flag and the stage call exist ------------------------------------------------------------------
def test_flag_is_accepted_and_stage_call_exists(gpu):
    """Without the feature: FT8_E_ARG "unknown bits in ft8_params.flags", and no ft8_bp_f32."""
    _lib = _L()
    assert _lib.FT8_FLAG_BP_F32 == 32 and _lib.lib().ft8_abi_version() == 2
    assert hasattr(_lib.lib(), "ft8_bp_f32")
    x = gpu.from_numpy(np.array(A.e2e_samples())).cuda()
    dec = R.decoder(A.E2E_FS, dict(max_candidates=40, min_score=2), flags=_lib.FT8_FLAG_TOPK | _lib.FT8_FLAG_BP_F32)
    out, counts = dec.run(x)                       # raises unless FT8_OK
    assert int(counts.sum()) >= 1
    ctx = _lib.Context(0)
    st = _lib.stream_handle(0)
    assert _lib.lib().ft8_bp_f32(ctx.handle, None, 1, ITERS, None, None, st) == _lib.FT8_E_ARG
    assert _lib.lib().ft8_bp_f32(ctx.handle, None, 0, ITERS, None, None, st) == _lib.FT8_OK
    assert _lib.lib().ft8_bp_f32(None, None, 0, ITERS, None, None, st) == _lib.FT8_E_ARG


# ---- the stage call, bit for bit --------------------------------------------------------------------------
@pytest.mark.parametrize("iters", [1, 2, 20, 50])
@pytest.mark.parametrize("n", [1, 2, 3, 129])
def test_stage_equals_restatement(gpu, oracle, n, iters):
    llr = C.stage_pool()[0][:n]
    plain, err, it = C.stage_expect(n, iters)
    ctx = _L().Context(0)
    ctx.set_timing(True, stages=[])     # allocates the work counters (and runs the kernel's clock path)
    ctx.counters(reset=True)
    got_plain, got = _bp(ctx, llr, iters)
    assert np.array_equal(got_plain, plain), np.nonzero((got_plain != plain).any(axis=1))[0].tolist()
    A.records_equal(got, _records32(plain, err))
    cnt = ctx.counters()
    want = {"candidates": n, "iterations": int(it.sum()), "passes": int(np.maximum(it - 1, 0).sum()),
            "converged": int((err == 0).sum())}
    assert cnt == want, (cnt, want)
    if n == 129 and iters >= 20:   # the pool decodes both ways
        assert 20 < want["converged"] < 110 and int(got["ok"].sum()) >= 20


def test_stage_more_items_than_resident_waves(gpu, oracle):
    """bp_waves_per_simd = 1 makes the persistent grid 1024 waves; 2100 vectors are 1050 pairs, so waves claim
    a second time, and the host's ticket base must follow: a second call on the same context decodes too."""
    llr = C.stress(2100, 0.85, 41)[0]
    plain, err, it = C.restated(2100, 0.85, 41, 10, "float32")
    want = _records32(plain, err)
    ctx = _L().Context(0)
    ctx.set_pipeline(0, 0, 1)
    ctx.set_timing(True, stages=[])
    for _ in range(2):
        ctx.counters(reset=True)
        got_plain, got = _bp(ctx, llr, 10)
        assert np.array_equal(got_plain, plain)
        A.records_equal(got, want)
        cnt = ctx.counters()
        assert (cnt["candidates"], cnt["iterations"], cnt["converged"]) == (2100, int(it.sum()), int((err == 0).sum()))
    # the float64 kernel on the same counter afterwards
    p64, r64 = _bp(ctx, llr[:65], 10, f32=False)
    A.records_equal(r64, A.plain_records(llr[:65], 10))


def test_python_layer(gpu, oracle):
    from ft8_demodulator_amd import ldpc_decoder
    llr = C.stage_pool()[0][:9]
    plain, err, _ = C.stage_expect(9, ITERS)
    p, e = ldpc_decoder.bp_decode_batch(np.array(llr), ITERS, f32=True)
    assert np.array_equal(p, plain) and np.array_equal(e, err)
    p64, e64 = ldpc_decoder.bp_decode_batch(np.array(llr), ITERS)
    ref = A.plain_records(llr)
    assert np.array_equal(e64, ref["ldpc_errors"])


# ---- FT8 batches: the device's own LLRs through the restatement -------------------------------------------
E2E = dict(max_candidates=40, min_score=2)
AP = ["CQ ? ?"]


def _expectation32(x, fs, search, cap=None, ap=None, flags=None):
    """retry_cases.expectation with the float32 restatement in place of the oracle's BP: the device's stage
    calls give the candidates and LLRs (STFT and coherent), bp32_restate + the oracle's tail the records."""
    from ft8_demodulator_amd import ap as _ap
    from ft8_demodulator_amd import bp32, coherent
    from ft8_demodulator_amd.ldpc_decoder import coherent_llr_batch
    O = A.oracle_lib()
    x = np.array(x)
    llr, rows, rec64 = R.stage_records(x, fs, search["max_candidates"], search["min_score"],
                                       _L().FT8_FLAG_TOPK if flags is None else flags)
    plain, err, _ = bp32.bp32_restate(llr, ITERS)
    rec0 = _records32(plain, err, rec64)
    coh, listed = np.array(rec0, copy=True), np.zeros(0, dtype=np.int64)
    if cap is not None:
        listed = coherent.retry_list(rec0, cap)
        cllr, fits = coherent_llr_batch(x, [rows[i][1:] for i in listed], [rows[i][0] for i in listed], fs)
        coh = coherent.coherent_pass_restate(rec0, listed, cllr, fits, ITERS, _bp32, O.decode_tail, None, None)
    both = None
    if ap:
        hyps = [_ap.ap_hypothesis(t) for t in ap]
        both = _ap.ap_restate(llr, coh, hyps, ITERS, _ap.DEFAULT_MAX_HARD_ERRORS, _bp32, O.decode_tail)[0]
    return {"x": x, "plain64": rec64, "plain": rec0, "coherent": coh, "both": both, "listed": listed}


@pytest.fixture(scope="module")
def e2e32(gpu, oracle):
    return _expectation32(A.e2e_samples(), A.E2E_FS, E2E, ap=AP)


def test_batch_equals_restatement(gpu, e2e32):
    """The main pass: the flagged batch's records equal bp32_restate + the tail on the device's own LLRs
    (FT8_FLAG_TOPK, the construction's selection)."""
    _lib = _L()
    x = gpu.from_numpy(e2e32["x"]).cuda()
    got = R.decoder(A.E2E_FS, E2E, bp32=True).records(x)
    for s in range(2):
        A.records_equal(got[s], R.per_slot(e2e32["plain"], s))
    assert sum(len(g) for g in got) >= 1
    # the reference's heap selection (min_score 5 keeps fewer than 40 candidates, so it drops none), and
    # ft8_replay_stage on a flagged batch: the BP and compact stages replayed leave the records as they were
    heap = dict(max_candidates=40, min_score=5)
    e = _expectation32(e2e32["x"], A.E2E_FS, heap, flags=0)
    dec = R.decoder(A.E2E_FS, heap, flags=_lib.FT8_FLAG_BP_F32, context=_lib.Context(0))
    got = dec.records(x)
    for s in range(2):
        A.records_equal(got[s], R.per_slot(e["plain"], s))
    out, counts = dec.run(x)
    before = (out.cpu().numpy().copy(), counts.cpu().numpy().copy())
    assert int(before[1].sum()) >= 1
    dec.ctx.replay("bp")
    dec.ctx.replay("compact")
    assert np.array_equal(out.cpu().numpy(), before[0]) and np.array_equal(counts.cpu().numpy(), before[1])
    sent = {bytes(p) for p in A.e2e_payloads()}
    assert {bytes(p) for r in dec.records(x) for p in r["payload"]} <= sent


def test_batch_with_ap_equals_restatement(gpu, e2e32):
    from ft8_demodulator_amd import ap
    x = gpu.from_numpy(e2e32["x"]).cuda()
    got = R.decoder(A.E2E_FS, E2E, ap=AP, bp32=True).records(x)
    for s in range(2):
        A.records_equal(got[s], R.per_slot(e2e32["both"], s))
    assert sum(ap.ap_index(r) > 0 for r in got[0]) >= 1


# ---- coherent pass with the flag ------------------------------------------------------------------------------
COH = dict(max_candidates=20, min_score=2)
CAP = 4


@pytest.fixture(scope="module")
def coh32(gpu, oracle):
    return _expectation32(CC.stage_case_12k()["x"], CC.FS, COH, cap=CAP, ap=AP)


def test_coherent_batch_equals_restatement(gpu, coh32):
    x = gpu.from_numpy(coh32["x"]).cuda()
    got = R.decoder(CC.FS, COH, coherent=CAP, bp32=True).records(x)
    for s in range(3):
        A.records_equal(got[s], R.per_slot(coh32["coherent"], s))
    assert sum(int((g["pass_index"] & 2).astype(bool).sum()) for g in got) >= 1
    got = R.decoder(CC.FS, COH, coherent=CAP, ap=AP, bp32=True).records(x)
    for s in range(3):
        A.records_equal(got[s], R.per_slot(coh32["both"], s))


# ---- subtraction with the flag: what the contract alone implies -------------------------------------------
def test_subtract_batch(gpu):
    from ft8_demodulator_amd.subtract import subtract_index
    x = gpu.from_numpy(np.array(A.e2e_samples())).cuda()
    sent = {bytes(p) for p in A.e2e_payloads()}
    one = R.decoder(A.E2E_FS, E2E, bp32=True).records(x)
    two = R.decoder(A.E2E_FS, E2E, subtract=2, bp32=True).records(x)
    two64 = R.decoder(A.E2E_FS, E2E, subtract=2).records(x)
    print("subtract=2 rows per slot: float32", [len(r) for r in two], "float64", [len(r) for r in two64])
    for s in range(2):
        assert {bytes(p) for p in two[s]["payload"]} <= sent, s
        first = two[s][[subtract_index(r) == 0 for r in two[s]]] if len(two[s]) else two[s]
        A.records_equal(first, one[s])


# ---- FT4 ----------------------------------------------------------------------------------------------------------
def _ft4_restate32(wf, oracle, topk, kw, slot=0, hyps=None, osd=None):
    from ft8_demodulator_amd import ft4
    return ft4.ft4_decode_restate(np.asarray(wf), F4.SPS, F4.BPT, kw["max_candidates"], kw["min_score"], F4.ITERS,
                                  select=oracle.select_topk if topk else oracle.select, bp_decode=_bp32,
                                  decode_tail=oracle.decode_tail, slot=slot, hyps=hyps,
                                  ap_max_hard_errors=F4.RETRY_AP_MAX_HARD, osd=osd)[0]


def _same_ft4(got, ref, what):
    assert len(got) == len(ref), (what, len(got), len(ref))
    for f in _L().RESULT_DTYPE.names if len(got) else ():
        assert np.array_equal(got[f], np.asarray(ref[f]).reshape(got[f].shape)), (what, f)


def test_ft4_batches_equal_restatement(gpu, oracle):
    """The FT4 retry slot, plain and with ap= and osd=: ft8_stft (FT4), then the restated chain with the
    float32 decoder on that waterfall, equals the flagged batch's records."""
    from ft8_demodulator_amd import SlotDecoder, _device, ap
    _lib = _L()
    x, pays = F4.retry_slot()
    x = x.cuda()
    wf, _ = _device.ft4_stft(x, F4.FS, F4.BPT, F4.SPS, code=_lib.FT8_F32)
    wf = wf.cpu().numpy()
    order, cap, max_hard = F4.RETRY_OSD
    hyps = [ap.ap_hypothesis(p) for p in F4.RETRY_AP]
    base = dict(flags=_lib.FT8_FLAG_TOPK, protocol="ft4", bp32=True)
    args = (F4.FS, F4.BPT, F4.SPS, F4.RETRY["max_candidates"], F4.RETRY["min_score"], F4.ITERS)
    got = SlotDecoder(*args, **base).records(x, _lib.FT8_F32)[0]
    _same_ft4(got, _ft4_restate32(wf[0], oracle, True, F4.RETRY), "plain")
    assert len(got) >= 1
    got = SlotDecoder(*args, ap=F4.RETRY_AP, ap_max_hard_errors=F4.RETRY_AP_MAX_HARD, osd=(order, cap),
                      osd_max_hard_errors=max_hard, **base).records(x, _lib.FT8_F32)[0]
    _same_ft4(got, _ft4_restate32(wf[0], oracle, True, F4.RETRY, hyps=hyps, osd=F4.RETRY_OSD), "retries")
    assert {bytes(p) for p in got["payload"]} <= {bytes(p) for p in pays}


# ---- one context, both kernels: the claim counters and their host bases are shared ---------------------
def test_context_reuse(gpu):
    _lib = _L()
    x = gpu.from_numpy(np.array(A.e2e_samples())).cuda()
    llr = C.stage_pool()[0][:67]

    def calls(ctx):
        return [
            lambda: b"".join(r.tobytes() for r in R.decoder(A.E2E_FS, E2E, ap=AP, bp32=True, context=ctx).records(x)),
            lambda: b"".join(r.tobytes() for r in R.decoder(A.E2E_FS, E2E, ap=AP, context=ctx).records(x)),
            lambda: b"".join(a.tobytes() for a in _bp(ctx, llr, ITERS, f32=True)),
            lambda: b"".join(a.tobytes() for a in _bp(ctx, llr, ITERS, f32=False)),
        ]
    fresh = [calls(_lib.Context(0))[i]() for i in range(4)]
    shared = _lib.Context(0)
    for rnd in range(2):
        for i, call in enumerate(calls(shared)):
            assert call() == fresh[i], (rnd, i)
    shared.set_ap([])
