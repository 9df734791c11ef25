"""FT4 on the device (csrc/ft4.hip) against ft4.py's NumPy restatements: encoder, synthesis, the score grids
of both kernels bit for bit, selection on them, LLRs bit for bit, the descrambler, the whole batch on the
device's own waterfall (records field for field), the a-priori and OSD retries, the refusals, and FT8 left
intact.  ft4_cases.py holds the constructions; test_ft4_reference.py shows on the CPU that they decode."""
import ctypes

import numpy as np
import pytest

import ft4_cases as C

pytestmark = pytest.mark.gpu

FIELDS = ("score", "slot", "abs_time", "abs_freq", "crc_extracted", "crc_calculated", "ldpc_errors", "cand_index",
          "payload", "ok", "pass_index")


def _same_records(got, want, tag):
    assert len(got) == len(want), (tag, len(got), len(want))
    for f in FIELDS:
        assert np.array_equal(got[f], want[f]), (tag, f, got[f].tolist(), want[f].tolist())


# ---- transmit chain ------------------------------------------------------------------------------------
def test_encode_matches_definition(gpu):
    from ft8_demodulator_amd import ft4, ft8_generator as G, synth
    rng = np.random.default_rng(11)
    pays = np.concatenate([synth.random_payloads(64, rng), np.zeros((1, 10), np.uint8)])
    a91, cw, tones = (t.cpu().numpy() for t in G.ft4_encode_batch(pays))
    for i, p in enumerate(pays):
        scr = ft4.ft4_scramble(p.tobytes())
        assert a91[i].tobytes() == synth.add_crc(scr), i
        assert cw[i].tobytes() == synth.ldpc_encode(synth.add_crc(scr)), i
        assert np.array_equal(tones[i], ft4.ft4_itones(p.tobytes())), i
    assert np.array_equal(G.ft4_encode(pays[3]), ft4.ft4_itones(pays[3].tobytes()))
    # each output is nullable
    import torch
    from ft8_demodulator_amd import _lib
    ctx = _lib.context()
    m = torch.from_numpy(pays).cuda()
    t = torch.zeros(len(pays), 103, dtype=torch.uint8, device="cuda")
    ctx.check(_lib.lib().ft8_ft4_encode(ctx.handle, _lib.ptr(m), len(pays), None, None, _lib.ptr(t),
                                        _lib.stream_handle()), "ft8_ft4_encode")
    assert np.array_equal(t.cpu().numpy(), tones)


@pytest.mark.parametrize("fs", [12000, 6000])
def test_synthesis_matches_waveforms(gpu, fs):
    """Unit amplitude against ft4_waveforms with test_gpu_tx.py's bounds: 1e-8 (float64), 2e-6 (float32); a
    signal starting before sample 0, one running past the end, two overlapping."""
    import torch
    from ft8_demodulator_amd import _lib, ft4, ft8_generator as G, synth
    nsps = ft4.ft4_nsps(fs)
    rng = np.random.default_rng(12)
    pays = synth.random_payloads(4, rng)
    tones = np.stack([ft4.ft4_itones(p.tobytes()) for p in pays])
    f0 = np.array([400.0, 1234.5, 1300.25, 2000.0])
    n = 110 * nsps
    # slot 0: a signal whose ramp symbol starts before sample 0; slot 1: two overlapping; slot 2: past the end
    start = [nsps // 3, 2 * nsps, 2 * nsps + 777, 40 * nsps]
    slot = [0, 1, 1, 2]
    sig = np.zeros(4, dtype=_lib.TX_SIGNAL_DTYPE)
    sig["f0"], sig["amplitude"], sig["start"], sig["slot"] = f0, 1.0, start, slot
    ref = np.zeros((3, n))
    w = ft4.ft4_waveforms(tones, fs, f0).numpy()
    for i in range(4):
        s0 = start[i] - nsps
        a, e = max(s0, 0), min(s0 + w.shape[1], n)
        ref[slot[i], a:e] += w[i, a - s0:e - s0]
    for dtype, bound in ((torch.float64, 1e-8), (torch.float32, 2e-6)):
        out = G.synthesize(tones, sig, 3, n, fs, dtype=dtype, protocol="ft4").cpu().numpy().astype(np.float64)
        d = np.max(np.abs(out - ref))
        print(fs, dtype, "max |diff|", d)
        assert d < bound, (fs, dtype, d)
    # it ADDS into out, and the complex baseband's real part is the real waveform
    base = torch.ones(3, n, dtype=torch.float64, device="cuda")
    out = G.synthesize(tones, sig, 3, n, fs, out=base, protocol="ft4").cpu().numpy()
    assert np.max(np.abs(out - 1.0 - ref)) < 1e-8
    z = G.synthesize(tones, sig, 3, n, fs, dtype=torch.complex128, protocol="ft4").cpu().numpy()
    assert np.max(np.abs(z.real - ref)) < 1e-8
    with pytest.raises(NotImplementedError):
        G.synthesize(tones, sig, 3, n, 44100, protocol="ft4")


# ---- score grids and selection ---------------------------------------------------------------------------
def _check_grids_and_selection(oracle, T, F, seed, sps, bpt, tag, dtype=np.float32, special=False, sel=True):
    """The full grid of every slot (three per call) bit for bit, then (sel) the selection with and without a
    caller grid -- without one the tiled kernel writes the compact layout -- under both rules at
    N = 1, 37, 4096."""
    from ft8_demodulator_amd import _device, _lib, ft4
    S = 3
    t0, NT, NF = ft4.ft4_grid_shape(T, F, sps, bpt)
    if sel:
        wf, ref, ms = C.untied_waterfall(T, F, S, seed, sps, bpt, dtype, special)
    else:
        wf = C.waterfall(T, F, S, seed, dtype, special)
        ref = [ft4.ft4_score_grid_restate(wf[b], sps, bpt) for b in range(S)]
    _, grid, _ = _device.ft4_sync_select(wf, sps, bpt, 1, 0.0, want_grid=True)
    for b in range(S):
        assert ref[b].shape == (NT, NF)
        assert np.array_equal(grid[b].view(np.uint32 if wf.dtype == np.float32 else np.uint64),
                              ref[b].view(np.uint32 if wf.dtype == np.float32 else np.uint64)), (tag, b)
    if not sel:
        return
    assert C.untied(ref, ms), (tag, "equal passing scores")
    for N in (1, 37, 4096):
        for flags, select in ((0, oracle.select), (_lib.FT8_FLAG_TOPK, oracle.select_topk)):
            for want_grid in (False, True):
                got, _, _ = _device.ft4_sync_select(wf, sps, bpt, N, ms, flags=flags, want_grid=want_grid)
                for b in range(S):
                    idx, sc = select(ref[b], N, ms)[:2]
                    want = [(int(i // NF) + t0, int(i % NF), float(v)) for i, v in zip(idx, sc)]
                    assert got[b] == want, (tag, N, flags, want_grid, b)


@pytest.mark.parametrize("B", [1, 2, 3, 4])
def test_score4_tiled_bit_exact(gpu, oracle, B):
    """k_score4<B, B>: full grid and compact, every shape class of ft4_cases.tiled_shapes."""
    seen = set()
    for i, (T, NF, what) in enumerate(C.tiled_shapes(B)):
        F = NF + 3 * B
        t0, NT, nf = C.grid_shape(T, F, B, B)
        assert nf == NF and NT > 0
        rows = NT // B                                   # grid rows of a residue class (NT is a multiple of B)
        if what == "smallest grid":
            assert T // B == 74 and NT == B
        if what == "T % sps != 0" and B > 1:
            assert T % B != 0
        if what == "ragged row tile":
            assert rows > C.S4_R and rows % C.S4_R != 0
        seen.add((NF - 1) // C.S4_TW + 1)                # column tiles
        seen.add("vec" if F % 4 == 0 else "scalar")      # float4 staging or the element-wise one
        _check_grids_and_selection(oracle, T, F, 100 * B + i, B, B, (B, T, NF, what), special=(i % 2 == 1),
                                   sel=(i % 3 == 0))
    assert {1, 2, 3, "vec", "scalar"} <= seen


@pytest.mark.parametrize("bpt,sps,dtype,T", [
    (3, 2, np.float32, 180), (3, 2, np.float32, 480), (1, 2, np.float32, 181), (2, 4, np.float32, 360),
    (2, 2, np.float64, 180), (2, 2, np.float64, 481), (3, 2, np.float64, 180)])
def test_score4g_bit_exact(gpu, oracle, bpt, sps, dtype, T):
    """k_score4g: float64 waterfalls and bpt != sps, staged in LDS and not."""
    F = 150 + 3 * bpt
    lds = C.score4g_in_lds(T, F, sps, bpt, np.dtype(dtype).itemsize)
    assert lds == (T <= 181 and sps == 2), (T, lds)      # both stagings occur across the cases
    _check_grids_and_selection(oracle, T, F, T + bpt, sps, bpt, (bpt, sps, dtype.__name__, T), dtype=dtype,
                               special=(T % 2 == 1), sel=(T in (180, 360)))


# ---- LLRs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bpt,sps", [(2, 2), (3, 2), (2, 4)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_llr_bit_exact(gpu, bpt, sps, dtype):
    from ft8_demodulator_amd import _device, ft4
    T, F = 95 * sps + 1, 60 + 3 * bpt
    wf = C.waterfall(T, F, 3, 7 * bpt + sps, dtype=dtype)
    t0, NT, NF = ft4.ft4_grid_shape(T, F, sps, bpt)
    cands = []
    for b in range(3):
        g = ft4.ft4_score_grid_restate(wf[b], sps, bpt)
        best = np.argsort(-g.reshape(-1), kind="stable")[:6]
        cands += [(b, int(i // NF) + t0, int(i % NF)) for i in best]
        # the grid corners: the first or the last data symbols lie outside the waterfall and give zeros
        cands += [(b, t0, 0), (b, t0, NF - 1), (b, t0 + NT - 1, 0), (b, t0 + NT - 1, NF - 1)]
    rng = np.random.default_rng(3)
    lists = [cands[:n] for n in (1, 2, 3, 4, 5)] + [[cands[i] for i in rng.integers(0, len(cands), 63)], cands]
    for norm in (False, True):
        for lst in lists:
            got = _device.ft4_llr(wf, sps, bpt, lst, normalize=norm)
            for r, (b, at, af) in enumerate(lst):
                want = ft4.ft4_llr_restate(wf[b], sps, bpt, at, af, normalize=norm)
                assert np.array_equal(got[r].view(np.uint64), want.view(np.uint64)), (norm, len(lst), r, b, at, af)
    raw = _device.ft4_llr(wf, sps, bpt, [(0, t0, 0), (0, t0 + NT - 1, 0)], normalize=False)
    assert not raw[0][:12].any() and raw[0][12:].all()       # ten symbols early: data symbols 0 .. 5 are zeros
    assert not raw[1][144:].any() and raw[1][:144].all()     # twenty late: data symbols 72 .. 86 are


# ---- descrambler ------------------------------------------------------------------------------------------
def test_unscramble(gpu):
    from ft8_demodulator_amd import _device, _lib, ft4
    rng = np.random.default_rng(9)
    rec = np.frombuffer(rng.integers(0, 256, 301 * _lib.RESULT_DTYPE.itemsize, dtype=np.uint8).tobytes(),
                        dtype=_lib.RESULT_DTYPE).copy()
    once = _device.ft4_unscramble(rec)
    want = rec.copy()
    want["payload"] ^= np.frombuffer(ft4.FT4_RVEC, dtype=np.uint8)[None, :]
    assert once.tobytes() == want.tobytes()                  # every other byte untouched, the low 3 bits of [9] too
    assert np.array_equal(once["payload"][:, 9] & 7, rec["payload"][:, 9] & 7)
    assert _device.ft4_unscramble(once).tobytes() == rec.tobytes()


# ---- the whole batch ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def e2e(gpu):
    x, want, _ = C.e2e_slots()
    return x.cuda(), want


def _stft_and_restate(oracle, x, code, topk, kw, hyps=None, osd=None):
    from ft8_demodulator_amd import _device
    wf, plan = _device.ft4_stft(x, C.FS, C.BPT, C.SPS, code=code)
    assert (plan.nperseg, plan.hop, plan.nfft, plan.frames) == (576, 288, 1152, 311)
    wf = wf.cpu().numpy()
    return wf, [C.restate(wf[b], oracle, topk, slot=b, hyps=hyps, osd=osd, **kw)[0] for b in range(wf.shape[0])]


def test_ft4_stft_matches_numpy(gpu, e2e):
    """The FT4 STFT against a NumPy float64 STFT within test_gpu_stft.py's tolerances."""
    from ft8_demodulator_amd import _device, _lib, ft4
    x, _ = e2e
    wf, plan = _device.ft4_stft(x[:2], C.FS, C.BPT, C.SPS, code=_lib.FT8_F32)
    ctx = _lib.context()
    assert _lib.lib().ft8_stft_method(ctx.handle, 12000, 2, 2, C.N_SAMPLES, _lib.FT8_F32) in (0, 1, 2, 3)
    for b in range(2):
        ref = ft4.ft4_stft_restate(x[b].cpu().numpy().astype(np.float64), C.FS, C.BPT, C.SPS, np.float64)
        got = wf[b].cpu().numpy().astype(np.float64)
        assert got.shape == ref.shape == (311, 576)
        strong = ref >= (ref.max(axis=1, keepdims=True) - 60.0)
        d = np.abs(got - ref)
        assert d[strong].max() <= 1e-3 and d.max() <= 0.25, (d[strong].max(), d.max())


@pytest.mark.parametrize("topk", [False, True])
@pytest.mark.parametrize("i16", [False, True])
def test_batch_equals_restatement(gpu, oracle, e2e, topk, i16):
    """ft8_stft (FT4), then the restated chain on THAT waterfall, equals ft8_decode_batch's records field for
    field; chunked pipelining gives the same records; the payload sets are the transmitted ones."""
    import torch
    from ft8_demodulator_amd import SlotDecoder, _lib
    x, want = e2e
    code = _lib.FT8_F32
    if i16:
        x = torch.round(x / x.abs().max() * 20000.0).to(torch.int16)
        code = _lib.FT8_I16
    kw = C.E2E_TOPK if topk else C.E2E_HEAP
    dec = SlotDecoder(C.FS, C.BPT, C.SPS, kw["max_candidates"], kw["min_score"], C.ITERS,
                      flags=_lib.FT8_FLAG_TOPK if topk else 0, protocol="ft4")
    got = dec.records(x, code)
    _, ref = _stft_and_restate(oracle, x, code, topk, kw)
    for b in range(x.shape[0]):
        _same_records(got[b], ref[b], (topk, i16, b))
        assert {bytes(p) for p in got[b]["payload"]} == want[b], b
    dec.ctx.set_pipeline(2, 2, 4)
    try:
        chunked = dec.records(x, code)
    finally:
        dec.ctx.set_pipeline(0, 0, 4)
    for b in range(x.shape[0]):
        assert chunked[b].tobytes() == got[b].tobytes(), b


def test_retries_equal_restatement(gpu, oracle):
    """The retry slot with FT8_FLAG_AP | FT8_FLAG_OSD: the a-priori pass with the scrambled hypothesis, then
    OSD, as the restatement applies them to the device's waterfall; at least one record of each kind."""
    from ft8_demodulator_amd import SlotDecoder, _lib, ap
    x, pays = C.retry_slot()
    x = x.cuda()
    order, cap, max_hard = C.RETRY_OSD
    dec = SlotDecoder(C.FS, C.BPT, C.SPS, C.RETRY["max_candidates"], C.RETRY["min_score"], C.ITERS,
                      flags=_lib.FT8_FLAG_TOPK, ap=C.RETRY_AP, ap_max_hard_errors=C.RETRY_AP_MAX_HARD,
                      osd=(order, cap), osd_max_hard_errors=max_hard, protocol="ft4")
    got = dec.records(x, _lib.FT8_F32)[0]
    hyps = [ap.ap_hypothesis(p) for p in C.RETRY_AP]
    _, ref = _stft_and_restate(oracle, x, _lib.FT8_F32, True, C.RETRY, hyps=hyps, osd=C.RETRY_OSD)
    _same_records(got, ref[0], "retry")
    kinds = [int(r["pass_index"]) >> 4 for r in got]
    assert any(0 < k < 15 for k in kinds) and 15 in kinds
    assert {bytes(p) for p in got["payload"]} <= {bytes(p) for p in pays}
    with pytest.raises(ValueError):          # ft8_replay_stage after an FT4 batch
        dec.ctx.replay("bp")


# ---- refusals, and FT8 intact --------------------------------------------------------------------------
def test_refusals(gpu, e2e):
    import torch
    from ft8_demodulator_amd import SlotDecoder, _lib
    from ft8_demodulator_amd._pipeline import make_params, make_plan
    x, _ = e2e
    L, ctx = _lib.lib(), _lib.context()
    n = C.N_SAMPLES
    plan = make_plan(n, C.FS, 2, 2, protocol="ft4")
    st = _lib.stream_handle()
    out = torch.zeros(5 * 10 * 40, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(5, dtype=torch.int32, device="cuda")
    big = torch.zeros(5 * n, dtype=torch.float32, device="cuda")
    i32 = torch.zeros(4096, dtype=torch.int32, device="cuda")
    f64 = torch.zeros(4096, dtype=torch.float64, device="cuda")

    def batch(p):
        return L.ft8_decode_batch(ctx.handle, _lib.ptr(x), _lib.FT8_F32, n, 5, n, ctypes.byref(p), _lib.ptr(out),
                                  _lib.ptr(cnt), 10, st)

    p = make_params(plan, 10, 1.0, 5)
    assert p.protocol == _lib.FT8_PROTO_FT4
    assert batch(p) == _lib.FT8_OK
    assert L.ft8_snr_last(ctx.handle, _lib.ptr(out), _lib.ptr(cnt), 5, 10, _lib.ptr(big), st) == _lib.FT8_E_UNSUPPORTED
    assert batch(p) == _lib.FT8_OK
    assert L.ft8_replay_stage(ctx.handle, 3, 1, st) == _lib.FT8_E_ARG
    for flag in (_lib.FT8_FLAG_COHERENT, _lib.FT8_FLAG_SUBTRACT):
        q = make_params(plan, 10, 1.0, 5, flags=flag)
        assert batch(q) == _lib.FT8_E_UNSUPPORTED, flag
    U = _lib.FT8_E_UNSUPPORTED
    assert L.ft8_stft_argmax(ctx.handle, _lib.ptr(x), _lib.FT8_F32, n, 5, n, ctypes.byref(p), _lib.ptr(i32), st) == U
    assert L.ft8_subtract(ctx.handle, _lib.ptr(x), _lib.FT8_F32, _lib.ptr(big), n, 5, n, ctypes.byref(p), _lib.ptr(out),
                          _lib.ptr(cnt), 10, st) == U
    assert L.ft8_snr(ctx.handle, _lib.ptr(big), 0, 5, plan.T, plan.F, ctypes.byref(p), n, _lib.ptr(out), _lib.ptr(cnt),
                     10, _lib.ptr(f64), 1, _lib.ptr(big), st) == U
    assert L.ft8_coherent_llr(ctx.handle, _lib.ptr(x), _lib.FT8_F32, n, 5, n, ctypes.byref(p), _lib.ptr(i32),
                              _lib.ptr(i32), 1, _lib.ptr(f64), _lib.ptr(big), st) == U
    assert L.ft8_coherent_drift_llr(ctx.handle, _lib.ptr(x), _lib.FT8_F32, n, 5, n, ctypes.byref(p), _lib.ptr(i32),
                                    _lib.ptr(i32), 1, 1.0, 3, _lib.ptr(f64), _lib.ptr(big), None, st) == U
    assert L.ft8_coherent_nsym_llr(ctx.handle, _lib.ptr(x), _lib.FT8_F32, n, 5, n, ctypes.byref(p), _lib.ptr(i32),
                                   _lib.ptr(i32), 1, 0.0, 1, _lib.ptr(f64), _lib.ptr(big), None, 2, None, st) == U
    # an unknown protocol is an argument error wherever the field is read
    p.protocol = 2
    assert batch(p) == _lib.FT8_E_ARG
    assert L.ft8_stft(ctx.handle, _lib.ptr(x), _lib.FT8_F32, n, 5, n, ctypes.byref(p), _lib.ptr(big), st) == _lib.FT8_E_ARG
    assert L.ft8_sync_select(ctx.handle, _lib.ptr(big), 0, 1, 311, 576, ctypes.byref(p), _lib.ptr(i32), _lib.ptr(f64),
                             _lib.ptr(cnt), None, st) == _lib.FT8_E_ARG
    assert L.ft8_stft_argmax(ctx.handle, _lib.ptr(x), _lib.FT8_F32, n, 5, n, ctypes.byref(p), _lib.ptr(i32), st) \
        == _lib.FT8_E_ARG
    # a rate whose symbol is no whole number of samples
    p.protocol, p.sample_rate, p.sample_rate_hz = _lib.FT8_PROTO_FT4, 44100, 44100.0
    assert L.ft8_stft(ctx.handle, _lib.ptr(x), _lib.FT8_F32, n, 5, n, ctypes.byref(p), _lib.ptr(big), st) == U
    torch.cuda.synchronize()
    # the Python layer says so before anything is launched
    for kw in (dict(coherent=True), dict(subtract=True), dict(flags=_lib.FT8_FLAG_SUBTRACT)):
        with pytest.raises(NotImplementedError):
            SlotDecoder(protocol="ft4", **kw)
    with pytest.raises(NotImplementedError):
        SlotDecoder(protocol="ft4", min_score=1.0).reports(x[:1])
    with pytest.raises(ValueError):
        SlotDecoder(protocol="ft5")


def test_ft8_batch_after_ft4_equals_fresh_context(gpu, e2e):
    from ft8_demodulator_amd import SlotDecoder, _lib, synth
    x8, _ = synth.make_slots(2, 5, snr_db=(-6.0, 0.0), seed=31)
    x8 = x8.cuda()
    x4, _ = e2e
    ctx = _lib.Context(0)
    SlotDecoder(protocol="ft4", context=ctx, **C.E2E_TOPK).records(x4, _lib.FT8_F32)
    after = SlotDecoder(context=ctx, max_candidates=40).records(x8, _lib.FT8_F32)
    fresh = SlotDecoder(context=_lib.Context(0), max_candidates=40).records(x8, _lib.FT8_F32)
    assert sum(len(r) for r in fresh) >= 4
    for a, f in zip(after, fresh):
        assert a.tobytes() == f.tobytes()


# ---- Python layer -----------------------------------------------------------------------------------------
def test_python_layer(gpu):
    from ft8_demodulator_amd import SlotDecoder, _lib, decode_ft4_message, ft4, message
    text = "CQ K1ABC FN42"
    pay = message.pack77(text)
    x, truths = ft4.make_slots_ft4(1, 1, snr_db=-6.0, seed=77, payloads=[pay])
    dec = SlotDecoder(protocol="ft4", max_candidates=20, min_score=1.0, flags=_lib.FT8_FLAG_TOPK)
    rows = dec.messages(x.cuda())[0]
    assert [r[0] for r in rows] == [text]
    assert [t["text"].decode() for t in dec.texts(x.cuda())[0]][0] == text
    res = decode_ft4_message(x[0].numpy(), 12000, max_candidates=20, min_score=1.0, flags=_lib.FT8_FLAG_TOPK)
    hits = [r for r in res if bytes(r[0].payload) == bytes(pay)]
    assert hits and dec.decode(x.cuda())[0][0][0].payload == hits[0][0].payload
    hop_s, bin_hz = 288 / 12000.0, 12000.0 / 1152
    best = hits[0]
    assert abs(best[2] - truths[0].start_s[0]) <= hop_s, (best[2], truths[0].start_s[0])
    assert abs(best[3] - truths[0].f0[0]) <= bin_hz, (best[3], truths[0].f0[0])
