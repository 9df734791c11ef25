"""Transmit chain on the GPU (csrc/tx.hip) and the build-defined decode options (top-k selection,
subtract-and-redecode; csrc/sync.hip k_topk, csrc/subtract.hip).

Pinned: the encoder against the reference generator's known answers (golden.json "tx", bit-exact)
and the GFSK waveforms against the reference modulator's outputs (tx_wave.npz, |diff| <= 1e-8 for
a unit-amplitude float64 waveform: the reference accumulates its phase sequentially, the kernel in
closed form).  Top-k selection: bit-exact against oracle.select_topk on injected waterfalls.
Subtraction: no reference exists (parity unpinned); checked by residual
energy, pass-1 invariance, truth membership and determinism."""
import json
import os

import numpy as np
import pytest

from conftest import GOLD

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def txw():
    with open(os.path.join(GOLD, "tx_wave.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLD, "tx_wave.npz"), allow_pickle=False)


def test_encoder_known_answers(golden, gpu):
    from ft8_demodulator_amd import ft8_generator as G
    meta, _ = golden
    for r in meta["tx"]:
        p = np.frombuffer(bytes.fromhex(r["payload"]), dtype=np.uint8)
        a91 = G.crc_generator(p)
        assert bytes(a91).hex() == r["a91"]
        assert int(G.get_crc_from_a91(a91)) == r["crc"]
        assert bytes(G.ldpc_generator(a91)).hex() == r["codeword"]
        assert "".join(map(str, G.ft8_encode(p))) == r["itones"]


def test_encoder_batch_vs_oracle(gpu, oracle):
    from ft8_demodulator_amd import ft8_generator as G
    rng = np.random.default_rng(5)
    pays = rng.integers(0, 256, size=(3000, 10), dtype=np.uint8)
    a91, cw, tones = G.encode_batch(pays)
    a91, cw, tones = a91.cpu().numpy(), cw.cpu().numpy(), tones.cpu().numpy()
    for i in range(0, 3000, 7):
        ra = oracle.crc_generator(bytes(pays[i]))
        assert bytes(a91[i]) == ra
        assert bytes(cw[i]) == oracle.ldpc_encode(ra)
        assert np.array_equal(tones[i], oracle.tx_itones(bytes(pays[i])))
    # a91 taken as given (arbitrary low bits of byte 11 are copied, parity OR-ed in: ldpc.py:106-129)
    raw = rng.integers(0, 256, size=(64, 12), dtype=np.uint8)
    _, cw2, _ = G.encode_batch(raw, msg_bytes=12)
    cw2 = cw2.cpu().numpy()
    for i in range(64):
        assert bytes(cw2[i]) == oracle.ldpc_encode(bytes(raw[i]))


def test_reference_waveforms(txw, gpu):
    from ft8_demodulator_amd import _lib
    from ft8_demodulator_amd import ft8_generator as G
    meta, arr = txw
    n = 0
    for c in meta["cases"]:
        if c["kind"] == "freq":
            continue
        p = np.frombuffer(bytes.fromhex(c["payload"]), dtype=np.uint8)
        if c["kind"] == "baseband":
            got = G.ft8_baseband_generator(p, c["fs"], c["f0"])
            assert got.dtype == np.complex128
        else:
            got = G.ft8_generator(p, c["fs"], c["f0"], c["fc"])
            assert got.dtype == np.float64
        assert got.shape[0] == c["length"]
        if c["segment"]:
            a0, a1, b0, b1 = c["segment"]
            got = np.concatenate([got[a0:a1], got[b0:b1]])
        ref = arr[c["name"]]
        assert np.max(np.abs(got - ref)) < 1e-8, c["name"]
        n += 1
    assert n == 3
    # float32 output of the same kernel
    c = [c for c in meta["cases"] if c["name"] == "real_6k"][0]
    _, _, tones = G.encode_batch(np.frombuffer(bytes.fromhex(c["payload"]), dtype=np.uint8)[None])
    sig = np.zeros(1, dtype=_lib.TX_SIGNAL_DTYPE)
    sig["f0"], sig["amplitude"] = c["f0"], 1.0
    out = G.synthesize(tones, sig, 1, c["length"], c["fs"], _lib.FT8_TX_REFERENCE, dtype=gpu.float32)
    assert np.max(np.abs(out[0].cpu().numpy().astype(np.float64) - arr["real_6k"])) < 2e-6


def test_protocol_timing_vs_oracle(gpu, oracle):
    from ft8_demodulator_amd import _lib
    from ft8_demodulator_amd import ft8_generator as G
    for fs, f0 in ((12000, 1234.5), (10000, 640.0), (2000, 0.0)):
        pay = bytes(range(3, 13))
        it = oracle.tx_itones(pay)
        ref = np.real(oracle.gfsk_waveform(it, fs, f0, style=0))
        sig = np.zeros(1, dtype=_lib.TX_SIGNAL_DTYPE)
        sig["f0"], sig["amplitude"] = f0, 1.0
        out = G.synthesize(gpu.as_tensor(it[None]), sig, 1, ref.size, fs, _lib.FT8_TX_PROTOCOL, dtype=gpu.float64)
        assert np.max(np.abs(out[0].cpu().numpy() - ref)) < 1e-8, fs


def test_synthesize_batch_sum_and_clipping(gpu, oracle):
    """Many signals, several slots, unsorted input, starts before 0 and past the end: equal to the
    sum of single-signal syntheses."""
    from ft8_demodulator_amd import _lib
    from ft8_demodulator_amd import ft8_generator as G
    rng = np.random.default_rng(9)
    fs, n_slots, N = 6000, 3, 60000
    n = 7
    pays = rng.integers(0, 256, size=(n, 10), dtype=np.uint8)
    _, _, tones = G.encode_batch(pays)
    sig = np.zeros(n, dtype=_lib.TX_SIGNAL_DTYPE)
    sig["f0"] = rng.uniform(100, 2500, n)
    sig["amplitude"] = rng.uniform(0.1, 2.0, n)
    sig["phase"] = rng.uniform(-3, 3, n)
    sig["start"] = [-5000, 100, 4000, 55000, 0, 12345, -80000]
    sig["slot"] = [2, 0, 1, 0, 2, 1, 0]
    out = G.synthesize(tones, sig, n_slots, N, fs, dtype=gpu.float64)
    ref = gpu.zeros((n_slots, N), dtype=gpu.float64, device="cuda")
    for i in range(n):
        one = G.synthesize(tones[i:i + 1], sig[i:i + 1].copy(), n_slots, N, fs, dtype=gpu.float64)
        ref += one
    assert gpu.allclose(out, ref, rtol=0, atol=1e-12)
    # the signal that starts 80000 samples before the slot (79 * 960 long) lies wholly outside it
    only = G.synthesize(tones[6:7], sig[6:7].copy(), n_slots, N, fs, dtype=gpu.float64)
    assert float(only.abs().max()) == 0.0
    # accumulation into an existing buffer (noise + signals)
    base = gpu.ones((n_slots, N), dtype=gpu.float32, device="cuda")
    acc = G.synthesize(tones, sig, n_slots, N, fs, out=base.clone())
    assert gpu.allclose(acc.double() - 1.0, out, atol=1e-5)


def _wf(mag, sps, bpt):
    from ft8_demodulator_amd import FT8Waterfall
    return FT8Waterfall(mag=mag, time_osr=sps, freq_osr=bpt)


def test_topk_selection_vs_oracle(golden, gpu, oracle):
    from ft8_demodulator_amd import _device
    meta, arr = golden
    n = 0
    for c in meta["sync"]:
        mag = arr[f"sync_{c['name']}_mag"]
        wf = _wf(mag, c["sps"], c["bpt"])
        grid = arr[f"sync_{c['name']}_grid"]
        for N, ms in ((5, 1), (50, 0.5), (300, -1000), (7, 10), (4096, 2)):
            cands, _, warn = _device.sync_select(wf, N, ms, flags=1)
            idx, sc = oracle.select_topk(grid, N, ms)
            t0 = -10 * c["sps"]
            NF = grid.shape[1]
            exp = [(int(i // NF) + t0, int(i % NF)) for i in idx]
            assert [(a, b) for a, b, _ in cands] == exp, (c["name"], N, ms)
            assert np.array_equal(np.array([s for _, _, s in cands], dtype=np.float64), sc)
            assert warn == 0
            n += 1
    assert n >= 40


def test_topk_compact_paths_vs_oracle(gpu, oracle):
    """k_topkc (top-k from the compact score segments) on full-size 12 kHz waterfalls against
    oracle.select_topk and against k_topk on the full grid (want_grid): passing scores staged in LDS
    (min_score 2, ~10^4 passing) and streamed from HBM past the LDS budget (min_score -1000, every
    grid point passes); quantised levels put thousands of exactly equal scores at the threshold,
    which takes the ordered (scan-order) compaction instead of the unordered collection."""
    from ft8_demodulator_amd import _device
    rng = np.random.default_rng(77)
    F, T = 1920, 186
    cases = 0
    for trial in range(4):
        if trial < 2:   # ~20 k (streamed) and ~6.4 k (staged) scores >= 2
            mag = (rng.standard_normal((F, T)) * (6.0 if trial == 0 else 4.0) - 60.0).astype(np.float32)
        else:
            mag = (rng.integers(0, 3, size=(F, T)) * 4.0 - 60.0).astype(np.float32)
        grid = oracle.score_grid(mag, 2, 2)
        NF = grid.shape[1]
        for N, ms in ((300, 2), (300, -1000), (4096, 0.5), (1, -1000), (2000, 1)):
            cands, _, warn = _device.sync_select(_wf(mag, 2, 2), N, ms, flags=1)
            full, _, _ = _device.sync_select(_wf(mag, 2, 2), N, ms, want_grid=True, flags=1)
            idx, sc = oracle.select_topk(grid, N, ms)
            exp = [(int(i // NF) - 20, int(i % NF)) for i in idx]
            assert [(a, b) for a, b, _ in cands] == exp, (trial, N, ms)
            assert np.array_equal(np.array([s_ for _, _, s_ in cands], dtype=np.float64), sc), (trial, N, ms)
            assert [(a, b) for a, b, _ in full] == exp, (trial, N, ms)
            assert warn == 0
            cases += 1
    assert cases == 20


def test_topk_ties_in_scan_order(gpu, oracle):
    """Silence scores exactly 0 everywhere: the top-k set is the first N grid points."""
    from ft8_demodulator_amd import _device
    mag = np.full((120, 186), -120.0, dtype=np.float32)
    cands, _, _ = _device.sync_select(_wf(mag, 2, 2), 37, 0, flags=1)
    grid_nf = 120 - 14
    assert [(a, b) for a, b, _ in cands] == [(-20 + i // grid_nf, i % grid_nf) for i in range(37)]


def _slots(gpu, n_slots, n_sig, seed, snr=(-20.0, -8.0), fs=12000):
    from ft8_demodulator_amd import _lib
    from ft8_demodulator_amd import ft8_generator as G
    rng = np.random.default_rng(seed)
    N = 15 * fs
    pays = rng.integers(0, 256, size=(n_slots * n_sig, 10), dtype=np.uint8)
    pays[:, 9] &= 0xF8
    _, _, tones = G.encode_batch(pays)
    sig = np.zeros(n_slots * n_sig, dtype=_lib.TX_SIGNAL_DTYPE)
    sig["slot"] = np.repeat(np.arange(n_slots), n_sig)
    sig["f0"] = rng.uniform(200, 2800, sig.size)
    sig["amplitude"] = np.sqrt(2 * 10 ** (rng.uniform(*snr, sig.size) / 10))
    sig["phase"] = rng.uniform(0, 2 * np.pi, sig.size)
    sig["start"] = (rng.uniform(0, 2.0, sig.size) * fs).astype(np.int64)
    g = gpu.Generator(device="cuda")
    g.manual_seed(seed)
    x = gpu.randn((n_slots, N), generator=g, device="cuda", dtype=gpu.float32)
    G.synthesize(tones, sig, n_slots, N, fs, out=x)
    truth = [set(bytes(pays[s * n_sig + i]) for i in range(n_sig)) for s in range(n_slots)]
    return x, truth


@pytest.mark.parametrize("fs", [12000, 24000, 48000])
def test_subtract_clean_signal_residual(gpu, fs):
    """One noiseless signal at an off-grid time and frequency: after decode + subtraction the
    residual holds < 1 % of the signal energy.  24 and 48 kHz: the pulse table (nsps float4s in
    dynamic LDS) exceeds 64 KB there, so both subtraction kernels need their LDS limit raised
    (ADVICE r4)."""
    from ft8_demodulator_amd import _lib
    from ft8_demodulator_amd import ft8_generator as G
    from ft8_demodulator_amd._pipeline import SlotDecoder, make_params
    N = 15 * fs
    pay = np.frombuffer(bytes.fromhex("4a1b9c0e77d2335a10f8"), dtype=np.uint8)
    _, _, tones = G.encode_batch(pay[None])
    sig = np.zeros(1, dtype=_lib.TX_SIGNAL_DTYPE)
    sig["f0"], sig["amplitude"], sig["phase"], sig["start"] = 1012.7, 1.0, 0.4, fs // 2 + 337
    x = G.synthesize(tones, sig, 1, N, fs)
    dec = SlotDecoder(fs, 2, 2, max_candidates=20, min_score=2, flags=_lib.FT8_FLAG_TOPK)
    out, counts = dec.run(x)
    recs = dec.records(x, _lib.FT8_F32)[0]
    assert len(recs) >= 1 and bytes(recs[0]["payload"]) == bytes(pay)
    res = gpu.empty_like(x)
    p = make_params(dec.plan(N), 20, 2, 20, _lib.FT8_FLAG_TOPK)
    ctx = dec.ctx
    import ctypes
    ctx.check(_lib.lib().ft8_subtract(ctx.handle, _lib.ptr(x), _lib.FT8_F32, _lib.ptr(res), N, 1, N, ctypes.byref(p),
                                      _lib.ptr(out), _lib.ptr(counts), dec.cap, _lib.stream_handle()), "ft8_subtract")
    e_sig = float((x.double() ** 2).sum())
    e_res = float((res.double() ** 2).sum())
    assert e_res < 1e-2 * e_sig, e_res / e_sig
    # the same slot as int16 PCM with 40 candidates (above the 32 fits of the first k_sub_est
    # launch, so the rest launch runs), on the same context: the int16 kernels ask for no more LDS
    # than the float32 kernels above were granted, and every kernel needs its own grant
    pcm = (x / x.abs().max() * 32000).round().to(gpu.int16)
    dec16 = SlotDecoder(fs, 2, 2, max_candidates=40, min_score=2, flags=_lib.FT8_FLAG_TOPK, context=ctx)
    out16, counts16 = dec16.run(pcm, _lib.FT8_I16)
    recs16 = dec16.records(pcm, _lib.FT8_I16)[0]
    assert len(recs16) >= 1 and bytes(recs16[0]["payload"]) == bytes(pay)
    res16 = gpu.empty_like(x)
    p16 = make_params(dec16.plan(N), 40, 2, 20, _lib.FT8_FLAG_TOPK)
    ctx.check(_lib.lib().ft8_subtract(ctx.handle, _lib.ptr(pcm), _lib.FT8_I16, _lib.ptr(res16), N, 1, N,
                                      ctypes.byref(p16), _lib.ptr(out16), _lib.ptr(counts16), 40,
                                      _lib.stream_handle()), "ft8_subtract")
    e_sig16 = float(((pcm.double() / 32767) ** 2).sum())
    e_res16 = float((res16.double() ** 2).sum())
    assert e_res16 < 1e-2 * e_sig16, e_res16 / e_sig16


def test_subtract_redecode_crowded(gpu):
    from ft8_demodulator_amd import _lib
    from ft8_demodulator_amd._pipeline import SlotDecoder
    x, truth = _slots(gpu, 4, 40, seed=21)
    kw = dict(sample_rate=12000, bins_per_tone=2, steps_per_symbol=2, max_candidates=150, min_score=2,
              max_iterations=20)
    one = SlotDecoder(**kw, flags=_lib.FT8_FLAG_TOPK).records(x, _lib.FT8_F32)
    two_dec = SlotDecoder(**kw, flags=_lib.FT8_FLAG_TOPK | _lib.FT8_FLAG_SUBTRACT)
    two = two_dec.records(x, _lib.FT8_F32)
    again = two_dec.records(x, _lib.FT8_F32)
    n_new = 0
    for s in range(4):
        p1 = two[s][two[s]["pass_index"] == 0]
        p2 = two[s][two[s]["pass_index"] == 1]
        assert np.array_equal(p1.view(np.uint8), one[s].view(np.uint8)), s   # pass 1 untouched
        assert np.array_equal(two[s].view(np.uint8), again[s].view(np.uint8)), s  # deterministic
        first = set(bytes(r["payload"]) for r in p1)
        for r in p2:
            pb = bytes(r["payload"])
            assert pb not in first
            assert pb in truth[s], (s, pb.hex())
        n_new += len(set(bytes(r["payload"]) for r in p2))
        assert len(first - truth[s]) == 0
    assert n_new >= 2, n_new


def test_subtract_int16_and_batch_consistency(gpu):
    from ft8_demodulator_amd import _lib
    from ft8_demodulator_amd._pipeline import SlotDecoder
    x, truth = _slots(gpu, 3, 25, seed=4)
    pcm = (x / x.abs().max() * 32000).round().to(gpu.int16)
    kw = dict(sample_rate=12000, max_candidates=120, min_score=2, flags=_lib.FT8_FLAG_TOPK | _lib.FT8_FLAG_SUBTRACT)
    dec = SlotDecoder(**kw)
    batch = dec.records(pcm, _lib.FT8_I16)
    for s in range(3):
        single = SlotDecoder(**kw).records(pcm[s:s + 1], _lib.FT8_I16)[0]
        b = batch[s].copy()
        b["slot"] = 0
        assert np.array_equal(b.view(np.uint8), single.view(np.uint8)), s
        assert set(bytes(r["payload"]) for r in batch[s]) <= truth[s]
    # float64 input is refused with a clear error (subtraction supports float32 / int16)
    with pytest.raises(NotImplementedError):
        SlotDecoder(**kw).records(x.double(), _lib.FT8_F64)


def test_subtract_mixed_batch_with_silent_and_dense_slots(gpu):
    """k_sub_list / k_sub_est / k_sub_apply per-slot indexing (round 4): a batch with a silent slot
    (no decodes), a dense one (> 32 distinct decodes, so the rest launch fits some) and an ordinary
    one decodes each slot exactly as that slot alone; the silent slot's residual is its samples."""
    import ctypes
    from ft8_demodulator_amd import _lib
    from ft8_demodulator_amd._pipeline import SlotDecoder, make_params
    from ft8_demodulator_amd import ft8_generator as G
    # the dense slot: 42 strong signals on a 62.5 Hz grid (no two share a channel), staggered starts
    rng = np.random.default_rng(501)
    fs, N, n_sig = 12000, 180000, 42
    pays = rng.integers(0, 256, size=(n_sig, 10), dtype=np.uint8)
    pays[:, 9] &= 0xF8
    _, _, tones = G.encode_batch(pays)
    sig = np.zeros(n_sig, dtype=_lib.TX_SIGNAL_DTYPE)
    sig["f0"] = 200.0 + 62.5 * np.arange(n_sig)
    sig["amplitude"] = np.sqrt(2 * 10 ** (rng.uniform(-5.0, 5.0, n_sig) / 10))
    sig["phase"] = rng.uniform(0, 2 * np.pi, n_sig)
    sig["start"] = (rng.uniform(0.2, 1.5, n_sig) * fs).astype(np.int64)
    g_ = gpu.Generator(device="cuda")
    g_.manual_seed(501)
    xa = gpu.randn((1, N), generator=g_, device="cuda", dtype=gpu.float32)
    G.synthesize(tones, sig, 1, N, fs, out=xa)
    ta = [set(bytes(p_) for p_ in pays)]
    xb, tb = _slots(gpu, 1, 20, seed=502)
    silent = gpu.zeros_like(xa)
    x = gpu.cat([xa, silent, xb]).contiguous()
    kw = dict(sample_rate=12000, max_candidates=300, min_score=2, flags=_lib.FT8_FLAG_TOPK | _lib.FT8_FLAG_SUBTRACT)
    dec = SlotDecoder(**kw)
    batch = dec.records(x, _lib.FT8_F32)
    assert len(batch[1]) == 0
    n_dense = len(set(bytes(r["payload"]) for r in batch[0] if r["pass_index"] == 0))
    assert n_dense > 32, n_dense
    for s in (0, 2):
        single = SlotDecoder(**kw).records(x[s:s + 1], _lib.FT8_F32)[0]
        b = batch[s].copy()
        b["slot"] = 0
        assert np.array_equal(b.view(np.uint8), single.view(np.uint8)), s
        assert set(bytes(r["payload"]) for r in batch[s]) <= (ta[0] if s == 0 else tb[0])
    # the residual of the silent slot is its (zero) samples; the dense slot lost most of its energy
    d1 = SlotDecoder(**dict(kw, flags=_lib.FT8_FLAG_TOPK))
    out, counts = d1.run(x)
    N = x.shape[1]
    p = make_params(d1.plan(N), 300, 2, 20, _lib.FT8_FLAG_TOPK)
    res = gpu.empty_like(x)
    ctx = d1.ctx
    ctx.check(_lib.lib().ft8_subtract(ctx.handle, _lib.ptr(x), _lib.FT8_F32, _lib.ptr(res), N, 3, N, ctypes.byref(p),
                                      _lib.ptr(out), _lib.ptr(counts), d1.cap, _lib.stream_handle()), "ft8_subtract")
    gpu.cuda.synchronize()
    assert float(res[1].abs().max()) == 0.0
    assert float((res[0].double() ** 2).sum()) < float((x[0].double() ** 2).sum())


def test_make_slots_gpu_matches_cpu(gpu):
    """The benchmark generator on the GPU (HIP transmit chain) equals the PyTorch CPU restatement."""
    from ft8_demodulator_amd import synth
    xg, tg = synth.make_slots(2, 12, seed=77, device="cuda")
    xc, tc = synth.make_slots(2, 12, seed=77, device="cpu", noise=False)
    xg0, _ = synth.make_slots(2, 12, seed=77, device="cuda", noise=False)
    assert [t.payloads for t in tg] == [t.payloads for t in tc]
    assert float((xg0.cpu() - xc).abs().max()) < 1e-5
    assert xg.shape == xc.shape and xg.dtype == gpu.float32


def test_subtract_capacity_holds_both_passes(gpu):
    """decode_ft8_message(subtract=True) with a small max_candidates on crowded slots: pass 1 can fill
    all max_candidates rows, so the default capacity (2 x max_candidates) must keep every pass-2
    record; an explicit smaller capacity warns instead of dropping records silently."""
    import warnings
    from ft8_demodulator_amd import SlotDecoder, _lib, decode_ft8_message, synth
    x, _ = synth.make_slots(6, 50, seed=777, device="cuda")
    N = 12
    flags = _lib.FT8_FLAG_TOPK | _lib.FT8_FLAG_SUBTRACT
    dec = SlotDecoder(12000, 2, 2, N, 2, 30, flags=flags)
    assert dec.cap == 2 * N
    out, counts = dec.run(x)
    c = counts.cpu().numpy()
    assert c.max() > N // 2 and c.max() <= 2 * N
    recs = dec.records(x)
    assert [len(r) for r in recs] == list(c)
    assert any((r["pass_index"] == 1).any() for r in recs)
    full = decode_ft8_message(x[int(c.argmax())].cpu().numpy(), 12000, max_candidates=N, min_score=2,
                              max_iterations=30, selection="topk", subtract=True)
    assert len(full) == int(c.max())
    small = SlotDecoder(12000, 2, 2, N, 2, 30, flags=flags, max_results_per_slot=2)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        r2 = small.records(x)
    assert any("max_results_per_slot=2" in str(m.message) for m in w)
    assert all(len(r) <= 2 for r in r2)
    # the warning names this file, the caller of the package, once per call, through however many
    # of the package's own wrappers the call goes
    for method in (small.records, small.texts, small.messages):
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            method(x)
        assert [os.path.abspath(m.filename) for m in w if "max_results_per_slot=2" in str(m.message)] == \
               [os.path.abspath(__file__)], method.__name__
