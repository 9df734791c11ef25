"""coherent_restate(nsym=...), the NumPy restatement of the coherent pass's joint LLRs over 2 and 3 symbols
(include/ft8hip.h, step 4b): phase continuity, group structure, validity, its gain on weak synthetic slots,
noise, and the Python plumbing (CPU only, no library)."""
import numpy as np
import pytest

import coherent_cases as C
import multisym_cases as M
from ft8_demodulator_amd import coherent, synth

FS, NSPS, NFFT = M.FS, M.NSPS, M.NFFT


def _stage(case, key, fs, nsps, nfft, sps, **kw):
    return coherent.coherent_restate(case["x"] if key == "f32" else case["pcm"], case["cand"], case["slot_of"], fs,
                                     nsps, nfft, sps, **kw)


@pytest.fixture(scope="module")
def stage3():
    """The restatement at max_nsym 3 on stage_case_12k (float32), with details."""
    return _stage(C.stage_case_12k(), "f32", FS, NSPS, NFFT, 2, nsym=3, details=True)


def test_nsym_1_is_todays_restatement(stage3):
    """nsym=1 returns today's arrays exactly; set 1 of nsym=3 equals them exactly (12 kHz and 10 kHz)."""
    c = C.stage_case_12k()
    llr, fits, grids = c["f32"]
    one = _stage(c, "f32", FS, NSPS, NFFT, 2, nsym=1, details=True)
    assert len(one) == 3 and one[0].shape == (85, 174)
    assert one[0].tobytes() == llr.tobytes() and one[1].tobytes() == fits.tobytes()
    l3, f3, v3, g3, rot = stage3
    assert l3.shape == (85, 3, 174) and v3.dtype == np.uint8 and v3.shape == (85,)
    assert np.array_equal(l3[:, 0], llr) and f3.tobytes() == fits.tobytes()
    assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(g3, grids))
    c10 = C.stage_case_10k()
    l10 = coherent.coherent_restate(c10["x"], c10["cand"], c10["slot_of"], C.FS10, C.NSPS10, C.NFFT10, C.SPS10, nsym=3)
    assert np.array_equal(l10[0][:, 0], c10["f32"][0]) and l10[1].tobytes() == c10["f32"][1].tobytes()
    # with the drift search the sets follow the drift records
    d = _stage(c, "f32", FS, NSPS, NFFT, 2, nsym=2, drift=(1.0, 3))
    d1 = _stage(c, "f32", FS, NSPS, NFFT, 2, drift=(1.0, 3))
    assert len(d) == 4 and d[0].shape == (85, 2, 174) and np.array_equal(d[0][:, 0], d1[0])
    assert d[2].tobytes() == d1[2].tobytes() and d[3].dtype == np.uint8


def test_groups():
    """14 pairs and 1 single per half for n = 2, 9 triples and 1 pair for n = 3; in order, all 58 data
    symbols once, no group across a Costas block."""
    for n, sizes in ((1, [1] * 29), (2, [2] * 14 + [1]), (3, [3] * 9 + [2])):
        g = coherent.symbol_groups(n)
        assert [len(v) for v in g] == sizes * 2
        assert tuple(k for v in g for k in v) == coherent.DATA_SYMBOLS
        assert all(v[-1] <= 35 or v[0] >= 43 for v in g)


def test_phase_continuity_on_noiseless_slots(oracle):
    """Noiseless GFSK slots, seeds 77 .. 80: with the true tones the median pair coherence
    |c'_k + c'_{k+1}| / (|c'_k| + |c'_{k+1}|) over the 28 pairs of n = 2 is >= 0.9, and all three sets' hard
    decisions decode to the transmitted payload."""
    x, pays, cands, tones = M.clean_slots()
    llr, fits, valid, grids, rot = coherent.coherent_restate(x, np.array(cands), np.arange(len(x)), FS, NSPS, NFFT, 2,
                                                             nsym=3, details=True)
    assert (valid == 7).all() and (fits["status"] == 0).all()
    assert fits["df_hz"].min() < -0.5 and fits["df_hz"].max() > 1.0
    pairs = [g for g in coherent.symbol_groups(2) if len(g) == 2]
    assert len(pairs) == 28
    for s in range(len(x)):
        cp = rot[s]
        assert cp.shape == (79, 8)
        a = np.array([cp[k, tones[s][k]] for k, _ in pairs])
        b = np.array([cp[k, tones[s][k]] for _, k in pairs])
        med = float(np.median(np.abs(a + b) / (np.abs(a) + np.abs(b))))
        print("seed", M.CLEAN_SEEDS[s], "df", float(fits["df_hz"][s]), "median pair coherence", med)
        assert med >= 0.9
        bits = synth.codeword_bits(pays[s]).astype(bool)
        for n in range(3):
            assert abs(np.var(llr[s, n]) - 24.0) < 1e-9
            assert C.decode_llr(oracle, np.sign(llr[s, n]) * 4.0)[:2] == (True, pays[s]), (s, n)   # the signs alone
            print("  set", n + 1, "hard errors", int(((llr[s, n] > 0) != bits).sum()))


def test_set_structure_absent_symbols_and_status(stage3):
    """174 LLRs per set; the bits of absent symbols are 0 in every set (the stage case's candidates that run
    past the slot, and four more windows off either edge of its first slot); status 2 or 3 gives zeros and a
    validity byte of 0."""
    c = C.stage_case_12k()
    more = np.array([(-20, 700), (-31, 500), (140, 600), (121, 450)], dtype=np.int32)
    extra = coherent.coherent_restate(c["x"], more, [0] * 4, FS, NSPS, NFFT, 2, nsym=3, details=True)
    cand = np.concatenate([c["cand"], more])
    l3, f3, v3 = (np.concatenate([a, b]) for a, b in zip(stage3[:3], extra[:3]))
    rot = stage3[4] + extra[4]
    assert (v3[f3["status"] == 0] == 7).all() and (v3[f3["status"] != 0] == 0).all()
    assert (f3["status"] == 2).any() and (l3[f3["status"] != 0] == 0.0).all()
    hop, Q, D, Mt, Mg = coherent.geometry(NSPS, 2)
    data_k = np.array(coherent.DATA_SYMBOLS)
    seen = 0
    for i in np.flatnonzero(f3["status"] == 0):
        first = (int(cand[i, 0]) * hop - Mg * D) + (Mg + int(f3["dt_index"][i]) + data_k * Q) * D
        absent = (first < 0) | (first + NSPS > c["x"].shape[1])
        if not absent.any():
            continue
        seen += 1
        assert (rot[i][data_k[absent]] == 0).all()
        for n in range(3):
            L = l3[i, n].reshape(58, 3)
            assert (L[absent] == 0.0).all() and (L[~absent] != 0.0).any(axis=1).all()
    assert seen >= 5
    out = coherent.coherent_restate(c["x"], c["cand"][:2], [3, -1], FS, NSPS, NFFT, 2, nsym=3, details=True)
    assert (out[1]["status"] == 3).all() and (out[0] == 0.0).all() and (out[2] == 0).all() and out[4] == [None, None]
    z = coherent.coherent_restate(np.zeros((1, 180000), np.float32), [(12, 400)], [0], FS, NSPS, NFFT, 2, nsym=3)
    assert z[1]["status"][0] == 2 and (z[0] == 0.0).all() and z[2][0] == 0


def test_gain_on_the_weak_slots(oracle):
    """32 slots at -23 dB full-band (-19.2 dB in 2500 Hz), candidates at the nearest grid point: a = set-1
    decodes, u = first-of-three decodes (float64 prototype: 18 and 24; set 2 first on 5 slots, set 3 on 1).
    Every decoded payload is the transmitted one; a <= 20 and u >= a + 4."""
    llr, fits, valid = M.weak_restated()
    _, pays, _ = M.weak_slots()
    assert (fits["status"] == 0).all() and (valid == 7).all()
    first = []
    for s in range(M.N_WEAK):
        for n in range(3):
            ok, pay = C.decode_llr(oracle, llr[s, n])[:2]
            assert not ok or pay == pays[s]
        first.append(M.first_set(oracle, llr[s], valid[s])[0])
    a, u = sum(f == 1 for f in first), sum(f > 0 for f in first)
    print("set 1 decodes", a, "first of three", u, "of", M.N_WEAK, "first sets", first)
    assert a <= 20
    assert u >= a + 4
    later = tuple(M.WEAK_SEED0 + s for s in range(M.N_WEAK) if first[s] > 1)
    assert later == M.LATER_SET_SEEDS


def test_noise_only_slots_decode_nothing(oracle):
    """64 noise-only slots, arbitrary candidates: 0 decodes from 192 attempts."""
    x, cand = M.noise_slots()
    llr, fits, valid = coherent.coherent_restate(x, cand, np.arange(M.N_NOISE), FS, NSPS, NFFT, 2, nsym=3)
    assert (valid == 7).all()
    assert sum(C.decode_llr(oracle, llr[s, n])[0] for s in range(M.N_NOISE) for n in range(3)) == 0


def test_multisymbol_index():
    assert coherent.multisymbol_index({"pass_index": 0x0A}) == 1 and coherent.multisymbol_index({"pass_index": 0x0E}) == 1
    assert coherent.multisymbol_index({"pass_index": 0x06}) == 0 and coherent.multisymbol_index({"pass_index": 0x12}) == 0
    assert coherent.coherent_index({"pass_index": 0x0A}) == 1 and coherent.drift_index({"pass_index": 0x0A}) == 0


@pytest.mark.parametrize("bad", [0, 4, -1, 2.5])
def test_setting_errors(bad):
    """What ft8_set_coherent_nsym answers with FT8_E_ARG is a ValueError before any library call."""
    with pytest.raises(ValueError, match="nsym"):
        coherent.check_nsym(bad)
    with pytest.raises(ValueError, match="nsym"):
        coherent.coherent_restate(np.zeros(4000, np.float32), [(0, 400)], [0], FS, NSPS, NFFT, 2, nsym=bad)
    from ft8_demodulator_amd._pipeline import SlotDecoder
    with pytest.raises(ValueError, match="nsym"):
        SlotDecoder(FS, coherent=4, coherent_nsym=bad)


def test_decoder_settings(monkeypatch):
    """SlotDecoder(coherent_nsym=) needs coherent, and the setter is called before every batch, 1 included."""
    import types
    from ft8_demodulator_amd import _lib, _pipeline
    from ft8_demodulator_amd._pipeline import SlotDecoder
    with pytest.raises(ValueError, match="needs coherent"):
        SlotDecoder(FS, coherent_nsym=2)
    monkeypatch.setattr(_lib, "device_index", lambda device=None: 0)
    assert SlotDecoder(FS, context=object()).coherent_nsym == 1
    assert [coherent.check_nsym(v) for v in (1, 2, 3)] == [1, 2, 3] and coherent.MAX_NSYM == 3

    class Stop(Exception):
        pass

    class Ctx:
        def __init__(self):
            self.calls = []

        def set_coherent(self, m):
            self.calls.append(("cap", m))

        def set_coherent_drift(self, a, r):
            self.calls.append(("drift", a, r))

        def set_coherent_nsym(self, s):
            self.calls.append(("nsym", s))
            raise Stop

    import torch
    monkeypatch.setattr(_pipeline, "make_params", lambda *a: None)
    for S in (1, 3):
        dec = SlotDecoder(FS, coherent=4, coherent_nsym=S, context=Ctx())
        monkeypatch.setattr(dec, "_buffers", lambda n: (None, torch.zeros(n, dtype=torch.int32)))
        monkeypatch.setattr(dec, "plan", lambda n: types.SimpleNamespace(empty=False))
        with pytest.raises(Stop):
            dec.run(torch.zeros(1, 1000), code=_lib.FT8_F32)
        assert dec.ctx.calls == [("cap", 4), ("drift", 0.0, 1), ("nsym", S)]


PAYLOAD = bytes((np.arange(10, dtype=np.uint8) * 37 + 11) & np.array([255] * 9 + [0xF8], dtype=np.uint8))


@pytest.mark.parametrize("argv, want", [(["--coherent", "--coherent-nsym", "3"], 3),
                                        (["--coherent", "8", "--coherent-nsym", "2", "--coherent-drift"], 2),
                                        (["--coherent", "--coherent-nsym", "1"], 1),
                                        (["--coherent"], None)])
def test_from_wave_coherent_nsym_dispatch(monkeypatch, capsys, tmp_path, argv, want):
    """from_wave --coherent-nsym N reaches _decode_file as coherent_nsym = N, and the `Coherent:` line of a
    record with bit 3 ends with `, multi-symbol`, after the drift rate if there is one; without the flag
    neither the keyword nor the text appears."""
    from ft8_demodulator_amd import from_wave
    from ft8_demodulator_amd.ftx_types import FT8DecodeStatus, FT8Message
    path = str(tmp_path / "slot.wav")
    open(path, "wb").close()
    calls = []
    status = FT8DecodeStatus(ldpc_errors=0, crc_extracted=7, crc_calculated=7)
    results = [(FT8Message(payload=bytearray(PAYLOAD), hash=7), status, 0.5, 1000.0, np.float32(6.0))] * 3

    def decode_file(p, **kw):
        calls.append(kw)
        fit = (0.015, -0.39, 0.5) if "coherent_drift" in kw else (0.015, -0.39)
        multi = (from_wave.MULTI_SYMBOL,) if kw.get("coherent_nsym", 1) > 1 else ()
        return results, None, None, [None, fit, fit + multi]

    monkeypatch.setattr(from_wave, "_decode_file", decode_file)
    got = from_wave.main([path] + argv)
    out = capsys.readouterr().out
    assert got == results and len(calls) == 1
    if want is None:
        assert "coherent_nsym" not in calls[0] and "multi-symbol" not in out
        return
    assert calls[0]["coherent_nsym"] == want and calls[0]["max_candidates"] == 20
    drift = ", drift +0.50 Hz/s" if "--coherent-drift" in argv else ""
    line = f"Coherent: dt +15.00 ms, df -0.39 Hz{drift}"
    assert out.count(line) == 2 and out.count(line + ", multi-symbol\n") == (1 if want > 1 else 0)
    assert out.count(line + "\n") == (1 if want > 1 else 2)


def test_from_wave_coherent_nsym_needs_coherent(tmp_path):
    from ft8_demodulator_amd import from_wave
    path = str(tmp_path / "slot.wav")
    open(path, "wb").close()
    with pytest.raises(SystemExit):
        from_wave.main([path, "--coherent-nsym", "2"])
    with pytest.raises(SystemExit):
        from_wave.main([path, "--coherent", "--coherent-nsym", "4"])
