"""coherent_restate, the NumPy restatement of the coherent re-demodulation (ft8_demodulator_amd/
coherent.py): its gain over the STFT LLRs on weak synthetic slots, and hand cases (CPU only, no library)."""
import numpy as np
import pytest

import coherent_cases as C
from ft8_demodulator_amd import coherent, synth

FS, NSPS, NFFT, HOP = C.FS, C.NSPS, C.NFFT, C.HOP
D = NSPS // 32


def _restate(x, cand, **kw):
    cand = np.asarray(cand).reshape(-1, 2)
    return coherent.coherent_restate(x, cand, np.zeros(len(cand), dtype=np.int32), FS, NSPS, NFFT, 2, **kw)


def test_geometry():
    assert coherent.sub_q(1920) == 32 and coherent.sub_q(1600) == 32 and coherent.sub_q(1921) == 17
    assert coherent.sub_q(2 * 37) == 0
    assert coherent.geometry(1920, 2) == (960, 32, 60, 8, 9)
    assert coherent.geometry(1600, 4) == (400, 32, 50, 4, 5)
    with pytest.raises(ValueError):
        coherent.geometry(1921, 2)          # fs = 12006.3: hop does not divide nsps
    assert coherent.FIT_DTYPE.itemsize == 16
    rec = {"pass_index": 0x12}
    assert coherent.coherent_index(rec) == 1 and coherent.coherent_index({"pass_index": 0x11}) == 0


def test_gain_over_stft_llrs(oracle):
    """16 slots at -22 dB full-band (-18.2 dB in 2500 Hz): the oracle's STFT LLRs decode none of them at
    any of the nine grid points around the truth, the coherent LLRs at the nearest point at least 12
    (the float64 prototype: 15); every decoded payload is the transmitted one."""
    O = oracle
    x, pays, cands = C.weak_slots()
    plain = 0
    for s in range(C.N_WEAK):
        mag = O.waterfall(x[s], FS, 2, 2)
        at, af = cands[s]
        for a in (-1, 0, 1):
            for b in (-1, 0, 1):
                ok, pay = C.decode_llr(O, O.llr(mag, 2, 2, at + a, af + b))[:2]
                assert not ok or pay == pays[s]
                plain += ok
    llr, fits = coherent.coherent_restate(x, np.array(cands), np.arange(C.N_WEAK), FS, NSPS, NFFT, 2)
    assert (fits["status"] == 0).all() and (fits["n_sync"] == 21).all()
    got = 0
    for s in range(C.N_WEAK):
        ok, pay = C.decode_llr(O, llr[s])[:2]
        assert not ok or pay == pays[s]
        got += ok
    print("plain (best of 3 x 3)", plain, "coherent (1 point)", got, "of", C.N_WEAK)
    assert plain == 0
    assert got >= 12


# ---- hand cases -------------------------------------------------------------------------------------------
PAYLOAD = bytes((np.arange(10, dtype=np.uint8) * 37 + 11) & np.array([255] * 9 + [0xF8], dtype=np.uint8))
N = 180000


def test_on_grid_tone_sequence():
    at, af = 12, 400
    x = C.fsk_tones(PAYLOAD, FS, NSPS, af * C.BIN, at * HOP, N)
    llr, fits = _restate(x, [(at, af)])
    f = fits[0]
    assert f["status"] == 0 and f["dt_index"] == 0 and f["dt_s"] == 0.0 and f["n_sync"] == 21
    assert abs(f["df_hz"]) < 0.05
    assert np.array_equal(llr[0] > 0, synth.codeword_bits(PAYLOAD).astype(bool))
    assert abs(np.var(llr[0]) - 24.0) < 1e-9


def test_shifted_tone_sequence():
    at, af = 12, 400
    x = C.fsk_tones(PAYLOAD, FS, NSPS, af * C.BIN + 1.0, at * HOP + 3 * D, N)
    llr, fits = _restate(x, [(at, af)])
    f = fits[0]
    assert f["status"] == 0 and f["dt_index"] == 3 and abs(f["dt_s"] - 3 * D / FS) < 1e-9
    assert f["df_index"] == 3 and abs(f["df_hz"] - 1.0) < 0.1
    assert np.array_equal(llr[0] > 0, synth.codeword_bits(PAYLOAD).astype(bool))


def test_symbols_before_the_slot():
    """abs_time = -20: symbols 0 .. 9 start before sample 0.  Their data symbols (7, 8, 9) give zeros for
    bits 0 .. 8, and only the 14 Costas symbols of the second and third block count."""
    at, af = -20, 400
    x = C.fsk_tones(PAYLOAD, FS, NSPS, af * C.BIN, at * HOP, N)
    llr, fits = _restate(x, [(at, af)])
    f = fits[0]
    assert f["status"] == 0 and f["dt_index"] == 0 and f["n_sync"] == 14
    assert (llr[0][:9] == 0.0).all() and (llr[0][9:] != 0.0).all()
    assert np.array_equal(llr[0][9:] > 0, synth.codeword_bits(PAYLOAD)[9:].astype(bool))
    # one step later dt = 0 still misses symbol 9's first half: at dt >= 0 symbols 0 .. 9 are absent
    _, fits = _restate(x, [(at + 1, af)])
    assert fits[0]["n_sync"] == 14


def test_nothing_to_measure():
    x = C.fsk_tones(PAYLOAD, FS, NSPS, 1250.0, 12 * HOP, N)
    for cand in ((-200, 400), (400, 400)):          # the window wholly outside the slot
        llr, fits = _restate(x, [cand])
        assert fits[0]["status"] == 2 and (llr == 0.0).all()
        blank = np.zeros((), dtype=coherent.FIT_DTYPE)
        blank["status"] = 2
        assert fits[0].tobytes() == blank.tobytes()
    llr, fits = _restate(np.zeros(N, dtype=np.float32), [(12, 400)])   # variance 0
    assert fits[0]["status"] == 2 and (llr == 0.0).all() and fits[0]["n_sync"] == 21
    llr, fits = coherent.coherent_restate(x[None, :], [(12, 400)], [1], FS, NSPS, NFFT, 2)   # no such slot
    assert fits[0]["status"] == 3 and (llr == 0.0).all()


def test_int16_is_scaled_float32():
    x, _, cands = C.weak_slots()
    pcm = np.clip(np.round(x[0] / 8.0 * 32767.0), -32767, 32767).astype(np.int16)
    a = _restate(pcm, [cands[0]])
    b = _restate(pcm.astype(np.float32) / np.float32(32767.0), [cands[0]])
    assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()
    with pytest.raises(NotImplementedError):
        _restate(x[0].astype(np.float64), [cands[0]])


def test_stage_inputs_have_no_near_ties():
    """The inputs of the device's stage test: the restatement alone leaves no candidate out of the
    index comparison (two largest metrics closer than 1e-5 relative), and they hold every case the
    test is about."""
    for case, key in ((C.stage_case_12k(), "f32"), (C.stage_case_12k(), "i16"), (C.stage_case_10k(), "f32")):
        llr, fits, grids = case[key]
        assert not any(coherent.near_tie(g) for g in grids if g is not None)
    _, fits, _ = C.stage_case_12k()["f32"]
    assert (fits["status"] == 0).sum() >= 81 and (fits["status"] == 2).any()
    assert ((fits["n_sync"] > 0) & (fits["n_sync"] < 21)).sum() >= 3
    # the third signal of every slot ends past the slot: from its own grid row on, the last Costas
    # block is incomplete
    for s in range(3):
        assert (fits["n_sync"][27 * s + 21:27 * s + 27] < 21).all()


@pytest.mark.parametrize("argv, want", [(["--coherent"], True), (["--coherent", "8"], 8), (["--coherent", "0"], 0)])
def test_from_wave_coherent_dispatch(monkeypatch, capsys, tmp_path, argv, want):
    """from_wave --coherent [N] goes through _decode_file with coherent = True | N, and a decode's block
    carries the fit's offsets in a `Coherent:` line; no other keyword changes."""
    from ft8_demodulator_amd import from_wave
    from ft8_demodulator_amd.ftx_types import FT8DecodeStatus, FT8Message
    path = str(tmp_path / "slot.wav")
    open(path, "wb").close()
    calls = []
    status = FT8DecodeStatus(ldpc_errors=0, crc_extracted=7, crc_calculated=7)
    results = [(FT8Message(payload=bytearray(PAYLOAD), hash=7), status, 0.5, 1000.0, np.float32(6.0))] * 2

    def decode_file(p, **kw):
        calls.append(kw)
        return results, None, None, [None, (0.015, -0.39)]

    monkeypatch.setattr(from_wave, "_decode_file", decode_file)
    got = from_wave.main([path] + argv)
    out = capsys.readouterr().out
    assert got == results and len(calls) == 1
    assert type(calls[0]["coherent"]) is type(want) and calls[0]["coherent"] == want
    assert calls[0]["snr"] is False and calls[0]["ap"] is None and calls[0]["max_candidates"] == 20
    assert out.count("Coherent: dt +15.00 ms, df -0.39 Hz") == 1 and out.count("Payload:") == 2
