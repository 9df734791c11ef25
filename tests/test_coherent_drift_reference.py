"""The drift search of the coherent re-demodulation in its NumPy restatement
(coherent.coherent_restate(drift=...)): hand cases, its gain on drifting weak slots against the oracle's
BP, the settings' errors, synth's drift, and from_wave's dispatch (CPU only, no GPU)."""
import numpy as np
import pytest

import coherent_cases as C
import drift_cases as Dc
from ft8_demodulator_amd import coherent, synth

FS, NSPS, NFFT, HOP = C.FS, C.NSPS, C.NFFT, C.HOP
PAYLOAD = bytes((np.arange(10, dtype=np.uint8) * 37 + 11) & np.array([255] * 9 + [0xF8], dtype=np.uint8))
N = 180000
AT, AF = 12, 400


def _restate(x, cand, **kw):
    cand = np.asarray(cand).reshape(-1, 2)
    return coherent.coherent_restate(x, cand, np.zeros(len(cand), dtype=np.int32), FS, NSPS, NFFT, 2, **kw)


def _hand(rate):
    """A noiseless tone sequence drifting by `rate` at the grid point (12, 400) + 0.5 Hz + 120 samples
    -> (sign errors and LLRs of today's call, sign errors, LLRs and drift record of the search)."""
    x = Dc.fsk_tones_drift(PAYLOAD, FS, NSPS, AF * C.BIN + 0.5, AT * HOP + 120, N, rate)
    bits = synth.codeword_bits(PAYLOAD).astype(bool)
    l0, f0 = _restate(x, [(AT, AF)])
    l1, f1, d1 = _restate(x, [(AT, AF)], drift=Dc.DRIFT)
    assert f0[0]["status"] == 0 and f1[0]["status"] == 0 and f1[0]["n_sync"] == 21
    return int(((l0[0] > 0) != bits).sum()), l0[0], int(((l1[0] > 0) != bits).sum()), l1[0], d1[0]


def test_rates_and_records():
    assert coherent.DRIFT_DTYPE.itemsize == 8
    assert coherent.drift_rates(1.0, 9).tolist() == [-1.0, -0.75, -0.5, -0.25, 0.0, 0.25, 0.5, 0.75, 1.0]
    r = coherent.drift_rates(4.0, 33)
    assert len(r) == 33 and r[0] == -4.0 and r[16] == 0.0 and r[32] == 4.0 and np.allclose(np.diff(r), 0.25)
    assert coherent.drift_rates(0.3, 3).tolist() == [-float(np.float32(0.3)), 0.0, float(np.float32(0.3))]
    assert coherent.drift_rates(2.0, 1).tolist() == [0.0] and coherent.drift_rates(0.0, 9).tolist() == [0.0]
    assert coherent.drift_index({"pass_index": 6}) == 1 and coherent.drift_index({"pass_index": 0x12}) == 0
    assert coherent.coherent_index({"pass_index": 6}) == 1


def test_hand_rate_zero_equals_the_plain_call():
    e0, l0, e1, l1, d = _hand(0.0)
    assert d["rate_index"] == 4 and d["rate_hz_per_s"] == 0.0
    assert e0 == 0 and e1 == 0 and np.array_equal(l0, l1)


def test_hand_rate_plus_one():
    """+1.0 Hz/s, two tones over the slot: today's call has sign errors (22), the search none."""
    e0, _, e1, l1, d = _hand(1.0)
    assert d["rate_index"] == 8 and d["rate_hz_per_s"] == 1.0
    assert e1 == 0 and e0 > 0
    assert abs(np.var(l1) - 24.0) < 1e-9


def test_hand_negative_rate_rescues_bp(oracle):
    e0, l0, e1, l1, d = _hand(-0.75)
    assert d["rate_index"] == 1 and d["rate_hz_per_s"] == -0.75 and e1 == 0
    assert not C.decode_llr(oracle, l0)[0]
    ok, pay = C.decode_llr(oracle, l1)[:2]
    assert ok and pay == PAYLOAD


def test_hand_rate_between_two_hypotheses():
    _, _, e1, _, d = _hand(0.6)
    assert d["rate_index"] == 6 and d["rate_hz_per_s"] == 0.5 and e1 == 0


def test_search_off_is_the_plain_call():
    """R = 1 or A = 0 with a drift argument: the plain LLRs and fits, zeros in the drift records."""
    x = Dc.fsk_tones_drift(PAYLOAD, FS, NSPS, AF * C.BIN + 0.5, AT * HOP + 120, N, 0.5)
    l0, f0 = _restate(x, [(AT, AF), (400, 400)])
    for off in ((2.0, 1), (0.0, 9)):
        l1, f1, d1, vol = _restate(x, [(AT, AF), (400, 400)], drift=off, details=True)
        assert np.array_equal(l0, l1) and f0.tobytes() == f1.tobytes()
        assert d1.tobytes() == np.zeros(2, coherent.DRIFT_DTYPE).tobytes()
        assert vol[0].shape == (1, 17, 5) and vol[1] is None
    # nothing to measure and no such slot: zeros in the drift record with the search on, too
    _, f1, d1 = coherent.coherent_restate(x[None, :], [(400, 400), (AT, AF)], [0, 1], FS, NSPS, NFFT, 2, drift=Dc.DRIFT)
    assert f1["status"].tolist() == [2, 3] and d1.tobytes() == np.zeros(2, coherent.DRIFT_DTYPE).tobytes()


def test_drift_none_is_unchanged():
    """drift=None returns two arrays, byte-equal on stage_case_12k to the call without the argument (the
    one coherent_cases makes), and a search of the single rate 0 reproduces them bit for bit."""
    c = C.stage_case_12k()
    got = coherent.coherent_restate(c["x"], c["cand"], c["slot_of"], FS, NSPS, NFFT, 2, drift=None)
    assert len(got) == 2
    llr, fits, _ = c["f32"]
    assert got[0].tobytes() == llr.tobytes() and got[1].tobytes() == fits.tobytes()
    l1, f1, _ = coherent.coherent_restate(c["x"], c["cand"][:12], c["slot_of"][:12], FS, NSPS, NFFT, 2, drift=(0.0, 1))
    assert l1.tobytes() == llr[:12].tobytes() and f1.tobytes() == fits[:12].tobytes()


def test_gain_over_the_plain_coherent_pass(oracle):
    """16 one-signal slots drifting by 0.5 Hz/s at -23 dB full-band (-19.2 dB in 2500 Hz; at -22 dB synth's
    GFSK does not separate the two: 8 and 16), each at the grid point nearest the truth: the oracle's BP
    decodes at most 2 from today's coherent LLRs (float64: 0) and at least 14 - 3 from the LLRs of the
    search over (1.0, 9) (float64: 14); every decoded payload is the transmitted one."""
    x, pays, cands = Dc.gain_slots()
    so = np.arange(Dc.N_GAIN)
    l0, f0 = coherent.coherent_restate(x, np.array(cands), so, FS, NSPS, NFFT, 2)
    l1, f1, d1 = coherent.coherent_restate(x, np.array(cands), so, FS, NSPS, NFFT, 2, drift=Dc.DRIFT)
    assert (f1["status"] == 0).all() and (f1["n_sync"] == 21).all()
    plain = got = 0
    for s in range(Dc.N_GAIN):
        for llr in (l0[s], l1[s]):
            ok, pay = C.decode_llr(oracle, llr)[:2]
            assert not ok or pay == pays[s]
        plain += C.decode_llr(oracle, l0[s])[0]
        got += C.decode_llr(oracle, l1[s])[0]
    print("coherent", plain, "with the drift search", got, "of", Dc.N_GAIN, "rates", d1["rate_index"].tolist())
    assert plain <= 2
    assert got >= 14 - 3
    assert (np.abs(d1["rate_hz_per_s"] - Dc.GAIN_RATE) <= 0.25).all()


def test_stage_inputs_have_no_near_ties():
    """The inputs of the device's stage test, on the restatement alone: no metric volume whose two
    largest values are closer than 1e-5 relative, so the device's index comparison leaves out no
    candidate; and they hold the cases the test is about."""
    cases = [Dc.stage_case_12k("f32"), Dc.stage_case_12k("i16"), Dc.stage_case_wide()[2], Dc.stage_case_10k()["ref"]]
    for llr, fits, drifts, vols in cases:
        assert not any(coherent.near_tie(v, 1e-5) for v in vols if v is not None)
    llr, fits, drifts, vols = cases[0]
    assert vols[0].shape == (9, 17, 5) and cases[2][3][0].shape == (33, 17, 5) and cases[3][3][0].shape == (9, 9, 5)
    assert (fits["status"] == 0).sum() >= 81 and (fits["status"] == 2).any()
    assert ((fits["n_sync"] > 0) & (fits["n_sync"] < 21)).sum() >= 3
    for s in range(3):
        # at the truth's own grid point: the static signal at rate 0, +1.0 at index 8, -0.6 at -0.5 or -0.75
        assert drifts["rate_index"][27 * s + 4] == 4 and drifts["rate_index"][27 * s + 13] == 8
        assert drifts["rate_index"][27 * s + 22] in (1, 2)
        assert 0 < fits["n_sync"][27 * s + 22] < 21                      # the late signal's last Costas block
    # the widest search finds the same rates on its finer grid: 0, +1.0 and -0.5 / -0.75 of 33 over +-4
    wide = cases[2][2]["rate_hz_per_s"]
    assert wide[4] == 0.0 and wide[13] == 1.0 and wide[22] in (-0.5, -0.75)
    d10 = cases[3][2]["rate_index"]
    assert d10[4] == 4 and d10[13] == 8


@pytest.mark.parametrize("bad", [(1.0, 8), (1.0, 35), (-0.5, 9), (4.5, 9), (1.0, 0), (float("nan"), 9)])
def test_setting_errors(bad):
    with pytest.raises(ValueError):
        coherent.drift_rates(*bad)
    x = np.zeros(4000, dtype=np.float32)
    with pytest.raises(ValueError):
        _restate(x, [(0, 400)], drift=bad)
    from ft8_demodulator_amd._pipeline import SlotDecoder
    with pytest.raises(ValueError):
        SlotDecoder(FS, coherent=4, coherent_drift=bad)


def test_decoder_settings():
    from ft8_demodulator_amd._pipeline import SlotDecoder
    with pytest.raises(ValueError, match="needs coherent"):
        SlotDecoder(FS, coherent_drift=True)
    assert coherent.DEFAULT_DRIFT == (1.0, 9)


def test_synth_drift():
    """drift_hz_per_s=None is bit-identical to the call without it; a drift moves the instantaneous
    frequency linearly about the waveform's centre and draws nothing from the generators."""
    import torch
    a, ta = synth.make_slots(1, 2, fs=FS, seeds=[31])
    b, tb = synth.make_slots(1, 2, fs=FS, seeds=[31], drift_hz_per_s=None)
    c, tc = synth.make_slots(1, 2, fs=FS, seeds=[31], drift_hz_per_s=[0.0, 1.0])
    assert torch.equal(a, b) and ta[0].f0 == tc[0].f0 and ta[0].payloads == tc[0].payloads
    assert not torch.equal(a, c)
    tones = torch.zeros(1, 79, dtype=torch.int64)
    f0 = torch.tensor([1000.0])
    w0 = synth.gfsk_waveforms(tones, FS, f0)
    assert torch.equal(w0, synth.gfsk_waveforms(tones, FS, f0, None))
    w = synth.gfsk_waveforms(tones, FS, f0, 2.0).numpy()
    # instantaneous frequency from the analytic signal, away from the ramps: 1000 + 2 (t - t_c)
    spec = np.fft.fft(w[0])
    spec[len(spec) // 2:] = 0.0
    ph = np.unwrap(np.angle(np.fft.ifft(2.0 * spec)))
    f = np.diff(ph) * FS / (2.0 * np.pi)
    n = len(w[0])
    for k in (n // 4, n // 2, 3 * n // 4):
        assert abs(f[k - 200:k + 200].mean() - (1000.0 + 2.0 * (k - n / 2) / FS)) < 0.05


@pytest.mark.parametrize("argv, want", [(["--coherent", "--coherent-drift"], True),
                                        (["--coherent", "8", "--coherent-drift", "2"], (2.0, 9)),
                                        (["--coherent", "--coherent-drift", "0.5:5"], (0.5, 5))])
def test_from_wave_coherent_drift_dispatch(monkeypatch, capsys, tmp_path, argv, want):
    """from_wave --coherent-drift [MAX[:N]] reaches _decode_file as coherent_drift = True | (MAX, N), and
    the decode's `Coherent:` line ends with the rate; without the flag neither the keyword nor the text
    appears."""
    from ft8_demodulator_amd import from_wave
    from ft8_demodulator_amd.ftx_types import FT8DecodeStatus, FT8Message
    path = str(tmp_path / "slot.wav")
    open(path, "wb").close()
    calls = []
    status = FT8DecodeStatus(ldpc_errors=0, crc_extracted=7, crc_calculated=7)
    results = [(FT8Message(payload=bytearray(PAYLOAD), hash=7), status, 0.5, 1000.0, np.float32(6.0))] * 2

    def decode_file(p, **kw):
        calls.append(kw)
        fit = (0.015, -0.39, 0.5) if "coherent_drift" in kw else (0.015, -0.39)
        return results, None, None, [None, fit]

    monkeypatch.setattr(from_wave, "_decode_file", decode_file)
    got = from_wave.main([path] + argv)
    out = capsys.readouterr().out
    assert got == results and len(calls) == 1
    assert calls[0]["coherent_drift"] == want and type(calls[0]["coherent_drift"]) is type(want)
    assert out.count("Coherent: dt +15.00 ms, df -0.39 Hz, drift +0.50 Hz/s\n") == 1 and out.count("Payload:") == 2
    from_wave.main([path, "--coherent"])
    out = capsys.readouterr().out
    assert "coherent_drift" not in calls[1] and out.count("Coherent: dt +15.00 ms, df -0.39 Hz\n") == 1
    with pytest.raises(SystemExit):
        from_wave.main([path, "--coherent-drift"])
    capsys.readouterr()
