"""FT4 on the CPU: the protocol's constants, the transmit chain of ft4.py, the host geometry and the restated
receive chain on a NumPy STFT.  The last is the condition that keeps the GPU tests honest: the slots
test_gpu_ft4.py decodes must be decodable by the definition itself, and the retry slot must hold rescues of
both kinds."""
import ctypes

import numpy as np
import pytest

import ft4_cases as C


def test_rvec_packs_to_its_hex():
    from ft8_demodulator_amd import ft4
    assert ft4.FT4_RVEC.hex() == "4a5e89b4b08a7955be28"
    bits = np.unpackbits(np.frombuffer(ft4.FT4_RVEC, dtype=np.uint8))
    assert len(bits[:77]) == 77 and not bits[77:].any()      # 77 bits, MSB first; the low 3 bits of byte 9 are 0
    assert np.packbits(np.concatenate([bits[:77], np.zeros(3, np.uint8)])).tobytes() == ft4.FT4_RVEC


def test_sync_rows_are_distinct_permutations():
    from ft8_demodulator_amd import ft4
    rows = ft4.FT4_COSTAS
    assert len(rows) == 4
    for r in rows:
        assert sorted(r) == [0, 1, 2, 3]
    assert len(set(rows)) == 4


def test_symbol_map_covers_the_frame_once():
    from ft8_demodulator_amd import ft4
    sync = [s0 + k for s0 in ft4.FT4_SYNC_START for k in range(4)]
    assert sorted(sync + list(ft4.FT4_DATA_SYMBOL)) == list(range(103))
    assert len(ft4.FT4_DATA_SYMBOL) == 87 and ft4.FT4_GRAY == (0, 1, 3, 2)


def test_zero_message_scrambles_to_rvec():
    from ft8_demodulator_amd import ft4, synth
    assert ft4.ft4_scramble(bytes(10)) == ft4.FT4_RVEC
    assert ft4.ft4_scramble(ft4.ft4_scramble(b"\x12\x34\x56\x78\x9a\xbc\xde\xf0\x11\x20")) == \
        b"\x12\x34\x56\x78\x9a\xbc\xde\xf0\x11\x20"
    # CRC and parity are over the scrambled bits
    assert np.array_equal(ft4.ft4_codeword_bits(bytes(10)), synth.codeword_bits(ft4.FT4_RVEC))
    tones = ft4.ft4_itones(bytes(10))
    assert tones.shape == (103,) and tones.max() <= 3
    for m, s0 in enumerate(ft4.FT4_SYNC_START):
        assert tuple(tones[s0:s0 + 4]) == ft4.FT4_COSTAS[m]


@pytest.mark.parametrize("fs", [12000, 6000])
def test_waveform_shape_envelope_and_frequency(fs):
    from ft8_demodulator_amd import ft4, synth
    nsps = ft4.ft4_nsps(fs)
    assert nsps == fs * 6 // 125
    rng = np.random.default_rng(4)
    tones = ft4.ft4_itones(synth.random_payload(rng))
    f0 = 1000.0
    w = ft4.ft4_waveforms(tones[None, :], fs, [f0])[0].numpy()
    assert w.shape == (105 * nsps,)
    env = ft4.ft4_envelope(nsps)
    assert np.all(env[nsps:-nsps] == 1.0) and env[0] == 0.0 and np.all(np.diff(env[:nsps]) > 0)
    assert np.array_equal(env[-nsps:], env[:nsps][::-1])
    assert np.max(np.abs(w)) <= 1.0 + 1e-12
    # the instantaneous frequency, rebuilt here pulse by pulse: symbol j's pulse covers the waveform samples
    # [j nsps, (j + 3) nsps).  At each symbol centre it is within 1e-3 of a tone spacing of f0 + tone (the
    # BT = 1 pulse's centre value is erf(2.67) ~ 0.9998 and the neighbours' tails add ~ 1e-4 of their tones)
    p = synth._pulse(nsps, bt=ft4.FT4_BT).numpy()
    freq = np.zeros(105 * nsps)
    for j in range(103):
        freq[j * nsps:(j + 3) * nsps] += float(tones[j]) * p
    centres = (np.arange(103) + 1) * nsps + nsps // 2
    assert np.max(np.abs(freq[centres] - tones)) <= 1e-3
    # ... and the waveform is the sine of that frequency's running sum (phase 0 at the first sample)
    dphi = 2.0 * np.pi / fs * (f0 + fs / nsps * freq)
    phi = np.concatenate([[0.0], np.cumsum(dphi[:-1])])
    assert np.max(np.abs(w - env * np.sin(phi))) <= 1e-9


def test_geometry_proto():
    from ft8_demodulator_amd import _lib, ft4
    v = [ctypes.c_int32() for _ in range(4)]
    L = _lib.lib()
    rc = L.ft8_geometry_proto(_lib.FT8_PROTO_FT4, 12000.0, 2, 2, 90000, *[ctypes.byref(x) for x in v])
    assert rc == 0 and tuple(x.value for x in v) == (576, 288, 1152, 311)
    assert ft4.ft4_geometry(12000, 2, 2, 90000) == (576, 288, 1152, 311)
    assert L.ft8_geometry_proto(_lib.FT8_PROTO_FT4, 44100.0, 2, 2, 90000, *[ctypes.byref(x) for x in v]) \
        == _lib.FT8_E_UNSUPPORTED
    assert L.ft8_geometry_proto(2, 12000.0, 2, 2, 90000, *[ctypes.byref(x) for x in v]) == _lib.FT8_E_ARG
    # protocol 0 is ft8_geometry_hz
    w = [ctypes.c_int32() for _ in range(4)]
    assert L.ft8_geometry_proto(_lib.FT8_PROTO_FT8, 12000.0, 2, 2, 180000, *[ctypes.byref(x) for x in v]) == 0
    assert L.ft8_geometry_hz(12000.0, 2, 2, 180000, *[ctypes.byref(x) for x in w]) == 0
    assert [x.value for x in v] == [x.value for x in w]
    with pytest.raises(NotImplementedError):
        _lib.geometry(44100, 2, 2, 90000, _lib.FT8_PROTO_FT4)
    with pytest.raises(ValueError):
        ft4.ft4_nsps(44100)


def test_params_field_lists_agree():
    """ft8_params.reserved became `protocol` in the header and in both bindings together."""
    import os
    import re
    from ft8_demodulator_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "ft8hip.h")).read()
    body = hdr[hdr.index("typedef struct ft8_params {"):hdr.index("} ft8_params;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in re.findall(r"(?:int32_t|double)\s+([^;]+);", body) for n in re.split(r"\s*,\s*", decl.strip())]
    assert names == [f[0] for f in _lib.Ft8Params._fields_]
    assert "protocol" in names and "reserved" not in names


def test_normalize_is_the_oracles(oracle):
    from ft8_demodulator_amd import ft4
    rng = np.random.default_rng(6)
    for _ in range(20):
        x = rng.normal(0, 7, 174)
        assert np.array_equal(ft4.ft4_normalize(x), oracle.normalize(x))


def test_restated_chain_decodes_every_signal(oracle):
    """The e2e slots of test_gpu_ft4.py through a NumPy float32 STFT and the restated chain, under both
    selections: every transmitted payload is decoded, nothing false, nothing from noise or silence."""
    from ft8_demodulator_amd import ft4
    x, want, _ = C.e2e_slots()
    for topk, kw in ((True, C.E2E_TOPK), (False, C.E2E_HEAP)):
        for b in range(x.shape[0]):
            wf = ft4.ft4_stft_restate(x[b].numpy(), C.FS, C.BPT, C.SPS, np.float32)
            assert wf.shape == (311, 576)
            out, _, _ = C.restate(wf, oracle, topk, slot=b, **kw)
            assert {bytes(p) for p in out["payload"]} == want[b], (topk, b)


def test_restated_retry_slot_has_both_kinds_of_rescue(oracle):
    from ft8_demodulator_amd import ap, ft4
    x, pays = C.retry_slot()
    wf = ft4.ft4_stft_restate(x[0].numpy(), C.FS, C.BPT, C.SPS, np.float32)
    hyps = [ap.ap_hypothesis(p) for p in C.RETRY_AP]
    out, _, _ = C.restate(wf, oracle, True, hyps=hyps, osd=C.RETRY_OSD, **C.RETRY)
    kinds = [int(r["pass_index"]) >> 4 for r in out]
    n_ap, n_osd = sum(1 for k in kinds if 0 < k < 15), kinds.count(15)
    print("plain", kinds.count(0), "ap", n_ap, "osd", n_osd)
    assert n_ap >= 2 and n_osd >= 2
    got = {bytes(p) for p in out["payload"]}
    assert got <= {bytes(p) for p in pays}                   # no false decode
    plain, _, _ = C.restate(wf, oracle, True, **C.RETRY)
    assert len(got) > len({bytes(p) for p in plain["payload"]})    # the retries add messages
