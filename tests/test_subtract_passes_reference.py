"""The host side of the n-pass subtraction (ft8_demodulator_amd/subtract.py, the CLI's new flags), on
the CPU: the merge's restatement against oracle/subtract.py merge, the marks an appended row keeps,
the pass of a row from the per-pass counts, the pass-count check and the parser's errors."""
import numpy as np
import pytest

import subtract_cases as C


def _lists():
    """The nine record lists of tests/subtract_cases.py (pass_index 0 throughout), as each slot lists them."""
    _, records, counts, _ = C.batch()
    out = [records[s, :min(int(counts[s]), C.CAP)].copy() for s in range(C.N_SLOTS)]
    assert len(out) == 9 and all(np.all(r["pass_index"] == 0) for r in out)
    return out


def test_merge_restate_equals_oracle_merge():
    """Every ordered pair of the nine lists (failed rows, good duplicates, empty lists and the list of 132
    included), as (accumulated, this pass's): the restatement gives the oracle's merge byte for byte."""
    from ft8_demodulator_amd.subtract import merge_restate
    from oracle import subtract as OS
    lists = _lists()
    appended = 0
    for a in lists:
        for b in lists:
            want, got = OS.merge(a, b), merge_restate(a, b)
            assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
            appended += len(got) - len(a)
    assert appended > 0
    # both slots of one row name carry the same payloads: nothing new; the inputs are left as they were
    assert len(merge_restate(lists[0], lists[2])) == len(lists[0])
    assert all(np.all(r["pass_index"] == 0) for r in lists)


def test_merge_restate_keeps_the_marks_of_appended_rows():
    """An appended row keeps bits 1 to 3 and the high nibble of pass_index and gains bit 0; accumulated
    rows are not touched; a failed row is never appended; two new rows of one payload both are, and a
    row whose payload a FAILED accumulated row carries is not (k_merge compares every row present)."""
    from ft8_demodulator_amd import _lib
    from ft8_demodulator_amd.subtract import merge_restate, subtract_index
    acc = np.zeros(3, dtype=_lib.RESULT_DTYPE)
    acc["payload"][:, 0] = [1, 2, 3]
    acc["ok"] = [1, 1, 0]
    acc["pass_index"] = [0, 0x22, 0]
    marks = [0x00, 0x02, 0x06, 0x0A, 0x0E, 0x30, 0x81, 0x00, 0x02, 0x00]
    recs = np.zeros(len(marks), dtype=_lib.RESULT_DTYPE)
    recs["payload"][:, 0] = [10, 11, 12, 13, 14, 15, 16, 1, 3, 10]
    recs["ok"] = [1, 1, 1, 1, 0, 1, 1, 1, 1, 1]
    recs["pass_index"] = marks
    recs["cand_index"] = np.arange(len(marks))
    before = recs.copy()
    out = merge_restate(acc, recs)
    assert out[:3].tobytes() == acc.tobytes() and recs.tobytes() == before.tobytes()
    tail = out[3:]
    assert list(tail["cand_index"]) == [0, 1, 2, 3, 5, 6, 9]
    assert list(tail["pass_index"]) == [0x01, 0x03, 0x07, 0x0B, 0x31, 0x81, 0x01]
    assert [subtract_index(r) for r in out] == [0, 0, 0] + [1] * 7
    for r in tail:
        src = before[int(r["cand_index"])]
        assert int(r["pass_index"]) & 0xFE == int(src["pass_index"]) & 0xFE
        for name in ("score", "abs_time", "abs_freq", "payload", "ok", "ldpc_errors"):
            assert np.array_equal(r[name], src[name])
    # chained: the third pass sees the second pass's rows as accumulated
    again = merge_restate(out, recs)
    assert again.tobytes() == out.tobytes()


def test_pass_of():
    from ft8_demodulator_amd.subtract import pass_of
    counts = [3, 3, 5, 6]
    assert [pass_of(counts, i) for i in range(6)] == [1, 1, 1, 3, 3, 4]
    assert pass_of(np.array([0, 2], dtype=np.int32), 1) == 2
    assert pass_of([4], 3) == 1
    for bad in (6, 7, -1):
        with pytest.raises(IndexError):
            pass_of(counts, bad)
    with pytest.raises(IndexError):
        pass_of([0, 0, 0], 0)


def test_check_passes():
    from ft8_demodulator_amd import _lib
    from ft8_demodulator_amd.subtract import MAX_PASSES, check_passes, passes_of
    assert MAX_PASSES == _lib.FT8_SUBTRACT_MAX_PASSES == 4
    assert [check_passes(n) for n in (2, 3, 4, np.int32(3))] == [2, 3, 4, 3]
    for bad in (1, 5, 0, -2, 2.0, 3.5, "3", None, True):
        with pytest.raises(ValueError):
            check_passes(bad)
    assert passes_of(None) is None and passes_of(False) is None and passes_of(True) == 2 and passes_of(4) == 4
    with pytest.raises(ValueError):
        passes_of(5)


def test_selection_flags_take_a_pass_count():
    from ft8_demodulator_amd import _lib
    from ft8_demodulator_amd.ft8_decode import selection_flags
    assert selection_flags("topk", 3) == _lib.FT8_FLAG_TOPK | _lib.FT8_FLAG_SUBTRACT
    assert selection_flags("reference", True) == _lib.FT8_FLAG_SUBTRACT
    assert selection_flags("topk") == _lib.FT8_FLAG_TOPK and selection_flags() == 0
    with pytest.raises(ValueError):
        selection_flags("topk", 5)


def test_from_wave_parser(monkeypatch, capsys, tmp_path):
    """--selection / --subtract reach _decode_file (no GPU touched), a later pass's decode gets its
    `Pass: k` line, and what the library would refuse is a parser error."""
    from ft8_demodulator_amd import from_wave
    from ft8_demodulator_amd.ftx_types import FT8DecodeStatus, FT8Message
    path = str(tmp_path / "slot.wav")
    open(path, "wb").close()
    status = FT8DecodeStatus(ldpc_errors=0, crc_extracted=7, crc_calculated=7)
    results = [(FT8Message(payload=bytearray(10), hash=7), status, 0.5, 1000.0, np.float32(6.0))] * 3
    calls = []

    def decode_file(p, **kw):
        calls.append(kw)
        out = (results, None, None)
        if kw.get("coherent") is not None:
            out += ([None, (0.015, -0.39), None],)
        if kw.get("subtract") is not None:
            out += ([1, 1, 3],)
        return out

    def unexpected(*a, **kw):
        raise AssertionError("the plain paths do not take the new flags")

    monkeypatch.setattr(from_wave, "_decode_file", decode_file)
    monkeypatch.setattr(from_wave, "decode_ft8_from_wave", unexpected)
    monkeypatch.setattr(from_wave, "_decode_many", unexpected)
    cases = [(["--subtract"], dict(subtract=2), 1), (["--subtract", "3", "--selection", "topk"],
                                                    dict(subtract=3, selection="topk"), 1),
             (["--selection", "topk"], dict(selection="topk"), 0),
             (["--subtract", "4", "--coherent", "8", "--ap", "CQ ? ?"], dict(subtract=4, coherent=8, ap=["CQ ? ?"]), 1)]
    for argv, want, n_pass in cases:
        calls.clear()
        got = from_wave.main([path] + argv)
        out = capsys.readouterr().out
        assert got == results and len(calls) == 1
        assert {k: calls[0].get(k) for k in want} == want, argv
        assert ("subtract" in calls[0]) == ("subtract" in want) and ("selection" in calls[0]) == ("selection" in want)
        assert out.count("Pass: 3") == n_pass and out.count("Pass:") == n_pass and out.count("Payload:") == 3
        assert out.count("Coherent:") == (1 if "coherent" in want else 0)
    for argv in (["--subtract", "1"], ["--subtract", "5"], ["--subtract", "x"], ["--subtract", "--snr"],
                 ["--subtract", "3", "--snr"], ["--selection", "best"]):
        calls.clear()
        with pytest.raises(SystemExit) as e:
            from_wave.main([path] + argv)
        assert e.value.code == 2 and not calls, argv
        assert "error" in capsys.readouterr().err
