"""The a-priori retries on the coherent LLRs restated (coherent.coherent_ap_restate; include/ft8hip.h,
"coherent_ap"): the record logic on scripted decode functions, the contract on the oracle's BP with
ap_cases.stage_case()'s vectors as the second of two sets, and the Python front ends' argument checks.  No GPU."""
import numpy as np
import pytest

import ap_cases as A
import coherent_ap_cases as K
from ft8_demodulator_amd import _lib, coherent

ITERS = 20
META = ("score", "slot", "abs_time", "abs_freq", "cand_index")
S = 3
BIG = 2.0                      # every vector's largest magnitude: a = 2.02
GOOD = bytes([0xFF, 0x00]) + bytes(8)     # agrees with both hypotheses below


def _hyp(byte, value):
    mask = bytearray(10)
    val = bytearray(10)
    mask[byte], val[byte] = 0xFF, value
    return bytes(mask), bytes(val)


HYPS = [_hyp(0, 0xFF), _hyp(1, 0x00)]     # h = 0 knows bits 0 .. 7 (ones), h = 1 bits 8 .. 15 (zeros)


def _vector(pos, n):
    """Set n of position pos: the signs agree with both hypotheses on bits 0 .. 15, element 170 carries BIG and
    element 173 names (pos, n)."""
    v = np.full(174, -0.5)
    v[:8] = 0.5
    v[170] = BIG
    v[173] = 0.01 * (10 * pos + n + 1)
    return v


class Script:
    """bp_decode / decode_tail that log every attempt as (pos, h, n) and answer from `plan`:
    (pos, h, n) -> (ok, payload, flips); flips hard decisions are turned over past bit 80."""

    def __init__(self, plan):
        self.plan, self.log, self.last = plan, [], None

    def bp(self, llr, iters):
        assert iters == ITERS and llr.shape == (174,)
        tag = int(round(float(llr[173]) / 0.01)) - 1
        pos, n = divmod(tag, 10)
        a = 1.01 * BIG
        clamped = np.nonzero(np.abs(llr[:77]) == a)[0].tolist()
        h = {tuple(range(8)): 0, tuple(range(8, 16)): 1}[tuple(clamped)]
        assert (llr[clamped] == (a if h == 0 else -a)).all() and llr[170] == BIG
        self.last = (pos, h, n)
        self.log.append(self.last)
        plain = (llr > 0).astype(np.uint8)
        flips = self.plan.get(self.last, (False, GOOD, 0))[2]
        plain[80:80 + flips] ^= 1
        return plain, 3 + h

    def tail(self, plain, err):
        ok, payload, _ = self.plan.get(self.last, (False, GOOD, 0))
        return ok, payload, 0x1234, 0x1234 if ok else 0x0001


def _records(n):
    rec = np.zeros(n, dtype=_lib.RESULT_DTYPE)
    rec["slot"], rec["cand_index"] = 1, np.arange(n)[::-1]
    rec["score"], rec["abs_time"], rec["abs_freq"] = 2.5 + np.arange(n), np.arange(n) - 4, 100 + 7 * np.arange(n)
    rec["payload"], rec["ldpc_errors"] = 0xA0, 9
    return rec


def _run(plan, n=4, ok=(), status=None, valid=None, drifts=None, llr=None, max_hard=174, listed=None):
    rec = _records(n)
    rec["ok"][list(ok)] = 1
    listed = np.arange(n) if listed is None else np.asarray(listed)
    m = len(listed)
    if llr is None:
        llr = np.stack([[_vector(p, s) for s in range(S)] for p in range(m)])
    fits = K.all_fits(m)
    if status is not None:
        fits["status"] = status
    sc = Script(plan)
    out, hard = coherent.coherent_ap_restate(rec, listed, llr, fits, HYPS, ITERS, max_hard, sc.bp, sc.tail, drifts=drifts,
                                             valid=valid)
    assert hard.dtype == np.int16 and len(hard) == len(out) == n and not np.shares_memory(out, rec)
    for f in META:
        assert out[f].tobytes() == rec[f].tobytes(), f
    return rec, out, hard, sc.log


def test_attempt_order_is_hypothesis_outer_set_inner():
    rec, out, hard, log = _run({}, n=2)
    assert log == [(p, h, s) for p in range(2) for h in range(2) for s in range(S)]
    assert out.tobytes() == rec.tobytes() and (hard == -1).all()


def test_first_accepted_attempt_wins_and_ends_the_position():
    plan = {(0, 0, 1): (True, GOOD, 0), (0, 0, 2): (True, GOOD, 0), (0, 1, 0): (True, GOOD, 0),
            (1, 1, 0): (True, GOOD, 0), (1, 1, 2): (True, GOOD, 0)}
    rec, out, hard, log = _run(plan, n=3)
    assert log == [(0, 0, 0), (0, 0, 1)] + [(1, 0, s) for s in range(S)] + [(1, 1, 0)] + \
        [(2, h, s) for h in range(2) for s in range(S)]
    assert out["ok"].tolist() == [1, 1, 0]
    assert out["pass_index"].tolist() == [2 | 8 | (1 << 4), 2 | (2 << 4), 0]
    assert bytes(out["payload"][0]) == GOOD and out["crc_extracted"][0] == out["crc_calculated"][0] == 0x1234
    assert out["ldpc_errors"].tolist() == [3, 4, 9]            # the attempt's, by hypothesis
    assert hard.tolist() == [0, 0, -1]
    assert out[2].tobytes() == rec[2].tobytes()


def test_ok_records_and_invalid_fits_are_not_tried():
    plan = {(p, h, s): (True, GOOD, 0) for p in range(4) for h in range(2) for s in range(S)}
    rec, out, hard, log = _run(plan, ok=(1,), status=[0, 0, 2, 3])
    assert log == [(0, 0, 0)]
    assert out[1:].tobytes() == rec[1:].tobytes() and hard.tolist() == [0, -1, -1, -1]
    assert out["pass_index"][0] == 2 | (1 << 4)


def test_validity_bits_skip_their_sets_only():
    rec, out, hard, log = _run({(1, 1, 2): (True, GOOD, 0)}, n=3, valid=np.array([5, 4, 0], dtype=np.uint8))
    assert log == [(0, 0, 0), (0, 0, 2), (0, 1, 0), (0, 1, 2), (1, 0, 2), (1, 1, 2)]
    assert out["pass_index"].tolist() == [0, 2 | 8 | (2 << 4), 0]
    # one set [n, 174]: no validity bytes, the fit's status alone
    rec, out, hard, log = _run({}, n=2, llr=np.stack([_vector(p, 0) for p in range(2)]), status=[2, 0])
    assert log == [(1, 0, 0), (1, 1, 0)]


def test_nan_and_zero_sets_are_skipped_for_every_hypothesis():
    llr = np.stack([[_vector(p, s) for s in range(S)] for p in range(2)])
    llr[0, 0, 100] = np.nan
    llr[1, 1] = 0.0
    rec, out, hard, log = _run({(0, 1, 1): (True, GOOD, 0)}, n=2, llr=llr)
    assert log == [(0, 0, 1), (0, 0, 2), (0, 1, 1), (1, 0, 0), (1, 0, 2), (1, 1, 0), (1, 1, 2)]
    assert out["pass_index"].tolist() == [2 | 8 | (2 << 4), 0]


def test_mask_disagreement_rejects():
    wrong0 = bytes([0x7F, 0x00]) + bytes(8)        # bit 0 disagrees with h = 0; fine for h = 1
    free = bytes([0xFF, 0x00, 0x55]) + bytes(7)    # bits outside both masks are free
    plan = {(0, 0, 0): (True, wrong0, 0), (0, 1, 1): (True, wrong0, 0), (1, 0, 0): (True, free, 0)}
    rec, out, hard, log = _run(plan, n=2)
    assert log[:5] == [(0, 0, 0), (0, 0, 1), (0, 0, 2), (0, 1, 0), (0, 1, 1)]
    assert out["pass_index"].tolist() == [2 | 8 | (2 << 4), 2 | (1 << 4)]
    assert bytes(out["payload"][0]) == wrong0 and bytes(out["payload"][1]) == free


def test_hard_errors_count_against_the_winning_sets_unclamped_llrs():
    """Set 1's signs disagree with h = 0 on three masked bits, which the clamp overrides: 3 hard errors that only the
    unclamped set shows; 4 flips more make 7.  At the limit it is accepted, one below it is not."""
    llr = np.stack([[_vector(0, s) for s in range(S)]])
    llr[0, 1, :3] = -0.5
    plan = {(0, 0, 1): (True, GOOD, 4), (0, 1, 2): (True, GOOD, 1)}
    rec, out, hard, log = _run(plan, n=1, llr=llr, max_hard=7)
    assert hard.tolist() == [7] and out["pass_index"][0] == 2 | 8 | (1 << 4) and log[-1] == (0, 0, 1)
    rec, out, hard, log = _run(plan, n=1, llr=llr, max_hard=6)
    assert hard.tolist() == [1] and out["pass_index"][0] == 2 | 8 | (2 << 4) and log[-1] == (0, 1, 2)
    rec, out, hard, log = _run(plan, n=1, llr=llr, max_hard=0)
    assert hard.tolist() == [-1] and out.tobytes() == rec.tobytes() and len(log) == 6


def test_pass_index_bits_and_metadata():
    drifts = np.zeros(4, dtype=coherent.DRIFT_DTYPE)
    drifts["rate_hz_per_s"] = [0.0, -0.25, 0.5, 0.0]
    plan = {(0, 0, 0): (True, GOOD, 0), (1, 0, 0): (True, GOOD, 0), (2, 1, 2): (True, GOOD, 0), (3, 1, 1): (True, GOOD, 0)}
    rec = _records(4)
    rec["pass_index"] = 1                                  # a low bit that is the caller's
    sc = Script(plan)
    llr = np.stack([[_vector(p, s) for s in range(S)] for p in range(4)])
    out, hard = coherent.coherent_ap_restate(rec, np.arange(4), llr, K.all_fits(4), HYPS, ITERS, 174, sc.bp, sc.tail,
                                             drifts=drifts)
    assert out["pass_index"].tolist() == [1 | 2 | 16, 1 | 2 | 4 | 16, 1 | 2 | 4 | 8 | 32, 1 | 2 | 8 | 32]
    for f in META:
        assert out[f].tobytes() == rec[f].tobytes(), f
    # without drift records no bit 2
    sc = Script(plan)
    out, _ = coherent.coherent_ap_restate(rec, np.arange(4), llr, K.all_fits(4), HYPS, ITERS, 174, sc.bp, sc.tail)
    assert out["pass_index"].tolist() == [19, 19, 43, 43]


def test_listed_is_an_indirection_and_hard_is_indexed_like_records():
    plan = {(0, 0, 0): (True, GOOD, 2), (1, 1, 0): (True, GOOD, 0)}
    rec, out, hard, log = _run(plan, n=6, listed=[4, 1])
    assert out["ok"].tolist() == [0, 1, 0, 0, 1, 0] and hard.tolist() == [-1, 0, -1, -1, 2, -1]
    assert out["pass_index"][4] == 18 and out["pass_index"][1] == 34


def test_empty_inputs():
    none = np.zeros(0, dtype=np.int64)
    for llr in (np.zeros((0, 174)), np.zeros((0, S, 174))):
        rec, out, hard, log = _run({}, n=3, listed=none, llr=llr)
        assert out.tobytes() == rec.tobytes() and (hard == -1).all() and log == []
    out, hard = coherent.coherent_ap_restate(_records(0), none, np.zeros((0, 174)), K.all_fits(0), HYPS, ITERS, 174, None,
                                             None)
    assert len(out) == 0 and out.dtype == _lib.RESULT_DTYPE and len(hard) == 0
    rec = _records(2)
    out, hard = coherent.coherent_ap_restate(rec, np.arange(2), np.zeros((2, S, 174)), K.all_fits(2), [], ITERS, 174, None,
                                             None)
    assert out.tobytes() == rec.tobytes()                  # no hypotheses: nothing to try


# ---- on the oracle's BP ---------------------------------------------------------------------------------
def test_contract_on_the_oracle(oracle):
    """ap_cases.stage_case()'s 67 vectors as set 1 behind a noisier set 0 of the same codewords, the three stage
    hypotheses: every rescue carries the transmitted payload, some come from the later set, some from h > 0, and a
    hard-error limit rejects some of them."""
    r = K.stage_reference()
    ref, hard, plain = r["ref"], r["hard"], r["records"]
    pay = A.stage_case()["payloads"]
    pi = ref["pass_index"]
    rescued = np.nonzero(pi != 0)[0]
    n_later, n_high = int(((pi & 8) != 0).sum()), int(((pi >> 4) > 1).sum())
    print("plain decodes", int(plain["ok"].sum()), "rescues", len(rescued), "from the later set", n_later, "at h > 0",
          n_high, "still failed", int((ref["ok"] == 0).sum()))
    assert len(rescued) >= 5 and n_later >= 1 and n_high >= 1 and int(((pi[rescued] & 8) == 0).sum()) >= 1
    assert all((pi[rescued] & 2) != 0) and all(plain["ok"][rescued] == 0)
    assert all(bytes(ref["payload"][i]) == bytes(pay[i]) for i in rescued)
    assert (hard[rescued] >= 0).all() and (np.delete(hard, rescued) == -1).all()
    keep = np.ones(len(ref), dtype=bool)
    keep[rescued] = False
    assert ref[keep].tobytes() == plain[keep].tobytes()
    # the winner is the first accepted attempt: no earlier (h, n) of a rescue decodes to an accepted record
    i = int(rescued[np.argmax(pi[rescued] >> 4)])
    h_win, n_win = (int(pi[i]) >> 4) - 1, int(pi[i] >> 3) & 1
    one = K.stage_restate(r["llr"][[i]], plain[[i]], list(r["hyps"])[:h_win], 174)[0]
    assert one["ok"][0] == 0
    if n_win:
        first = K.stage_restate(r["llr"][[i], :1], plain[[i]], list(r["hyps"])[:h_win + 1], 174)[0]
        assert first["ok"][0] == 0
    med = int(np.median(hard[rescued]))
    lim, lim_hard = K.stage_restate(r["llr"], plain, list(r["hyps"]), med)
    assert 1 <= int((lim_hard >= 0).sum()) < len(rescued) and int(lim_hard.max()) <= med


# ---- the Python front ends ------------------------------------------------------------------------------
def test_slot_decoder_needs_both_passes(monkeypatch):
    from ft8_demodulator_amd._pipeline import SlotDecoder
    monkeypatch.setattr(_lib, "device_index", lambda device=None: 0)
    for kw in (dict(), dict(ap=["CQ ? ?"]), dict(coherent=4), dict(ap=["CQ ? ?"], coherent=False)):
        with pytest.raises(ValueError, match="coherent_ap needs both ap and coherent"):
            SlotDecoder(12000, coherent_ap=True, context=object(), **kw)
    assert SlotDecoder(12000, context=object()).coherent_ap is False
    assert SlotDecoder(12000, ap=["CQ ? ?"], coherent=4, coherent_ap=True, context=object()).coherent_ap is True


def test_slot_decoder_sets_it_before_every_batch(monkeypatch):
    """Like the other coherent settings: a decoder that never mentions it sets 0."""
    import types
    import torch
    from ft8_demodulator_amd import _pipeline
    monkeypatch.setattr(_lib, "device_index", lambda device=None: 0)
    monkeypatch.setattr(_pipeline, "make_params", lambda *a: None)

    class Stop(Exception):
        pass

    class Ctx:
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            def setter(*a):
                self.calls.append((name,) + a)
                if name == "set_coherent_ap":
                    raise Stop
            return setter

    for kw, want in ((dict(), False), (dict(coherent_ap=False), False), (dict(coherent_ap=True), True)):
        dec = _pipeline.SlotDecoder(12000, ap=["CQ ? ?"], coherent=4, context=Ctx(), **kw)
        monkeypatch.setattr(dec, "_buffers", lambda n: (None, torch.zeros(n, dtype=torch.int32)))
        monkeypatch.setattr(dec, "plan", lambda n: types.SimpleNamespace(empty=False))
        for _ in range(2):
            with pytest.raises(Stop):
                dec.run(torch.zeros(1, 1000), code=_lib.FT8_F32)
        assert [c for c in dec.ctx.calls if c[0] == "set_coherent_ap"] == [("set_coherent_ap", want)] * 2
        assert dec.ctx.calls[-2][0] == "set_coherent_nsym"


@pytest.mark.parametrize("argv", [["--coherent-ap"], ["--coherent-ap", "--ap", "CQ ? ?"], ["--coherent-ap", "--coherent"]])
def test_from_wave_coherent_ap_needs_both(tmp_path, argv, capsys):
    from ft8_demodulator_amd import from_wave
    with pytest.raises(SystemExit):
        from_wave.main([str(tmp_path / "x.wav")] + argv)
    assert "--coherent-ap needs --ap and --coherent" in capsys.readouterr().err


def test_from_wave_coherent_ap_dispatch_and_both_marks(monkeypatch, capsys, tmp_path):
    """--coherent-ap reaches _decode_file as coherent_ap=True (and is absent without the flag), and a block whose
    record carries both marks prints its `AP:` line and its `Coherent:` line."""
    from ft8_demodulator_amd import from_wave
    from ft8_demodulator_amd.ftx_types import FT8DecodeStatus, FT8Message
    path = tmp_path / "x.wav"
    path.write_bytes(b"")
    calls = []

    def fake(p, **kw):
        calls.append(kw)
        msg, st = FT8Message(), FT8DecodeStatus()
        msg.payload = bytes(10)
        res = [(msg, st, 1.0, 500.0, 3.0)] * 2
        return res, None, ["CQ ? ?", None], [(0.015, -0.39), (0.0, 0.25)]

    monkeypatch.setattr(from_wave, "_decode_file", fake)
    from_wave.main([str(path), "--ap", "CQ ? ?", "--coherent", "8", "--coherent-ap"])
    out = capsys.readouterr().out
    assert calls[0]["coherent_ap"] is True and calls[0]["coherent"] == 8 and calls[0]["ap"] == ["CQ ? ?"]
    blocks = [b for b in out.split("-" * 50) if "Payload" in b]
    assert len(blocks) == 2
    assert "AP: CQ ? ?\n" in blocks[0] and "Coherent: dt +15.00 ms, df -0.39 Hz\n" in blocks[0]
    assert "AP: " not in blocks[1] and "Coherent: dt +0.00 ms, df +0.25 Hz\n" in blocks[1]
    from_wave.main([str(path), "--ap", "CQ ? ?", "--coherent", "8"])
    assert "coherent_ap" not in calls[1]
