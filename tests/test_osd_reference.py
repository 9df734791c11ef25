"""Ordered-statistics decoding on the CPU: the restatement (osd.osd_restate / osd_pass_restate) against first
principles, on the stage recipe, on noise and on the edge vectors, all on the oracle's BP and decode tail; and
the argument checks of the Python front ends.  No GPU and no library."""
import numpy as np
import pytest

import ap_cases as A
import osd_cases as C
from ft8_demodulator_amd import _lib, ap, osd


@pytest.fixture(scope="module")
def oracle():
    return A.oracle_lib()


# ---- 1. the restatement against first principles -----------------------------------------------------
def gf2_rank(cols):
    """Rank over GF(2) of the column vectors `cols` (a list of uint8 [91]), by plain elimination."""
    rows = [int("".join(map(str, c)), 2) for c in cols]   # each column as an integer
    rank = 0
    while rows:
        p = rows.pop()
        if p:
            rank += 1
            low = p & -p
            rows = [r ^ p if r & low else r for r in rows]
    return rank


def greedy_pivots(perm):
    """Rule 3 by rank tests alone: positions in perm order of the columns that raise the rank."""
    G = osd.generator()
    basis, out = [], []
    for j, c in enumerate(perm):
        if gf2_rank(basis + [G[:, c]]) > len(basis):
            basis.append(G[:, c])
            out.append(j)
            if len(out) == 91:
                break
    return out


def brute_force(r, order):
    """(weight, enumeration index, flips) of rule 5's winner by direct XOR in natural bit order, one candidate
    at a time with a strict <."""
    perm, q, hard = r["perm"], r["q"], r["hard"]
    M = np.zeros_like(r["M"])
    M[:, perm] = r["M"]                                   # rows in natural bit order
    c0 = np.zeros(174, dtype=np.uint8)
    c0[perm] = r["c0"]
    cands = [((), c0)]
    if order >= 1:
        cands += [((k,), c0 ^ M[k]) for k in range(91)]
    if order >= 2:
        cands += [((k1, k2), c0 ^ M[k1] ^ M[k2]) for k1 in range(91) for k2 in range(k1 + 1, 91)]
    assert len(cands) == osd.n_candidates(order)
    best = None
    for e, (flips, c) in enumerate(cands):
        w = int(q[c != hard].sum())
        if best is None or w < best[0]:
            best = (w, e, flips)
    return best, cands


def first_failed(n):
    s = C.stage_vectors()
    return [s["llr"][i] for i in np.nonzero(s["plain"]["ok"] == 0)[0][:n]]


@pytest.mark.parametrize("i", range(8))
def test_restatement_from_first_principles(oracle, i):
    r = osd.osd_restate(first_failed(8)[i], 2)
    assert sorted(r["perm"].tolist()) == list(range(174))
    qp = r["q"][r["perm"]]
    assert all(qp[j] > qp[j + 1] or (qp[j] == qp[j + 1] and r["perm"][j] < r["perm"][j + 1]) for j in range(173))
    assert r["pivots"].tolist() == greedy_pivots(r["perm"])
    assert np.array_equal(r["M"][:, r["pivots"]], np.eye(91, dtype=np.uint8))
    best, cands = brute_force(r, 2)
    assert all(oracle.ldpc_check(c) == 0 for _, c in cands)
    assert (r["weight"], r["index"]) == best[:2]
    assert tuple(k for k in r["flip"] if k >= 0) == best[2] and r["n_flips"] == len(best[2])
    assert np.array_equal(r["codeword"], cands[best[1]][1])
    assert r["n_hard"] == int((r["codeword"] != r["hard"]).sum())
    for order in (0, 1):
        ro = osd.osd_restate(first_failed(8)[i], order)
        assert (ro["weight"], ro["index"]) == brute_force(ro, order)[0][:2]


def test_systematic_basis_reencodes(oracle):
    """The dependent-column-free case: in `flipped` the basis is the 91 message bits, so candidate e is the
    encoding of the hard message bits with the flipped rows' bits inverted."""
    e = C.edge_vectors()
    r = osd.osd_restate(e["llr"][C.EDGE_NAMES.index("flipped")], 2)
    basis = r["perm"][r["pivots"]]
    assert sorted(basis.tolist()) == list(range(91))
    best = None
    pairs = [()] + [(k,) for k in range(91)] + [(a, b) for a in range(91) for b in range(a + 1, 91)]
    for idx, flips in enumerate(pairs):
        msg = r["hard"][:91].copy()
        msg[basis[list(flips)]] ^= 1
        cw = np.unpackbits(np.frombuffer(oracle.ldpc_encode(np.packbits(np.append(msg, [0] * 5)).tobytes()), np.uint8))[:174]
        w = int(r["q"][cw != r["hard"]].sum())
        if best is None or w < best[0]:
            best = (w, idx, flips, cw)
    assert (r["weight"], r["index"], tuple(r["flip"])) == best[:3]
    assert np.array_equal(r["codeword"], best[3])


def test_generator_is_the_encoder(oracle):
    G = osd.generator()
    for k in (0, 1, 45, 63, 64, 90):
        unit = np.zeros(96, dtype=np.uint8)
        unit[k] = 1
        cw = np.unpackbits(np.frombuffer(oracle.ldpc_encode(np.packbits(unit).tobytes()), np.uint8))[:174]
        assert np.array_equal(G[k], cw)


# ---- 2. the stage recipe ------------------------------------------------------------------------------
RESCUED = {0: 2, 1: 7, 2: 26}


def test_plain_bp_on_the_stage_recipe():
    s = C.stage_vectors()
    assert int(s["plain"]["ok"].sum()) == 21
    assert all(bytes(s["plain"]["payload"][i]) == bytes(s["payloads"][i]) for i in np.nonzero(s["plain"]["ok"])[0])


@pytest.mark.parametrize("order", C.ORDERS)
def test_stage_recipe_rescues(order):
    s = C.stage_vectors()
    out, info, cw = (x[:C.STAGE_N] for x in C.expected(order))
    idx = C.rescued(out, s["plain"])
    assert len(idx) == RESCUED[order]
    assert all(bytes(out["payload"][i]) == bytes(s["payloads"][i]) for i in idx)          # all true, none false
    assert all(osd.osd_index(out[i]) and ap.ap_index(out[i]) == 0 and out["ldpc_errors"][i] == 0 for i in idx)
    assert (info["status"][idx] == osd.ACCEPTED).all()
    assert (info["status"][s["plain"]["ok"] == 1] == osd.ALREADY_OK).all()
    untouched = np.setdiff1d(np.arange(C.STAGE_N), idx)
    A.records_equal(out[untouched], s["plain"][untouched])
    if order == 2:
        assert 16 <= int(info["n_hard"][idx].min()) and int(info["n_hard"][idx].max()) <= 28


def test_hard_error_limit_keeps_only_the_close_rescues():
    s = C.stage_vectors()
    out, info, _ = (x[:C.STAGE_N] for x in C.expected(2))
    lim, lim_info, _ = C.restate(s["llr"], s["plain"], 2, 20)
    idx = C.rescued(out, s["plain"])
    keep = idx[info["n_hard"][idx] <= 20]
    assert 0 < len(keep) < len(idx)
    assert C.rescued(lim, s["plain"]).tolist() == keep.tolist()
    A.records_equal(lim[keep], out[keep])
    dropped = np.setdiff1d(idx, keep)
    assert (lim_info["status"][dropped] == osd.REJECTED).all()
    assert np.array_equal(lim_info["weight"], info["weight"]) and np.array_equal(lim_info["flip"], info["flip"])


def test_second_seed():
    """Seed 7 at sigma 0.95: plain BP decodes 2, order 2 adds 22, none false."""
    s = C.stage_vectors(7, C.STAGE_N, 0.95)
    assert int(s["plain"]["ok"].sum()) == 2
    out = C.restate(s["llr"], s["plain"], 2)[0]
    idx = C.rescued(out, s["plain"])
    assert len(idx) == 22 and all(bytes(out["payload"][i]) == bytes(s["payloads"][i]) for i in idx)


# ---- 3. noise -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", (0, 2))
def test_noise_is_not_accepted(order):
    n = C.noise_vectors()
    assert not n["plain"]["ok"].any()
    out, info, _ = C.restate(n["llr"], n["plain"], order)
    assert not out["ok"].any() and (info["status"] == osd.REJECTED).all()
    A.records_equal(out, n["plain"])


# ---- 4. edge vectors ----------------------------------------------------------------------------------
# name -> per order (status, weight, n_hard, flips); the reasons are in osd_cases.edge_vectors.  `flipped`:
# 3 x 768 + 2 x 128 = 2560 would be the true codeword's weight, three flips away; what orders 0 .. 2 reach
# instead is pinned here and checked against re-encoding in test_systematic_basis_reencodes.  `halves`: the
# winners among many equal weights, checked against the strict-< brute force below.
SKIP = (osd.NOT_ATTEMPTED, 0, -1, (-1, -1))
EDGES = {
    "nan": (SKIP,) * 3,
    "zeros": (SKIP,) * 3,
    "tiny": (SKIP,) * 3,
    "minus5": ((osd.REJECTED, 0, 0, (-1, -1)),) * 3,
    "codeword": ((osd.ACCEPTED, 0, 0, (-1, -1)),) * 3,
    "flipped": ((osd.REJECTED, 21248, 43, (-1, -1)), (osd.REJECTED, 15616, 29, (87, -1)),
                (osd.REJECTED, 14080, 23, (25, 77))),
    "inf": ((osd.ACCEPTED, 256, 1, (-1, -1)),) * 3,
    "halves": ((osd.REJECTED, 5632, 44, (-1, -1)), (osd.REJECTED, 3968, 30, (27, -1)),
               (osd.REJECTED, 3072, 22, (40, 48))),
    "already_ok": ((osd.ALREADY_OK, 0, -1, (-1, -1)),) * 3,
}


@pytest.mark.parametrize("order", C.ORDERS)
@pytest.mark.parametrize("name", C.EDGE_NAMES)
def test_edge_vectors(name, order):
    e = C.edge_vectors()
    i = C.EDGE_NAMES.index(name)
    out, info, cw = (x[C.STAGE_N + i] for x in C.expected(order))
    status, weight, n_hard, flips = EDGES[name][order]
    assert (int(info["status"]), int(info["weight"]), int(info["n_hard"]), tuple(info["flip"].tolist())) == \
        (status, weight, n_hard, flips)
    assert int(info["n_flips"]) == sum(k >= 0 for k in flips)
    want = np.array(e["records"][i:i + 1], copy=True)
    if status == osd.ACCEPTED:
        assert np.array_equal(np.unpackbits(cw)[:174], e["bits"])
        want["ok"], want["ldpc_errors"], want["pass_index"] = 1, 0, want["pass_index"] | 0xF0
        want["payload"] = np.frombuffer(C.EDGE_PAYLOAD, dtype=np.uint8)
        crc = A.oracle_lib().crc14(C.EDGE_PAYLOAD + b"\0\0", 82)
        want["crc_extracted"] = want["crc_calculated"] = crc
    if status in (osd.NOT_ATTEMPTED, osd.ALREADY_OK):
        assert not cw.any()
    if name == "minus5":
        assert not cw.any()          # the all-zero codeword: the tail passes it, rule 6 does not
    A.records_equal(out.reshape(1), want)


def test_inf_and_clipping():
    q, hard = osd.reliabilities(C.edge_vectors()["llr"][C.EDGE_NAMES.index("inf")])
    assert (q[:50] == 65535).all() and set(q[50:].tolist()) == {512, 256} and q[C.INF_ERROR] == 256
    assert osd.reliabilities([1.0 / 256] + [0.0] * 173)[0][0] == 1
    assert osd.reliabilities([255.99609375] + [0.0] * 173)[0][0] == 65535
    assert osd.reliabilities([255.9921875] + [0.0] * 173)[0][0] == 65534


@pytest.mark.parametrize("order", C.ORDERS)
def test_equal_q_pins_the_tie_breaks(order):
    """`halves` has two distinct q: perm is the stable order, and at orders 1 and 2 the winner is the first of
    three candidates of the smallest weight."""
    r = osd.osd_restate(C.edge_vectors()["llr"][C.EDGE_NAMES.index("halves")], order)
    assert set(r["q"].tolist()) == {128, 256}
    assert r["perm"].tolist() == sorted(range(174), key=lambda i: (-int(r["q"][i]), i))
    best, cands = brute_force(r, order)
    assert (r["weight"], r["index"]) == best[:2]
    ties = [e for e, (_, c) in enumerate(cands) if int(r["q"][c != r["hard"]].sum()) == best[0]]
    assert len(ties) == (1, 3, 3)[order] and ties[0] == r["index"]


def test_ap_index_is_zero_for_the_osd_mark():
    rec = np.zeros(1, dtype=_lib.RESULT_DTYPE)
    for pi, want in ((0x00, 0), (0x10, 1), (0x80, 8), (0x32, 3), (0xF0, 0), (0xF1, 0)):
        rec["pass_index"] = pi
        assert ap.ap_index(rec[0]) == want and osd.osd_index(rec[0]) == (pi >> 4 == 15)


# ---- 5. the Python front ends ---------------------------------------------------------------------------
def test_slot_decoder_osd_arguments(monkeypatch):
    from ft8_demodulator_amd._pipeline import SlotDecoder
    monkeypatch.setattr(_lib, "device_index", lambda device=None: 0)
    for bad in (3, -1, 1.5, "2", (2,), (2, -1), (3, 4), (2, 1.5), (1, 2, 3)):
        with pytest.raises(ValueError):
            SlotDecoder(12000, osd=bad, context=object())
    for bad in (-1, 175, 2.5):
        with pytest.raises(ValueError):
            SlotDecoder(12000, osd=True, osd_max_hard_errors=bad, context=object())
    for arg, want in ((None, None), (False, None), (True, (2, 32)), (0, (0, 32)), (1, (1, 32)), ((2, 0), (2, 0)),
                      ((1, 100), (1, 100))):
        dec = SlotDecoder(12000, osd=arg, context=object())
        assert dec.osd == want and bool(dec.flags & _lib.FT8_FLAG_OSD) == (want is not None)
        assert dec.osd_max_hard_errors == 36
    assert SlotDecoder(12000, osd=True, osd_max_hard_errors=174, context=object()).osd_max_hard_errors == 174


def test_slot_decoder_sets_osd_before_the_batch(monkeypatch):
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
                if name == "set_osd":
                    raise Stop
            return setter

    dec = _pipeline.SlotDecoder(12000, osd=(1, 7), osd_max_hard_errors=40, context=Ctx())
    monkeypatch.setattr(dec, "_buffers", lambda n: (None, torch.zeros(n, dtype=torch.int32)))
    monkeypatch.setattr(dec, "plan", lambda n: types.SimpleNamespace(empty=False))
    with pytest.raises(Stop):
        dec.run(torch.zeros(1, 1000), code=_lib.FT8_F32)
    assert dec.ctx.calls == [("set_osd", 1, 7, 40)]


@pytest.mark.parametrize("argv", [["--osd", "3"], ["--osd", "2:-1"], ["--osd", "x"], ["--osd-max-hard-errors", "20"],
                                  ["--osd", "--osd-max-hard-errors", "175"]])
def test_from_wave_refuses_bad_osd_arguments(tmp_path, argv):
    from ft8_demodulator_amd import from_wave
    with pytest.raises(SystemExit):
        from_wave.main([str(tmp_path / "x.wav")] + argv)


def test_from_wave_osd_dispatch_and_mark(monkeypatch, capsys, tmp_path):
    """--osd reaches _decode_file (True for the bare flag, (order, n) else), and a decode it produced prints its
    `OSD: order k` line and no `AP:` line."""
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
        return (res, None, ["CQ ? ?", None] if kw.get("ap") else None) + (([None, 1],) if "osd" in kw else ())

    monkeypatch.setattr(from_wave, "_decode_file", fake)
    from_wave.main([str(path), "--osd", "1:8", "--ap", "CQ ? ?", "--osd-max-hard-errors", "30"])
    assert calls[-1]["osd"] == (1, 8) and calls[-1]["osd_max_hard_errors"] == 30
    blocks = [b for b in capsys.readouterr().out.split("-" * 50) if "Payload" in b]
    assert "AP: CQ ? ?\n" in blocks[0] and "OSD:" not in blocks[0]
    assert "OSD: order 1\n" in blocks[1] and "AP:" not in blocks[1]
    from_wave.main([str(path), "--osd"])
    assert calls[-1]["osd"] is True and "osd_max_hard_errors" not in calls[-1]
    from_wave.main([str(path), "--osd", "0"])
    assert calls[-1]["osd"] == (0, 32)
    capsys.readouterr()
    from_wave.main([str(path), "--snr"])
    assert "osd" not in calls[-1] and "OSD:" not in capsys.readouterr().out
