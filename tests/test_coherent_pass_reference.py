"""The coherent pass's record logic restated (coherent.retry_list, coherent.coherent_pass_restate: k_retry_list,
k_coh_merge and retry_accept on the CPU) on hand-made inputs: twelve records in two slots, three sets per listed
candidate, LLR vectors that the oracle's BP either decodes or does not.  No GPU."""
import numpy as np
import pytest

import ap_cases as A
from ft8_demodulator_amd import _lib, coherent, synth

ITERS = A.ITERS
S = 3
CAP = 3
# (slot, cand_index, ok) in the array's order: neither the slots nor a slot's candidates are sorted
LAYOUT = ((1, 3, 0), (0, 2, 0), (0, 0, 1), (1, 0, 0), (0, 5, 0), (0, 1, 0), (1, 1, 1), (0, 3, 0), (0, 6, 0), (1, 4, 0),
          (0, 4, 1), (1, 2, 0))
META = ("score", "slot", "abs_time", "abs_freq", "cand_index")
G0, G1, G2, G3, B0, B1, B2, B3 = range(8)          # four vectors that decode, four that do not


def _bp(x, iters):
    with np.errstate(all="ignore"):
        return A.oracle_lib().bp_decode(x, iters)


def _restate(case, listed, llr, fits, **kw):
    tail = A.oracle_lib().decode_tail
    return coherent.coherent_pass_restate(case["records"], listed, llr, fits, ITERS, _bp, tail, **kw)


@pytest.fixture(scope="module")
def case(oracle):
    """-> the records, the eight vectors with the payloads of the first four, and per (slot, cand_index) the three
    sets' vectors, the fit's status, the validity byte and the drift rate of every failed candidate."""
    rng = np.random.default_rng(11)
    pay = synth.random_payloads(4, rng)
    pay[:, 9] &= 0xF8
    bits = synth.codeword_bits_batch(pay)
    vec = np.concatenate([A.normalize_rows((2.0 * bits - 1.0) + 0.3 * rng.standard_normal(bits.shape)),
                          rng.standard_normal((4, 174))])
    rec = np.zeros(len(LAYOUT), dtype=_lib.RESULT_DTYPE)
    for k, (slot, ci, ok) in enumerate(LAYOUT):
        rec["slot"][k], rec["cand_index"][k], rec["ok"][k] = slot, ci, ok
        rec["score"][k], rec["abs_time"][k], rec["abs_freq"][k] = 2.5 + k, k - 4, 100 + 7 * k
        rec["payload"][k], rec["ldpc_errors"][k] = 0xA0 + k, 0 if ok else 9
    rec["pass_index"][5] = 1                       # (0, 1): a low bit that is the caller's
    plan = {                                       # (slot, cand): (sets, status, valid, rate)
        (0, 1): ((G0, G1, G1), 0, 7, 0.0),         # set 1 decodes: 2, and the later sets do not overwrite it
        (0, 2): ((B0, G1, G2), 0, 5, -0.5),        # set 2 decodes but is not valid; set 3 wins: 10, drifting 14
        (0, 3): ((G3, G3, G3), 2, 7, 0.25),        # no valid fit: stays failed
        (0, 5): ((G0, G0, G0), 0, 7, 0.0),         # beyond the cap of slot 0
        (0, 6): ((B1, B1, B1), 0, 7, 0.0),
        (1, 0): ((G2, B0, B0), 0, 7, 0.25),        # set 1 at another rate: 6
        (1, 2): ((B1, G3, B2), 0, 7, 0.0),         # a later set at rate 0: 10
        (1, 3): ((B2, B3, B0), 0, 7, 0.75),        # nothing decodes
        (1, 4): ((G1, G1, G1), 0, 7, 0.0),         # beyond the cap of slot 1
    }
    rec.setflags(write=False)
    vec.setflags(write=False)
    return {"records": rec, "vec": vec, "pay": pay, "plan": plan}


def _inputs(case, listed):
    """The stage call's results for the listed records -> (llr [n, S, 174], fits, drifts, valid)."""
    rec = case["records"]
    n = len(listed)
    llr, fits = np.zeros((n, S, 174)), np.zeros(n, dtype=coherent.FIT_DTYPE)
    drifts, valid = np.zeros(n, dtype=coherent.DRIFT_DTYPE), np.zeros(n, dtype=np.uint8)
    for pos, i in enumerate(listed):
        sets, fits["status"][pos], valid[pos], drifts["rate_hz_per_s"][pos] = case["plan"][int(rec["slot"][i]),
                                                                                          int(rec["cand_index"][i])]
        llr[pos] = case["vec"][list(sets)]
    return llr, fits, drifts, valid


def _at(rec, slot, ci):
    return rec[(rec["slot"] == slot) & (rec["cand_index"] == ci)][0]


def _decoded(case, r, g):
    return r["ok"] == 1 and bytes(r["payload"]) == bytes(case["pay"][g]) and r["ldpc_errors"] == 0 and \
        r["crc_extracted"] == r["crc_calculated"]


def test_the_vectors_decode_or_fail(case, oracle):
    for g, v in enumerate(case["vec"]):
        plain, err = _bp(v, ITERS)
        ok, pay = oracle.decode_tail(plain, err)[:2]
        assert bool(ok) == (g <= G3), g
        if ok:
            assert bytes(pay) == bytes(case["pay"][g])


def test_list_takes_the_first_cap_failed_per_slot_in_candidate_order(case):
    rec = case["records"]
    listed = coherent.retry_list(rec, CAP)
    assert listed.dtype == np.int64
    got = [(int(rec["slot"][i]), int(rec["cand_index"][i])) for i in listed]
    assert got == [(0, 1), (0, 2), (0, 3), (1, 0), (1, 2), (1, 3)]
    # an ok record is never listed, whatever the cap
    everything = coherent.retry_list(rec)
    assert (rec["ok"][everything] == 0).all() and len(everything) == int((rec["ok"] == 0).sum()) == 9
    assert coherent.retry_list(rec, 100).tolist() == everything.tolist()
    assert [int(rec["cand_index"][i]) for i in coherent.retry_list(rec, 1)] == [1, 0]
    assert len(coherent.retry_list(rec, 0)) == 0


def test_sets_validity_and_drift_bits(case):
    rec = case["records"]
    listed = coherent.retry_list(rec, CAP)
    llr, fits, drifts, valid = _inputs(case, listed)
    out = _restate(case, listed, llr, fits, drifts=drifts, valid=valid)
    want = {(0, 1): (G0, 2 | 1), (0, 2): (G2, 14), (1, 0): (G2, 6), (1, 2): (G3, 10)}
    for (slot, ci), (g, bits) in want.items():
        r = _at(out, slot, ci)
        assert _decoded(case, r, g) and r["pass_index"] == bits, (slot, ci)
    # no valid fit, nothing that decodes, beyond the cap: as they were
    touched = np.array([(int(s), int(c)) in want for s, c in zip(rec["slot"], rec["cand_index"])])
    assert out[~touched].tobytes() == rec[~touched].tobytes()
    assert _at(out, 0, 3)["ok"] == 0 and _at(out, 0, 5)["ok"] == 0 and _at(out, 1, 3)["ok"] == 0
    # the metadata comes back byte for byte, and the input is not modified
    for f in META:
        assert out[f].tobytes() == rec[f].tobytes(), f
    assert not np.shares_memory(out, rec)
    # without the drift records no bit 2; without the validity bytes every set is tried, so set 2 of (0, 2) wins
    out = _restate(case, listed, llr, fits, valid=valid)
    assert [int(_at(out, *k)["pass_index"]) for k in want] == [3, 10, 2, 10]
    out = _restate(case, listed, llr, fits, drifts=drifts)
    assert _decoded(case, _at(out, 0, 2), G1) and _at(out, 0, 2)["pass_index"] == 14


def test_beyond_the_cap_is_decodable_but_stays_failed(case):
    rec = case["records"]
    listed = coherent.retry_list(rec)
    out = _restate(case, listed, *_inputs(case, listed)[:2])
    assert _decoded(case, _at(out, 0, 5), G0) and _decoded(case, _at(out, 1, 4), G1)
    assert _at(out, 0, 6)["ok"] == 0 and _at(out, 0, 3)["ok"] == 0
    assert int(out["ok"].sum()) == 3 + 6


def test_one_set_and_an_ok_record(case):
    """LLRs [n, 174] are one set; a listed record that is ok already is never touched."""
    rec = case["records"]
    listed = coherent.retry_list(rec, CAP)
    llr, fits, drifts, _ = _inputs(case, listed)
    out = _restate(case, listed, llr[:, 0], fits, drifts=drifts)
    assert [int(r["pass_index"]) for r in out[listed]] == [3, 0, 0, 6, 0, 0]
    assert out["ok"][listed].tolist() == [1, 0, 0, 1, 0, 0]
    ok = np.nonzero(rec["ok"])[0][:1]
    good = np.zeros(1, dtype=coherent.FIT_DTYPE)
    out = _restate(case, ok, case["vec"][[G3]], good)
    assert out.tobytes() == rec.tobytes()


def test_nothing_listed_and_no_records(case):
    rec = case["records"]
    none = np.zeros(0, dtype=np.int64)
    fits = np.zeros(0, dtype=coherent.FIT_DTYPE)
    for llr in (np.zeros((0, 174)), np.zeros((0, S, 174))):
        assert _restate(case, none, llr, fits).tobytes() == rec.tobytes()
    empty = rec[:0]
    assert len(coherent.retry_list(empty, CAP)) == 0
    out = coherent.coherent_pass_restate(empty, none, np.zeros((0, 174)), fits, ITERS, _bp, None)
    assert len(out) == 0 and out.dtype == rec.dtype
