"""A-priori decoding on the CPU: the hypotheses ap_hypothesis builds, the clamp, the acceptance test,
and the restatement of the device contract (ap.ap_restate) on the oracle's BP."""
import numpy as np
import pytest

import ap_cases as C
from ft8_demodulator_amd import ap, synth
from ft8_demodulator_amd.message import pack77

PATTERNS = {
    "CQ ? ?": (32, ["CQ K1ABC FN42", "CQ W9XYZ EN37", "CQ JA1XYZ PM95"], "CQ DX K1ABC FN42"),
    "K1ABC ? ?": (32, ["K1ABC W9XYZ EN37", "K1ABC G4ABC -12", "K1ABC JA1XYZ RR73"], "K1ABD W9XYZ EN37"),
    "? K1ABC ?": (32, ["CQ K1ABC FN42", "W9XYZ K1ABC R-07", "G4ABC K1ABC 73"], "W9XYZ K1ABD R-07"),
    "K1ABC W9XYZ ?": (61, ["K1ABC W9XYZ EN37", "K1ABC W9XYZ R+03", "K1ABC W9XYZ RR73"], "K1ABC W9XYA EN37"),
    "K1ABC W9XYZ EN37": (77, ["K1ABC W9XYZ EN37"] * 3, "K1ABC W9XYZ EN38"),
}


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
def test_hypothesis_matches_packed_messages(pattern):
    nbits, matching, other = PATTERNS[pattern]
    mask, value = ap.ap_hypothesis(pattern)
    assert len(mask) == 10 and len(value) == 10 and not (mask[9] | value[9]) & 7
    m = ap.hyp_bits(mask).astype(bool)
    assert int(m.sum()) == nbits
    assert not np.any(ap.hyp_bits(value)[~m])          # value bits only under the mask
    assert m[74:77].all() and list(ap.hyp_bits(value)[74:77]) == [0, 0, 1]   # i3 = 1, always
    for text in matching:
        assert np.array_equal(ap.hyp_bits(pack77(text))[m], ap.hyp_bits(value)[m]), text
    assert not np.array_equal(ap.hyp_bits(pack77(other))[m], ap.hyp_bits(value)[m])


def test_hypothesis_field_layout():
    m = ap.hyp_bits(ap.ap_hypothesis("? K1ABC ?")[0])
    assert list(np.nonzero(m)[0]) == list(range(29, 58)) + [74, 75, 76]
    m = ap.hyp_bits(ap.ap_hypothesis("K1ABC W9XYZ ?")[0])
    assert list(np.nonzero(~m.astype(bool))[0]) == list(range(58, 74))


@pytest.mark.parametrize("bad", ["? ? ?", "CQ ?", "CQ ? FN42", "K1ABC/P ? ?", "CQ DX ? ?", "TOOLONGCALL ? ?", "CQ  ? ?",
                                 "? ?", "HELLO WORLD 73", "", 5])
def test_hypothesis_rejects(bad):
    with pytest.raises(ValueError):
        ap.ap_hypothesis(bad)


def test_ap_llr_hand_made():
    mask, value = ap.ap_hypothesis("CQ ? ?")
    L = np.linspace(-3.0, 4.0, 174)
    out = ap.ap_llr(L, mask, value)
    a = 1.01 * 4.0
    m, v = ap.hyp_bits(mask).astype(bool), ap.hyp_bits(value).astype(bool)
    assert np.array_equal(out[:77][m & v], np.full((m & v).sum(), a))
    assert np.array_equal(out[:77][m & ~v], np.full((m & ~v).sum(), -a))
    assert np.array_equal(out[:77][~m], L[:77][~m]) and np.array_equal(out[77:], L[77:])
    assert out is not L and L[0] == -3.0
    # the largest magnitude may sit on a negative LLR, and beyond the 77 message bits
    L2 = L.copy()
    L2[170] = -9.5
    assert ap.ap_llr(L2, mask, value)[0] == -(1.01 * 9.5)
    # a NaN vector, a vector with one NaN and the zero vector are left alone
    for x in (np.full(174, np.nan), np.where(np.arange(174) == 100, np.nan, L), np.zeros(174)):
        assert np.array_equal(ap.ap_llr(x, mask, value), x, equal_nan=True)


def test_ap_accept_hand_made():
    mask, value = ap.ap_hypothesis("CQ ? ?")
    payload = pack77("CQ K1ABC FN42")
    plain = synth.codeword_bits(payload)
    L = np.where(plain > 0, 2.0, -2.0)
    assert ap.ap_accept(True, payload, plain, L, mask, value, 0) == (True, 0)
    L[[3, 90, 173]] *= -1.0                       # three signs of the unclamped LLRs disagree
    assert ap.ap_accept(True, payload, plain, L, mask, value, 3) == (True, 3)
    assert ap.ap_accept(True, payload, plain, L, mask, value, 2) == (False, 3)
    assert ap.ap_accept(False, payload, plain, L, mask, value, 174) == (False, 3)
    L[5] = 0.0                                    # L > 0 is false for 0: plain bit 5 is 0 for CQ
    assert plain[5] == 0 and ap.ap_accept(True, payload, plain, L, mask, value, 174) == (True, 3)
    other = pack77("K1ABC W9XYZ EN37")            # a valid decode that contradicts the hypothesis
    assert ap.ap_accept(True, other, synth.codeword_bits(other), L, mask, value, 174)[0] is False


def test_ap_index():
    rec = np.zeros(3, dtype=C._lib.RESULT_DTYPE)
    rec["pass_index"] = (0, 1, (3 << 4) | 1)
    assert [ap.ap_index(r) for r in rec] == [0, 0, 3]


@pytest.mark.parametrize("sigma,plain,rescued", [(0.85, 27, 29), (0.95, 12, 19)])
def test_restatement_reproduces_the_measured_rescues(oracle, sigma, plain, rescued):
    """67 stress vectors, 20 iterations, the 32 bits of a CQ ? ? hypothesis taken from each vector's own
    codeword: plain BP decodes 27 (12), AP rescues 29 (19) more, every one the transmitted codeword;
    the CQ hypothesis itself, wrong for these random payloads, rescues none."""
    llr, bits = synth.bp_stress_llrs(67, sigma=sigma, seed=11)
    x = C.normalize_rows(llr)
    rec0 = C.plain_records(x)
    assert int(rec0["ok"].sum()) == plain
    mask, cq = ap.ap_hypothesis("CQ ? ?")
    m = ap.hyp_bits(mask)
    n_resc = 0
    for i in np.nonzero(rec0["ok"] == 0)[0]:
        v = np.zeros(80, dtype=np.uint8)
        v[:77] = bits[i, :77] * m
        out, hard = C.restate(x[i:i + 1], rec0[i:i + 1], [(mask, np.packbits(v).tobytes())], 174)
        if out["ok"][0]:
            n_resc += 1
            assert np.array_equal(ap.hyp_bits(out["payload"][0].tobytes()), bits[i, :77])
            assert ap.ap_index(out[0]) == 1 and hard[0] >= 0
        else:
            assert hard[0] == -1 and out[0].tobytes() == rec0[i].tobytes()
    assert n_resc == rescued
    wrong, hard = C.restate(x, rec0, [(mask, cq)], 174)
    assert np.array_equal(wrong, rec0) and np.all(hard == -1)


def test_stage_case_shows_every_outcome(oracle):
    """The conditions the GPU stage test relies on, on the reference alone."""
    c = C.stage_case()
    idx = c["ref"]["pass_index"] >> 4
    assert int(c["plain"]["ok"].sum()) >= 5 and int((idx > 0).sum()) >= 5 and int((idx == 3).sum()) >= 3
    assert int((idx == 1).sum()) == 0 and int((c["ref"]["ok"] == 0).sum()) >= 5
    rescued = np.nonzero(idx > 0)[0]
    for i in rescued:   # every rescue is the transmitted payload
        assert np.array_equal(c["ref"]["payload"][i], c["payloads"][i])
    med = int(np.median(c["hard"][rescued]))
    lim, hard = C.restate(c["llr"], c["plain"], c["hyps"], med)
    assert 1 <= int((hard >= 0).sum()) < len(rescued)
