"""A-priori (AP) decoding: hypotheses, the LLR clamp and the acceptance test, in NumPy.

A candidate that belief propagation fails on is retried with the message bits a receiver already
knows (CQ in the first call field, its own callsign, the station it works) clamped to certainty.
The device runs the retries (csrc/ap.hip, ft8_ap_decode / FT8_FLAG_AP); this module builds the
hypotheses and restates the contract of include/ft8hip.h for tests and tools.  Nothing here runs on
the decode path.

Field layout of a standard (i3 = 1) message, payload bit 0 = MSB of byte 0:
n28a 0-27, ipa 28, n28b 29-56, ipb 57, ir 58, igrid4 59-73, i3 74-76.
"""
from __future__ import annotations

import numpy as np

from . import message

AP_SCALE = 1.01               # a = AP_SCALE * max |L|
DEFAULT_MAX_HARD_ERRORS = 36  # WSJT-X's nharderrors limit; measurements in DESIGN.md section 11

_CALL_A = (0, 29)    # n28a + ipa
_CALL_B = (29, 58)   # n28b + ipb
_I3 = (74, 77)


def _bits_to_bytes(bits77: np.ndarray) -> bytes:
    b = np.zeros(80, dtype=np.uint8)
    b[:77] = bits77
    return np.packbits(b).tobytes()


def hyp_bits(mask_or_value) -> np.ndarray:
    """10 bytes of a hypothesis (or a payload) -> its 77 bits, MSB first."""
    return np.unpackbits(np.frombuffer(bytes(mask_or_value), dtype=np.uint8))[:77]


def _call_field(tok: str) -> int:
    """One token as the call field of a standard message -> n28 (ip = 0)."""
    got = [(n28, sfx, j) for n28, sfx, j in message._std_calls([tok], 0)]
    if len(got) != 1 or got[0][1] or got[0][2] != 1:
        raise ValueError(f"not a call field of a standard message: {tok!r}")
    return got[0][0]


def ap_hypothesis(pattern: str):
    """A pattern over the three fields of a standard message -> (mask bytes, value bytes), 10 each.

    `?` frees a whole field: "CQ ? ?", "K1ABC ? ?", "? K1ABC ?", "K1ABC W9XYZ ?", or a full text
    ("CQ K1ABC FN42").  A known call fixes its n28 and ip bits, i3 is always fixed to 1, `?` as the
    last field frees bits 58-73.  ValueError for anything else."""
    if not isinstance(pattern, str):
        raise ValueError("pattern must be a str")
    tok = pattern.split(" ")
    if not all(tok):
        raise ValueError(f"single spaces only: {pattern!r}")
    mask = np.zeros(77, dtype=np.uint8)
    value = np.zeros(77, dtype=np.uint8)
    mask[_I3[0]:_I3[1]] = 1
    value[_I3[0]:_I3[1]] = (0, 0, 1)
    if "?" not in tok:
        v = message._pack_std(tok)
        if v is None or (v & 7) != 1:
            raise ValueError(f"not a standard (i3 = 1) message: {pattern!r}")
        mask[:] = 1
        value[:] = hyp_bits(message.pack77(pattern))
        return _bits_to_bytes(mask), _bits_to_bytes(value)
    if len(tok) != 3 or tok[2] != "?" or (tok[0] == "?" and tok[1] == "?"):
        raise ValueError(f"unsupported AP pattern: {pattern!r}")
    for t, (lo, hi) in ((tok[0], _CALL_A), (tok[1], _CALL_B)):
        if t == "?":
            continue
        n28 = _call_field(t)
        mask[lo:hi] = 1
        value[lo:hi - 1] = [(n28 >> (27 - k)) & 1 for k in range(28)]  # ip = 0
    return _bits_to_bytes(mask), _bits_to_bytes(value)


def ap_magnitude(llr: np.ndarray) -> float:
    """a = 1.01 max |L| in double (NaN when any L is NaN)."""
    return AP_SCALE * float(np.max(np.abs(np.asarray(llr, dtype=np.float64))))


def ap_llr(llr, mask, value) -> np.ndarray:
    """The clamp: L_h[i] = +a / -a where mask bit i < 77 is set (by value bit i), else L[i].
    A vector whose a is NaN or 0 is returned unchanged."""
    L = np.array(llr, dtype=np.float64, copy=True)
    a = ap_magnitude(L)
    if a != a or a == 0.0:
        return L
    m, v = hyp_bits(mask).astype(bool), hyp_bits(value).astype(bool)
    L[:77][m & v] = a
    L[:77][m & ~v] = -a
    return L


def ap_accept(ok, payload, plain, llr, mask, value, max_hard_errors):
    """The acceptance test of one attempt -> (accepted, hard).  ok / payload: the reference tail on
    the attempt's hard decisions `plain`; llr: the UNCLAMPED LLRs."""
    hard = int(np.count_nonzero(np.asarray(plain, dtype=np.uint8)[:174] != (np.asarray(llr)[:174] > 0)))
    if not ok:
        return False, hard
    m = hyp_bits(mask).astype(bool)
    agree = bool(np.array_equal(hyp_bits(payload)[m], hyp_bits(value)[m]))
    return agree and hard <= int(max_hard_errors), hard


def ap_index(record) -> int:
    """Which attempt produced a record: 0 plain BP, h + 1 hypothesis h (0 as well for high nibble 15, the
    ordered-statistics pass's mark: osd.osd_index)."""
    h = int(record["pass_index"]) >> 4
    return 0 if h == 15 else h


def ap_restate(llrs, records, hyps, max_iterations, max_hard_errors, bp_decode, decode_tail):
    """The contract of ft8_ap_decode on the CPU: llrs [n, 174], records (a structured array with the
    ft8_result fields, as ft8_bp wrote them) -> (updated copy of records, hard int16 [n]).
    bp_decode(llr, iters) -> (plain, errors) and decode_tail(plain, errors) -> (ok, payload, crc_e,
    crc_c) are the reference's (tests pass the oracle's)."""
    llrs = np.asarray(llrs, dtype=np.float64).reshape(-1, 174)
    out = np.array(records, copy=True)
    hard_out = np.full(len(out), -1, dtype=np.int16)
    for i in range(len(out)):
        if out["ok"][i]:
            continue
        a = ap_magnitude(llrs[i])
        if a != a or a == 0.0:
            continue
        for h, (mask, value) in enumerate(hyps):
            plain, err = bp_decode(ap_llr(llrs[i], mask, value), max_iterations)
            ok, payload, ce, cc = decode_tail(plain, err)
            good, hard = ap_accept(ok, payload, plain, llrs[i], mask, value, max_hard_errors)
            if good:
                out["ok"][i] = 1
                out["payload"][i] = np.frombuffer(bytes(payload), dtype=np.uint8)
                out["crc_extracted"][i] = ce
                out["crc_calculated"][i] = cc
                out["ldpc_errors"][i] = err
                out["pass_index"][i] |= (h + 1) << 4
                hard_out[i] = hard
                break
    return out, hard_out
