"""Ordered-statistics decoding (OSD) of the LDPC(174, 91) code, order 0 to 2, in NumPy.

A candidate that belief propagation fails on is decoded again from the 91 most reliable independent
bit positions: the codeword those bits determine, and every codeword that differs from it in one or
two of them, are compared by an integer metric, and the best one goes through the CRC.  The device
runs the retries (csrc/osd.hip, ft8_osd_decode / FT8_FLAG_OSD); this module restates the contract of
include/ft8hip.h ("ordered-statistics decoding") for tests and tools.  Nothing here runs on the
decode path, and nothing here needs the library or a GPU.

Every quantity is an integer, the echelon form is the unique reduced one and the candidates have a
fixed order, so the device and this module agree bit for bit.
"""
from __future__ import annotations

import numpy as np

from . import _ldpc_tables as T
from .coherent import retry_list  # noqa: F401  (the pass's list is the other retries')

DEFAULT_ORDER = 2
DEFAULT_MAX_PER_SLOT = 32        # SlotDecoder(osd=True)
DEFAULT_MAX_HARD_ERRORS = 36     # the context's default, ap.DEFAULT_MAX_HARD_ERRORS
MAX_ORDER = 2
PASS_BITS = 0xF0                 # pass_index high nibble 15
Q_SCALE, Q_MAX = 256, 65535
K, N = 91, 174

ACCEPTED, REJECTED, NOT_ATTEMPTED, ALREADY_OK = 0, 1, 2, 3

# ft8_osd_rec (12 bytes), as _lib.OSD_DTYPE states it for the binding
OSD_DTYPE = np.dtype({
    "names": ["weight", "n_hard", "flip", "n_flips", "status"],
    "formats": ["<i4", "<i2", ("<i2", (2,)), "u1", "u1"],
    "offsets": [0, 4, 6, 10, 11],
    "itemsize": 12,
})


def generator() -> np.ndarray:
    """G = [I | P], uint8 [91, 174]: column 91 + m is parity row m of the code's generator table."""
    rows = np.unpackbits(np.array(T.GEN_ROWS, dtype=np.uint8).reshape(83, 12), axis=1)[:, :K]
    return np.concatenate([np.eye(K, dtype=np.uint8), rows.T], axis=1)


_G = generator()
_K1, _K2 = np.triu_indices(K, 1)   # k1 < k2 in lexicographic order


def check_order(order) -> int:
    if isinstance(order, bool) or int(order) != order or not 0 <= int(order) <= MAX_ORDER:
        raise ValueError(f"osd order must be 0, 1 or 2, got {order!r}")
    return int(order)


def n_candidates(order: int) -> int:
    return (1, 1 + K, 1 + K + K * (K - 1) // 2)[check_order(order)]


def reliabilities(llr):
    """Rule 1: (q int64 [174], hard uint8 [174]), or None where the vector is not attempted."""
    L = np.asarray(llr, dtype=np.float64).reshape(N)
    if np.isnan(L).any():
        return None
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.abs(L) * float(Q_SCALE)
        q = np.where(a >= Q_MAX, Q_MAX, np.floor(np.where(a >= Q_MAX, 0.0, a))).astype(np.int64)
    if not q.any():
        return None
    return q, (L > 0).astype(np.uint8)


def echelon(perm):
    """Rule 3 for the column order perm: (pivots int64 [91], positions in perm order of the basis columns;
    M uint8 [91, 174], the reduced row echelon form with its columns in perm order)."""
    A = _G[:, perm].copy()
    pivots = []
    for j in range(N):
        r = len(pivots)
        if r == K:
            break
        rows = np.nonzero(A[r:, j])[0]
        if rows.size == 0:
            continue
        p = r + int(rows[0])
        if p != r:
            A[[r, p]] = A[[p, r]]
        others = np.nonzero(A[:, j])[0]
        others = others[others != r]
        A[others] ^= A[r]
        pivots.append(j)
    return np.array(pivots, dtype=np.int64), A


def enumerate_candidates(d0, M, order):
    """Rule 4 as difference patterns against the hard decisions, in perm order: uint8 [n_candidates, 174],
    row e is candidate e ^ hard."""
    out = [d0[None, :]]
    if order >= 1:
        out.append(d0[None, :] ^ M)
    if order >= 2:
        out.append(d0[None, :] ^ M[_K1] ^ M[_K2])
    return np.concatenate(out, axis=0)


def flips_of(index: int):
    """Enumeration index -> (n_flips, (k1, k2)) with -1 where none."""
    if index == 0:
        return 0, (-1, -1)
    if index <= K:
        return 1, (index - 1, -1)
    return 2, (int(_K1[index - 1 - K]), int(_K2[index - 1 - K]))


def osd_restate(llr, order=DEFAULT_ORDER):
    """Rules 1 to 5 for one LLR vector -> dict, or None where rule 1 says not attempted:
    codeword uint8 [174] (natural bit order), weight, n_hard, n_flips, flip (k1, k2), index (the winner's
    enumeration index), q, hard, perm, pivots, M (columns in perm order), c0 (perm order)."""
    order = check_order(order)
    r = reliabilities(llr)
    if r is None:
        return None
    q, hard = r
    perm = np.lexsort((np.arange(N), -q))            # q descending, equal q by index ascending
    pivots, M = echelon(perm)
    qp, hp = q[perm], hard[perm]
    c0 = (hp[pivots].astype(np.int64) @ M.astype(np.int64) & 1).astype(np.uint8)
    D = enumerate_candidates(c0 ^ hp, M, order)
    w = D.astype(np.int64) @ qp
    e = int(np.argmin(w))                             # the first of the smallest weight
    cw = np.zeros(N, dtype=np.uint8)
    cw[perm] = D[e] ^ hp
    n_flips, flip = flips_of(e)
    return {"codeword": cw, "weight": int(w[e]), "n_hard": int(D[e].sum()), "n_flips": n_flips, "flip": flip,
            "index": e, "q": q, "hard": hard, "perm": perm, "pivots": pivots, "M": M, "c0": c0}


def pack_codeword(bits) -> np.ndarray:
    """174 bits -> 22 bytes, MSB first."""
    b = np.zeros(176, dtype=np.uint8)
    b[:N] = bits
    return np.packbits(b)


def osd_pass_restate(llrs, records, order, max_hard_errors, tail):
    """The contract of ft8_osd_decode on the CPU (rules 6 and 7): llrs [n, 174], records (a structured array
    with the ft8_result fields) -> (updated copy of records, info OSD_DTYPE [n], codewords uint8 [n, 22]).
    tail(plain, 0) -> (ok, payload, crc_e, crc_c) is the reference's decode tail (tests pass the oracle's)."""
    order = check_order(order)
    llrs = np.asarray(llrs, dtype=np.float64).reshape(-1, N)
    out = np.array(records, copy=True)
    info = np.zeros(len(out), dtype=OSD_DTYPE)
    info["n_hard"], info["flip"] = -1, -1
    cws = np.zeros((len(out), 22), dtype=np.uint8)
    for i in range(len(out)):
        if out["ok"][i]:
            info["status"][i] = ALREADY_OK
            continue
        r = osd_restate(llrs[i], order)
        if r is None:
            info["status"][i] = NOT_ATTEMPTED
            continue
        info["weight"][i], info["n_hard"][i] = r["weight"], r["n_hard"]
        info["flip"][i], info["n_flips"][i] = r["flip"], r["n_flips"]
        cws[i] = pack_codeword(r["codeword"])
        ok, payload, ce, cc = tail(r["codeword"], 0)
        good = bool(ok) and r["n_hard"] <= int(max_hard_errors) and r["codeword"][:77].any()
        info["status"][i] = ACCEPTED if good else REJECTED
        if good:
            out["ok"][i] = 1
            out["payload"][i] = np.frombuffer(bytes(payload), dtype=np.uint8)
            out["crc_extracted"][i], out["crc_calculated"][i], out["ldpc_errors"][i] = ce, cc, 0
            out["pass_index"][i] |= PASS_BITS
    return out, info, cws


def osd_index(record) -> bool:
    """Whether the OSD pass produced a record (pass_index high nibble 15)."""
    return (int(record["pass_index"]) >> 4) == 15


def parse_option(osd):
    """SlotDecoder's osd= / from_wave's --osd value -> (order, max_per_slot) or None: None / False: off,
    True: (2, 32), an order, or (order, max_per_slot).  ValueError for what ft8_set_osd would refuse."""
    if osd is None or osd is False:
        return None
    if osd is True:
        return DEFAULT_ORDER, DEFAULT_MAX_PER_SLOT
    if isinstance(osd, (tuple, list)):
        if len(osd) != 2:
            raise ValueError(f"osd must be (order, max_per_slot), got {osd!r}")
        order, cap = osd
    else:
        order, cap = osd, DEFAULT_MAX_PER_SLOT
    order = check_order(order)
    if isinstance(cap, bool) or int(cap) != cap or int(cap) < 0:
        raise ValueError(f"osd max_per_slot must be an integer >= 0, got {cap!r}")
    return order, int(cap)


def check_max_hard_errors(v) -> int:
    if isinstance(v, bool) or int(v) != v or not 0 <= int(v) <= N:
        raise ValueError(f"osd_max_hard_errors must be in [0, 174], got {v!r}")
    return int(v)
