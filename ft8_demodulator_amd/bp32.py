"""float32 belief propagation of the LDPC(174, 91) code, restated in NumPy.

The device's opt-in float32 decoder (csrc/bp32.hip: ft8_bp_f32, FT8_FLAG_BP_F32) runs the reference's
sum-product decoder (ldpc_decoder.py:54-113) in IEEE binary32 instead of float64.  This module restates
the contract of include/ft8hip.h ("float32 belief propagation") for tests and tools, vectorised over the
batch and with the dtype as a parameter: at float64 it is the reference's bp_decode, at float32 it is
what the kernel computes, bit for bit.  Nothing here runs on the decode path, and nothing here needs the
library or a GPU.

Operation order (every operation rounds to nearest in `dtype`, none is fused):

    c        = dtype(llr)                                  the 174 inputs, rounded once
    per iteration, while it < max_iterations:
      messages = c + ((t0 + t1) + t2)                      t_k = tov[n][k], k in kFTX_LDPC_Mn order
      plain    = messages > 0                              all zero -> stop
      errors   = unsatisfied checks of plain               errors < min_errors -> min_errors = errors;
                                                           0 -> stop
      Tnm      = (c + t_a) + t_b                           a < b the two positions other than the edge's own
      toc      = fast_tanh(-Tnm / 2)                       x = clip(x, -4.97, 4.97) (bounds rounded to dtype,
                                                           NaN passes); x2 = x x;
                                                           (x (945 + x2 (105 + x2))) / (945 + x2 (420 + x2 15))
      Tmn      = ((1 toc_0) toc_1) ...                     the check's other toc in row order, left to right
      tov      = -2 fast_atanh(Tmn)                        x2 = x x;
                                                           (x (945 + x2 (-735 + x2 64))) / (945 + x2 (-1050 + x2 225))

The hard decision returned is the last evaluated iteration's (all zero when none ran); the update of the
last iteration is never read, so max_iterations = 1 updates no message and 2 exactly one set.
"""
from __future__ import annotations

import numpy as np

from . import _ldpc_tables as T

N, M, E = 174, 83, 522

_CHK_START = np.array(T.CHK_START, dtype=np.int64)
_EDGE_VAR = np.array(T.EDGE_VAR, dtype=np.int64)              # edge -> variable
_VAR_EDGE = np.array(T.VAR_EDGE, dtype=np.int64).reshape(N, 3)  # variable, kFTX_LDPC_Mn position -> edge
_EDGE_CHK = np.repeat(np.arange(M), np.diff(_CHK_START))      # edge -> check
_EDGE_Q = np.arange(E) - _CHK_START[_EDGE_CHK]                # edge -> position in its check's row
# edge -> its position k among its variable's three edges, and the other two positions a < b
_EDGE_K = np.array([int(np.nonzero(_VAR_EDGE[_EDGE_VAR[e]] == e)[0][0]) for e in range(E)])
_OTHER_A = np.where(_EDGE_K == 0, 1, 0)
_OTHER_B = np.where(_EDGE_K == 2, 1, 2)
# toc padded to [M, 7]: a degree-6 row's seventh factor is a constant 1 (p * 1 == p exactly)
_ROW_EDGE = np.full((M, 7), E, dtype=np.int64)                # E: the padding column
for _m in range(M):
    _ROW_EDGE[_m, :_CHK_START[_m + 1] - _CHK_START[_m]] = np.arange(_CHK_START[_m], _CHK_START[_m + 1])
_H = np.zeros((M, N), dtype=np.int64)
_H[_EDGE_CHK, _EDGE_VAR] = 1


def fast_tanh(x, dtype=np.float32):
    """ldpc_decoder.py:11-20 in `dtype`."""
    f = np.dtype(dtype).type
    x = np.clip(x, f(-4.97), f(4.97))
    x2 = x * x
    a = x * (f(945.0) + x2 * (f(105.0) + x2))
    b = f(945.0) + x2 * (f(420.0) + x2 * f(15.0))
    return a / b


def fast_atanh(x, dtype=np.float32):
    """ldpc_decoder.py:22-30 in `dtype`."""
    f = np.dtype(dtype).type
    x2 = x * x
    a = x * (f(945.0) + x2 * (f(-735.0) + x2 * f(64.0)))
    b = f(945.0) + x2 * (f(-1050.0) + x2 * f(225.0))
    return a / b


def bp32_restate(llrs, max_iterations, dtype=np.float32):
    """LLRs [n, 174] -> (plain uint8 [n, 174], min_errors int64 [n], iterations int64 [n]): the hard
    decision of the last evaluated iteration, the smallest number of unsatisfied checks seen (83 when no
    iteration was evaluated past the all-zero stop) and the iterations entered, per vector."""
    f = np.dtype(dtype).type
    with np.errstate(all="ignore"):
        c = np.asarray(llrs, dtype=np.float64).reshape(-1, N).astype(dtype)
        n = c.shape[0]
        tov = np.zeros((n, N, 3), dtype=dtype)
        plain = np.zeros((n, N), dtype=np.uint8)
        min_errors = np.full(n, M, dtype=np.int64)
        iterations = np.zeros(n, dtype=np.int64)
        active = np.ones(n, dtype=bool)
        for _ in range(int(max_iterations)):
            idx = np.nonzero(active)[0]
            if idx.size == 0:
                break
            iterations[idx] += 1
            cv, t = c[idx], tov[idx]
            messages = cv + ((t[:, :, 0] + t[:, :, 1]) + t[:, :, 2])
            hard = (messages > 0).astype(np.uint8)
            plain[idx] = hard
            zero = hard.sum(axis=1) == 0
            errors = ((hard.astype(np.int64) @ _H.T) & 1).sum(axis=1)
            better = ~zero & (errors < min_errors[idx])
            min_errors[idx[better]] = errors[better]
            go = ~zero & ~(better & (errors == 0))
            active[idx[~go]] = False
            idx, cv, t = idx[go], cv[go], t[go]
            if idx.size == 0:
                break
            ce = cv[:, _EDGE_VAR]
            Tnm = (ce + t[:, _EDGE_VAR, _OTHER_A]) + t[:, _EDGE_VAR, _OTHER_B]
            toc = np.ones((idx.size, E + 1), dtype=dtype)
            toc[:, :E] = fast_tanh(-Tnm / f(2.0), dtype)
            rows = toc[:, _ROW_EDGE]                           # [n, M, 7]
            Tmn = np.ones((idx.size, M, 7), dtype=dtype)
            for q in range(7):
                p = np.ones((idx.size, M), dtype=dtype)
                for k in range(7):
                    if k != q:
                        p = p * rows[:, :, k]
                Tmn[:, :, q] = p
            upd = f(-2.0) * fast_atanh(Tmn[:, _EDGE_CHK, _EDGE_Q], dtype)   # per edge
            t[:, _EDGE_VAR, _EDGE_K] = upd
            tov[idx] = t
    return plain, min_errors, iterations


def bp_decode_f32(llr, max_iterations):
    """bp32_restate shaped like the reference's bp_decode: one vector -> (plain uint8 [174], errors).
    ap.ap_restate, coherent.coherent_pass_restate / coherent_ap_restate and ft4.ft4_decode_restate take it
    as their bp_decode."""
    plain, err, _ = bp32_restate(np.asarray(llr, dtype=np.float64).reshape(1, N), max_iterations, np.float32)
    return plain[0], int(err[0])


def bp_decode_f64(llr, max_iterations):
    """The same at float64: the reference's bp_decode."""
    plain, err, _ = bp32_restate(np.asarray(llr, dtype=np.float64).reshape(1, N), max_iterations, np.float64)
    return plain[0], int(err[0])
