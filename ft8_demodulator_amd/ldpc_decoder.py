"""Mirror of the reference ldpc_decoder.py (ldpc_decoder.py:33-113), run on the GPU.

bp_decode and ldpc_check call the k_bp / k_ldpc_check HIP kernels (csrc/bp.hip): float64 sum-product
BP with the reference's rational tanh/atanh and evaluation order, bit-identical hard decisions.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

from . import _device
from .constants import FTX_LDPC_M, FTX_LDPC_N, kFTX_LDPC_Mn, kFTX_LDPC_Nm, kFTX_LDPC_Num_rows  # noqa: F401


def ldpc_check(codeword: np.ndarray) -> int:
    """ldpc_decoder.py:33-52: number of unsatisfied parity checks of a 174-bit codeword."""
    return int(_device.ldpc_check(np.asarray(codeword).reshape(1, FTX_LDPC_N))[0])


def bp_decode(codeword: np.ndarray, max_iterations: int) -> Tuple[np.ndarray, int]:
    """ldpc_decoder.py:54-113: (hard decision of the last evaluated iteration, min parity errors)."""
    plain, rec = _device.bp(np.asarray(codeword, dtype=np.float64).reshape(1, FTX_LDPC_N), max_iterations)
    return plain[0].astype(np.uint8), int(rec[0]["ldpc_errors"])


def bp_decode_batch(codewords: np.ndarray, max_iterations: int, f32: bool = False):
    """Batched bp_decode: LLRs [n, 174] -> (plain [n, 174] uint8, min_errors [n]).  f32: the opt-in float32
    decoder (k_bp32, csrc/bp32.hip), bit-identical to bp32.bp32_restate instead of the reference."""
    plain, rec = _device.bp(np.asarray(codewords, dtype=np.float64).reshape(-1, FTX_LDPC_N), max_iterations, f32)
    return plain, rec["ldpc_errors"].astype(np.int64)


def ap_decode_batch(llrs: np.ndarray, records: np.ndarray, max_iterations: int):
    """A-priori retry (ft8_ap_decode) of the failed records ft8_bp wrote from llrs [n, 174], with the
    hypotheses of the thread's context (_lib.context().set_ap): -> (updated records, hard int16 [n]:
    the hard errors of an accepted AP decode, -1 otherwise).  The contract is in include/ft8hip.h;
    ap.ap_restate is its NumPy restatement."""
    return _device.ap_decode(llrs, records, max_iterations)


def osd_decode_batch(llrs: np.ndarray, records: np.ndarray):
    """Ordered-statistics retry (ft8_osd_decode) of the failed records ft8_bp wrote from llrs [n, 174], with
    the order and hard-error limit of the thread's context (_lib.context().set_osd): -> (updated records,
    info _lib.OSD_DTYPE [n]: weight, hard errors, flips and status of every attempt, codewords uint8 [n, 22]:
    the winning codewords, MSB first).  The contract is in include/ft8hip.h; osd.osd_pass_restate is its NumPy
    restatement."""
    return _device.osd_decode(llrs, records)


def coherent_ap_decode_batch(llrs: np.ndarray, records: np.ndarray, max_iterations: int, valid=None):
    """A-priori retry on coherent LLRs (ft8_coherent_ap_decode) of the failed records among `records`, with
    the hypotheses of the thread's context (_lib.context().set_ap): llrs [n, 174] or [n, S, 174] as
    coherent_llr_batch gives them, valid its validity bytes (None: every set usable) -> (updated records,
    hard int16 [n]: the hard errors of an accepted attempt, -1 otherwise).  The contract is in
    include/ft8hip.h; coherent.coherent_ap_restate is its NumPy restatement."""
    return _device.coherent_ap_decode(llrs, records, max_iterations, valid)


def coherent_llr_batch(samples, cand, slot_of, sample_rate=12000, bins_per_tone=2, steps_per_symbol=2, t_lo=0,
                       f_lo=0, code=None, drift=None, nsym=1):
    """Coherent re-demodulation (ft8_coherent_llr) of the candidates cand [n, 2] = (abs_time, abs_freq) of
    the slots slot_of [n] from samples [n_slots, n_samples] (float32 or int16 PCM): -> (LLRs float64
    [n, 174], fits coherent.FIT_DTYPE [n]).  drift = (max_rate Hz/s, n_rates): with the search over
    linear frequency drift (ft8_coherent_drift_llr) -> (LLRs, fits, drifts coherent.DRIFT_DTYPE [n]).
    nsym = S in {2, 3}: with the joint LLRs over 2 .. S symbols (ft8_coherent_nsym_llr): LLRs [n, S, 174],
    and the validity bytes uint8 [n] come last.
    The contract is in include/ft8hip.h; coherent.coherent_restate is its NumPy restatement."""
    return _device.coherent_llr(samples, cand, slot_of, sample_rate, bins_per_tone, steps_per_symbol, t_lo, f_lo, code,
                                drift, nsym)
