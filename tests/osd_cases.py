"""Shared inputs and expectations for the ordered-statistics decoding tests (test_osd_reference.py,
test_gpu_osd.py): everything here runs on the CPU, on the oracle's bp_decode / decode_tail and on
osd.osd_pass_restate.  Every array is computed once and read-only."""
import functools

import numpy as np

import ap_cases as A
from ft8_demodulator_amd import _lib, osd, synth

ITERS = A.ITERS
ORDERS = (0, 1, 2)
STAGE_SEED, STAGE_N, STAGE_SIGMA = 5, 67, 0.85
NOISE_SEED = 11


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def stage_vectors(seed=STAGE_SEED, n=STAGE_N, sigma=STAGE_SIGMA):
    """ap_cases.stage_case's recipe without its a-priori field groups: n random payloads (one more than a
    wave), (2b - 1) + sigma N(0, 1), normalised -> payloads, LLRs and the plain-BP records (20 iterations)."""
    rng = np.random.default_rng(seed)
    pay = synth.random_payloads(n, rng)
    bits = synth.codeword_bits_batch(pay)
    llr = A.normalize_rows((2.0 * bits - 1.0) + sigma * rng.standard_normal(bits.shape))
    rec0 = A.plain_records(llr)
    _freeze(pay, llr, rec0)
    return {"payloads": pay, "llr": llr, "plain": rec0}


@functools.lru_cache(maxsize=None)
def noise_vectors(seed=NOISE_SEED, n=STAGE_N):
    """The same recipe with the signal term 0 and sigma 1.0: pure noise."""
    rng = np.random.default_rng(seed)
    llr = A.normalize_rows(rng.standard_normal((n, 174)))
    rec0 = A.plain_records(llr)
    _freeze(llr, rec0)
    return {"llr": llr, "plain": rec0}


EDGE_NAMES = ("nan", "zeros", "tiny", "minus5", "codeword", "flipped", "inf", "halves", "already_ok")
EDGE_PAYLOAD = bytes([0x1C, 0x3F, 0x8A, 0x6A, 0xE2, 0x07, 0xA1, 0xE3, 0x94, 0x50])   # fixed 77 bits
FLIPPED_BASIS, FLIPPED_OTHER = (3, 40, 77), (100, 150)     # the bits inverted in `flipped`
INF_ERROR = 120                                            # the one wrong bit of `inf`
HALVES_ERRORS = (5, 17, 60, 95, 130, 171)                  # the wrong bits of `halves`


@functools.lru_cache(maxsize=None)
def edge_vectors():
    """The nine edge vectors, in EDGE_NAMES' order, each with a hand-built record (ok = 0 but the last):
    nan         one NaN among ordinary values: not attempted
    zeros       all 0.0: every q is 0, not attempted
    tiny        all |L| = 1 / 512 < 1 / 256: every q is 0, not attempted
    minus5      all -5.0: equal q, so perm is the identity and the basis the 91 message bits; c0 is the all-zero
                codeword at weight 0, which the tail passes (CRC 0 of a zero payload) and rule 6 rejects
    codeword    an exact codeword at +-8: c0 is that codeword at weight 0 at every order
    flipped     the codeword with message bits at +-8 and parity bits at +-2, so the basis is the 91 message
                bits; message bits 3, 40, 77 inverted at magnitude 3 (they stay in the basis) and parity bits
                100, 150 inverted at 0.5: the true codeword is three flips away, out of reach of order 2
    inf         the codeword at +-inf (bits 40 .. 49), +-300 (bits 0 .. 39: 76 800 clips to 65 535) and +-2, bit
                120 inverted at magnitude 1: c0 is the codeword, weight 256, one hard error
    halves      the codeword at magnitudes 0.5 and 1.0 (seeded), six bits inverted: two values of q, and at
                orders 1 and 2 three candidates share the smallest weight
    already_ok  the `codeword` vector with a record that is ok already: untouched"""
    bits = synth.codeword_bits(EDGE_PAYLOAD).astype(np.float64)
    sign = 2.0 * bits - 1.0
    v = np.zeros((len(EDGE_NAMES), 174))
    v[0] = 8.0 * sign
    v[0, 9] = np.nan
    v[2] = sign / 512.0
    v[3] = -5.0
    v[4] = 8.0 * sign
    v[5] = np.where(np.arange(174) < 91, 8.0, 2.0) * sign
    v[5, list(FLIPPED_BASIS)] = -3.0 * sign[list(FLIPPED_BASIS)]
    v[5, list(FLIPPED_OTHER)] = -0.5 * sign[list(FLIPPED_OTHER)]
    v[6] = 2.0 * sign
    v[6, :40] = 300.0 * sign[:40]
    v[6, 40:50] = np.inf * sign[40:50]
    v[6, INF_ERROR] = -1.0 * sign[INF_ERROR]
    rng = np.random.default_rng(5)
    v[7] = 0.5 * rng.integers(1, 3, size=174) * sign
    v[7, list(HALVES_ERRORS)] *= -1.0
    v[8] = v[4]
    rec = np.zeros(len(EDGE_NAMES), dtype=_lib.RESULT_DTYPE)
    for i in range(len(rec)):   # fields the pass must leave alone
        rec["score"][i], rec["slot"][i], rec["abs_time"][i], rec["abs_freq"][i] = 2.5 + i, i % 3, -4 + i, 100 + 7 * i
        rec["cand_index"][i], rec["ldpc_errors"][i], rec["pass_index"][i] = i, 5 + i, i & 1
    rec["ok"][8] = 1
    rec["payload"][8] = np.frombuffer(EDGE_PAYLOAD, dtype=np.uint8)
    rec["ldpc_errors"][8] = 0
    _freeze(v, rec)
    return {"llr": v, "records": rec, "bits": bits.astype(np.uint8)}


@functools.lru_cache(maxsize=None)
def all_vectors():
    """The 67 stage vectors followed by the 9 edge vectors, with their records."""
    s, e = stage_vectors(), edge_vectors()
    llr = np.concatenate([s["llr"], e["llr"]])
    rec = np.concatenate([s["plain"], e["records"]])
    _freeze(llr, rec)
    return llr, rec


def restate(llr, rec, order, max_hard_errors=174):
    return osd.osd_pass_restate(llr, rec, order, max_hard_errors, A.oracle_lib().decode_tail)


@functools.lru_cache(maxsize=None)
def expected(order, max_hard_errors=174):
    """osd_pass_restate over all_vectors(): (records, info, codewords)."""
    out = restate(*all_vectors(), order, max_hard_errors)
    _freeze(*out)
    return out


def rescued(out, rec0):
    """Indices of the records the pass turned ok."""
    return np.nonzero((out["ok"] == 1) & (rec0["ok"] == 0))[0]
