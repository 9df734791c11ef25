"""Shared inputs and the CPU restatement for the a-priori decoding tests (test_ap_reference.py,
test_gpu_ap.py): everything here runs on the CPU, on the oracle's bp_decode / decode_tail."""
import functools

import numpy as np

from ft8_demodulator_amd import _lib, ap, synth
from ft8_demodulator_amd.message import pack77

ITERS = 20
STAGE_SEED = 5
STAGE_PATTERNS = ("W1AW K9AN EN50", "CQ ? ?", "K1ABC ? ?")


def oracle_lib():
    from oracle import oracle as O
    O.lib()
    return O


def plain_records(llrs, iters=ITERS):
    """The records ft8_bp writes for LLRs [n, 174] (score / slot / abs_* / cand_index 0), from the oracle."""
    O = oracle_lib()
    rec = np.zeros(len(llrs), dtype=_lib.RESULT_DTYPE)
    for i, x in enumerate(llrs):
        with np.errstate(all="ignore"):
            plain, err = O.bp_decode(x, iters)
        ok, pay, ce, cc = O.decode_tail(plain, err)
        rec["ldpc_errors"][i], rec["crc_extracted"][i], rec["crc_calculated"][i], rec["ok"][i] = err, ce, cc, ok
        rec["payload"][i] = np.frombuffer(pay, dtype=np.uint8)
    return rec


def restate(llrs, records, hyps, max_hard_errors, iters=ITERS):
    O = oracle_lib()

    def bp(x, it):
        with np.errstate(all="ignore"):
            return O.bp_decode(x, it)
    return ap.ap_restate(llrs, records, hyps, iters, max_hard_errors, bp, O.decode_tail)


def normalize_rows(llr):
    O = oracle_lib()
    return np.stack([O.normalize(x) for x in llr])


def _with_fields(payloads, value, lo, hi):
    """payloads [n, 10] with bits [lo, hi) replaced by those of `value` (10 bytes)."""
    bits = np.unpackbits(np.asarray(payloads, dtype=np.uint8), axis=1)
    bits[:, lo:hi] = ap.hyp_bits(value)[lo:hi]
    return np.packbits(bits, axis=1)


@functools.lru_cache(maxsize=None)
def stage_case(seed=STAGE_SEED, n=67, sigma=0.85):
    """The stage test's input: n normalised LLR vectors (one more than a wave) in three groups --
    A: CQ in the first call field and i3 = 1, B: K1ABC as the first call and i3 = 1, C: random -- at
    (2b - 1) + sigma N(0, 1), the three hypotheses in the test's order, the plain-BP records and the
    restatement's output without a hard-error limit.  Computed once, never modified."""
    rng = np.random.default_rng(seed)
    pay = synth.random_payloads(n, rng)
    hyps = tuple(ap.ap_hypothesis(p) for p in STAGE_PATTERNS)
    ga, gb = n // 3, 2 * (n // 3)
    for lo, hi, (_, value) in ((0, ga, hyps[1]), (ga, gb, hyps[2])):
        pay[lo:hi] = _with_fields(_with_fields(pay[lo:hi], value, 0, 29), value, 74, 77)
    pay[:, 9] &= 0xF8
    bits = synth.codeword_bits_batch(pay)
    llr = normalize_rows((2.0 * bits - 1.0) + sigma * rng.standard_normal(bits.shape))
    rec0 = plain_records(llr)
    ref, hard = restate(llr, rec0, hyps, 174)
    for a in (pay, llr, rec0, ref, hard):
        a.setflags(write=False)
    return {"payloads": pay, "llr": llr, "hyps": hyps, "plain": rec0, "ref": ref, "hard": hard}


def records_equal(got, want):
    """Field-by-field equality of two ft8_result arrays; a failure names the field and the records."""
    assert len(got) == len(want), (len(got), len(want))
    for f in _lib.RESULT_DTYPE.names if len(got) else ():
        diff = (got[f] != want[f]).reshape(len(got), -1).any(axis=1)
        assert not diff.any(), (f, np.nonzero(diff)[0].tolist())


E2E_CALLS = ("K1ABC FN42", "W9XYZ EN37", "G4ABC IO91", "JA1XYZ PM95", "VK2DEF QF56", "DL1ABC JO62", "EA3GHI JN11",
             "PY2JKL GG66")


E2E_FS, E2E_N = 12000, 180000
E2E_SEED = 6
E2E_SNR_DB = (-20.0, -21.0, -21.5, -22.0, -22.5, -23.0, -23.5, -24.0)   # full-band SNR, around the plain threshold


def e2e_payloads():
    return [pack77("CQ " + c) for c in E2E_CALLS]


@functools.lru_cache(maxsize=None)
def e2e_samples(seed=E2E_SEED, snr_db=E2E_SNR_DB):
    """Two 12 kHz slots (float32 [2, 180000], read-only): slot 0 holds the eight CQ signals of
    E2E_CALLS, 300 Hz apart, in seeded unit-variance noise; slot 1 is noise only."""
    import torch
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((2, E2E_N))
    tones = torch.as_tensor(np.stack([synth.itones(p) for p in e2e_payloads()]).astype(np.int64))
    f0 = torch.as_tensor(400.0 + 300.0 * np.arange(len(E2E_CALLS)))
    wav = synth.gfsk_waveforms(tones, E2E_FS, f0).numpy()
    start = rng.integers(int(0.2 * E2E_FS), int(1.0 * E2E_FS), size=len(E2E_CALLS))
    for w, s0, snr in zip(wav, start, snr_db):
        x[0, s0:s0 + w.shape[0]] += np.sqrt(2.0 * 10.0 ** (snr / 10.0)) * w
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x
