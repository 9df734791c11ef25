"""k_bp phase D: every edge's product must skip exactly its own factor, in both parts of the lane
mapping (rows 0..63 check-major with shared prefixes, rows 64..82 edge-major on two slots).

A zero (or NaN) variable->check message must vanish from its own edge's product and zero (poison)
the product of every other edge of the same check; a wrong skip flips decisions from iteration 2 on.
Every variable has three edges, so one vector per variable covers all 522 edges.  Hard decisions and
ldpc_errors are compared bit for bit with the oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ITERS = (2, 3, 6, 20)


@pytest.fixture(scope="module")
def base_llr(oracle):
    """One seeded, normalised noisy codeword (read-only)."""
    from ft8_demodulator_amd import synth
    rng = np.random.default_rng(522)
    bits = synth.codeword_bits(synth.random_payload(rng)).astype(np.float64)
    x = oracle.normalize((2 * bits - 1) + 0.9 * rng.standard_normal(174))
    x.setflags(write=False)
    return x


def _check_vars():
    from ft8_demodulator_amd._ldpc_tables import CHK_START, EDGE_VAR
    return [list(EDGE_VAR[CHK_START[m]:CHK_START[m + 1]]) for m in range(len(CHK_START) - 1)]


def _compare(oracle, llrs):
    from ft8_demodulator_amd import _device
    for it in ITERS:
        p, rec = _device.bp(llrs, it)
        for i in range(len(llrs)):
            pr, er = oracle.bp_decode(llrs[i], it)
            assert er == int(rec[i]["ldpc_errors"]), (it, i)
            assert np.array_equal(pr, p[i]), (it, i)


def test_zero_llr_per_variable(gpu, oracle, base_llr):
    llrs = np.tile(base_llr, (174, 1))
    llrs[np.arange(174), np.arange(174)] = 0.0
    _compare(oracle, llrs)


def test_nan_llr_per_variable(gpu, oracle, base_llr):
    llrs = np.tile(base_llr, (174, 1))
    llrs[np.arange(174), np.arange(174)] = np.nan
    _compare(oracle, llrs)


def test_zero_llr_per_check(gpu, oracle, base_llr):
    rows = _check_vars()
    assert len(rows) == 83 and sorted(len(r) for r in rows) == [6] * 59 + [7] * 24
    llrs = np.tile(base_llr, (83, 1))
    for m, vs in enumerate(rows):
        llrs[m, vs] = 0.0
    _compare(oracle, llrs)
