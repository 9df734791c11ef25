"""k_bp's shared-reciprocal division on the GPU (csrc/div_shared.h: one v_rcp_f64 per sharing group).

(a) tools/probe/div_probe.hip runs div_shared<K> with the hardware seed over arrays drawn like
    tools/div_model.cc draws them (the kernel's own polynomials over fast_tanh's and fast_atanh's
    ranges, a share of tiny arguments, a share of all-ones / 1.0...01 denominators) plus whole waves
    at the range ends; every quotient must equal NumPy's float64 division bit for bit.
(b) _device.bp against oracle.bp_decode on vectors whose variable n carries 2^-101 (below
    sweep_fast's bound: the wave must leave the shared path for that sweep), 2^-99 (just above it) or
    +-inf: hard decisions and ldpc_errors equal.  The zero and NaN cases per variable -- the check that
    a poisoned denominator stays on its own edge -- are test_gpu_bp_check_products.py's."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

LIB = os.path.join(ROOT, "tools", "probe", "libdivprobe.so")
GROUPS = 1 << 16      # per range
ITERS = (2, 3, 20)


def _scaled(rng, bound, max_down, n):
    v = bound * rng.uniform(-1.0, 1.0, n)
    down = rng.integers(0, 8, n) == 0
    return np.where(down, np.ldexp(v, -rng.integers(0, max_down + 1, n)), v)


def _hard(rng, nb):
    """one in eight denominators: significand all ones, or 1.0...01 (exponent and sign kept)"""
    c = rng.integers(0, 16, nb.size)
    b = nb.view(np.uint64).copy()
    top = b & np.uint64(0xFFF0000000000000)
    b = np.where(c == 0, top | np.uint64(0x000FFFFFFFFFFFFF), b)
    b = np.where(c == 1, top | np.uint64(1), b)
    return b.view(np.float64)


def _tanh_pairs(yv):  # bp.hip tanh_group, folded form
    z = yv * yv
    return yv * (15120.0 + z * (420.0 + z)), -30240.0 + z * (-3360.0 + z * -30.0)


def _atanh_pairs(xv):  # bp.hip atanh_group (64 x2 is exact, so the fma is the plain sum)
    x2 = xv * xv
    return xv * (945.0 + x2 * (x2 * 64.0 - 735.0)), -472.5 + x2 * (525.0 + x2 * -112.5)


@pytest.fixture(scope="module")
def division_inputs():
    """(x, y) float64 arrays, a multiple of 18 long so they split into groups of 3, 6 and 9; a group
    is all fast_tanh or all fast_atanh, as in the kernel (read-only)."""
    rng = np.random.default_rng(0xD1F)
    n = GROUPS * 18
    xa, ya = _tanh_pairs(_scaled(rng, 9.94, 100, n))
    xb, yb = _atanh_pairs(_scaled(rng, 1.0073, 600, n))
    xs, ys = [xa, xb], [_hard(rng, ya), _hard(rng, yb)]
    # whole waves (64 groups of 18) with every member at an end of its range
    sign = np.where(np.arange(64 * 18) % 2 == 0, 1.0, -1.0)
    for end in (9.94, 2.0 ** -100):
        a, b = _tanh_pairs(end * sign)
        xs.append(a), ys.append(b)
    for end in (1.0073, 1.0073 ** 6, 2.0 ** -600):
        a, b = _atanh_pairs(end * sign)
        xs.append(a), ys.append(b)
    x, y = np.ascontiguousarray(np.concatenate(xs)), np.ascontiguousarray(np.concatenate(ys))
    assert x.size % 18 == 0 and np.isfinite(x).all() and np.isfinite(y).all() and (np.abs(y) > 16.0).all()
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


@pytest.fixture(scope="module")
def probe(gpu):
    if not os.path.exists(LIB):
        pytest.skip("tools/probe/libdivprobe.so not built (make -C tools/probe)")
    lib = ctypes.CDLL(LIB)
    dp = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
    lib.ft8probe_div_shared.argtypes = [ctypes.c_int, dp, dp, dp, ctypes.c_int]
    lib.ft8probe_div_shared.restype = ctypes.c_int

    def run(k, x, y):
        assert x.size == y.size and x.size % k == 0
        q = np.empty_like(x)
        rc = lib.ft8probe_div_shared(k, x, y, q, x.size // k)
        assert rc == 0, rc
        return q
    return run


@pytest.mark.parametrize("k", [3, 6, 9])
def test_probe_quotients_are_bit_exact(probe, division_inputs, k):
    x, y = division_inputs
    got = probe(k, x, y)
    want = x / y
    bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    print(f"K={k}: {x.size} divisions, {bad.size} differ")
    assert bad.size == 0, [(float(x[i]).hex(), float(y[i]).hex(), float(got[i]).hex(), float(want[i]).hex())
                           for i in bad[:5]]


@pytest.fixture(scope="module")
def base_llr(oracle):
    """One seeded, normalised noisy codeword (read-only)."""
    from ft8_demodulator_amd import synth
    rng = np.random.default_rng(174)
    bits = synth.codeword_bits(synth.random_payload(rng)).astype(np.float64)
    x = oracle.normalize((2 * bits - 1) + 0.9 * rng.standard_normal(174))
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("value", [2.0 ** -101, 2.0 ** -99, np.inf, -np.inf],
                         ids=["below_bound", "above_bound", "plus_inf", "minus_inf"])
def test_bp_matches_oracle_with_one_special_llr(gpu, oracle, base_llr, value):
    from ft8_demodulator_amd import _device
    llrs = np.tile(base_llr, (174, 1))
    llrs[np.arange(174), np.arange(174)] = value
    for it in ITERS:
        p, rec = _device.bp(llrs, it)
        for i in range(len(llrs)):
            pr, er = oracle.bp_decode(llrs[i], it)
            assert er == int(rec[i]["ldpc_errors"]), (it, i)
            assert np.array_equal(pr, p[i]), (it, i)
