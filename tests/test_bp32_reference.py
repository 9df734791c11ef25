"""bp32.bp32_restate on the CPU: at float64 it is the reference's bp_decode (the oracle), at float32 it is the
contract of the float32 decoder (include/ft8hip.h, "float32 belief propagation"), and the two precisions
decode the same vectors.  No GPU."""
import warnings

import numpy as np
import pytest

import ap_cases as A
import bp32_cases as C
from ft8_demodulator_amd import bp32

ITERS = 20
SIGMAS = (0.6, 0.85, 1.0)


def test_restatement_is_the_oracle_at_float64():
    llr, _ = C.stress(60, 0.9, 3)
    plain, err, _ = C.restated(60, 0.9, 3, ITERS, "float64")
    O = A.oracle_lib()
    conv = 0
    for i, x in enumerate(llr):
        with np.errstate(all="ignore"):
            p, e = O.bp_decode(x, ITERS)
        assert np.array_equal(p, plain[i]), i
        assert (e == 0) == (err[i] == 0) and e == err[i], (i, e, err[i])
        conv += e == 0
    assert 0 < conv < 60, conv   # the input exercises both outcomes


def test_precisions_agree():
    """Condition (not a measurement): at most 1 vector in 100 may differ in errors == 0; every converged
    float32 codeword is the transmitted one.  (These inputs give 0 of 1200.)"""
    differ = total = 0
    for sigma in SIGMAS:
        _, bits = C.stress(400, sigma, 11)
        p32, e32, i32 = C.restated(400, sigma, 11, ITERS, "float32")
        p64, e64, i64 = C.restated(400, sigma, 11, ITERS, "float64")
        d = (e32 == 0) != (e64 == 0)
        print(f"sigma {sigma}: converged f32 {(e32 == 0).sum()} f64 {(e64 == 0).sum()} outcome differs {d.sum()} "
              f"hard decisions differ {(p32 != p64).any(axis=1).sum()} iterations differ {(i32 != i64).sum()}")
        differ += int(d.sum())
        total += len(d)
        ok = e32 == 0
        assert np.array_equal(p32[ok], bits[ok]), sigma
    assert differ * 100 <= total, (differ, total)


def test_edge_inputs_run_clean():
    names, llr, cw = C.edge_inputs()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        plain, err, it = bp32.bp32_restate(llr, ITERS)
        for k in (1, 2, 50):
            bp32.bp32_restate(llr, k)
        bp32.bp_decode_f32(llr[1], ITERS)
    got = {n: (plain[i], int(err[i]), int(it[i])) for i, n in enumerate(names)}
    zeros = np.zeros(174, np.uint8)
    # nothing is positive: the all-zero stop in the first iteration, before any parity check
    for n in ("zero", "all_nan", "1e-46"):
        assert np.array_equal(got[n][0], zeros) and got[n][1:] == (83, 1), n
    # a codeword's signs at any magnitude float32 can hold, subnormals and inf included: converged at once
    for n in ("inf_codeword", "1e300", "1e-40", "1e-30", "1e-3", "30"):
        assert np.array_equal(got[n][0], cw[names.index(n)]) and got[n][1:] == (0, 1), n
    # three wrong signs: the sweeps run (and at 1e-30 the check products are subnormal or zero)
    for n in ("1e-30_flipped", "1e-40_flipped", "1e-3_flipped", "30_flipped"):
        assert got[n][2] > 1, (n, got[n][1:])
    # the NaN stays on the messages it reaches: its own bit reads 0 in the first hard decision
    assert got["one_nan"][2] >= 1 and got["one_nan_codeword"][2] > 1


def test_iteration_edges():
    llr, _ = C.stress(60, 0.9, 3)
    x = llr[:12]
    c = x.astype(np.float32)
    p0, e0, i0 = bp32.bp32_restate(x, 0)
    assert not p0.any() and (e0 == 83).all() and (i0 == 0).all()
    # 1: the hard decision of the LLRs themselves, no message update
    p1, e1, i1 = bp32.bp32_restate(x, 1)
    assert np.array_equal(p1, (c + np.float32(0) > 0).astype(np.uint8)) and (i1 == 1).all()
    # 2: exactly one update, stated here by the scalar port of the reference's loops
    p2, e2, i2 = bp32.bp32_restate(x, 2)
    assert (i2[e1 > 0] == 2).all() and (i2[e1 == 0] == 1).all() and (e1 > 0).any()
    for i in range(4):
        sp, se, si = C.scalar_bp(x[i], 2, np.float32)
        assert np.array_equal(sp, p2[i]) and (se, si) == (e2[i], i2[i]), i


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_vectorised_equals_scalar_port(dtype):
    """The vectorised restatement against the reference's loops on scalars of the same dtype, edge inputs
    included (hard decisions, errors, iterations)."""
    names, edge, _ = C.edge_inputs()
    pick = [names.index(n) for n in ("one_nan", "plus_inf_one", "1e-30_flipped", "1e-40_flipped", "30_flipped")]
    x = np.concatenate([C.stress(60, 0.9, 3)[0][:3], edge[pick]])
    plain, err, it = bp32.bp32_restate(x, 6, np.dtype(dtype))
    for i in range(len(x)):
        sp, se, si = C.scalar_bp(x[i], 6, np.dtype(dtype))
        assert np.array_equal(sp, plain[i]) and (se, si) == (err[i], it[i]), (i, se, si, err[i], it[i])


def test_wrapper_shapes():
    llr, _ = C.stress(60, 0.9, 3)
    plain, err, _ = C.restated(60, 0.9, 3, ITERS, "float64")
    p, e = bp32.bp_decode_f64(llr[5], ITERS)
    assert p.dtype == np.uint8 and p.shape == (174,) and np.array_equal(p, plain[5]) and e == err[5]
    p, e = bp32.bp_decode_f32(llr[5], ITERS)
    assert p.shape == (174,) and isinstance(e, int)
