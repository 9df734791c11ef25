"""Shared inputs of the float32 belief-propagation tests (test_bp32_reference.py, test_gpu_bp32.py):
computed once on the CPU, cached, read-only."""
import functools

import numpy as np

import ap_cases as A
from ft8_demodulator_amd import bp32, synth
from ft8_demodulator_amd.constants import kFTX_LDPC_Mn, kFTX_LDPC_Nm, kFTX_LDPC_Num_rows

KINDS = ("stress", "edge", "instant")


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def stress(n, sigma, seed):
    """synth.bp_stress_llrs normalised to variance 24 (ftx_normalize_logl, the oracle's) -> (LLRs, bits)."""
    llr, bits = synth.bp_stress_llrs(n, sigma=sigma, seed=seed)
    return _ro(A.normalize_rows(llr), np.asarray(bits, dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def restated(n, sigma, seed, iters, dtype):
    """bp32_restate of stress(n, sigma, seed) in np.dtype(dtype)."""
    return _ro(*bp32.bp32_restate(stress(n, sigma, seed)[0], iters, np.dtype(dtype)))


@functools.lru_cache(maxsize=None)
def edge_inputs():
    """(names, LLRs [k, 174], bits [k, 174]): the inputs the contract defines through the restatement alone.
    `bits` is the codeword behind a vector (all zero where there is none)."""
    rng = np.random.default_rng(21)
    bits = np.asarray(synth.codeword_bits_batch(synth.random_payloads(16, rng)), dtype=np.float64)
    sign = 2.0 * bits - 1.0
    noisy = stress(4, 0.85, 23)[0]
    flipped = np.array(sign[7])
    flipped[[3, 77, 140]] *= -1.0          # three wrong signs: not a codeword, so the sweeps run
    rows = [
        ("zero", np.zeros(174), None),
        ("one_nan", np.where(np.arange(174) == 50, np.nan, noisy[0]), None),
        ("one_nan_codeword", np.where(np.arange(174) == 9, np.nan, 4.0 * sign[0]), None),
        ("all_nan", np.full(174, np.nan), None),
        ("plus_inf_one", np.where(np.arange(174) == 17, np.inf, noisy[1]), None),
        ("minus_inf_one", np.where(np.arange(174) == 99, -np.inf, noisy[2]), None),
        ("inf_codeword", np.inf * sign[1], 1),
        ("1e300", 1e300 * sign[2], 2),
        ("1e-46", 1e-46 * sign[3], None),          # 0 after rounding
        ("1e-40", 1e-40 * sign[4], 4),             # a float32 subnormal after rounding
        ("1e-30", 1e-30 * sign[5], 5),
        ("1e-30_flipped", 1e-30 * flipped, None),  # products reach float32 subnormals within a sweep
        ("1e-40_flipped", 1e-40 * flipped, None),
        ("1e-3", 1e-3 * sign[8], 8),
        ("1e-3_flipped", 1e-3 * flipped, None),
        ("30", 30.0 * sign[9], 9),
        ("30_flipped", 30.0 * flipped, None),
    ]
    names = tuple(r[0] for r in rows)
    llr = np.stack([np.asarray(r[1], dtype=np.float64) for r in rows])
    cw = np.stack([bits[r[2]].astype(np.uint8) if r[2] is not None else np.zeros(174, np.uint8) for r in rows])
    return (names,) + _ro(llr, cw)


@functools.lru_cache(maxsize=None)
def stage_pool(n=129, seed=31):
    """The stage test's input: n vectors of three kinds -- sigma-0.85 stress vectors (about half converge), the
    edge inputs, vectors that converge at iteration 0 (noiseless codewords at +-4.9) -- shuffled so that every
    kind sits beside every other kind in some pair (2 k, 2 k + 1), the unit a two-per-wave kernel decodes
    together, and so that the first three hold one of each.  -> (LLRs [n, 174], kind index [n])."""
    _, edge, _ = edge_inputs()
    rng = np.random.default_rng(seed)
    n_inst = 30
    inst = 4.9 * (2.0 * np.asarray(synth.codeword_bits_batch(synth.random_payloads(n_inst, rng)), dtype=np.float64) - 1.0)
    st = stress(n - len(edge) - n_inst, 0.85, 29)[0]
    llr = np.concatenate([st, edge, inst])
    kind = np.concatenate([np.zeros(len(st), int), np.ones(len(edge), int), np.full(n_inst, 2)])
    perm = rng.permutation(n)
    # the first three: one of each kind (stress, edge, instant)
    head = [int(np.nonzero(kind[perm] == k)[0][0]) for k in range(3)]
    rest = [i for i in range(n) if i not in head]
    perm = perm[head + rest]
    llr, kind = llr[perm], kind[perm]
    pairs = {(int(kind[i]), int(kind[i + 1])) for i in range(0, n - 1, 2)}
    pairs |= {(b, a) for a, b in pairs}
    assert all((a, b) in pairs for a in range(3) for b in range(3)), sorted(pairs)
    return _ro(llr, kind)


@functools.lru_cache(maxsize=None)
def stage_expect(n, iters):
    """bp32_restate (float32) of the first n vectors of stage_pool."""
    return _ro(*bp32.bp32_restate(stage_pool()[0][:n], iters, np.float32))


def scalar_bp(llr, max_iterations, dtype):
    """The reference's bp_decode (ldpc_decoder.py:54-113), line by line, on NumPy scalars of `dtype`: an
    independent, slow statement of what bp32_restate vectorises.  -> (plain, min_errors, iterations)."""
    f = np.dtype(dtype).type
    M, N = 83, 174
    with np.errstate(all="ignore"):
        c = np.asarray(llr, dtype=np.float64).astype(dtype)
        tov = np.zeros((N, 3), dtype=dtype)
        toc = np.zeros((M, 7), dtype=dtype)
        plain = np.zeros(N, dtype=np.uint8)
        min_errors, entered = M, 0
        for _ in range(max_iterations):
            entered += 1
            messages = np.array([c[n] + ((tov[n][0] + tov[n][1]) + tov[n][2]) for n in range(N)], dtype=dtype)
            plain = (messages > 0).astype(np.uint8)
            if plain.sum() == 0:
                break
            errors = 0
            for m in range(M):
                x = 0
                for i in range(kFTX_LDPC_Num_rows[m]):
                    x ^= int(plain[kFTX_LDPC_Nm[m][i] - 1])
                errors += x != 0
            if errors < min_errors:
                min_errors = errors
                if errors == 0:
                    break
            for m in range(M):
                for n_idx in range(kFTX_LDPC_Num_rows[m]):
                    n = kFTX_LDPC_Nm[m][n_idx] - 1
                    Tnm = c[n]
                    for m_idx in range(3):
                        if (kFTX_LDPC_Mn[n][m_idx] - 1) != m:
                            Tnm = Tnm + tov[n][m_idx]
                    toc[m][n_idx] = bp32.fast_tanh(-Tnm / f(2.0), dtype)
            for n in range(N):
                for m_idx in range(3):
                    m = kFTX_LDPC_Mn[n][m_idx] - 1
                    Tmn = f(1.0)
                    for n_idx in range(kFTX_LDPC_Num_rows[m]):
                        if (kFTX_LDPC_Nm[m][n_idx] - 1) != n:
                            Tmn = Tmn * toc[m][n_idx]
                    tov[n][m_idx] = f(-2.0) * bp32.fast_atanh(Tmn, dtype)
    return plain, min_errors, entered
