"""Constructions the FT4 tests share (test_ft4_reference.py on the CPU, test_gpu_ft4.py on the device): the
end-to-end slots, the retry slot, the injected waterfalls of the score / selection / LLR tests and the
kernels' tile constants those shapes are chosen against."""
import numpy as np

FS = 12000
N_SAMPLES = 90000            # a 7.5-s slot: 311 frames of 576 bins at bpt = sps = 2
BPT = SPS = 2
ITERS = 20

# ---- end to end: three slots of six signals at -8 dB, a noise-only slot, an all-zero slot ---------------
E2E_SEED = 100
E2E_TOPK = dict(max_candidates=100, min_score=1.0)     # FT8_FLAG_TOPK
E2E_HEAP = dict(max_candidates=400, min_score=4.5)     # the heap rule keeps the FIRST passing grid points


def e2e_slots():
    """-> (samples float32 [5, N_SAMPLES], payload sets per slot)."""
    import torch
    from ft8_demodulator_amd import ft4
    x, truths = ft4.make_slots_ft4(3, 6, fs=FS, snr_db=-8.0, seed=E2E_SEED)
    noise, _ = ft4.make_slots_ft4(1, 0, fs=FS, seed=E2E_SEED + 3)
    x = torch.cat([x, noise, torch.zeros(1, N_SAMPLES)], 0)
    return x, [set(t.payloads) for t in truths] + [set(), set()], truths


# ---- the retry slot: 12 CQ messages on a -13 .. -17 dB ladder ----------------------------------------------
RETRY_SEED = 214
RETRY = dict(max_candidates=100, min_score=1.0)        # FT8_FLAG_TOPK | FT8_FLAG_AP | FT8_FLAG_OSD
RETRY_AP = ["CQ ? ?"]
RETRY_AP_MAX_HARD = 36
RETRY_OSD = (2, 32, 36)                                # order, candidates per slot, hard-error limit
_CALLS = ["K1ABC", "W9XYZ", "G4ABC", "JA1XYZ", "VK2DEF", "DL1ABC", "F5XYZ", "EA3GHI", "I2JKL", "OH2MNO", "SM5PQR",
          "PA3STU"]
_GRIDS = ["FN42", "EN37", "IO91", "PM95", "QF56", "JO62", "JN18", "JN11", "JN45", "KP20", "JO89", "JO22"]


def retry_slot():
    """-> (samples float32 [1, N_SAMPLES], the 12 payloads)."""
    from ft8_demodulator_amd import ft4, message
    pays = [message.pack77(f"CQ {c} {g}") for c, g in zip(_CALLS, _GRIDS)]
    x, _ = ft4.make_slots_ft4(1, 12, fs=FS, snr_db=np.linspace(-13.0, -17.0, 12), seed=RETRY_SEED, payloads=pays)
    return x, pays


def restate(wf, oracle, topk, max_candidates, min_score, slot=0, hyps=None, osd=None, sps=SPS, bpt=BPT):
    """ft4.ft4_decode_restate with the oracle's selection, BP and tail."""
    from ft8_demodulator_amd import ft4
    return ft4.ft4_decode_restate(np.asarray(wf), sps, bpt, max_candidates, min_score, ITERS,
                                  select=oracle.select_topk if topk else oracle.select, bp_decode=oracle.bp_decode,
                                  decode_tail=oracle.decode_tail, slot=slot, hyps=hyps,
                                  ap_max_hard_errors=RETRY_AP_MAX_HARD, osd=osd)


# ---- the kernels' tile constants (csrc/ft4.hip) the shapes below are chosen against ----------------------
S4_TW, S4_R = 128, 22                 # k_score4: grid columns and grid rows (of one residue class) per workgroup
G_TW = {4: 64, 8: 32}                 # k_score4g: grid columns per workgroup by element size
G_LDS_BUDGET = 64 * 1024              # k_score4g stages its rows in LDS when they fit this


def grid_shape(T, F, sps, bpt):
    from ft8_demodulator_amd import ft4
    return ft4.ft4_grid_shape(T, F, sps, bpt)


def score4g_in_lds(T, F, sps, bpt, itemsize):
    """Whether k_score4g stages this waterfall's rows in LDS (launch_score4_t's rule)."""
    t0, NT, _ = grid_shape(T, F, sps, bpt)
    rlo = max(0, t0)
    rhi = min(T - 1, t0 + NT - 1 + 102 * sps)
    return (rhi - rlo + 1) * (G_TW[itemsize] + 3 * bpt) * itemsize <= G_LDS_BUDGET


def tiled_shapes(B):
    """(T, NF, what) for k_score4<B, B>: every condition named in `what` is asserted by the test."""
    nfs = sorted({128, 129, 144, 257, 128 + (-3 * B) % 4})
    out = [(74 * B, 129, "smallest grid"), (83 * B, 144, "ten symbols"), (90 * B, 128, "T % sps == 0"),
           (90 * B + (1 if B > 1 else 0), 129, "T % sps != 0"), (103 * B, 144, "ragged row tile")]
    out += [(95 * B, nf, "columns") for nf in nfs]
    return out


def waterfall(T, F, n_slots, seed, dtype=np.float32, special=False):
    """An injected dB-like waterfall [n_slots, T, F]: continuous values, so no two scores are equal; with
    `special` a NaN patch and +-inf values."""
    rng = np.random.default_rng(seed)
    wf = (rng.normal(-20.0, 6.0, size=(n_slots, T, F))).astype(dtype)
    if special:
        wf[:, T // 2:T // 2 + 3, F // 3:F // 3 + 5] = np.nan
        wf[:, T // 3, F // 2] = np.inf
        wf[:, T // 4, F // 4] = -np.inf
        wf[:, 0, 0] = np.inf
        wf[:, T - 1, F - 1] = np.nan
    return wf


def selection_threshold(grids, n_pass=150):
    """A min_score that about n_pass scores of every grid pass: few enough that no two passing float32
    scores are equal (the selection tests assert that; thousands of passing scores would hold chance ties),
    more than the N = 37 the tests select, fewer than their N = 4096."""
    v = np.sort(np.concatenate([g[np.isfinite(g)] for g in grids]).astype(np.float64))[::-1]
    return float(np.round(v[min(n_pass * len(grids), len(v) - 1)], 3))


def untied(grids, ms):
    """Whether no two passing scores of a grid are equal, and more than 37 pass."""
    for g in grids:
        ok = g[np.isfinite(g) & (g >= ms)]
        if len(ok) <= 37 or len(np.unique(ok)) != len(ok):
            return False
    return True


def untied_waterfall(T, F, n_slots, seed, sps, bpt, dtype=np.float32, special=False):
    """waterfall() at the first of the seeds seed, seed + 1000, ... whose restated grids hold no equal passing
    scores under selection_threshold (two float32 means of 48 differences do coincide now and then, and the
    reference's order of equal scores is not what these tests are about) -> (wf, grids, min_score)."""
    from ft8_demodulator_amd import ft4
    for k in range(16):
        wf = waterfall(T, F, n_slots, seed + 1000 * k, dtype, special)
        grids = [ft4.ft4_score_grid_restate(wf[b], sps, bpt) for b in range(n_slots)]
        ms = selection_threshold(grids)
        if untied(grids, ms):
            return wf, grids, ms
    raise AssertionError("no seed without equal passing scores")
