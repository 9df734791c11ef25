"""Shared by tests/test_geometry_golden.py (CPU) and tests/test_gpu_stage_geometry.py: the reference's
vectors at unequal oversampling factors (tests/golden/geometry.*, tools/make_golden_geometry.py), seeded
waterfalls, the oracle's expectations per waterfall, and direct multi-slot calls of ft8_sync_select / ft8_llr."""
import ctypes
import functools
import json
import os

import numpy as np

from conftest import GOLD


@functools.lru_cache(maxsize=None)
def fixtures():
    """-> (cases of geometry.json, arrays of geometry.npz)."""
    with open(os.path.join(GOLD, "geometry.json")) as f:
        meta = json.load(f)
    return meta["cases"], np.load(os.path.join(GOLD, "geometry.npz"), allow_pickle=False)


def fixture_llrs(c, arr):
    """The candidates whose LLRs case c records and those LLRs: the first six of selection llr_sel, then the four
    grid corners -> ([(abs_time, abs_freq)], raw [n, 174], normalised [n, 174])."""
    n = c["name"]
    cands = [tuple(x) for x in c["corners"]]
    raw, nl = arr[f"geo_{n}_corner_llr_raw"], arr[f"geo_{n}_corner_llr"]
    if c["llr_sel"] is not None:
        top = arr[f"geo_{n}_sel_llr_raw"]
        cands = [tuple(x) for x in c["sel"][c["llr_sel"]]["cands"][: len(top)]] + cands
        raw, nl = np.concatenate([top, raw]), np.concatenate([arr[f"geo_{n}_sel_llr"], nl])
    return cands, raw, nl


def grid_bounds(F, T, bpt, sps):
    """ft8_find_candidates' ranges (ft8_decode.py:108-109) -> (t0, NT, NF)."""
    nb = T // sps
    return -10 * sps, (nb - 59) * sps + 10 * sps, F - 7 * bpt


def waterfall(seed, F, T, dtype=np.float32, quantised=False, tones=True):
    """-50 + 6 N(0,1) [F, T]; `tones`: a few stronger stripes, so that a min_score passes about a tenth of the
    grid and late maxima (records) exist; `quantised`: np.round, exact score ties."""
    rng = np.random.default_rng(seed)
    mag = -50 + 6 * rng.standard_normal((F, T))
    if tones:
        for _ in range(3):
            f, t = int(rng.integers(0, F - 1)), int(rng.integers(0, T // 2))
            mag[f:f + 2, t:] += 9.0
    if quantised:
        mag = np.round(mag)
    return mag.astype(dtype)


def tenth_score(grid):
    """A min_score that roughly a tenth of the grid passes: its 0.9 quantile, rounded to 1/8 so that it is exact
    in float32 and the comparison dtype cannot matter."""
    g = grid[np.isfinite(grid)]
    return float(np.round(np.quantile(g.astype(np.float64), 0.9) * 8) / 8)


def expected(oracle, grid, t0, N, min_score, topk):
    """The oracle's selection on its own grid -> ([(abs_time, abs_freq)], scores float64, tie flag or None)."""
    NF = grid.shape[1]
    if topk:
        idx, sc = oracle.select_topk(grid, N, min_score)
        tie = None
    else:
        idx, sc, tie = oracle.select(grid, N, min_score)
    return [(int(i // NF) + t0, int(i % NF)) for i in idx], sc, tie


def check_selection(oracle, wf, mag, grid, N, min_score, topk, tag):
    """Compact selection == full-grid selection == the oracle's (candidates, scores in the waterfall dtype, tie
    flag for the reference heap); the full-grid call's grid equals the oracle's byte for byte.  -> warning word."""
    from ft8_demodulator_amd import _device
    t0 = -10 * int(wf.time_osr)
    flags = 1 if topk else 0
    compact, _, w1 = _device.sync_select(wf, N, min_score, flags=flags)
    full, g, w2 = _device.sync_select(wf, N, min_score, want_grid=True, flags=flags)
    assert g.dtype == grid.dtype and g.shape == grid.shape, tag
    assert np.array_equal(g.view(np.uint8), grid.view(np.uint8)), tag
    assert compact == full and w1 == w2, tag
    exp, sc, tie = expected(oracle, grid, t0, N, min_score, topk)
    assert [(a, b) for a, b, _ in compact] == exp, tag
    got = np.array([s for _, _, s in compact], dtype=mag.dtype)
    assert np.array_equal(got, sc.astype(mag.dtype)), tag
    if tie is not None:
        assert bool(w1 & 1) == tie, tag
    return w1


def sync_select_slots(mags, bpt, sps, N, min_score, flags=0):
    """One ft8_sync_select call over the waterfalls mags [n_slots][F, T] (one dtype, one shape) on a context of
    its own -> (candidates [n_slots, N, 2], scores [n_slots, N] float64, counts [n_slots], warnings [n_slots])."""
    from ft8_demodulator_amd import _lib
    torch = _lib.require_gpu()
    n_slots = len(mags)
    F, T = mags[0].shape
    f64 = mags[0].dtype == np.float64
    ctx = _lib.Context(0)
    L, st = _lib.lib(), _lib.stream_handle(0)
    d_wf = torch.from_numpy(np.ascontiguousarray(np.stack([m.T for m in mags]))).cuda()   # [n_slots, T, F]
    p = _lib.Ft8Params()
    p.sample_rate, p.bins_per_tone, p.steps_per_symbol = 1, int(bpt), int(sps)
    p.max_candidates, p.min_score, p.flags = int(N), float(min_score), int(flags)
    d_cand = torch.zeros(n_slots, N, 2, dtype=torch.int32, device="cuda")
    d_score = torch.zeros(n_slots, N, dtype=torch.float64, device="cuda")
    d_cnt = torch.full((n_slots,), -1, dtype=torch.int32, device="cuda")
    d_warn = torch.zeros(n_slots, dtype=torch.int32, device="cuda")
    ctx.check(L.ft8_sync_select(ctx.handle, _lib.ptr(d_wf), int(f64), n_slots, T, F, ctypes.byref(p), _lib.ptr(d_cand),
                                _lib.ptr(d_score), _lib.ptr(d_cnt), None, st), "ft8_sync_select")
    ctx.check(L.ft8_select_warnings(ctx.handle, _lib.ptr(d_warn), n_slots, st), "ft8_select_warnings")
    return d_cand.cpu().numpy(), d_score.cpu().numpy(), d_cnt.cpu().numpy(), d_warn.cpu().numpy()


def llr_slots(mags, bpt, sps, rows, normalize):
    """One ft8_llr call over the waterfalls mags [n_slots][F, T] with the explicit list rows
    [(slot, abs_time, abs_freq)] -> LLRs [len(rows), 174]."""
    from ft8_demodulator_amd import _lib
    torch = _lib.require_gpu()
    F, T = mags[0].shape
    f64 = mags[0].dtype == np.float64
    ctx = _lib.Context(0)
    d_wf = torch.from_numpy(np.ascontiguousarray(np.stack([m.T for m in mags]))).cuda()
    d_c3 = torch.tensor(rows, dtype=torch.int32, device="cuda")
    d_llr = torch.empty(len(rows), 174, dtype=torch.float64, device="cuda")
    ctx.check(_lib.lib().ft8_llr(ctx.handle, _lib.ptr(d_wf), int(f64), T, F, int(sps), int(bpt), _lib.ptr(d_c3),
                                 len(rows), int(bool(normalize)), _lib.ptr(d_llr), _lib.stream_handle(0)), "ft8_llr")
    return d_llr.cpu().numpy()


def llr_points(F, T, bpt, sps, n, seed):
    """n on-grid candidates: the four grid corners, the four edge midpoints, then seeded interior points."""
    t0, NT, NF = grid_bounds(F, T, bpt, sps)
    t1, f1, tm, fm = t0 + NT - 1, NF - 1, t0 + NT // 2, NF // 2
    pts = [(t0, 0), (t0, f1), (t1, 0), (t1, f1), (t0, fm), (t1, fm), (tm, 0), (tm, f1)]
    rng = np.random.default_rng(seed)
    while len(pts) < n:
        pts.append((int(rng.integers(t0 + 1, t1)), int(rng.integers(1, f1))))
    assert all(t0 <= a < t0 + NT and 0 <= b < NF for a, b in pts)
    return pts[:n]
