"""The front end (k_score2 / k_score, k_select / k_topk / k_topkc, k_llr) where bins_per_tone and
steps_per_symbol differ, and every k_score2 / k_score instantiation on each of its staging paths.

tests/test_gpu_stages.py feeds the kernels only waterfalls with bpt == sps; here the reference's own vectors
at unequal factors (tests/golden/geometry.*) and the oracle (pinned to them by tests/test_geometry_golden.py)
are the expectation.  Every comparison is bit-exact: grids by bytes, candidates by (time, freq), scores equal in
the waterfall dtype, LLRs raw by value and normalised as uint64 -- except the end-to-end scores, which carry the
float32 STFT's rounding."""
import functools

import numpy as np
import pytest

import geometry_cases as G

pytestmark = pytest.mark.gpu


def _wf(mag, sps, bpt):
    from ft8_demodulator_amd import FT8Waterfall
    return FT8Waterfall(mag=mag, time_osr=sps, freq_osr=bpt)


# ---- a. the reference's fixtures ---------------------------------------------------------------------
_FIX = [c["name"] for c in G.fixtures()[0]]


@pytest.mark.parametrize("name", _FIX)
def test_fixture_grid_selection_llr(gpu, name):
    from ft8_demodulator_amd import _device, ft8_find_candidates, ft8_score_grid
    cases, arr = G.fixtures()
    c = next(x for x in cases if x["name"] == name)
    mag = arr[f"geo_{name}_mag"]
    wf = _wf(mag, c["sps"], c["bpt"])
    ref = arr[f"geo_{name}_grid"]
    g = ft8_score_grid(wf)
    assert g.dtype == ref.dtype and g.shape == ref.shape
    assert np.array_equal(g.view(np.uint8), ref.view(np.uint8))
    NF = ref.shape[1]
    for s in c["sel"]:
        tag = (name, s["N"], s["min_score"])
        compact, _, w1 = _device.sync_select(wf, s["N"], s["min_score"])
        full, g2, w2 = _device.sync_select(wf, s["N"], s["min_score"], want_grid=True)
        assert np.array_equal(g2.view(np.uint8), ref.view(np.uint8)), tag
        assert compact == full and w1 == w2, tag
        # bit 0 <=> the reference raised TypeError (an exact tie reached a heap comparison)
        assert bool(w1 & 1) == (s["error"] is not None), tag
        # top-k is build-defined: the N highest passing scores of the reference's grid, ties in scan order
        tk, _, _ = _device.sync_select(wf, s["N"], s["min_score"], flags=1)
        tkf, _, _ = _device.sync_select(wf, s["N"], s["min_score"], want_grid=True, flags=1)
        ok = np.isfinite(ref) & (ref >= ref.dtype.type(s["min_score"]))
        idx = np.nonzero(ok.reshape(-1))[0]
        idx = idx[np.lexsort((idx, -ref.reshape(-1)[idx].astype(np.float64)))][: s["N"]]
        assert tk == tkf, tag
        assert [(a, b) for a, b, _ in tk] == [(int(i // NF) - 10 * c["sps"], int(i % NF)) for i in idx], tag
        assert np.array_equal(np.array([x for _, _, x in tk], dtype=ref.dtype), ref.reshape(-1)[idx]), tag
        if s["error"] is not None:
            continue
        assert [[a, b] for a, b, _ in compact] == s["cands"], tag
        got = ft8_find_candidates(wf, s["N"], s["min_score"])
        assert [[x.abs_time, x.abs_freq] for x in got] == s["cands"], tag
        sc = arr[f"geo_{name}_N{s['N']}_ms{s['min_score']}_scores"]
        assert np.array_equal(np.array([x.score for x in got], dtype=sc.dtype), sc), tag
        assert np.array_equal(np.array([x for _, _, x in compact], dtype=sc.dtype), sc), tag
        if got:
            assert type(got[0].score) is type(sc[0]), tag
    cands, raw, nl = G.fixture_llrs(c, arr)
    assert np.array_equal(_device.llr(wf, cands, normalize=False), raw)
    with np.errstate(all="ignore"):
        x = _device.llr(wf, cands, normalize=True)
    assert np.array_equal(x.view(np.uint64), nl.view(np.uint64))


# ---- b. k_score2, every instantiation --------------------------------------------------------------
# (B, F, T): bins_per_tone = steps_per_symbol = B, float32
SCORE2 = (
    (1, 263, 93), (1, 136, 95), (1, 208, 75),
    (2, 270, 125), (2, 143, 150), (2, 144, 160),
    (3, 277, 281), (3, 150, 280), (3, 152, 300),
    (4, 284, 372), (4, 157, 372), (4, 158, 290),
    (10, 326, 700), (10, 199, 650), (10, 200, 720),
)
S2_TW, S2_R = 128, 22   # kS2TW, kS2R (csrc/sync.hip): grid columns and rows of one k_score2 workgroup
SELECTIONS = tuple((N, which, topk) for topk in (False, True) for N in (1, 37, 4096) for which in ("tenth", "all"))


def test_score2_table_meets_its_conditions():
    """Pure arithmetic on SCORE2: what its rows must reach between them (no GPU work; marked with the file)."""
    for B in (1, 2, 3, 4, 10):
        rows = [(F, T) for b, F, T in SCORE2 if b == B]
        assert any(F % 4 == 0 for F, _ in rows), B                 # float4 staging
        assert any(F % 4 != 0 for F, _ in rows), B                 # scalar staging
        nf = [F - 7 * B for F, _ in rows]
        assert any(n % S2_TW == 0 for n in nf) and any(n % S2_TW == 1 for n in nf), B
        assert any(n % S2_TW > 1 for n in nf), B
        assert all(n > S2_TW for n in nf), B                       # at least two column tiles in every row
        assert all(T // B >= 60 for _, T in rows), B               # a non-empty grid
    # a residue class with more than 22 rows whose second row tile is ragged (rows per class: NT / B = nb - 49)
    assert any(S2_R < T // B - 49 < 2 * S2_R for _, _, T in SCORE2)
    assert any(T % B != 0 for B, _, T in SCORE2)
    # nb < 79; below 69 the third Costas band of EVERY grid row (blocks base + 72 .. base + 78, base >= -10)
    # crosses the last block
    assert any(T // B < 69 for B, _, T in SCORE2)


@functools.lru_cache(maxsize=None)
def _case(oracle_mod, seed, bpt, sps, F, T, dtype, quantised=False):
    """(waterfall, the oracle's grid, a min_score about a tenth of it passes), computed once, read-only."""
    mag = G.waterfall(seed, F, T, np.dtype(dtype), quantised)
    grid = oracle_mod.score_grid(mag, sps, bpt)
    mag.setflags(write=False)
    grid.setflags(write=False)
    return mag, grid, G.tenth_score(grid)


def _check_all(oracle, mag, grid, tenth, bpt, sps, tag):
    from ft8_demodulator_amd import ft8_score_grid
    wf = _wf(mag, sps, bpt)
    g = ft8_score_grid(wf)
    assert g.dtype == grid.dtype and g.shape == grid.shape, tag
    assert np.array_equal(g.view(np.uint8), grid.view(np.uint8)), tag
    frac = np.mean(grid >= tenth)
    assert 0.05 < frac < 0.2, (tag, frac)
    for N, which, topk in SELECTIONS:
        ms = tenth if which == "tenth" else -100
        G.check_selection(oracle, wf, mag, grid, N, ms, topk, tag + (N, ms, topk))


@pytest.mark.parametrize("B,F,T", SCORE2)
def test_score2_grid_and_selection_vs_oracle(gpu, oracle, B, F, T):
    mag, grid, tenth = _case(oracle, 7000 + 13 * B + F, B, B, F, T, "float32")
    _check_all(oracle, mag, grid, tenth, B, B, (B, F, T))


# ---- c. the generic k_score ---------------------------------------------------------------------------
# (bpt, sps, F, T, dtype)
GENERIC = (
    (3, 2, 121, 186, "float32"), (3, 2, 121, 200, "float32"), (1, 2, 77, 150, "float32"),
    (2, 1, 79, 80, "float32"), (2, 4, 104, 259, "float32"), (2, 8, 84, 501, "float32"),
    (5, 5, 107, 317, "float32"), (7, 7, 119, 437, "float32"),
    (3, 2, 66, 125, "float64"), (3, 2, 66, 170, "float64"), (1, 3, 77, 187, "float64"),
    (2, 8, 54, 501, "float64"), (2, 2, 64, 130, "float64"),
)


def _staged(bpt, sps, F, T, dtype):
    """launch_score_t's staging rule (csrc/sync.hip, `if (lds <= kScoreLdsBudget)`): the tile holds the rows
    [max(0, t0 - sps), min(T - 1, t0 + NT - 1 + 79 sps)] of TW + 7 bpt columns (TW = 64 float32, 32 float64,
    launch_score) and is staged in LDS while it fits 64 KiB."""
    item = np.dtype(dtype).itemsize
    TW = 64 if item == 4 else 32
    t0, NT, _ = G.grid_bounds(F, T, bpt, sps)
    rlo, rhi = max(0, t0 - sps), min(T - 1, t0 + NT - 1 + 79 * sps)
    return (rhi - rlo + 1) * (TW + 7 * bpt) * item <= 64 * 1024


def test_generic_table_meets_its_conditions():
    """Pure arithmetic on GENERIC (no GPU work; marked with the file)."""
    f32 = {(b, s) for b, s, _, _, d in GENERIC if d == "float32"}
    f64 = {(b, s) for b, s, _, _, d in GENERIC if d == "float64"}
    assert f32 == {(3, 2), (1, 2), (2, 1), (2, 4), (2, 8), (5, 5), (7, 7)}
    assert f64 == {(3, 2), (1, 3), (2, 8), (2, 2)}
    for b, s, F, T, d in GENERIC:
        TW = 64 if d == "float32" else 32
        NF = F - 7 * b
        assert NF > TW and NF % TW != 0, (b, s, F, T, d)        # two column tiles or more, a ragged tail
        # none of these float32 rows is a k_score2 geometry (score2_path: bpt == sps in 1..4 or 10)
        assert d == "float64" or b != s or b not in (1, 2, 3, 4, 10)
    for d in ("float32", "float64"):
        assert {_staged(*r) for r in GENERIC if r[4] == d} == {True, False}, d
    assert _staged(3, 2, 121, 186, "float32") and not _staged(3, 2, 121, 200, "float32")   # 63 240 B / 68 000 B


@pytest.mark.parametrize("bpt,sps,F,T,dtype", GENERIC)
def test_generic_score_grid_and_selection_vs_oracle(gpu, oracle, bpt, sps, F, T, dtype):
    mag, grid, tenth = _case(oracle, 8000 + 100 * bpt + sps + T, bpt, sps, F, T, dtype)
    _check_all(oracle, mag, grid, tenth, bpt, sps, (bpt, sps, F, T, dtype, "staged" if _staged(bpt, sps, F, T, dtype)
                                                    else "unstaged"))


def test_generic_score_quantised_ties_vs_oracle(gpu, oracle):
    """Exactly equal scores at (3, 2): the selected set, its heap-array order and the TypeError flag follow the
    oracle's heapq simulation, and the replay path ran (bit 2 of the warning word)."""
    rng = np.random.default_rng(3232)
    seen4 = n_tie = 0
    for F, T in ((121, 186), (90, 200)):
        mag = (np.round((-50 + 6 * rng.standard_normal((F, T))) / 3) * 3).astype(np.float32)
        grid = oracle.score_grid(mag, 2, 3)
        wf = _wf(mag, 2, 3)
        for N, ms in ((5, 0), (50, 1), (300, 0), (1000, -100)):
            exp, sc, tie = G.expected(oracle, grid, -20, N, ms, False)
            w = G.check_selection(oracle, wf, mag, grid, N, ms, False, (F, T, N, ms))
            if len(set(sc.tolist())) < len(sc):      # equal scores inside the selected set
                assert w & 4, (F, T, N, ms)
                seen4 += 1
            n_tie += tie
    assert seen4 >= 4 and n_tie >= 1


# ---- d. several slots in one call ---------------------------------------------------------------------
@pytest.mark.parametrize("bpt,sps,F,T,dtype,n_slots", (
    (3, 3, 161, 187, "float32", 9),      # k_score2<3, 3>: slots 0 and 8 on one XCD residue
    (3, 2, 121, 186, "float32", 9),      # k_score<float, LDS, 64>: blockIdx.y = slot
    (3, 2, 66, 125, "float64", 9),       # k_score<double, LDS, 32>
    (3, 2, 121, 200, "float32", 3),      # k_score<float, no LDS, 64>
))
def test_several_slots_in_one_call(gpu, oracle, bpt, sps, F, T, dtype, n_slots):
    mags = [G.waterfall(9100 + 10 * s + bpt + sps, F, T, np.dtype(dtype)) for s in range(n_slots)]
    assert len({m.tobytes() for m in mags}) == n_slots
    grids = [oracle.score_grid(m, sps, bpt) for m in mags]
    for N, ms, flags in ((37, 1.0, 0), (37, 1.0, 1), (200, 3.0, 0)):
        cand, score, cnt, warn = G.sync_select_slots(mags, bpt, sps, N, ms, flags)
        for s in range(n_slots):
            exp, sc, tie = G.expected(oracle, grids[s], -10 * sps, N, ms, bool(flags))
            tag = (s, N, ms, flags)
            assert int(cnt[s]) == len(exp), tag
            assert [tuple(x) for x in cand[s, : cnt[s]].tolist()] == exp, tag
            assert np.array_equal(score[s, : cnt[s]].astype(mags[s].dtype), sc.astype(mags[s].dtype)), tag
            if not flags:
                assert bool(warn[s] & 1) == tie, tag


# ---- e. k_llr at unequal factors -------------------------------------------------------------------------
LLR_GEO = ((3, 2, 51, 125, "float32"), (1, 2, 37, 124, "float32"), (2, 4, 44, 251, "float32"),
           (2, 8, 44, 501, "float32"), (3, 2, 51, 125, "float64"))


def _oracle_llrs(oracle, mag, sps, bpt, pts):
    raw = np.array([oracle.llr(mag, sps, bpt, a, b, normalize=False) for a, b in pts])
    with np.errstate(all="ignore"):
        nl = np.array([oracle.llr(mag, sps, bpt, a, b) for a, b in pts])
    return raw, nl


@pytest.mark.parametrize("bpt,sps,F,T,dtype", LLR_GEO)
def test_llr_unequal_factors_vs_oracle(gpu, oracle, bpt, sps, F, T, dtype):
    """_device.llr on grid corners, edge midpoints and interior points, list lengths around k_llr's four
    candidates per wave; one direct ft8_llr call over three slots with a non-zero slot column."""
    from ft8_demodulator_amd import _device
    mags = [G.waterfall(9500 + s + bpt + 10 * sps, F, T, np.dtype(dtype), tones=False) for s in range(3)]
    pts = G.llr_points(F, T, bpt, sps, 63, 77 + bpt)
    raw, nl = _oracle_llrs(oracle, mags[0], sps, bpt, pts)
    # the corners' first / last data symbols lie outside the waterfall: zeroed triples (ft8_decode.py:177-181)
    assert (raw[0, :9] == 0).all() and (raw[2, -36:] == 0).all() and (raw[4:, 9:-36] != 0).any()
    wf = _wf(mags[0], sps, bpt)
    for n in (1, 2, 3, 4, 5, 63):
        for first in ((0,) if n == 63 else (0, 3)):     # the list starting at a corner / at another corner
            sel = [(first + i) % 63 for i in range(n)]
            got = _device.llr(wf, [pts[i] for i in sel], normalize=False)
            assert np.array_equal(got, raw[sel]), (n, first)
            with np.errstate(all="ignore"):
                got = _device.llr(wf, [pts[i] for i in sel], normalize=True)
            assert np.array_equal(got.view(np.uint64), nl[sel].view(np.uint64)), (n, first)
    # three slots, the slot column mixed so that one wave's four candidates come from different slots
    rows = [((2 * i + 1) % 3, *pts[i]) for i in range(21)]
    per = [_oracle_llrs(oracle, mags[s], sps, bpt, pts[:21]) for s in range(3)]
    got = G.llr_slots(mags, bpt, sps, rows, normalize=False)
    assert np.array_equal(got, np.array([per[s][0][i] for i, (s, _, _) in enumerate(rows)]))
    with np.errstate(all="ignore"):
        got = G.llr_slots(mags, bpt, sps, rows, normalize=True)
    assert np.array_equal(got.view(np.uint64), np.array([per[s][1][i] for i, (s, _, _) in enumerate(rows)]).view(np.uint64))


# ---- f. end to end ---------------------------------------------------------------------------------------
ST, P38, CZ, DFT = 0, 1, 2, 3  # ft8_stft_method: Stockham, packed 3840, chirp-z, direct DFT


@functools.lru_cache(maxsize=None)
def _slots():
    from ft8_demodulator_amd import synth
    x, _ = synth.make_slots(2, 6, snr_db=(-12.0, -4.0), seed=6100, device="cpu")
    return x.numpy()


# ft8_stft_method at 12 kHz: nfft = 1920 bpt, hop = 1920 / sps.  The packed 3840 kernel needs nfft 3840 AND hop
# 960 (stft3840_eligible), so (2, 4) and (2, 1) miss it on the hop, (3, 2) (nfft 5760) and (1, 2) (nfft 1920) on
# the length: all four take the LDS Stockham FFT.
@pytest.mark.parametrize("bpt,sps,method", ((3, 2, ST), (2, 4, ST), (2, 1, ST), (1, 2, ST)))
def test_end_to_end_unequal_factors_matches_oracle(gpu, oracle, bpt, sps, method):
    from ft8_demodulator_amd import _lib, decode_ft8_message
    x = _slots()
    assert _lib.lib().ft8_stft_method(_lib.context().handle, 12000, bpt, sps, x.shape[1], _lib.FT8_F32) == method
    kw = dict(max_candidates=300, min_score=6, max_iterations=20)
    for s in range(x.shape[0]):
        got = decode_ft8_message(x[s], 12000, bpt, sps, **kw)
        ref = oracle.decode_ft8_message(x[s], 12000, bpt, sps, **kw)
        assert len({r[0] for r in ref}) >= 3, (bpt, sps, s)
        assert sorted((m.payload.hex(), m.hash, t, f) for m, _s, t, f, _sc in got) == \
            sorted((p.hex(), h, t, f) for (p, h, _e, _ce, _cc, t, f, _sc) in ref), (bpt, sps, s)
        for (m, _s, t, f, sc), r in zip(sorted(got, key=lambda g: (g[2], g[3])), sorted(ref, key=lambda r: (r[5], r[6]))):
            assert abs(float(sc) - float(r[7])) <= 1e-4
