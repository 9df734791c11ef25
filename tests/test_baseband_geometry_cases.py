"""What the baseband geometry cases (tests/baseband_geometry_cases.py) must hold for
test_gpu_baseband_geometry.py to reach the paths it is about and for its comparisons to be live, checked
on the float64 restatements alone (coherent.coherent_restate, oracle/subtract.py, snr.snr_reference): an
edit of a seed or of the table that emptied one of those paths, broke the near-tie cap or made a
transposed pair of factors invisible fails here, on the CPU."""
import numpy as np
import pytest

from conftest import ROOT  # noqa: F401  (puts the repo root on sys.path)

import baseband_geometry_cases as B
import coherent_cases as C
import subtract_cases as S

ROWS = B.ROWS


# ---- the table ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ROWS)
def test_table_columns(row):
    g = B.geo(row)
    assert g.columns() == B.TABLE[row]
    assert g.nT <= 33 and g.Q in range(8, 33) and g.nsps == g.Q * g.D == g.hop * g.sps
    assert g.nfft >= g.nsps                                   # what the library's geometry() asks


def test_table_claims():
    g = {r: B.geo(r) for r in ROWS}
    # the third term of zp[jj + (jj >= Q) + (jj >= 2 Q)] (coherent.hip) and dq = d + (d >= Q) (subtract.hip)
    # are live where the largest jj = 2 Mt + Q - 1 reaches 2 Q: odd Q with sps 1
    assert [r for r in ROWS if 2 * g[r].Mt + g[r].Q - 1 >= 2 * g[r].Q] == ["e", "g"]
    assert [r for r in ROWS if g[r].D % 4 == 0] == ["a", "b", "c", "d", "e", "f", "i", "k", "l", "m"]
    assert g["b"].Mz == 2562 and g["b"].nT == 33              # kCohOwn's last slot, kCohMaxT
    assert max(v.Mz for v in g.values()) == 2562
    assert (g["c"].Mt * g["c"].D, g["c"].hop // 2) == (360, 320) and g["f"].Mt * g["f"].D > g["f"].hop / 2
    # bb_mix_down's trips of 8 four-sample loads: D 4 and 8 clamp to D - 4 = 0 and 4, D 40 has a tail
    # trip with two live loads, D 240 eight trips, the last with four
    assert (g["l"].D, g["k"].D, g["e"].D, g["m"].D) == (4, 8, 40, 240)
    assert (40 - 32) // 4 == 2 and 240 // 32 == 7 and (240 - 7 * 32) // 4 == 4
    assert g["h"].Q == 8 and 8 * (8 + 1) + 58 * 8 > 5 * 8 * (8 + 1)      # coh_multi_words grows below Q 14
    # the transposed pair is a geometry everywhere but at row g
    for r in ROWS:
        if g[r].bpt != g[r].sps:
            ok = g[r].nsps % g[r].bpt == 0 and int(g[r].fs / 6.25 * g[r].sps) >= g[r].nsps
            assert ok == (r in B.TRANSPOSABLE_ROWS), r
    assert set(B.TRANSPOSED_ROWS) <= set(B.TRANSPOSABLE_ROWS) and "g" not in B.TRANSPOSABLE_ROWS


# ---- the coherent case ---------------------------------------------------------------------------------
def _option_sets(row):
    """(key, drift, nsym, masked) of every restatement the device test compares at this row."""
    out = [("f32", None, 1, False)]
    if row in B.PCM_ROWS:
        out.append(("i16", None, 1, False))
    if row in B.DRIFT_ROWS:
        out.append(("f32", B.DRIFT, 1, False))
    if row in B.NSYM_ROWS:
        out.append(("f32", None, 3, False))
    if row in B.MASK_ROWS:
        out.append(("f32", None, 1, True))
    return out


@pytest.mark.parametrize("row", ROWS)
def test_coherent_case_is_measured_and_within_the_tie_cap(row):
    """Every grid candidate has status 0, the edge candidates lack sync symbols or have none, and no
    option set leaves out more than one measured candidate in twenty for a near tie."""
    g, c = B.geo(row), B.coherent_case(row)
    assert len(c["cand"]) == 27 + B.N_EDGE and len(set(c["payloads"])) == 3
    e = B.edge(row)
    nb = c["cand"][e, 0].astype(np.int64) * g.hop - g.Mg * g.D
    assert (nb[:2] < 0).all() and (nb[2:] + g.Mz * g.D > g.n).all()
    for key, drift, nsym, masked in _option_sets(row):
        ref = B.coherent_ref(row, key, drift, nsym, masked=masked)
        fits = ref[1]
        assert (fits["status"][:27] == 0).all(), (row, key, drift, nsym)
        assert (((fits["n_sync"][e] % 21) != 0) | (fits["status"][e] == 2)).all()
        assert (fits["status"][e] == 2).any() and ((fits["n_sync"][e] % 21) != 0).any()
        n_measured, n_tie = B.ties(ref, drift is not None, nsym)
        assert n_measured >= 27 and n_tie * 20 <= n_measured, (row, key, drift, nsym, n_tie, n_measured)
        if nsym > 1:
            assert (ref[2][:27] == 7).all()                  # every set of every grid candidate is valid
        if drift is not None:
            assert len(set(ref[2]["rate_index"].tolist())) >= 2


@pytest.mark.parametrize("row", ["b", "e"])
def test_winners_at_both_ends_of_the_start_search(row):
    """jj = d + q is largest at dt_index = +Mt; at sps 1 the time neighbours of a signal's grid point win
    at either end of the search."""
    g = B.geo(row)
    dt = B.coherent_ref(row)[1]["dt_index"][:27]
    assert {-g.Mt, g.Mt} <= set(dt.tolist())
    if row in B.DRIFT_ROWS:
        assert g.Mt in B.coherent_ref(row, "f32", B.DRIFT)[1]["dt_index"][:27].tolist()
    if row in B.NSYM_ROWS:
        assert g.Mt in B.coherent_ref(row, "f32", None, 3)[1]["dt_index"][:27].tolist()


@pytest.mark.parametrize("row", B.TRANSPOSABLE_ROWS)
def test_transposed_factors_change_every_llr_vector(row):
    """coherent_restate with bins_per_tone and steps_per_symbol exchanged differs from the right call by
    more than the LLR bound at every grid candidate: a transposed pair anywhere between the wrappers
    and the kernel fails the device test."""
    g = B.geo(row)
    right = B.coherent_ref(row)[0][:27]
    wrong = B.coherent_ref(row, bpt=g.sps, sps=g.bpt)[0][:27]
    assert np.abs(right - wrong).max(axis=1).min() > C.LLR_BOUND


@pytest.mark.parametrize("row", B.MASK_ROWS)
def test_masks_are_live_and_name_the_same_samples(row):
    """The renumbered candidates with t_lo, f_lo restate to the unmasked run's results exactly (s0 and
    fmix are the same doubles); without t_lo, f_lo they differ by more than the bound everywhere."""
    g, c = B.geo(row), B.coherent_case(row)
    mc = B.masked_cand(row)
    for (at, af), (mt, mf) in zip(c["cand"].tolist(), mc.tolist()):
        assert (B.T_LO + mt) * g.hop == at * g.hop
        assert (B.F_LO + mf) * g.binw + 3.5 * 6.25 == af * g.binw + 3.5 * 6.25
    plain, masked = B.coherent_ref(row), B.coherent_ref(row, masked=True)
    assert np.array_equal(plain[0], masked[0]) and plain[1].tobytes() == masked[1].tobytes()
    dropped = B.coherent_ref(row, cand_shift=(B.T_LO, B.F_LO))
    assert np.abs(plain[0][:27] - dropped[0][:27]).max(axis=1).min() > C.LLR_BOUND
    # the plan of the subtraction's masked run starts at that frame and bin
    time_min, freq_min = B.mask_plan_args(row)
    t = (g.nsps / 2 + np.arange(8) * g.hop) / g.fs
    assert int(np.argmax(t >= time_min)) == B.T_LO and int(np.argmax(np.arange(64) * g.binw >= freq_min)) == B.F_LO


# ---- the subtract case ---------------------------------------------------------------------------------
def _fit_moved(a, b, g):
    """Whether two fits differ beyond check_fits' tolerance in start or tone-0 frequency."""
    return abs(a["start"] - b["start"]) > 1 or abs(a["f0"] - b["f0"]) > 1e-3


@pytest.mark.parametrize("row", ROWS)
def test_subtract_case_covers_the_slot_edges(row, oracle):
    g, r = B.geo(row), B.subtract_row(row)
    assert r["start"][0] == -(g.nsps + 7) and r["start"][2] + g.L == g.n + g.nsps + 5
    assert 0 < r["start"][1] and r["start"][1] + g.L < g.n
    for key in ("f32",) + (("i16",) if row in B.PCM_ROWS else ()):
        fits = B.subtract_fits(row, key)
        assert len(fits) == len(B.sub_lists(row)) and [len(v) for v in fits[:2]] == [3, 1]
        for lst in fits:
            assert all(f is not None for f in lst)
        f = fits[0]
        # the records sit at the nearest grid point: the fit returns to the signal
        assert [abs(f[i]["start"] - int(r["start"][i])) <= g.D for i in range(3)] == [True] * 3
        assert f[0]["start"] < 0 and f[2]["start"] + g.L > g.n
        # list 1 holds the inner signal alone: samples no fit covers exist on either side of it
        res = B.subtract_residual(row, key)
        x = np.asarray(B.sub_host(row, key), dtype=np.float64)
        one = fits[1][0]
        assert one["start"] == f[1]["start"] and one["start"] > g.nsps and one["start"] + g.L < g.n - g.nsps
        res1 = B.subtract_residual(row, key, 1)
        assert np.array_equal(res1[:one["start"]], x[:one["start"]])
        assert np.array_equal(res1[one["start"] + g.L:], x[one["start"] + g.L:])
        # at least the energy of the signal inside the slot is taken out (int16: the samples are x / 8)
        scale = 1.0 if key == "f32" else 1.0 / 64.0
        assert np.sum((x - res) ** 2) > 0.5 * g.L * 10.0 ** (B.SUB_LEVEL_DB / 10.0) * scale


def test_subtract_row_b_fits_at_the_edges_of_the_search(oracle):
    """Records moved one grid point early in time fit at start offset +Mt = 16, the last of the 33;
    moved one bin up they fit at tone-0 offset -KMF."""
    g = B.geo("b")
    base, _, early, up = B.subtract_fits("b")
    assert [f["dt"] for f in early] == [g.Mt] * 3
    assert [f["df"] for f in up] == [-S.KMF] * 3
    assert all(abs(f["dt"]) < g.Mt for f in base)


@pytest.mark.parametrize("row", B.TRANSPOSABLE_ROWS)
def test_transposed_factors_move_every_fit(row, oracle):
    g = B.geo(row)
    right = B.subtract_fits(row)[0]
    wrong = B.subtract_fits(row, bpt=g.sps, sps=g.bpt)[0]
    assert all(_fit_moved(a, b, g) for a, b in zip(right, wrong))


@pytest.mark.parametrize("row", B.MASK_ROWS)
def test_subtract_masks_are_live(row, oracle):
    g = B.geo(row)
    plain, masked, dropped = B.subtract_fits(row)[0], B.subtract_fits(row, masked=True)[0], \
        B.subtract_fits(row, drop_masks=True)[0]
    for a, b, c in zip(plain, masked, dropped):
        assert a["start"] == b["start"] and a["f0"] == b["f0"] and np.array_equal(a["amp"], b["amp"])
        assert _fit_moved(a, c, g)
    recs, mrecs = B.subtract_records(row)[0][0], B.subtract_records(row, B.T_LO, B.F_LO)[0][0]
    assert ((mrecs["abs_time"] + B.T_LO) * g.hop == recs["abs_time"] * g.hop).all()
    assert ((mrecs["abs_freq"] + B.F_LO) * g.fs / g.nfft == recs["abs_freq"] * g.fs / g.nfft).all()


# ---- the SNR ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", B.TRANSPOSABLE_ROWS)
def test_transposed_factors_change_every_report(row):
    """snr_reference with the factors exchanged reads other rows and bins: every report moves by more
    than the 1e-6 dB the device test allows."""
    from ft8_demodulator_amd._lib import RESULT_DTYPE
    from ft8_demodulator_amd.snr import snr_reference
    g = B.geo(row)
    rng = np.random.default_rng(12)
    T, F = 100, 200
    wf = rng.normal(-50.0, 10.0, size=(1, T, F))
    recs = np.zeros((1, 6), dtype=RESULT_DTYPE)
    pay = rng.integers(0, 256, size=(6, 10), dtype=np.uint8)
    pay[:, 9] &= 0xF8
    recs["payload"], recs["ok"] = pay, 1
    recs["abs_time"], recs["abs_freq"] = rng.integers(1, 5, 6), rng.integers(1, F - 2 - 7 * max(g.bpt, g.sps), 6)
    right = snr_reference(wf, recs, None, g.fs, g.bpt, g.sps)
    wrong = snr_reference(wf, recs, None, g.fs, g.sps, g.bpt)
    assert (right["status"] < 2).all() and (wrong["status"] < 2).all()
    assert (np.abs(right["snr_db"] - wrong["snr_db"]) > 1e-6).all()
