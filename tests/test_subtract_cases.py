"""The conditions the subtraction list cases (tests/subtract_cases.py) must meet for
test_gpu_subtract_lists.py to reach the paths it is about, checked on the float64 restatement alone
(oracle/subtract.py): an edit of the seeds that emptied one of those paths fails here, on the CPU."""
import numpy as np

from conftest import ROOT  # noqa: F401  (puts the repo root on sys.path)

import subtract_cases as C

REST_FROM = 32     # csrc/subtract.hip kSubRecStride: fits at and past this index belong to the rest launch
REST_GROUPS = 8    # kSubRestStride: rest workgroups per slot
WAVE = 64          # k_sub_list's chunk


def _fits(slot):
    return [f for f in C.oracle_fits("f32", slot) if f is not None]


def test_lists_have_the_shape_the_kernels_need(oracle):
    samples, records, counts, truth = C.batch()
    assert samples.shape == (C.N_SLOTS, C.N) and records.shape == (C.N_SLOTS, C.CAP)
    assert list(counts) == [132, 0, 33, 32, 0, 1, 2, 5, C.CAP + 5]
    # no two slots share a record list, and both rows are used
    lists = [records[s, :min(int(counts[s]), C.CAP)].tobytes() for s in range(C.N_SLOTS) if counts[s]]
    assert len(set(lists)) == len(lists) and set(truth["row"]) == {"A", "B"}
    for slot in range(C.N_SLOTS):
        ofit = C.oracle_fits("f32", slot)
        assert len(ofit) == min(int(counts[slot]), C.CAP)
        # the oracle keeps exactly the records the construction meant to be kept
        assert [j for j, f in enumerate(ofit) if f is not None] == list(truth["kept"][slot]), slot
    assert tuple(len(_fits(s)) for s in range(C.N_SLOTS)) == C.FITS_PER_SLOT
    # slot 0: kept records in k_sub_list's first and second chunk, each chunk with a kept record at a
    # lane above a skipped one (the ballot's prefix count is not the lane index), and a failed row
    # before its good row for every payload
    kept = truth["kept"][0]
    for lo in (0, WAVE):
        inside = [j for j in kept if lo <= j < lo + WAVE]
        assert inside and any(j > lo + i for i, j in enumerate(inside)), lo
    r0 = records[0, :132]
    for j in kept:
        same = [q for q in range(132) if bytes(r0[q]["payload"]) == bytes(r0[j]["payload"])]
        assert len(same) == 3 and same[1] == j and not r0[same[0]]["ok"] and r0[same[2]]["ok"]
        assert (r0[same[2]]["abs_time"], r0[same[2]]["abs_freq"]) != (r0[j]["abs_time"], r0[j]["abs_freq"])
    # the rest launch: groups 0-3 of slot 0 make two trips (fits 32-35, then 40-43), slot 2 has exactly
    # one rest fit, slot 3 none
    assert C.FITS_PER_SLOT[0] - REST_FROM - REST_GROUPS == 4
    assert C.FITS_PER_SLOT[2] == REST_FROM + 1 and C.FITS_PER_SLOT[3] == REST_FROM
    # slot 8: every one of the cap rows is a record, the count says more
    assert counts[8] > C.CAP and C.FITS_PER_SLOT[8] > REST_FROM


def test_fits_cover_the_search_grid_and_the_slot_edges(oracle):
    for slot in (0, 8):
        f = _fits(slot)
        dt, df = {q["dt"] for q in f}, {q["df"] for q in f}
        assert {-C.MT, C.MT} <= dt, (slot, sorted(dt))
        assert {-C.KMF, C.KMF} <= df, (slot, sorted(df))
        assert min(q["start"] for q in f) < 0, slot
        assert max(q["start"] for q in f) + C.L > C.N, slot
    # the rest launch's own fits (index >= 32) reach both ends of the start search in slot 0
    rest = _fits(0)[REST_FROM:]
    assert len(rest) == 12
    # the fit found every signal: within one step of the start search (D samples; a best point on the
    # grid's edge is not refined) and one step of the tone-0 search of where it was put
    _, _, _, truth = C.batch()
    for slot in range(C.N_SLOTS):
        r = C.row(truth["row"][slot])
        for q, i in zip(_fits(slot), truth["signal"][slot]):
            assert abs(q["start"] - int(r["start"][i])) <= C.D, (slot, i, q["start"], int(r["start"][i]))
            assert abs(q["f0"] - r["f0"][i]) <= 0.25 * C.FS / C.NFFT, (slot, i, q["f0"], r["f0"][i])


def test_oracle_residual_is_the_noise(oracle):
    """Slot 0's list holds every signal of row A: the residual's energy is the noise row's within 10 %;
    slot 8's list leaves two signals of row B out: the noise's and theirs."""
    for slot, left in ((0, C.row("A")["noise"]), (8, C.row("B")["rest8"])):
        e = float(np.sum(C.oracle_residual("f32", slot) ** 2))
        e0 = float(np.sum(np.asarray(left, dtype=np.float64) ** 2))
        assert abs(e / e0 - 1.0) <= 0.10, (slot, e / e0)
    # a silent slot's residual is its samples
    assert np.array_equal(C.oracle_residual("f32", 1), C.batch()[0][1].astype(np.float64))
