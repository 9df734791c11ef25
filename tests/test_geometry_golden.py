"""The oracle (oracle/ft8_oracle.c) against the reference's own outputs at unequal oversampling factors
(tests/golden/geometry.*, captured by tools/make_golden_geometry.py): bins_per_tone != steps_per_symbol in
float32 and float64, T % sps != 0, and the grid corners whose first / last data symbols fall outside the
waterfall.  tests/test_oracle_golden.py pins it only where the two factors are equal.  Bit-exact throughout."""
import numpy as np

import geometry_cases as G


def test_fixture_set_is_the_one_described():
    cases, arr = G.fixtures()
    geo = {(c["bpt"], c["sps"], c["dtype"], c["quantised"]) for c in cases}
    assert geo == {(3, 2, "float32", False), (1, 2, "float32", False), (2, 1, "float32", False),
                   (2, 4, "float32", False), (2, 8, "float32", False), (5, 5, "float32", False),
                   (1, 1, "float32", False), (3, 2, "float64", False), (1, 4, "float64", False),
                   (3, 2, "float32", True)}
    for c in cases:
        mag = arr[f"geo_{c['name']}_mag"]
        assert mag.shape == (c["F"], c["T"]) and str(mag.dtype) == c["dtype"]
        t0, NT, NF = G.grid_bounds(c["F"], c["T"], c["bpt"], c["sps"])
        assert 26 <= NF <= 60 and 62 <= c["T"] // c["sps"] <= 75
        assert arr[f"geo_{c['name']}_grid"].shape == (NT, NF)
        assert c["corners"] == [[t0, 0], [t0, NF - 1], [t0 + NT - 1, 0], [t0 + NT - 1, NF - 1]]
        assert 2 <= len(c["sel"]) <= 3
    assert sum(c["T"] % c["sps"] != 0 for c in cases) >= 2
    assert all(np.array_equal(arr[f"geo_{c['name']}_mag"], np.round(arr[f"geo_{c['name']}_mag"]))
               for c in cases if c["quantised"])


def test_score_grids(oracle):
    cases, arr = G.fixtures()
    for c in cases:
        g = oracle.score_grid(arr[f"geo_{c['name']}_mag"], c["sps"], c["bpt"])
        ref = arr[f"geo_{c['name']}_grid"]
        assert g.dtype == ref.dtype and g.shape == ref.shape, c["name"]
        assert np.array_equal(g.view(np.uint8), ref.view(np.uint8)), c["name"]


def test_selection(oracle):
    cases, arr = G.fixtures()
    n_err = n = 0
    for c in cases:
        mag = arr[f"geo_{c['name']}_mag"]
        for s in c["sel"]:
            tag = (c["name"], s["N"], s["min_score"])
            cands, tie = oracle.find_candidates(mag, c["sps"], c["bpt"], s["N"], s["min_score"])
            # tie flag <=> the reference raised TypeError (an exact tie reached a heap comparison)
            assert tie == (s["error"] is not None), tag
            if s["error"] is not None:
                n_err += 1
                continue
            assert [[a, b] for a, b, _ in cands] == s["cands"], tag
            sc = arr[f"geo_{c['name']}_N{s['N']}_ms{s['min_score']}_scores"]
            assert str(sc.dtype) == c["dtype"]
            assert np.array_equal(np.array([x for _, _, x in cands], dtype=sc.dtype), sc), tag
            n += 1
    assert n_err >= 1 and n >= 20


def test_llr(oracle):
    cases, arr = G.fixtures()
    zeroed = 0
    for c in cases:
        mag = arr[f"geo_{c['name']}_mag"]
        cands, raw, nl = G.fixture_llrs(c, arr)
        assert len(cands) == 10 and raw.shape == nl.shape == (10, 174)
        for k, (a, b) in enumerate(cands):
            r = oracle.llr(mag, c["sps"], c["bpt"], a, b, normalize=False)
            assert np.array_equal(r.view(np.uint64), raw[k].view(np.uint64)), (c["name"], a, b)
            with np.errstate(all="ignore"):
                x = oracle.llr(mag, c["sps"], c["bpt"], a, b)
            assert np.array_equal(x.view(np.uint64), nl[k].view(np.uint64)), (c["name"], a, b)
        # the corners hold symbols before block 0 (first row) and past the last block (last row)
        for k in range(6, 10):
            z = raw[k].reshape(58, 3)
            zeroed += int((z == 0).all(axis=1).sum())
            assert (z[:3] == 0).all() if k < 8 else (z[-12:] == 0).all(), (c["name"], k)
    assert zeroed >= 10 * (2 * 3 + 2 * 12)
