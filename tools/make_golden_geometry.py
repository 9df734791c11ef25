"""Golden front-end vectors at UNEQUAL oversampling factors (bins_per_tone != steps_per_symbol), from
the reference itself (build container only; same import recipe as tools/make_golden.py::gold_sync).

Small seeded waterfalls -50 + 6 N(0,1) at (bpt, sps, dtype) = (3,2,f32) (1,2,f32) (2,1,f32) (2,4,f32)
(2,8,f32) (5,5,f32) (1,1,f32) (3,2,f64) (1,4,f64) and one quantised (3,2,f32) waterfall (np.round:
exact score ties).  Every F gives 26..60 grid columns, every T 62..75 blocks, five cases have
T % sps != 0.  Per case: the waterfall, the reference's score grid (ft8_sync_score over the
ft8_find_candidates ranges), two or three (N, min_score) selections (candidates and scores, or the
TypeError text when an exact tie reached a heap comparison), raw and normalised LLRs of the first
six candidates of the first selection that returned any, and of the four grid corners (whose first or
last data symbols lie before block 0 / past the last block: the zeroed triples).

-> tests/golden/geometry.json, tests/golden/geometry.npz.  No other golden file is read or written.

Usage:  python tools/make_golden_geometry.py   (from anywhere: it works in a scratch directory of its own)
"""
import contextlib
import io
import json
import os
import shutil
import sys
import tempfile
import zipfile

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLD = os.path.join(REPO, "tests", "golden")
sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")
sys.path.insert(0, "/root/reference/src")
with contextlib.redirect_stdout(io.StringIO()):
    from ft8_tools.ft8_demodulator import ft8_decode as R  # noqa: E402
    from ft8_tools.ft8_demodulator.ftx_types import FT8Waterfall, FT8Candidate  # noqa: E402

# name, bpt, sps, dtype, F, T, quantised, selections
CASES = (
    ("b3s2_32", 3, 2, "float32", 47, 125, False, ((25, 1), (7, -1000), (60, 0.5))),
    ("b1s2_32", 1, 2, "float32", 36, 124, False, ((25, 1), (80, -1000))),
    ("b2s1_32", 2, 1, "float32", 49, 64, False, ((25, 1), (9, 2.5), (40, -1000))),
    ("b2s4_32", 2, 4, "float32", 40, 251, False, ((25, 1), (5, -1000), (60, 0.25))),
    ("b2s8_32", 2, 8, "float32", 40, 501, False, ((25, 1), (60, 0.5))),
    ("b5s5_32", 5, 5, "float32", 61, 312, False, ((25, 1), (12, -1000))),
    ("b1s1_32", 1, 1, "float32", 51, 70, False, ((25, 1), (3, -1000), (80, 0.5))),
    ("b3s2_64", 3, 2, "float64", 47, 124, False, ((25, 1), (10, -1000))),
    ("b1s4_64", 1, 4, "float64", 33, 249, False, ((25, 1), (60, 0.5))),
    ("q_b3s2_32", 3, 2, "float32", 47, 124, True, ((10, 1), (300, -1000), (5, -1000))),
)
LLR_TOP = 6


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def ref_grid(wf, sps, bpt):
    F, _ = wf.mag.shape
    tr = range(-10 * sps, wf.num_blocks * sps - sps * 59)
    fr = range(0, F - 7 * bpt)
    out = np.empty((len(tr), len(fr)), dtype=wf.mag.dtype)
    for i, t in enumerate(tr):
        for j, f in enumerate(fr):
            out[i, j] = R.ft8_sync_score(wf, FT8Candidate(waterfall=wf, abs_time=t, abs_freq=f))
    return out, tr, fr


def ref_llr(wf, at, af, normalize):
    x = np.zeros(174)
    R.ft8_extract_likelihood(wf, FT8Candidate(waterfall=wf, abs_time=at, abs_freq=af), x)
    if normalize:
        with np.errstate(all="ignore"):
            R.ftx_normalize_logl(x)
    return x


def main():
    scratch = tempfile.mkdtemp(prefix="ft8geo_")
    os.chdir(scratch)
    rng = np.random.default_rng(3225)
    meta, arrays = [], {}
    for name, bpt, sps, dtype, F, T, quant, sels in CASES:
        mag = -50 + 6 * rng.standard_normal((F, T))
        if quant:
            mag = np.round(mag)
        mag = mag.astype(dtype)
        wf = FT8Waterfall(mag=mag, time_osr=sps, freq_osr=bpt)
        grid, tr, fr = ref_grid(wf, sps, bpt)
        assert 26 <= len(fr) <= 60 and 62 <= T // sps <= 75 and len(tr) > 0, name
        c = {"name": name, "bpt": bpt, "sps": sps, "dtype": dtype, "F": F, "T": T, "quantised": quant,
             "sel": [], "llr_sel": None}
        arrays[f"geo_{name}_mag"] = mag
        arrays[f"geo_{name}_grid"] = grid
        for N, ms in sels:
            try:
                got = quiet(R.ft8_find_candidates, wf, N, ms)
                e = {"N": N, "min_score": ms, "error": None, "cands": [[int(x.abs_time), int(x.abs_freq)] for x in got]}
                arrays[f"geo_{name}_N{N}_ms{ms}_scores"] = np.array([x.score for x in got], dtype=mag.dtype)
            except TypeError as err:  # an exact score tie reached a heap comparison
                e = {"N": N, "min_score": ms, "error": str(err)}
            if c["llr_sel"] is None and e["error"] is None and e["cands"]:
                c["llr_sel"] = len(c["sel"])
                top = e["cands"][:LLR_TOP]
                arrays[f"geo_{name}_sel_llr_raw"] = np.array([ref_llr(wf, a, b, False) for a, b in top])
                arrays[f"geo_{name}_sel_llr"] = np.array([ref_llr(wf, a, b, True) for a, b in top])
            c["sel"].append(e)
        c["corners"] = [[tr[0], fr[0]], [tr[0], fr[-1]], [tr[-1], fr[0]], [tr[-1], fr[-1]]]
        arrays[f"geo_{name}_corner_llr_raw"] = np.array([ref_llr(wf, a, b, False) for a, b in c["corners"]])
        arrays[f"geo_{name}_corner_llr"] = np.array([ref_llr(wf, a, b, True) for a, b in c["corners"]])
        meta.append(c)
    assert sum(c["T"] % c["sps"] != 0 for c in meta) >= 2
    q = [s["error"] is not None for c in meta if c["quantised"] for s in c["sel"]]
    assert any(q) and not all(q), "the quantised case needs a selection that raises and one that does not"
    # an .npz with LZMA members (np.load reads any zip method): the float mantissas fill most of the file, and
    # deflate (np.savez_compressed) leaves it 36 KB larger, above the 512 KB the two files are held to
    with zipfile.ZipFile(os.path.join(GOLD, "geometry.npz"), "w", zipfile.ZIP_LZMA) as z:
        for k, v in arrays.items():
            with z.open(k + ".npy", "w") as f:
                np.lib.format.write_array(f, np.asanyarray(v), allow_pickle=False)
    with open(os.path.join(GOLD, "geometry.json"), "w") as f:
        json.dump({"numpy": np.__version__, "cases": meta}, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    shutil.rmtree(scratch, ignore_errors=True)
    sizes = [os.path.getsize(os.path.join(GOLD, n)) for n in ("geometry.json", "geometry.npz")]
    for c in meta:
        print(c["name"], [("error" if s["error"] else len(s["cands"])) for s in c["sel"]], "llr_sel", c["llr_sel"])
    print("geometry.json", sizes[0], "geometry.npz", sizes[1], "total", sum(sizes), "bytes")
    assert sum(sizes) < 512 * 1024


if __name__ == "__main__":
    main()
