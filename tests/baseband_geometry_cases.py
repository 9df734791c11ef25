"""Shared inputs for the baseband geometry tests (test_baseband_geometry_cases.py,
test_gpu_baseband_geometry.py): the coherent pass (csrc/coherent.hip) and the subtraction
(csrc/subtract.hip) on csrc/baseband.h at bins_per_tone != steps_per_symbol, at Q != 32, at
steps_per_symbol 1 and at every trip count of bb_mix_down's vector loop, each input and each float64
restatement result (coherent.coherent_restate, oracle/subtract.py) computed once on the CPU and never
modified.

nsps = int(0.16 fs); Q, D, Mt, nT as coherent.geometry gives them; hop = nsps / sps.

| row | fs      | bpt | sps | nsps | Q  | D   | hop  | Mt | nT | what only this row reaches                         |
|-----|---------|-----|-----|------|----|-----|------|----|----|----------------------------------------------------|
| a   | 12000   | 3   | 2   | 1920 | 32 | 60  | 960  | 8  | 17 | bpt != sps on the production baseband (nfft 5760)  |
| b   | 12000   | 2   | 1   | 1920 | 32 | 60  | 1920 | 16 | 33 | nT = kCohMaxT, Mz = 2562 (last kCohOwn slot)       |
| c   | 12000   | 2   | 3   | 1920 | 32 | 60  | 640  | 6  | 13 | Mt D = 360 > hop / 2 = 320 (the ceiling not exact) |
| d   | 12000   | 1   | 8   | 1920 | 32 | 60  | 240  | 2  | 5  | smallest search, bin = tone spacing                |
| e   | 6250    | 2   | 1   | 1000 | 25 | 40  | 1000 | 13 | 27 | odd Q with sps 1: jj >= 2 Q, d >= Q; D = 40 tail   |
| f   | 6250    | 2   | 2   | 1000 | 25 | 40  | 500  | 7  | 15 | odd Q, Mt D > hop / 2                              |
| g   | 12006.3 | 2   | 1   | 1921 | 17 | 113 | 1921 | 9  | 19 | odd Q and odd D, range-checked loop, float rate    |
| h   | 2650    | 2   | 2   | 424  | 8  | 53  | 212  | 2  | 5  | smallest Q: coh_multi_words grows with nsym 3      |
| i   | 5500    | 2   | 2   | 880  | 22 | 40  | 440  | 6  | 13 | even Q != 32                                       |
| j   | 3000    | 2   | 2   | 480  | 32 | 15  | 240  | 8  | 17 | small odd D                                        |
| k   | 1600    | 2   | 2   | 256  | 32 | 8   | 128  | 8  | 17 | one partial trip: six of eight loads clamped to 4  |
| l   | 800     | 2   | 2   | 128  | 32 | 4   | 64   | 8  | 17 | D - 4 = 0                                          |
| m   | 48000   | 2   | 2   | 7680 | 32 | 240 | 3840 | 8  | 17 | eight trips, the last with four live loads         |

No row was dropped: the library's geometry() takes every rate of the table.  Of the rows with bpt != sps
(a, b, c, d, e, g) only g cannot be called with its factors transposed (nsps 1921 has no hop at sps 2);
the others are the transposition rows of the CPU test, a and d those of the device test.

Every row holds the bounds the 12 kHz (2, 2) and 10 kHz (4, 4) tests have (coherent_cases.LLR_BOUND,
subtract_cases.check_fits, the -40 dB residual): MEASURED below lists each row's figure on an MI355X
against the float64 restatement."""
import functools

import numpy as np

from ft8_demodulator_amd import coherent, synth
from ft8_demodulator_amd._lib import RESULT_DTYPE

import coherent_cases as C

#        fs       bpt sps nsps  Q   D   hop  Mt  nT
TABLE = {
    "a": (12000,   3, 2, 1920, 32, 60,  960,  8,  17),
    "b": (12000,   2, 1, 1920, 32, 60,  1920, 16, 33),
    "c": (12000,   2, 3, 1920, 32, 60,  640,  6,  13),
    "d": (12000,   1, 8, 1920, 32, 60,  240,  2,  5),
    "e": (6250,    2, 1, 1000, 25, 40,  1000, 13, 27),
    "f": (6250,    2, 2, 1000, 25, 40,  500,  7,  15),
    "g": (12006.3, 2, 1, 1921, 17, 113, 1921, 9,  19),
    "h": (2650,    2, 2, 424,  8,  53,  212,  2,  5),
    "i": (5500,    2, 2, 880,  22, 40,  440,  6,  13),
    "j": (3000,    2, 2, 480,  32, 15,  240,  8,  17),
    "k": (1600,    2, 2, 256,  32, 8,   128,  8,  17),
    "l": (800,     2, 2, 128,  32, 4,   64,   8,  17),
    "m": (48000,   2, 2, 7680, 32, 240, 3840, 8,  17),
}
ROWS = tuple(TABLE)
DRIFT = coherent.DEFAULT_DRIFT          # (1.0, 9)
DRIFT_ROWS = ("b", "e", "h")            # kCohOwn's last slot, odd Q, Q = 8
NSYM_ROWS = ("e", "g", "h")
PCM_ROWS = ("e", "k")
MISALIGNED_ROWS = ("a", "k")
TRANSPOSABLE_ROWS = ("a", "b", "c", "d", "e")   # bpt != sps and the transposed pair is a geometry
TRANSPOSED_ROWS = ("a", "d")            # ... run on the device by keyword and by position
MASK_ROWS = ("a", "f")
T_LO, F_LO = 3, 41                      # the masked runs' first kept frame and bin
SEEDS = {r: 9100 for r in ROWS}         # coherent case: the slot's seed (see test_baseband_geometry_cases.py)
SUB_SEED = 9400
SUB_LEVEL_DB = -4.0

# max |LLR_device - LLR_restate| of the plain float32 run of every row, measured once on an MI355X against
# the float64 restatement.  Every row is inside coherent_cases.LLR_BOUND = 1.49e-4, row m (D = 240) included,
# so no row has a bound of its own.  int16: e 1.79e-5, k 1.64e-5; drift (1.0, 9): b 3.27e-5, e 3.32e-5,
# h 3.27e-5, also inside LLR_BOUND; max_nsym 3 (sets 2 and 3, bound 6.50e-4): e 6.12e-5, g 2.01e-5, h 9.06e-5.
# The subtraction's residual stands 88 dB or more below the subtracted energy at every row (bound 40 dB).
MEASURED = {"a": 2.72e-5, "b": 4.27e-5, "c": 1.68e-5, "d": 2.82e-5, "e": 1.60e-5, "f": 2.68e-5, "g": 1.45e-5,
            "h": 2.62e-5, "i": 9.54e-6, "j": 1.73e-5, "k": 2.31e-5, "l": 3.39e-5, "m": 2.81e-5}


class Geo:
    """One row of the table, from the rate and the factors alone (the table's columns are asserted
    against it in test_baseband_geometry_cases.py)."""

    def __init__(self, row, bpt=None, sps=None):
        fs, tb, ts = TABLE[row][:3]
        self.row, self.fs = row, fs
        self.bpt, self.sps = (tb if bpt is None else bpt), (ts if sps is None else sps)
        self.nsps = int(0.16 * fs)                       # spectrogram_analyse.py:32
        self.nfft = int(fs / 6.25 * self.bpt)            # :34
        self.hop, self.Q, self.D, self.Mt, self.Mg = coherent.geometry(self.nsps, self.sps)
        self.nT = 2 * self.Mt + 1
        self.Mz = 79 * self.Q + 2 * self.Mg
        self.binw = fs / self.nfft
        self.n = int(15.0 * fs)                          # synth.make_slots: one 15 s slot
        self.L = 79 * self.nsps
        self.fhi = min(2500.0, fs / 2 - 80.0)

    def columns(self):
        return (self.fs, self.bpt, self.sps, self.nsps, self.Q, self.D, self.hop, self.Mt, self.nT)


@functools.lru_cache(maxsize=None)
def geo(row):
    return Geo(row)


def _pcm(x):
    """float32 samples as int16 PCM at x / 8 of full scale (coherent_cases.stage_case_12k's scaling)."""
    return np.clip(np.round(x / 8.0 * 32767.0), -32767, 32767).astype(np.int16)


def _frozen(*arrays):
    for v in arrays:
        v.setflags(write=False)


# ---- the coherent case --------------------------------------------------------------------------------
N_EDGE = 4


@functools.lru_cache(maxsize=None)
def coherent_case(row):
    """One slot of three signals at -14 .. -8 dB, tone 0 in [min(300, fhi / 3), fhi]; candidates: the
    3 x 3 grid points around every signal (27), then two whose window starts before the slot (6 and 1.5
    symbols before it) and two whose window ends past it (80 and 93.5 symbols in), at bins inside the
    band -> dict(x float32 [1, n], pcm int16 [1, n], cand int32 [31, 2], slot_of, payloads)."""
    g = geo(row)
    x, truth = synth.make_slots(1, 3, fs=g.fs, snr_db=(-14.0, -8.0), f0_range=(min(300.0, g.fhi / 3), g.fhi),
                                seeds=[SEEDS[row]])
    cand = []
    for k in range(3):
        cand += C._grid9(*C.nearest(truth[0], k, g.fs, g.hop, g.binw))
    for sym, frac in ((-6.0, 0.6), (-1.5, 0.4), (80.0, 0.5), (93.5, 0.7)):
        cand.append((int(np.rint(sym * g.sps)), int(np.rint(frac * g.fhi / g.binw))))
    x = x.numpy().astype(np.float32)
    assert x.shape == (1, g.n)
    cand = np.array(cand, dtype=np.int32)
    slot_of = np.zeros(len(cand), dtype=np.int32)
    out = {"x": x, "pcm": _pcm(x), "cand": cand, "slot_of": slot_of,
           "payloads": tuple(bytes(p) for p in truth[0].payloads)}
    _frozen(x, out["pcm"], cand, slot_of)
    return out


def edge(row):
    """The indices of the case's candidates whose windows lie across a slot edge."""
    n = len(coherent_case(row)["cand"])
    return np.arange(n - N_EDGE, n)


@functools.lru_cache(maxsize=None)
def coherent_ref(row, key="f32", drift=None, nsym=1, bpt=None, sps=None, masked=False, cand_shift=(0, 0)):
    """coherent.coherent_restate(details=True) of the row's case.  key: "f32" or "i16"; bpt, sps: other
    factors than the row's (the transposition check); masked: the candidates renumbered for t_lo = T_LO,
    f_lo = F_LO and the restatement called with both; cand_shift: subtracted from every candidate with
    t_lo = f_lo = 0 (what a run that dropped the masks would compute)."""
    g = geo(row) if bpt is None else Geo(row, bpt, sps)
    c = coherent_case(row)
    cand = c["cand"]
    t_lo = f_lo = 0
    if masked:
        cand, t_lo, f_lo = masked_cand(row), T_LO, F_LO
    elif cand_shift != (0, 0):
        cand = cand - np.array(cand_shift, dtype=np.int32)
    return coherent.coherent_restate(c["x"] if key == "f32" else c["pcm"], cand, c["slot_of"], g.fs, g.nsps, g.nfft,
                                     g.sps, t_lo=t_lo, f_lo=f_lo, details=True, drift=drift, nsym=nsym)


def masked_cand(row):
    """The case's candidates as a run with t_lo = T_LO, f_lo = F_LO numbers them: the same signals."""
    cand = coherent_case(row)["cand"] - np.array([T_LO, F_LO], dtype=np.int32)
    cand.setflags(write=False)
    return cand


def grids_of(ref, drift=False, nsym=1):
    """The metric grids (drift: volumes) of a coherent_ref result."""
    return ref[2 + int(drift) + int(nsym > 1)]


def ties(ref, drift=False, nsym=1):
    """-> (measured candidates, those among them whose two best metrics are within 1e-5): what
    coherent_cases.check_stage leaves out, at most one in twenty of the measured."""
    measured = ref[1]["status"] == 0
    tie = np.array([v is not None and coherent.near_tie(v) for v in grids_of(ref, drift, nsym)])
    return int(measured.sum()), int((measured & tie).sum())


# ---- the subtract case --------------------------------------------------------------------------------
_ALL = (0, 1, 2)
# one list (slot) per entry, every list subtracted from the same samples: the move of its records in grid
# points and the signals it holds.  List 1 holds the inner signal alone, so that samples no fit covers exist
SUB_LISTS = (((0, 0), _ALL), ((0, 0), (1,)))
SUB_LISTS_B = SUB_LISTS + (((-1, 0), _ALL), ((0, 1), _ALL))


def sub_lists(row):
    return SUB_LISTS_B if row == "b" else SUB_LISTS


@functools.lru_cache(maxsize=None)
def subtract_row(row):
    """Unit noise and three GFSK signals at -4 dB: one starts nsps + 7 samples before the slot, one lies
    inside, one ends nsps + 5 samples past it; tone 0 at 0.3, 0.55 and 0.8 fhi plus a fraction of a bin
    -> dict(x float32 [n], pcm int16 [n], payloads, f0, start)."""
    import torch
    g = geo(row)
    rng = np.random.default_rng(SUB_SEED)
    pays = [synth.random_payload(rng) for _ in range(3)]
    f0 = np.array([0.3, 0.55, 0.8]) * g.fhi + rng.uniform(-0.5, 0.5, 3) * g.binw
    start = np.array([-(g.nsps + 7), int(0.9 * g.fs) + 3, g.n - g.L + g.nsps + 5], dtype=np.int64)
    noise, _ = synth.make_slots(1, 0, fs=g.fs, seeds=[SUB_SEED])
    tones = torch.as_tensor(np.stack([synth.itones(p) for p in pays]))
    wav = synth.gfsk_waveforms(tones, g.fs, torch.as_tensor(f0))
    wav *= float(np.sqrt(2.0 * 10.0 ** (SUB_LEVEL_DB / 10.0)))
    assert wav.shape[1] == g.L and noise.shape[1] == g.n
    x = noise[0].to(torch.float64)
    for i, s in enumerate(start):
        lo, hi = max(int(s), 0), min(int(s) + g.L, g.n)
        x[lo:hi] += wav[i, lo - int(s):hi - int(s)]
    x = x.to(torch.float32).numpy()
    out = {"x": x, "pcm": _pcm(x), "payloads": tuple(bytes(p) for p in pays), "f0": f0, "start": start}
    _frozen(x, out["pcm"], f0, start)
    return out


def _rec(g, r, i, slot, t_lo=0, f_lo=0, dt=0, df=0):
    """The ft8_result of signal i at the grid point nearest it, moved by (dt, df) points, as a plan that
    starts at frame t_lo and bin f_lo numbers it (subtract_cases._rec at any geometry)."""
    q = np.zeros((), dtype=RESULT_DTYPE)
    q["payload"] = np.frombuffer(r["payloads"][i], dtype=np.uint8)
    q["abs_time"] = int(np.rint(r["start"][i] / g.hop)) - t_lo + dt
    q["abs_freq"] = int(np.rint(r["f0"][i] * g.nfft / g.fs)) - f_lo + df
    q["slot"], q["ok"], q["score"], q["cand_index"] = slot, 1, 10.0 + i, i
    return q


@functools.lru_cache(maxsize=None)
def subtract_records(row, t_lo=0, f_lo=0):
    """-> (records [n_lists, 3], counts int32 [n_lists]): list s holds the records of sub_lists(row)[s];
    rows at and past a list's count hold good records of the signals it leaves out: were they read, they
    would be fitted and subtracted."""
    g, r = geo(row), subtract_row(row)
    lists = sub_lists(row)
    recs = np.zeros((len(lists), 3), dtype=RESULT_DTYPE)
    counts = np.array([len(sig) for _, sig in lists], dtype=np.int32)
    for s, ((dt, df), sig) in enumerate(lists):
        order = list(sig) + [i for i in _ALL if i not in sig]
        for j, i in enumerate(order):
            recs[s, j] = _rec(g, r, i, s, t_lo, f_lo, dt, df)
            recs[s, j]["cand_index"] = j
    _frozen(recs, counts)
    return recs, counts


def sub_host(row, key):
    """What the oracle reads for "f32" (the samples) or "i16" (pcm / 32767)."""
    r = subtract_row(row)
    return r["x"] if key == "f32" else r["pcm"].astype(np.float64) / 32767.0


@functools.lru_cache(maxsize=None)
def subtract_fits(row, key="f32", bpt=None, sps=None, masked=False, drop_masks=False):
    """oracle/subtract.py's fits of every list -> tuple (per list) of tuples (per record).  bpt, sps:
    other factors than the row's; masked: the records numbered for t_lo = T_LO, f_lo = F_LO and fitted
    with both; drop_masks: those records fitted with t_lo = f_lo = 0."""
    from oracle import subtract as OS
    g = geo(row) if bpt is None else Geo(row, bpt, sps)
    recs, counts = subtract_records(row, T_LO, F_LO) if (masked or drop_masks) else subtract_records(row)
    t_lo, f_lo = (T_LO, F_LO) if masked else (0, 0)
    x = sub_host(row, key)
    cache = {}
    return tuple(tuple(OS.fits(x, recs[s, :counts[s]], g.fs, g.nsps, g.hop, g.nfft, t_lo, f_lo, cache=cache))
                 for s in range(len(recs)))


@functools.lru_cache(maxsize=None)
def subtract_residual(row, key, s=0):
    """oracle/subtract.py's residual of list s for its own fits (float64 [n])."""
    from oracle import subtract as OS
    g = geo(row)
    res = OS.residual(np.asarray(sub_host(row, key)), subtract_fits(row, key)[s], g.nsps, g.fs)
    _frozen(res)
    return res


def mask_plan_args(row):
    """time_min, freq_min for _pipeline.make_plan so that the plan starts at frame T_LO and bin F_LO:
    frame t is centred at (nsps / 2 + t hop) / fs, bin f at f binw; half a step below each."""
    g = geo(row)
    return (g.nsps / 2 + (T_LO - 0.5) * g.hop) / g.fs, (F_LO - 0.5) * g.binw
