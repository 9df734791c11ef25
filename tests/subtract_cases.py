"""Shared inputs for the subtraction list tests (test_subtract_cases.py, test_gpu_subtract_lists.py):
two synthetic 12 kHz rows of unit noise and dense signals, hand-written ft8_result lists over them
for a batch of nine slots, and the float64 restatement's results (oracle/subtract.py), each computed
once on the CPU and never modified.

ft8_subtract takes the record list from its caller, so the lists here are written by hand, with no
decoder: they fix the order of the records, their duplicates, their failures, the counts and the
offset of every signal from its record's grid point.

Geometry: 12 kHz at 2 bins per tone and 2 steps per symbol: nsps 1920, hop 960, nfft 3840, Q 32,
D 60, start offsets -8 .. 8 (units of D), tone-0 offsets -2 .. 2 (units of bin / 4).  The plan keeps
every frame and bin (t_lo = f_lo = 0), so a record's abs_time is rint(start / hop) -- negative for a
signal whose head lies before the slot; the sync grid reaches down to abs_time -20 -- and its abs_freq
rint(f0 nfft / fs).  That rounding spreads the true offsets over the whole search grid, its edges
(where the parabola is skipped) included.

| slot | row | records                                              | fits | purpose                            |
|------|-----|------------------------------------------------------|------|------------------------------------|
| 0    | A   | 132: (failed, good, good duplicate) x 44, shuffled   | 44   | k_sub_list's later chunks; every   |
|      |     |                                                      |      | fit of the rest launch, two trips  |
| 1    | B   | count 0                                              | 0    | residual = samples                 |
| 2    | A   | 33 distinct good                                     | 33   | exactly one rest fit               |
| 3    | B   | 32 distinct good                                     | 32   | rest launch runs, every group exits|
| 4    | A   | count 0                                              | 0    |                                    |
| 5    | B   | 1 good                                               | 1    |                                    |
| 6    | A   | 2 good                                               | 2    |                                    |
| 7    | B   | 5: failed a, good a, good b, duplicate a, good c     | 3    |                                    |
| 8    | B   | 136 = cap: (failed, good, 2 duplicates) x 34,        | 34   | count above capacity; second group |
|      |     | shuffled; counts[8] = cap + 5                        |      | of eight slots of both grids       |

A failed row sits one grid point before the good row in time, a duplicate one grid point after it in
time or in frequency: were the wrong row of a payload fitted, the fit would differ.  Rows at and past
a slot's count hold good records of signals the slot's list leaves out: were they read, they would be
fitted and subtracted."""
import functools

import numpy as np

from ft8_demodulator_amd import synth
from ft8_demodulator_amd._lib import RESULT_DTYPE

FS, NSPS, HOP, NFFT = 12000, 1920, 960, 3840
T_LO, F_LO = 0, 0
N = 15 * FS
Q, D, MT, KMF = 32, 60, 8, 2
L = 79 * NSPS
N_SLOTS, CAP = 9, 136
ROW_OF_SLOT = "ABABABABB"
FITS_PER_SLOT = (44, 0, 33, 32, 0, 1, 2, 3, 34)
CUT = 2900                              # samples of the cut-off signals that lie outside the slot
ROWS = {"A": dict(seed=9101, n_sig=44, head=5, tail=30), "B": dict(seed=9250, n_sig=36, head=20, tail=3)}
SLOT8_LEFT_OUT = (10, 25)               # row B's signals that slot 8's list does not hold
LIST_SEED = 9300


@functools.lru_cache(maxsize=None)
def row(name):
    """One row -> dict(x float32 [N], noise float32 [N], payloads, f0, level_db, start): tone 0 at
    200 + 56.25 k Hz plus U(-1.5, 1.5), levels U(-8, 2) dB, starts U(0.2, 1.5) s, but for one signal
    that starts CUT samples before the slot and one that ends CUT samples past it."""
    import torch
    cfg = ROWS[name]
    n_sig = cfg["n_sig"]
    rng = np.random.default_rng(cfg["seed"])
    pays = [synth.random_payload(rng) for _ in range(n_sig)]
    f0 = 200.0 + 56.25 * np.arange(n_sig) + rng.uniform(-1.5, 1.5, n_sig)
    level = rng.uniform(-8.0, 2.0, n_sig)
    start = (rng.uniform(0.2, 1.5, n_sig) * FS).astype(np.int64)
    start[cfg["head"]] = -CUT - int(rng.integers(0, 60))
    start[cfg["tail"]] = N - L + CUT + int(rng.integers(0, 60))
    noise, _ = synth.make_slots(1, 0, fs=FS, seeds=[cfg["seed"]])
    tones = torch.as_tensor(np.stack([synth.itones(p) for p in pays]))
    wav = synth.gfsk_waveforms(tones, FS, torch.as_tensor(f0))
    wav *= torch.as_tensor(np.sqrt(2.0 * 10.0 ** (level / 10.0)))[:, None]
    x = noise[0].to(torch.float64)
    for i, s in enumerate(start):
        lo, hi = max(int(s), 0), min(int(s) + L, N)
        x[lo:hi] += wav[i, lo - int(s):hi - int(s)]
    # the noise and the signals slot 8's list leaves out: what a complete subtraction of that list leaves
    rest = noise[0].to(torch.float64)
    for i in (SLOT8_LEFT_OUT if name == "B" else ()):
        rest[int(start[i]):int(start[i]) + L] += wav[i]
    out = {"x": x.to(torch.float32).numpy(), "noise": noise[0].numpy(), "rest8": rest.numpy(), "payloads": tuple(pays),
           "f0": f0, "level_db": level, "start": start}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _rec(r, i, slot, ok=1, dt=0, df=0):
    """The ft8_result of signal i of row r at the grid point nearest it, moved by (dt, df) points."""
    q = np.zeros((), dtype=RESULT_DTYPE)
    q["payload"] = np.frombuffer(r["payloads"][i], dtype=np.uint8)
    q["abs_time"] = int(np.rint(r["start"][i] / HOP)) - T_LO + dt
    q["abs_freq"] = int(np.rint(r["f0"][i] * NFFT / FS)) - F_LO + df
    q["slot"], q["ok"], q["score"] = slot, ok, 10.0 + i
    return q


def _shuffled(r, slot, signals, n_dup, rng):
    """Every signal's failed row, good row and n_dup good duplicates, in that order per signal, the
    signals' rows shuffled among each other -> (rows, indices of the good rows)."""
    labels = np.repeat(np.asarray(signals), 2 + n_dup)
    rng.shuffle(labels)
    seen, rows, kept = {}, [], []
    for j, i in enumerate(labels):
        v = seen.get(int(i), 0)
        seen[int(i)] = v + 1
        if v == 0:
            rows.append(_rec(r, i, slot, ok=0, dt=-1))
        elif v == 1:
            rows.append(_rec(r, i, slot))
            kept.append(j)
        elif n_dup == 2:
            rows.append(_rec(r, i, slot, dt=1) if v == 2 else _rec(r, i, slot, df=1))
        else:
            rows.append(_rec(r, i, slot, dt=1) if i % 2 == 0 else _rec(r, i, slot, df=1))
    return rows, kept


@functools.lru_cache(maxsize=None)
def batch():
    """-> (samples float32 [9, N], records [9, CAP] of RESULT_DTYPE, counts int32 [9], truth): truth
    holds per slot the row's name, the indices of the records a correct list keeps (kept) and the
    signal each of those carries (signal)."""
    rng = np.random.default_rng(LIST_SEED)
    A, B = row("A"), row("B")
    lists, kept, signal = [], [], []

    def plain(r, slot, sigs):
        return [_rec(r, i, slot) for i in sigs], list(range(len(sigs))), list(sigs)

    for slot in range(N_SLOTS):
        r = A if ROW_OF_SLOT[slot] == "A" else B
        n_sig = len(r["payloads"])
        if slot == 0:
            rows, kp = _shuffled(r, slot, range(n_sig), 1, rng)
            sg = None
        elif slot == 8:
            rows, kp = _shuffled(r, slot, [i for i in range(n_sig) if i not in SLOT8_LEFT_OUT], 2, rng)
            sg = None
        elif slot in (2, 3):
            rows, kp, sg = plain(r, slot, [int(i) for i in rng.permutation(n_sig)[:FITS_PER_SLOT[slot]]])
        elif slot == 5:
            rows, kp, sg = plain(r, slot, [7])
        elif slot == 6:
            rows, kp, sg = plain(r, slot, [ROWS["A"]["head"], 40])
        elif slot == 7:
            a, b, c = 12, ROWS["B"]["tail"], 31
            rows = [_rec(r, a, slot, ok=0, dt=-1), _rec(r, a, slot), _rec(r, b, slot), _rec(r, a, slot, df=1),
                    _rec(r, c, slot)]
            kp, sg = [1, 2, 4], [a, b, c]
        else:
            rows, kp, sg = [], [], []
        if sg is None:
            by_pay = {p: i for i, p in enumerate(r["payloads"])}
            sg = [by_pay[bytes(rows[j]["payload"])] for j in kp]
        lists.append(rows)
        kept.append(kp)
        signal.append(sg)
    records = np.zeros((N_SLOTS, CAP), dtype=RESULT_DTYPE)
    counts = np.zeros(N_SLOTS, dtype=np.int32)
    for slot, rows in enumerate(lists):
        assert len(rows) <= CAP
        counts[slot] = len(rows)
        for j, q in enumerate(rows):
            records[slot, j] = q
            records[slot, j]["cand_index"] = j
        # past the count: good records of signals the list leaves out
        r = A if ROW_OF_SLOT[slot] == "A" else B
        spare = [i for i in range(len(r["payloads"])) if i not in signal[slot]]
        for j in range(len(rows), CAP):
            if spare:
                records[slot, j] = _rec(r, spare[(j - len(rows)) % len(spare)], slot)
    counts[8] = CAP + 5
    samples = np.stack([(A if c == "A" else B)["x"] for c in ROW_OF_SLOT])
    for v in (samples, records, counts):
        v.setflags(write=False)
    truth = {"row": tuple(ROW_OF_SLOT), "kept": tuple(tuple(k) for k in kept),
             "signal": tuple(tuple(s) for s in signal)}
    return samples, records, counts, truth


@functools.lru_cache(maxsize=None)
def pcm():
    """The batch's samples as int16 PCM (x / 8 of full scale, the scaling of the slot-edge test)."""
    p = np.clip(np.round(batch()[0] / 8.0 * 32767.0), -32767, 32767).astype(np.int16)
    p.setflags(write=False)
    return p


def host_samples(key):
    """What the oracle reads for "f32" (the samples) or "i16" (pcm / 32767) -> float [9, N]."""
    return batch()[0] if key == "f32" else pcm().astype(np.float64) / 32767.0


_FIT_CACHE = {}


@functools.lru_cache(maxsize=None)
def oracle_fits(key, slot):
    """oracle/subtract.py's fits of one slot's list: one entry per record below min(count, cap), None
    for a record it does not fit.  Slots of one row share the fit of a record they share."""
    from oracle import subtract as OS
    _, records, counts, _ = batch()
    cache = _FIT_CACHE.setdefault((key, ROW_OF_SLOT[slot]), {})
    return tuple(OS.fits(host_samples(key)[slot], records[slot, :min(int(counts[slot]), CAP)], FS, NSPS, HOP, NFFT,
                         T_LO, F_LO, cache=cache))


@functools.lru_cache(maxsize=None)
def oracle_residual(key, slot):
    """oracle/subtract.py's residual of one slot for its own fits (float64 [N])."""
    from oracle import subtract as OS
    r = OS.residual(host_samples(key)[slot], oracle_fits(key, slot), NSPS, FS)
    r.setflags(write=False)
    return r


def check_fits(gfit, ofit):
    """Every device fit of one slot (ft8_sub_fit rows) against the oracle's fit of the same record:
    tones equal, start within +-1 sample, tone-0 frequency within 1e-3 Hz, the per-symbol amplitudes
    within 2e-3 of the largest where the starts agree -> (fits compared, fits whose start is off by one)."""
    n_fits = n_start_off = 0
    for j, of in enumerate(ofit):
        g = gfit[j]
        assert int(g["active"]) == (of is not None), j
        if of is None:
            continue
        n_fits += 1
        assert list(g["tones"][:79]) == list(of["tones"])
        assert abs(int(g["start"]) - of["start"]) <= 1, (j, int(g["start"]), of["start"])
        assert abs(float(g["f0"]) - of["f0"]) <= 1e-3, (j, float(g["f0"]), of["f0"])
        if int(g["start"]) == of["start"]:
            ga = g["amp"][:, 0] + 1j * g["amp"][:, 1]
            assert np.max(np.abs(ga - of["amp"])) <= 2e-3 * np.max(np.abs(of["amp"])), j
        else:
            n_start_off += 1
    return n_fits, n_start_off
