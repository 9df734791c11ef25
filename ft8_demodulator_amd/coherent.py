"""Coherent re-demodulation of a candidate from the samples: the contract of include/ft8hip.h
("coherent re-demodulation", ft8_coherent_llr / FT8_FLAG_COHERENT) restated in NumPy, in float64.

A candidate that belief propagation fails on is demodulated again from the slot's samples instead of
the Hann STFT's dB bins: mixed down and box-car decimated to Q samples per symbol, fine-synchronised
on the 21 Costas symbols (start offsets of D samples, tone-0 offsets of a quarter bin), and its LLRs
formed from matched rectangular symbol windows at the refined point; with nsym > 1 further LLR vectors
come from joint metrics over 2 and 3 adjacent symbols (the header's step 4b).  The device runs it
(csrc/coherent.hip); this module restates it for tests and tools.  Nothing here runs on the decode
path.
"""
from __future__ import annotations

import numpy as np

TONE_HZ = 6.25
COSTAS = (3, 1, 4, 0, 6, 5, 2)
GRAY = (0, 1, 3, 2, 5, 6, 4, 7)   # FT8_Gray_map: s2[j] = s[GRAY[j]] (ft8_extract_symbol)
SYNC_SYMBOLS = tuple(b + i for b in (0, 36, 72) for i in range(7))
SYNC_TONES = COSTAS * 3
DATA_SYMBOLS = tuple(range(7, 36)) + tuple(range(43, 72))
N_DF = 5                           # tone-0 offsets: (j - 2) bin / 4, j = 0 .. 4
DEFAULT_MAX_PER_SLOT = 32          # SlotDecoder(coherent=True)

# ft8_coh_fit (16 bytes)
FIT_DTYPE = np.dtype({
    "names": ["dt_s", "df_hz", "metric", "n_sync", "status", "dt_index", "df_index"],
    "formats": ["<f4", "<f4", "<f4", "u1", "u1", "i1", "u1"],
    "offsets": [0, 4, 8, 12, 13, 14, 15],
    "itemsize": 16,
})
STATUS_VALID, STATUS_NOTHING, STATUS_NOT_ATTEMPTED = 0, 2, 3

# ft8_coh_drift (8 bytes): the winning rate of the drift search
DRIFT_DTYPE = np.dtype([("rate_hz_per_s", "<f4"), ("rate_index", "<i4")])
MAX_DRIFT_RATES, MAX_DRIFT_HZ_PER_S = 33, 4.0
DEFAULT_DRIFT = (1.0, 9)           # SlotDecoder(coherent_drift=True)
MAX_NSYM = 3                       # ft8_set_coherent_nsym: joint metrics over up to 3 symbols


def sub_q(nsps: int) -> int:
    """Decimated samples per symbol: the largest divisor of nsps in [8, 32], 0 when there is none."""
    for q in range(32, 7, -1):
        if nsps % q == 0:
            return q
    return 0


def geometry(nperseg: int, steps_per_symbol: int):
    """-> (hop, Q, D, Mt, Mg); ValueError where the pass is unsupported (no Q, or hop does not divide nsps)."""
    nsps, sps = int(nperseg), int(steps_per_symbol)
    Q = sub_q(nsps)
    if Q == 0 or sps <= 0 or nsps % sps != 0:
        raise ValueError("coherent re-demodulation needs nsps with a divisor in [8, 32] and hop | nsps")
    hop, D = nsps // sps, nsps // Q
    Mt = -((-hop) // (2 * D))      # ceil((hop / 2) / D)
    return hop, Q, D, Mt, Mt + 1


def coherent_index(record) -> int:
    """1 when the coherent pass produced the record's decode (pass_index bit 1), else 0."""
    return (int(record["pass_index"]) >> 1) & 1


def drift_index(record) -> int:
    """1 when the record was rescued at a drift rate other than 0 (pass_index bit 2), else 0."""
    return (int(record["pass_index"]) >> 2) & 1


def multisymbol_index(record) -> int:
    """1 when the record was rescued by a joint metric over 2 or 3 symbols (pass_index bit 3), else 0."""
    return (int(record["pass_index"]) >> 3) & 1


def check_nsym(nsym) -> int:
    """max_nsym as ft8_set_coherent_nsym takes it; ValueError for what it answers with FT8_E_ARG."""
    S = int(nsym)
    if S != nsym or S < 1 or S > MAX_NSYM:
        raise ValueError(f"coherent nsym: max_nsym must be in [1, {MAX_NSYM}]")
    return S


def symbol_groups(n: int):
    """The groups of step 4b for n symbols per group: each half (symbols 7 .. 35, 43 .. 71) cut in order
    into groups of n with a shorter last group -> list of tuples of symbol indices."""
    out = []
    for lo in (7, 43):
        half = list(range(lo, lo + 29))
        out += [tuple(half[i:i + n]) for i in range(0, 29, n)]
    return out


def _joint_llr(cp: np.ndarray, n: int) -> np.ndarray:
    """cp [79, 8] rotated correlations (zeros for absent symbols) -> the 174 joint LLRs of set n before
    the normalisation (step 4b, items 3 and 4)."""
    L = np.zeros((79, 3), dtype=np.float64)
    g2 = cp[:, GRAY]                       # g2[k, j]: the tone that carries the bits of j
    zero = np.zeros(1, dtype=np.complex128)
    for grp in symbol_groups(n):
        a, b, c = [g2[k] for k in grp] + [zero] * (3 - len(grp))
        s = 10.0 * np.log10(1e-12 + np.abs(a[:, None, None] + b[None, :, None] + c[None, None, :]) ** 2)
        for i, k in enumerate(grp):
            m = np.moveaxis(s, i, 0).reshape(8, -1).max(axis=1)     # best tuple per value of a_i
            L[k] = (m[[4, 5, 6, 7]].max() - m[[0, 1, 2, 3]].max(),
                    m[[2, 3, 6, 7]].max() - m[[0, 1, 4, 5]].max(),
                    m[[1, 3, 5, 7]].max() - m[[0, 2, 4, 6]].max())
    return L[list(DATA_SYMBOLS)].reshape(174)


def drift_rates(max_rate, n_rates) -> np.ndarray:
    """The rates r_i = (i - (R - 1) / 2) * 2 A / (R - 1) of the drift search in Hz/s, float64 [R], A being
    max_rate as the float32 the C-ABI takes ([0.0] where the search is off: R = 1 or A = 0).  ValueError
    for what ft8_set_coherent_drift answers with FT8_E_ARG: R even or outside [1, 33], A outside [0, 4]."""
    R, A = int(n_rates), float(np.float32(max_rate))
    if R != n_rates or R < 1 or R > MAX_DRIFT_RATES or R % 2 == 0:
        raise ValueError(f"coherent drift: n_rates must be odd and in [1, {MAX_DRIFT_RATES}]")
    if not 0.0 <= A <= MAX_DRIFT_HZ_PER_S:
        raise ValueError(f"coherent drift: max_rate must be in [0, {MAX_DRIFT_HZ_PER_S:g}] Hz/s")
    if R == 1 or A == 0.0:
        return np.zeros(1)
    return (np.arange(R) - (R - 1) // 2).astype(np.float64) * (2.0 * A / (R - 1))


def _as_float64(x: np.ndarray) -> np.ndarray:
    x = np.asarray(x)
    if x.dtype == np.int16:
        return (x.astype(np.float32) / np.float32(32767.0)).astype(np.float64)   # as the STFT scales PCM
    if x.dtype != np.float32:
        raise NotImplementedError("coherent re-demodulation takes float32 or int16 samples")
    return x.astype(np.float64)


def _llr_of_spectra(s: np.ndarray) -> np.ndarray:
    """s [58, 8] dB by tone -> [58, 3] max-of-4 differences after the Gray map (ft8_extract_symbol)."""
    s2 = s[:, GRAY]
    return np.stack([
        s2[:, [4, 5, 6, 7]].max(1) - s2[:, [0, 1, 2, 3]].max(1),
        s2[:, [2, 3, 6, 7]].max(1) - s2[:, [0, 1, 4, 5]].max(1),
        s2[:, [1, 3, 5, 7]].max(1) - s2[:, [0, 2, 4, 6]].max(1)], axis=1)


def coherent_restate(samples, cand, slot_of, fs, nperseg, nfft, steps_per_symbol, t_lo=0, f_lo=0, details=False,
                     drift=None, nsym=1):
    """samples [n_slots, n_samples] (float32, or int16 PCM), cand [n, 2] = (abs_time, abs_freq), slot_of [n]
    -> (llr float64 [n, 174], fits FIT_DTYPE [n]); with details also the list of every candidate's
    metric grid [2 Mt + 1, 5] (None where no sync symbol was present).
    drift = (max_rate, n_rates): the search over linear drift rates (drift_rates; the header's step 1b)
    -> (llr, fits, drifts DRIFT_DTYPE [n]) and with details the metric volumes [R, 2 Mt + 1, 5].
    nsym = S > 1: the joint metrics over 2 .. S symbols (the header's step 4b): llr is [n, S, 174], set 1
    computed as without nsym, and a `valid` uint8 [n] follows the fits (and drifts): bit s - 1 for a valid set
    s; with details the list of every candidate's rotated correlations c' [79, 8] (None where none were
    formed) comes last."""
    S = check_nsym(nsym)
    rates = None if drift is None else drift_rates(*drift)
    x_all = np.asarray(samples)
    if x_all.ndim == 1:
        x_all = x_all[None, :]
    n_slots, n_samples = x_all.shape
    cand = np.asarray(cand, dtype=np.int64).reshape(-1, 2)
    slot_of = np.asarray(slot_of, dtype=np.int64).reshape(-1)
    n = len(cand)
    hop, Q, D, Mt, Mg = geometry(nperseg, steps_per_symbol)
    fs = float(fs)
    binw = fs / float(nfft)
    Mz = 79 * Q + 2 * Mg
    dts = np.arange(-Mt, Mt + 1)
    q = np.arange(Q)
    # window index of (dt, symbol, q) into z, and its first input sample relative to nb
    widx = Mg + dts[:, None, None] + np.arange(79)[None, :, None] * Q + q[None, None, :]
    sync_k, data_k = np.array(SYNC_SYMBOLS), np.array(DATA_SYMBOLS)
    df_grid = (np.arange(N_DF) - 2) * binw / 4.0
    sync_nu = np.array(SYNC_TONES, dtype=np.float64)[None, :] - 3.5 + df_grid[:, None] / TONE_HZ    # [5, 21]
    R = np.exp(-2j * np.pi * sync_nu[:, :, None] * q[None, None, :] / Q)                             # [5, 21, Q]

    llr = np.zeros((n, 174), dtype=np.float64)
    fits = np.zeros(n, dtype=FIT_DTYPE)
    drifts = np.zeros(n, dtype=DRIFT_DTYPE)
    llr_n = np.zeros((n, S, 174), dtype=np.float64)
    valid = np.zeros(n, dtype=np.uint8)
    rotated = [None] * n
    # centre of decimation block m relative to the centre of the nominal signal, squared
    tau2 = (((np.arange(Mz) - Mg + 0.5) * D - 39.5 * nperseg) / fs) ** 2
    grids = []
    cache = {}
    for i in range(n):
        grids.append(None)
        slot = int(slot_of[i])
        if not 0 <= slot < n_slots:
            fits["status"][i] = STATUS_NOT_ATTEMPTED
            continue
        if slot not in cache:
            cache[slot] = _as_float64(x_all[slot])
        x = cache[slot]
        s0 = (int(t_lo) + int(cand[i, 0])) * hop
        fmix = (int(f_lo) + int(cand[i, 1])) * binw + 3.5 * TONE_HZ
        nb = s0 - Mg * D
        # 1. baseband
        nidx = nb + np.arange(Mz * D, dtype=np.int64)
        inside = (nidx >= 0) & (nidx < n_samples)
        xw = np.where(inside, x[np.clip(nidx, 0, n_samples - 1)], 0.0)
        cyc = fmix * nidx.astype(np.float64) / fs
        z = (xw * np.exp(-2j * np.pi * (cyc - np.floor(cyc)))).reshape(Mz, D).sum(axis=1)
        # 2. presence of (dt, symbol)
        first = nb + (Mg + dts[:, None] + np.arange(79)[None, :] * Q) * D
        present = (first >= 0) & (first + Q * D <= n_samples)                                        # [nT, 79]
        if not present[:, sync_k].any():
            fits["status"][i] = STATUS_NOTHING
            continue
        # 3. sync on the Costas symbols
        if rates is not None and len(rates) > 1:
            # 1b. de-chirp by every rate; the first largest metric over (rate, dt, j) chooses z
            vol, zs = [], []
            for r in rates:
                cyc = 0.5 * r * tau2
                zs.append(z * np.exp(-2j * np.pi * (cyc - np.floor(cyc))))
                corr = np.einsum("dsq,jsq->djs", zs[-1][widx][:, sync_k], R)
                vol.append((np.abs(corr) ** 2 * present[:, None, sync_k]).sum(axis=2))
            vol = np.stack(vol)                                                                      # [R, nT, 5]
            ri = int(np.argmax(vol.reshape(-1))) // vol[0].size
            z, metric = zs[ri], vol[ri]
            drifts[i] = (rates[ri], ri)
            grids[-1] = vol
        W = z[widx]                                                                                  # [nT, 79, Q]
        if rates is None or len(rates) == 1:
            corr = np.einsum("dsq,jsq->djs", W[:, sync_k], R)
            metric = (np.abs(corr) ** 2 * present[:, None, sync_k]).sum(axis=2)                      # [nT, 5]
            grids[-1] = metric if rates is None else metric[None]
        best = int(np.argmax(metric.reshape(-1)))                                                    # the first largest
        di, j = divmod(best, N_DF)
        delta = 0.0
        if 0 < j < N_DF - 1:
            m_, m0, mp = metric[di, j - 1], metric[di, j], metric[di, j + 1]
            den = m_ - 2.0 * m0 + mp
            if den < 0.0:
                delta = 0.5 * (m_ - mp) / den
        df = (j - 2 + delta) * binw / 4.0
        f = fits[i]
        f["dt_s"], f["df_hz"], f["metric"] = dts[di] * D / fs, df, metric[di, j]
        f["n_sync"], f["dt_index"], f["df_index"] = int(present[di, sync_k].sum()), dts[di], j
        # 4. symbol spectra and LLRs
        E = np.exp(-2j * np.pi * (np.arange(8)[:, None] - 3.5 + df / TONE_HZ) * q[None, :] / Q)       # [8, Q]
        c = W[di, data_k] @ E.T                                                                      # [58, 8]
        s = 10.0 * np.log10(1e-12 + np.abs(c) ** 2)
        L = _llr_of_spectra(s) * present[di, data_k][:, None]
        L = L.reshape(174)
        var = np.mean((L - np.mean(L)) ** 2)
        if not var > 0.0:                                                                            # 0 or NaN
            f["status"] = STATUS_NOTHING
            continue
        llr[i] = L * np.sqrt(24.0 / var)
        f["status"] = STATUS_VALID
        if S == 1:
            continue
        # 4b. joint LLRs over groups of 2 .. S symbols from the phase-continued correlations
        llr_n[i, 0], valid[i] = llr[i], 1
        k79 = np.arange(79)
        cyc = (df / TONE_HZ - 3.5) * k79
        cp = (W[di] @ E.T) * present[di][:, None] * np.exp(-2j * np.pi * (cyc - np.floor(cyc)))[:, None]
        rotated[i] = cp
        for m in range(2, S + 1):
            Lm = _joint_llr(cp, m)
            var = np.mean((Lm - np.mean(Lm)) ** 2)
            if var > 0.0:
                llr_n[i, m - 1] = Lm * np.sqrt(24.0 / var)
                valid[i] |= 1 << (m - 1)
    out = (llr, fits) if S == 1 else (llr_n, fits)
    if rates is not None:
        out += (drifts,)
    if S > 1:
        out += (valid,)
    if details:
        out += (grids,)
        if S > 1:
            out += (rotated,)
    return out


def retry_list(records, cap=None):
    """The retry pass's list (k_retry_list without a gate; csrc/ft8_internal.h, RetryLists): records is a
    structured array with the ft8_result fields that holds every slot's candidates with slot and cand_index
    filled -> indices into records, int64: per slot, in slot order, the first `cap` (None: all) records with
    ok == 0, in cand_index order."""
    out = []
    for s in np.unique(records["slot"]):
        idx = np.nonzero((records["slot"] == s) & (records["ok"] == 0))[0]
        out += idx[np.argsort(records["cand_index"][idx], kind="stable")][:cap].tolist()
    return np.array(out, dtype=np.int64)


def coherent_pass_restate(records, listed, llr, fits, max_iterations, bp_decode, decode_tail, drifts=None, valid=None):
    """What the coherent pass of ft8_decode_batch does to the records, on the CPU: records as retry_list takes
    them, listed = retry_list(records, cap), and the stage call's results for the listed candidates -- llr
    [len(listed), 174] or [len(listed), S, 174], fits FIT_DTYPE, and where the pass ran with them drifts
    DRIFT_DTYPE and the validity bytes `valid` -> an updated copy of records.
    bp_decode(llr, iters) -> (plain, errors) and decode_tail(plain, errors) -> (ok, payload, crc_e, crc_c) are
    the reference's (tests pass the oracle's), as in ap.ap_restate.

    The pass decodes set after set over the lists and merges after each (coherent_pass, csrc/capi.hip); this
    walks the same attempts per list position.  k_coh_merge (csrc/coherent.hip) accepts the attempt of set s
    where the decode is ok and fits.status == 0, and with validity bytes only where bit s is set and the record
    is not ok yet, so the first valid set that decodes wins; a record that was ok before the pass is never
    listed and never touched.  retry_accept (csrc/ft8_internal.h) then writes ok, payload, crc_extracted,
    crc_calculated and ldpc_errors and ORs pass_index with 2, with 4 more where drifts.rate_hz_per_s != 0 and 8
    more for a set after the first; score, slot, abs_time, abs_freq and cand_index stay the record's."""
    out = np.array(records, copy=True)
    llr = np.asarray(llr, dtype=np.float64)
    if llr.ndim == 2:
        llr = llr[:, None, :]
    for pos, i in enumerate(listed):
        if out["ok"][i] or fits["status"][pos] != STATUS_VALID:
            continue
        for s in range(llr.shape[1]):
            if valid is not None and not (int(valid[pos]) >> s) & 1:
                continue
            plain, err = bp_decode(llr[pos, s], max_iterations)
            ok, payload, ce, cc = decode_tail(plain, err)
            if ok:
                out["ok"][i] = 1
                out["payload"][i] = np.frombuffer(bytes(payload), dtype=np.uint8)
                out["crc_extracted"][i], out["crc_calculated"][i], out["ldpc_errors"][i] = ce, cc, err
                drifted = drifts is not None and drifts["rate_hz_per_s"][pos] != 0
                out["pass_index"][i] |= 2 | (4 if drifted else 0) | (8 if s > 0 else 0)
                break
    return out


def coherent_ap_restate(records, listed, llr, fits, hyps, max_iterations, max_hard_errors, bp_decode, decode_tail,
                        drifts=None, valid=None):
    """The a-priori retries on the coherent LLRs (include/ft8hip.h, "coherent_ap"; ft8_set_coherent_ap), on the
    CPU: records as the coherent pass left them (coherent_pass_restate's result), listed, llr, fits, drifts and
    valid as that function takes them, hyps [(mask, value)] as ap.ap_hypothesis builds them -> (an updated copy
    of records, hard int16 indexed like records: the accepted attempt's hard errors, -1 elsewhere).
    bp_decode and decode_tail are the reference's, injected as in coherent_pass_restate and ap.ap_restate.

    A listed position is tried while its record is not ok and fits.status == 0.  Its sets n are those whose
    validity bit is set (every one without `valid`) and whose a_n = ap.ap_magnitude(L_n) is neither NaN nor 0.
    Attempts run hypothesis outer, set inner: BP and the tail on ap.ap_llr(L_n, mask, value), accepted by
    ap.ap_accept against the unclamped L_n.  The first accepted attempt writes ok, payload, crc_extracted,
    crc_calculated and ldpc_errors and ORs pass_index with 2 | (h + 1) << 4, with 4 more where
    drifts.rate_hz_per_s != 0 and 8 more for n > 0; later attempts of the position are not made."""
    from . import ap as _ap
    out = np.array(records, copy=True)
    hard_out = np.full(len(out), -1, dtype=np.int16)
    llr = np.asarray(llr, dtype=np.float64)
    if llr.ndim == 2:
        llr = llr[:, None, :]
    for pos, i in enumerate(listed):
        if out["ok"][i] or fits["status"][pos] != STATUS_VALID:
            continue
        sets = []
        for n in range(llr.shape[1]):
            if valid is not None and not (int(valid[pos]) >> n) & 1:
                continue
            a = _ap.ap_magnitude(llr[pos, n])
            if a == a and a != 0.0:
                sets.append(n)
        for h, n in ((h, n) for h in range(len(hyps)) for n in sets):
            mask, value = hyps[h]
            plain, err = bp_decode(_ap.ap_llr(llr[pos, n], mask, value), max_iterations)
            ok, payload, ce, cc = decode_tail(plain, err)
            good, hard = _ap.ap_accept(ok, payload, plain, llr[pos, n], mask, value, max_hard_errors)
            if good:
                out["ok"][i] = 1
                out["payload"][i] = np.frombuffer(bytes(payload), dtype=np.uint8)
                out["crc_extracted"][i], out["crc_calculated"][i], out["ldpc_errors"][i] = ce, cc, err
                drifted = drifts is not None and drifts["rate_hz_per_s"][pos] != 0
                out["pass_index"][i] |= 2 | ((h + 1) << 4) | (4 if drifted else 0) | (8 if n > 0 else 0)
                hard_out[i] = hard
                break
    return out, hard_out


def near_tie(metric, rel=1e-5) -> bool:
    """Whether a metric grid's two largest values differ by less than rel (relative to the largest)."""
    m = np.sort(np.asarray(metric, dtype=np.float64).reshape(-1))
    return bool(m[-1] - m[-2] < rel * m[-1])
