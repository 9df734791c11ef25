"""FT4: the protocol's constants, its transmit chain in PyTorch / NumPy and NumPy restatements of the
device's FT4 receive stages (ft8hip.h, "FT4").

FT4 is build-defined here: the reference decodes FT8 only, and no vector of another FT4 implementation
was available to the build, so interoperability with WSJT-X is NOT verified.  This module is the
definition the device is pinned to, as coherent.py and osd.py are for their passes:

  symbol      T = 0.048 s, nsps = fs * 6 / 125 samples (an integer: fs = 12000 gives 576), tone spacing
              fs / nsps (20.8333 Hz), 4-FSK, modulation index 1
  frame       103 symbols S4 D29 S4 D29 S4 D29 S4: sync groups at symbols 0, 33, 66, 99 with the tones
              FT4_COSTAS[m]; data symbol k (0 .. 86) at FT4_DATA_SYMBOL[k]; two bits per symbol, MSB
              first, Gray map FT4_GRAY
  scrambling  the 77 message bits are XORed with FT4_RVEC before CRC-14 and LDPC(174,91); the receiver
              XORs the decoded 77 bits again
  waveform    105 symbols (ramp-up, the 103, ramp-down), GFSK with BT = 1.0, no extension pulses
"""
from __future__ import annotations

import math

import numpy as np

from . import _lib, synth

FT4_SYMBOLS = 103
FT4_DATA_SYMBOLS = 87
FT4_SYMBOL_TIME_S = 0.048
FT4_BT = 1.0
FT4_COSTAS = ((0, 1, 3, 2), (1, 0, 2, 3), (2, 3, 1, 0), (3, 2, 0, 1))
FT4_SYNC_START = (0, 33, 66, 99)
FT4_GRAY = (0, 1, 3, 2)
FT4_RVEC = bytes.fromhex("4a5e89b4b08a7955be28")     # 77 bits, MSB first
FT4_DATA_SYMBOL = tuple(k + (4 if k < 29 else 8 if k < 58 else 12) for k in range(FT4_DATA_SYMBOLS))
PROTOCOLS = {"ft8": 0, "ft4": 1}


def protocol_code(protocol) -> int:
    """"ft8" / "ft4" (or 0 / 1) -> FT8_PROTO_*; ValueError for anything else."""
    if isinstance(protocol, str) and protocol.lower() in PROTOCOLS:
        return PROTOCOLS[protocol.lower()]
    if protocol in (0, 1) and not isinstance(protocol, bool):
        return int(protocol)
    raise ValueError(f"protocol must be 'ft8' or 'ft4', got {protocol!r}")


def ft4_nsps(fs) -> int:
    """Samples per FT4 symbol; ValueError where fs * 6 / 125 is no integer (44 100 Hz)."""
    v = float(fs) * 6.0 / 125.0
    if not (v >= 1.0 and v == int(v)):
        raise ValueError(f"FT4 needs fs * 6 / 125 to be an integer number of samples, got fs = {fs!r}")
    return int(v)


def ft4_geometry(fs, bins_per_tone, steps_per_symbol, n_samples):
    """(nperseg, hop, nfft, frames) of the FT4 STFT: nperseg = nsps, the reference's noverlap rule,
    nfft = nsps * bins_per_tone (ft8_geometry_proto on the host)."""
    nsps = ft4_nsps(fs)
    noverlap = nsps - nsps // int(steps_per_symbol)
    if noverlap >= nsps:
        noverlap = nsps - 1
    hop = nsps - noverlap
    frames = 0 if n_samples < nsps else (int(n_samples) - noverlap) // hop
    return nsps, hop, nsps * int(bins_per_tone), frames


def ft4_scramble(payload) -> bytes:
    """payload ^ rvec on the 77 message bits (its own inverse); the low 3 bits of byte 9 stay."""
    p = np.frombuffer(bytes(payload)[:10], dtype=np.uint8)
    return (p ^ np.frombuffer(FT4_RVEC, dtype=np.uint8)).tobytes()


def ft4_codeword_bits(payload) -> np.ndarray:
    """174 codeword bits of the scrambled payload (CRC-14 and parity are over the scrambled bits)."""
    return synth.codeword_bits(ft4_scramble(payload))


def ft4_itones(payload) -> np.ndarray:
    """103 channel symbols of a 10-byte payload."""
    bits = ft4_codeword_bits(payload)
    tones = np.zeros(FT4_SYMBOLS, dtype=np.uint8)
    for m, s0 in enumerate(FT4_SYNC_START):
        tones[s0:s0 + 4] = FT4_COSTAS[m]
    for k, sym in enumerate(FT4_DATA_SYMBOL):
        tones[sym] = FT4_GRAY[(int(bits[2 * k]) << 1) | int(bits[2 * k + 1])]
    return tones


def ft4_envelope(nsps: int) -> np.ndarray:
    """The amplitude of the 105-symbol waveform: a raised cosine over the first symbol, its mirror over
    the last, 1 between."""
    env = np.ones(105 * nsps)
    r = 0.5 * (1.0 - np.cos(np.pi * np.arange(nsps) / nsps))
    env[:nsps] = r
    env[-nsps:] = r[::-1]
    return env


def ft4_waveforms(tones, fs, f0):
    """tones [B, 103], f0 [B] Hz (tone 0) -> real unit-amplitude waveforms [B, 105 * nsps], float64 torch
    on the CPU.  Sample nsps of a row is the first sample of symbol 0 (ft8_tx_signal.start)."""
    import torch
    tones = torch.as_tensor(np.asarray(tones)).reshape(-1, FT4_SYMBOLS).to(torch.float64)
    B = tones.shape[0]
    nsps = ft4_nsps(fs)
    seg = synth._pulse(nsps, bt=FT4_BT).reshape(3, nsps)
    # block b of the waveform (b = 0 the ramp-up symbol) sums the pulses of symbols b, b - 1, b - 2
    blocks = torch.zeros(B, 105, nsps, dtype=torch.float64)
    for s in range(3):
        blocks[:, s:s + FT4_SYMBOLS] += tones[:, :, None] * seg[s][None, None, :]
    spacing = float(fs) / nsps
    f0 = torch.as_tensor(np.asarray(f0, dtype=np.float64)).reshape(B)
    dphi = (2.0 * math.pi / fs) * (spacing * blocks.reshape(B, -1) + f0[:, None])
    phi = torch.cat([torch.zeros(B, 1, dtype=torch.float64), torch.cumsum(dphi[:, :-1], 1)], 1)
    sig = torch.sin(torch.remainder(phi, 2.0 * math.pi))
    return sig * torch.from_numpy(ft4_envelope(nsps))[None, :]


def make_slots_ft4(n_slots, n_signals, fs=12000, snr_db=(-16.0, -6.0), f0_range=(300.0, 2700.0),
                   start_range=(0.3, 1.2), seed=0, slot_s=7.5, noise=True, payloads=None):
    """synth.make_slots for FT4 on the CPU: -> (samples float32 [n_slots, int(slot_s * fs)], list of
    synth.SlotTruth).  start_s is the time of symbol 0's first sample; the SNR convention is the
    project's (signal power over unit-variance noise in the full band).  payloads: a list of 10-byte
    payloads every slot carries instead of random ones (n_signals of them)."""
    import torch
    N = int(slot_s * fs)
    nsps = ft4_nsps(fs)
    out = torch.empty(n_slots, N, dtype=torch.float32)
    truths = []
    for b in range(n_slots):
        rng = np.random.default_rng(seed + b)
        pays = list(payloads) if payloads is not None else [synth.random_payload(rng) for _ in range(n_signals)]
        lo, hi = (snr_db, snr_db) if np.isscalar(snr_db) else (snr_db if len(snr_db) == 2 else (None, None))
        if lo is None:
            snr = np.asarray(snr_db, dtype=np.float64)
        else:
            snr = rng.uniform(lo, hi, n_signals) if n_signals else np.zeros(0)
        # one signal per lane of the band (in shuffled order, jittered over the lane's first 30 %), so no
        # two signals of a slot overlap in frequency: a signal is 4 tone spacings (83 Hz) wide
        lane = (f0_range[1] - f0_range[0]) / max(n_signals, 1)
        f0 = (f0_range[0] + (rng.permutation(n_signals) + 0.3 * rng.uniform(0.0, 1.0, n_signals)) * lane
              if n_signals else np.zeros(0))
        st = rng.uniform(*start_range, n_signals) if n_signals else np.zeros(0)
        g = torch.Generator()
        g.manual_seed(seed + b)
        acc = torch.randn(N, generator=g, dtype=torch.float64) if noise else torch.zeros(N, dtype=torch.float64)
        if n_signals:
            wav = ft4_waveforms(np.stack([ft4_itones(p) for p in pays]), fs, f0)
            wav *= torch.as_tensor(np.sqrt(2.0 * 10.0 ** (snr / 10.0)))[:, None]
            for i in range(n_signals):
                s0 = int(st[i] * fs) - nsps      # the ramp-up symbol comes first
                a, e = max(s0, 0), min(s0 + wav.shape[1], N)
                if e > a:
                    acc[a:e] += wav[i, a - s0:e - s0]
        out[b] = acc.to(torch.float32)
        truths.append(synth.SlotTruth(pays, list(f0), list(st), list(snr)))
    return out, truths


# ---- restatements of the device's FT4 stages ---------------------------------------------------------
def ft4_stft_restate(x, fs, bins_per_tone=2, steps_per_symbol=2, dtype=np.float64):
    """The FT4 dB waterfall [frames, nfft // 2 ... ] in NumPy: periodic Hann of nsps samples, hop
    nsps / sps, nfft = nsps * bpt, |X|^2 / (sum w)^2, 10 log10(1e-12 + .); time-major, the bins
    [0, (nfft + 1) // 2) that make_plan keeps."""
    x = np.asarray(x, dtype=dtype)
    nsps, hop, nfft, frames = ft4_geometry(fs, bins_per_tone, steps_per_symbol, len(x))
    w = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(nsps) / nsps)).astype(dtype)
    idx = np.arange(frames)[:, None] * hop + np.arange(nsps)[None, :]
    spec = np.fft.fft(x[idx] * w[None, :], n=nfft, axis=1)[:, :(nfft + 1) // 2]
    p = (spec.real.astype(np.float64) ** 2 + spec.imag.astype(np.float64) ** 2) / float(w.sum()) ** 2
    return (10.0 * np.log10(1e-12 + p)).astype(dtype)


def ft4_grid_shape(T, F, sps, bpt):
    """(t0, NT, NF) of the FT4 search grid: abs_time in [-10 sps, (T // sps - 83) sps), abs_freq in
    [0, F - 3 bpt)."""
    t0 = -10 * sps
    return t0, max((T // sps - 83) * sps - t0, 0), max(F - 3 * bpt, 0)


def ft4_score_grid_restate(wf, sps, bpt) -> np.ndarray:
    """The FT4 sync score of every grid point, [NT, NF] in the waterfall's dtype (wf [T, F], time-major).
    ft8_sync_score with the FT4 layout: m = 0 .. 3 outer, k = 0 .. 3 inner, block = 33 m + k, the terms
    tone - 1, tone + 1, time - 1, time + 1 added one after another in the waterfall's dtype."""
    wf = np.asarray(wf)
    T, F = wf.shape
    dt = wf.dtype.type
    nb = T // sps
    t0, NT, NF = ft4_grid_shape(T, F, sps, bpt)
    score = np.zeros((NT, NF), dtype=wf.dtype)
    cnt = np.zeros(NT, dtype=np.int64)
    if NT == 0 or NF == 0:
        return score
    at = t0 + np.arange(NT)
    base = at // sps
    col = np.arange(NF)
    with np.errstate(all="ignore"):
        for m in range(4):
            for k in range(4):
                block = 33 * m + k
                tone = FT4_COSTAS[m][k]
                ba = base + block
                inside = (ba >= 0) & (ba < nb)
                terms = []
                if tone > 0:
                    terms.append((inside, 0, -bpt))
                if tone < 3:
                    terms.append((inside, 0, bpt))
                if k > 0:
                    terms.append((inside & (ba > 0), -sps, 0))
                if k < 3:
                    terms.append((inside & (ba + 1 < nb), sps, 0))
                for ok, drow, dcol in terms:
                    r = np.nonzero(ok)[0]
                    if r.size == 0:
                        continue
                    rows = at[r] + block * sps
                    c = col + tone * bpt
                    p = wf[rows[:, None], c[None, :]]
                    q = wf[(rows + drow)[:, None], (c + dcol)[None, :]]
                    score[r] = score[r] + (p - q)
                    cnt[r] += 1
        bad = (cnt[:, None] == 0) | ~np.isfinite(score)
        out = score / np.maximum(cnt, 1).astype(wf.dtype)[:, None]
    out[bad] = dt(-np.inf)
    return out


def _pymax(a, b):
    return b if b > a else a    # Python's max(a, b): the first maximum under '>'


def ft4_normalize(llr) -> np.ndarray:
    """ftx_normalize_logl: x * sqrt(24 / var(x)) over the 174 values, NumPy's pairwise sums."""
    x = np.array(llr, dtype=np.float64, copy=True)
    with np.errstate(all="ignore"):
        mean = np.add.reduce(x) / 174.0
        d = x - mean
        var = np.add.reduce(d * d) / 174.0
        return x * np.sqrt(np.float64(24.0) / var)


def ft4_llr_restate(wf, sps, bpt, abs_time, abs_freq, normalize=True) -> np.ndarray:
    """The 174 LLRs of one candidate from the waterfall wf [T, F]: per data symbol s[j] = the bin of tone
    FT4_GRAY[j] in double, L[2k] = max(s2, s3) - max(s0, s1), L[2k+1] = max(s1, s3) - max(s0, s2); zeros
    where the symbol's block lies outside the waterfall."""
    wf = np.asarray(wf)
    T, _ = wf.shape
    nb = T // sps
    L = np.zeros(174, dtype=np.float64)
    base = int(abs_time) // sps
    with np.errstate(all="ignore"):
        for k, sym in enumerate(FT4_DATA_SYMBOL):
            if not 0 <= base + sym < nb:
                continue
            row = int(abs_time) + sym * sps
            s = [float(wf[row, int(abs_freq) + FT4_GRAY[j] * bpt]) for j in range(4)]
            L[2 * k] = _pymax(s[2], s[3]) - _pymax(s[0], s[1])
            L[2 * k + 1] = _pymax(s[1], s[3]) - _pymax(s[0], s[2])
    return ft4_normalize(L) if normalize else L


def ft4_scramble_hyps(hyps):
    """The a-priori hypotheses [(mask, value)] in message bits -> the same in the scrambled domain."""
    return [(bytes(m), ft4_scramble(v)) for m, v in hyps]


def ft4_decode_restate(wf, sps, bpt, max_candidates, min_score, max_iterations, *, select, bp_decode,
                       decode_tail, cmp_f64=False, slot=0, hyps=None, ap_max_hard_errors=174, osd=None):
    """ft8_decode_batch's FT4 chain on one waterfall wf [T, F]: grid -> select -> LLR -> BP -> tail ->
    [a-priori pass] -> [OSD pass] -> descramble; -> (ok records in candidate order, _lib.RESULT_DTYPE, the
    LLRs [n, 174] of all candidates, all records before the descramble).
    select(scores, N, min_score, cmp_f64) -> (scan index, score[, tie]), bp_decode(llr, iters) ->
    (plain, errors), decode_tail(plain, errors) -> (ok, payload, crc_e, crc_c): the reference's (tests pass
    the oracle's).  hyps: a-priori hypotheses in message bits; osd: (order, max_per_slot, max_hard_errors)."""
    from . import ap as _ap
    from . import osd as _osd
    wf = np.asarray(wf)
    T, F = wf.shape
    t0, NT, NF = ft4_grid_shape(T, F, sps, bpt)
    rec = np.zeros(0, dtype=_lib.RESULT_DTYPE)
    if NT == 0 or NF == 0 or max_candidates <= 0:
        return rec, np.zeros((0, 174)), rec
    grid = ft4_score_grid_restate(wf, sps, bpt)
    idx, sc = select(grid, max_candidates, min_score, cmp_f64)[:2]
    n = len(idx)
    rec = np.zeros(n, dtype=_lib.RESULT_DTYPE)
    llrs = np.zeros((n, 174))
    for c in range(n):
        at, af = int(idx[c] // NF) + t0, int(idx[c] % NF)
        llrs[c] = ft4_llr_restate(wf, sps, bpt, at, af)
        with np.errstate(all="ignore"):
            plain, err = bp_decode(llrs[c], max_iterations)
        ok, payload, ce, cc = decode_tail(plain, err)
        rec[c] = (float(sc[c]), slot, at, af, ce, cc, err, c, np.frombuffer(bytes(payload), dtype=np.uint8),
                  int(ok), 0)
    if hyps:
        rec, _ = _ap.ap_restate(llrs, rec, ft4_scramble_hyps(hyps), max_iterations, ap_max_hard_errors,
                                bp_decode, decode_tail)
    if osd is not None:
        order, cap, max_hard = osd
        failed = np.nonzero(rec["ok"] == 0)[0]
        if cap > 0:
            failed = failed[:cap]
        if failed.size:
            got, _, _ = _osd.osd_pass_restate(llrs[failed], rec[failed], order, max_hard, decode_tail)
            rec[failed] = got
    out = rec[rec["ok"] == 1].copy()
    rv = np.frombuffer(FT4_RVEC, dtype=np.uint8)
    out["payload"] ^= rv[None, :]
    return out, llrs, rec


def decode_ft4_message(wave_data, sample_rate=12000, bins_per_tone=2, steps_per_symbol=2, max_candidates=20,
                       min_score=10, max_iterations=20, freq_min=None, freq_max=None, time_min=None,
                       time_max=None, **kwargs):
    """decode_ft8_message for FT4: one slot of samples -> [(FT8Message, FT8DecodeStatus, time_sec, freq_hz,
    score)], the payloads descrambled.  time_sec is the start of symbol 0 (abs_time hops), freq_hz the
    frequency of tone 0 (abs_freq / bins_per_tone tone spacings)."""
    from ._pipeline import SlotDecoder, device_samples, records_to_results
    x, code, f64 = device_samples(wave_data)
    if x.dim() != 1:
        raise ValueError("wave_data must be one-dimensional")
    dec = SlotDecoder(sample_rate=sample_rate, bins_per_tone=bins_per_tone, steps_per_symbol=steps_per_symbol,
                      max_candidates=max_candidates, min_score=min_score, max_iterations=max_iterations,
                      freq_min=freq_min, freq_max=freq_max, time_min=time_min, time_max=time_max, protocol="ft4",
                      **kwargs)
    recs = dec.records(x, code)[0]
    plan = dec.plan(int(x.shape[0]))
    return records_to_results(recs, sample_rate, bins_per_tone, f64, protocol="ft4", plan=plan)
