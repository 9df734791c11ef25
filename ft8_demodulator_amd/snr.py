"""The signal report of a decode: SNR in 2500 Hz from the dB waterfall (build-defined; the
reference stops at the payload).

snr_reference is the estimator restated in NumPy, step by step as include/ft8hip.h and DESIGN.md
state it; it needs neither a GPU nor the library and is what the device kernels (csrc/snr.hip:
k_noise_floor, k_snr) are tested against.  noise_floor and snr are thin wrappers over the two stage
calls ft8_noise_floor / ft8_snr for waterfalls that live on the GPU; SlotDecoder.snr / .reports
use ft8_snr_last on the waterfall the decode itself left on the device.

  P[t][f]  = 10^(wf[t][f] / 10)                                  (double throughout)
  A[f]     = mean_t P[t][f], added in the order t = 0 .. T-1
  N0       = A sorted ascending (NaNs last) [floor(q (F-1))]
  M(dt,df) = mean over the symbols k whose row lies in [0, T) of
             P[abs_time + dt + k sps][abs_freq + df + tone[k] bpt], added in the order of k
  S        = max M - N0 (first largest in scan order), raised to 1e-3 N0 when below it
  snr_db   = 10 log10(S / N0) + 10 log10(enbw_hz / 2500),  enbw_hz = 1.5 fs / nperseg
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib

SNR_REF_BW_HZ = 2500.0
DEFAULT_Q = 0.25
DEFAULT_RADIUS = 1


def bandwidth_db(sample_rate, nperseg=None) -> float:
    """10 log10(enbw_hz / 2500): enbw_hz = 1.5 fs / nperseg is the equivalent noise bandwidth of the
    periodic Hann window of calculate_spectrogram (scaling='spectrum'); nperseg = int(0.16 fs)."""
    fs = float(sample_rate)
    n = int(0.16 * fs) if nperseg is None else int(nperseg)
    return float(10.0 * np.log10(1.5 * fs / n / SNR_REF_BW_HZ))


def noise_floor_reference(wf, q=DEFAULT_Q):
    """wf [n_slots, T, F] (dB) -> (N0 [n_slots], A [n_slots, F]) in float64."""
    wf = np.asarray(wf)
    n_slots, T, F = wf.shape
    rank = int(np.floor(q * (F - 1)))
    A = np.zeros((n_slots, F), dtype=np.float64)
    with np.errstate(all="ignore"):
        for t in range(T):
            A += np.power(10.0, wf[:, t, :].astype(np.float64) / 10.0)
        A /= float(T)
    N0 = np.sort(A, axis=1)[:, rank]  # np.sort orders NaNs last
    return N0, A


def snr_reference(wf, records, counts=None, sample_rate=12000, bins_per_tone=2, steps_per_symbol=2, nperseg=None,
                  q=DEFAULT_Q, radius=DEFAULT_RADIUS, floor=None, details=False):
    """The reports of records [n_slots, cap] (_lib.RESULT_DTYPE) on wf [n_slots, T, F]: an
    _lib.SNR_DTYPE array [n_slots, cap].  counts None: every slot holds cap records.  floor: N0 per
    slot when it is already known (else noise_floor_reference(wf, q)).  details: also return, per
    record, the list of (dt, df, M) of the offsets that were not skipped, in scan order."""
    from .synth import itones
    wf = np.asarray(wf)
    n_slots, T, F = wf.shape
    records = np.asarray(records).reshape(n_slots, -1)
    cap = records.shape[1]
    N0 = noise_floor_reference(wf, q)[0] if floor is None else np.asarray(floor, dtype=np.float64)
    bw_db = bandwidth_db(sample_rate, nperseg)
    sps, bpt = int(steps_per_symbol), int(bins_per_tone)
    out = np.zeros((n_slots, cap), dtype=_lib.SNR_DTYPE)
    info = [[None] * cap for _ in range(n_slots)]
    for s in range(n_slots):
        n = cap if counts is None else min(max(int(counts[s]), 0), cap)
        for r in range(cap):
            rec = records[s, r]
            if r >= n or int(rec["ok"]) == 0:
                out[s, r]["status"] = 3
                continue
            tone = itones(bytes(rec["payload"])).astype(np.int64)
            at, af = int(rec["abs_time"]), int(rec["abs_freq"])
            best, cands = None, []
            for dt in range(-radius, radius + 1):
                for df in range(-radius, radius + 1):
                    f0 = af + df
                    if f0 < 0 or f0 + 7 * bpt > F - 1:
                        continue
                    total, cnt = 0.0, 0
                    with np.errstate(all="ignore"):
                        for k in range(79):
                            row = at + dt + k * sps
                            if row < 0 or row >= T:
                                continue
                            total += float(np.power(10.0, np.float64(wf[s, row, f0 + int(tone[k]) * bpt]) / 10.0))
                            cnt += 1
                    if cnt == 0:
                        continue
                    m = total / cnt
                    if m != m:
                        continue
                    cands.append((dt, df, m))
                    if best is None or m > best[2]:
                        best = (dt, df, m, cnt)
            info[s][r] = cands
            o = out[s, r]
            if best is None:
                o["status"] = 2
                continue
            n0 = float(N0[s])
            S = best[2] - n0
            if S < 1e-3 * n0:
                S = 1e-3 * n0
                o["status"] = 1
            with np.errstate(all="ignore"):
                o["snr_db"] = 10.0 * np.log10(np.float64(S) / np.float64(n0)) + bw_db
                o["signal_db"] = np.float32(10.0 * np.log10(np.float64(S)))
                o["noise_db"] = np.float32(10.0 * np.log10(np.float64(n0)))
            o["dt"], o["df"], o["n_symbols"] = best[0], best[1], best[3]
    return (out, info) if details else out


def snr_db_or_nan(reports) -> list:
    """ft8_snr_rec records -> one Python float each: snr_db, NaN where the report's status is 2 or 3
    (nothing was measured)."""
    return [float(r["snr_db"]) if int(r["status"]) < 2 else float("nan") for r in reports]


# ---- the stage calls, for waterfalls on the GPU ---------------------------------------------------------
def _wf3(wf):
    torch = _lib.require_gpu()
    if not isinstance(wf, torch.Tensor) or not wf.is_cuda:
        raise TypeError("wf must be a GPU tensor [n_slots, T, F] (use snr_reference on the host)")
    if wf.dim() == 2:
        wf = wf.unsqueeze(0)
    if wf.dim() != 3 or wf.dtype not in (torch.float32, torch.float64):
        raise ValueError("wf must be a float32 or float64 tensor [n_slots, T, F]")
    return torch, wf.contiguous()


def noise_floor(wf, q=DEFAULT_Q, context=None):
    """ft8_noise_floor on a GPU waterfall [n_slots, T, F] -> (N0 [n_slots], A [n_slots, F]), float64
    tensors, asynchronous on the current stream."""
    torch, wf = _wf3(wf)
    n_slots, T, F = (int(v) for v in wf.shape)
    ctx = context if context is not None else _lib.context(wf.device)
    n0 = torch.empty(max(n_slots, 1), dtype=torch.float64, device=wf.device)
    A = torch.empty((n_slots, F), dtype=torch.float64, device=wf.device)
    rc = _lib.lib().ft8_noise_floor(ctx.handle, _lib.ptr(wf), int(wf.dtype == torch.float64), n_slots, T, F, float(q),
                                    _lib.ptr(n0), _lib.ptr(A), _lib.stream_handle(wf.device))
    ctx.check(rc, "ft8_noise_floor")
    return n0[:n_slots], A


def snr(wf, records, counts=None, floor=None, sample_rate=12000, bins_per_tone=2, steps_per_symbol=2, n_samples=0,
        q=DEFAULT_Q, radius=DEFAULT_RADIUS, context=None):
    """ft8_snr on a GPU waterfall [n_slots, T, F]: records is a uint8 GPU tensor of n_slots * cap
    ft8_result records or a NumPy _lib.RESULT_DTYPE array [n_slots, cap]; counts an int32 GPU tensor,
    a sequence or None (every slot full); floor the N0 tensor of noise_floor (computed with q when
    None).  -> _lib.SNR_DTYPE array [n_slots, cap] (synchronises)."""
    torch, wf = _wf3(wf)
    n_slots, T, F = (int(v) for v in wf.shape)
    ctx = context if context is not None else _lib.context(wf.device)
    if not isinstance(records, torch.Tensor):
        records = torch.from_numpy(np.ascontiguousarray(records).reshape(-1).view(np.uint8).copy())
    records = records.to(wf.device).contiguous()
    cap = records.numel() // _lib.RESULT_DTYPE.itemsize // n_slots if n_slots else 0
    if counts is not None and not isinstance(counts, torch.Tensor):
        counts = torch.as_tensor(np.asarray(counts, dtype=np.int32))
    if counts is not None:
        counts = counts.to(device=wf.device, dtype=torch.int32).contiguous()
    if floor is None:
        floor = noise_floor(wf, q, context=ctx)[0]
    p = _lib.Ft8Params()
    fs = _lib.sample_rate_hz(sample_rate)
    p.sample_rate, p.sample_rate_hz = int(fs), fs
    p.bins_per_tone, p.steps_per_symbol = int(bins_per_tone), int(steps_per_symbol)
    out = torch.empty(max(n_slots * cap, 1) * _lib.SNR_DTYPE.itemsize, dtype=torch.uint8, device=wf.device)
    rc = _lib.lib().ft8_snr(ctx.handle, _lib.ptr(wf), int(wf.dtype == torch.float64), n_slots, T, F, ctypes.byref(p),
                            int(n_samples), _lib.ptr(records), None if counts is None else _lib.ptr(counts), cap,
                            _lib.ptr(floor), int(radius), _lib.ptr(out), _lib.stream_handle(wf.device))
    ctx.check(rc, "ft8_snr")
    return out[: n_slots * cap * _lib.SNR_DTYPE.itemsize].cpu().numpy().view(_lib.SNR_DTYPE).reshape(n_slots, cap)
