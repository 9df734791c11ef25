"""Host orchestration of the device receive path.

Turns decode_ft8_message's arguments (ft8_decode.py:288-296) into an ft8_params block -- STFT
geometry (spectrogram_analyse.py:31-43), the f >= 0 / band / time masks as index ranges
(ft8_decode.py:322-341) -- launches ft8_decode_batch on the caller's stream, and assembles the
reference's 5-tuples (ft8_decode.py:383-391) from the fixed-size device records.

Only parameter bookkeeping and result formatting happen here; every sample, waterfall, score,
LLR and codeword is processed by the HIP kernels of libft8hip.so.
"""
from __future__ import annotations

import ctypes
import os
import sys
from dataclasses import dataclass

import numpy as np

from . import _lib
from .ftx_types import FT8DecodeStatus, FT8Message

FT8_SYMBOL_FREQ_INTERVAL_HZ = 6.25  # spectrogram_analyse.py:7


@dataclass
class Plan:
    sample_rate: float  # as the caller gave it (int or float Hz)
    bins_per_tone: int
    steps_per_symbol: int
    n_samples: int
    nperseg: int
    hop: int
    nfft: int
    frames: int
    f_lo: int
    f_hi: int
    t_lo: int
    t_hi: int
    f: np.ndarray  # kept frequencies (Hz)
    t: np.ndarray  # kept frame-centre times (s)
    protocol: int = _lib.FT8_PROTO_FT8  # FT8_PROTO_FT4: the FT4 geometry and receive path (ft4.py)

    @property
    def empty(self) -> bool:
        return self.f_hi <= self.f_lo or self.t_hi <= self.t_lo

    @property
    def F(self) -> int:
        return self.f_hi - self.f_lo

    @property
    def T(self) -> int:
        return self.t_hi - self.t_lo


def spectrogram_axes(sample_rate, nperseg, hop, nfft, n_samples):
    """Unshifted two-sided frequency axis and frame times exactly as scipy builds them
    (_spectral_helper: fftfreq(nfft, 1/fs); arange(nperseg/2, n - nperseg/2 + 1, step)/fs)."""
    f = np.fft.fftfreq(nfft, 1 / sample_rate)
    t = np.arange(nperseg / 2, n_samples - nperseg / 2 + 1, hop) / float(sample_rate)
    return f, t


def make_plan(n_samples, sample_rate, bins_per_tone=2, steps_per_symbol=2, freq_min=None, freq_max=None,
              time_min=None, time_max=None, protocol="ft8") -> Plan:
    from .ft4 import protocol_code
    proto = protocol_code(protocol)
    nperseg, hop, nfft, frames = _lib.geometry(sample_rate, bins_per_tone, steps_per_symbol, n_samples, proto)
    if frames == 0:  # len(wave_data) < nperseg: empty spectrogram (spectrogram_analyse.py:37-39)
        z = np.zeros(0)
        return Plan(sample_rate, bins_per_tone, steps_per_symbol, n_samples, nperseg, hop, nfft, 0, 0, 0, 0, 0, z, z,
                    proto)
    f_all, t = spectrogram_axes(sample_rate, nperseg, hop, nfft, n_samples)
    npos = (nfft + 1) // 2            # fftshift then f >= 0 keeps natural bins 0..npos-1
    f = f_all[:npos]
    f_lo, f_hi = 0, npos
    if freq_min is not None or freq_max is not None:  # ft8_decode.py:328-333 (inclusive)
        lo = freq_min if freq_min is not None else f[0]
        hi = freq_max if freq_max is not None else f[-1]
        idx = np.nonzero((f >= lo) & (f <= hi))[0]
        f_lo, f_hi = (int(idx[0]), int(idx[-1]) + 1) if idx.size else (0, 0)
    t_lo, t_hi = 0, len(t)
    if time_min is not None or time_max is not None:  # ft8_decode.py:336-341 (inclusive)
        lo = time_min if time_min is not None else t[0]
        hi = time_max if time_max is not None else t[-1]
        idx = np.nonzero((t >= lo) & (t <= hi))[0]
        t_lo, t_hi = (int(idx[0]), int(idx[-1]) + 1) if idx.size else (0, 0)
    return Plan(sample_rate, bins_per_tone, steps_per_symbol, n_samples, nperseg, hop, nfft, frames,
                f_lo, f_hi, t_lo, t_hi, f[f_lo:f_hi], t[t_lo:t_hi], proto)


def min_score_is_f64(min_score) -> bool:
    """NumPy-2 rule for `np.float32 < min_score`: a Python int/float adopts float32; a NumPy scalar
    (np.float64, np.int64, ...) promotes the comparison to float64."""
    if isinstance(min_score, np.generic):
        return np.result_type(np.float32, min_score) == np.float64
    return False


def make_params(plan: Plan, max_candidates, min_score, max_iterations, flags=0) -> _lib.Ft8Params:
    p = _lib.Ft8Params()
    fs = _lib.sample_rate_hz(plan.sample_rate)
    p.sample_rate = int(fs)
    p.sample_rate_hz = fs   # the geometry follows the float rate (spectrogram_analyse.py:32-34)
    p.bins_per_tone = int(plan.bins_per_tone)
    p.steps_per_symbol = int(plan.steps_per_symbol)
    p.max_candidates = int(max_candidates)
    p.max_iterations = int(max_iterations)
    p.min_score_f64 = int(min_score_is_f64(min_score))
    p.min_score = float(min_score)
    p.f_lo, p.f_hi, p.t_lo, p.t_hi = plan.f_lo, plan.f_hi, plan.t_lo, plan.t_hi
    p.flags = int(flags)
    p.protocol = int(plan.protocol)
    return p


_TORCH_CODES = None


def _torch_codes():
    global _TORCH_CODES
    if _TORCH_CODES is None:
        import torch
        _TORCH_CODES = {torch.float32: _lib.FT8_F32, torch.float64: _lib.FT8_F64,
                        torch.complex64: _lib.FT8_C64, torch.complex128: _lib.FT8_C128,
                        torch.int16: _lib.FT8_I16}
    return _TORCH_CODES


def device_samples(wave_data, device=None, int16_is_pcm=False):
    """-> (tensor on the GPU, ft8 dtype code, waterfall is float64).

    NumPy input follows scipy's promotion against complex64 (spectrogram_analyse.py:46-56): any
    real array that promotes to complex64 is transformed as float32, to complex128 as float64.
    int16 tensors are raw PCM (scaled x/32767 on the device, read_wave_file semantics) only when
    int16_is_pcm is set."""
    torch = _lib.require_gpu()
    dev = torch.device("cuda", _lib.device_index(device))
    if isinstance(wave_data, torch.Tensor):
        x = wave_data
        if x.dtype == torch.int16 and int16_is_pcm:
            code = _lib.FT8_I16
        elif x.dtype in (torch.float32, torch.float64, torch.complex64, torch.complex128):
            code = _torch_codes()[x.dtype]
        else:
            nd = np.result_type(np.dtype(str(x.dtype).replace("torch.", "")), np.complex64)
            x = x.to(torch.float32 if nd == np.complex64 else torch.float64)
            code = _torch_codes()[x.dtype]
        x = x.to(dev).contiguous()
    else:
        a = np.asarray(wave_data)
        rt = np.result_type(a, np.complex64)
        if np.iscomplexobj(a):
            a = a.astype(np.complex64 if rt == np.complex64 else np.complex128, copy=False)
            code = _lib.FT8_C64 if rt == np.complex64 else _lib.FT8_C128
        else:
            a = a.astype(np.float32 if rt == np.complex64 else np.float64, copy=False)
            code = _lib.FT8_F32 if rt == np.complex64 else _lib.FT8_F64
        x = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    wf_f64 = code in (_lib.FT8_F64, _lib.FT8_C128)
    return x, code, wf_f64


def record_columns(recs: np.ndarray, sample_rate, bins_per_tone: int, wf_f64: bool):
    """Device records -> (time_s, freq_hz, score), one entry per record: time_sec = abs_time /
    sample_rate and freq_hz = (abs_freq / bins_per_tone) * 6.25 as lists of Python floats
    (ft8_decode.py:387-388), score as an array of the waterfall's dtype."""
    tsec = [t / sample_rate for t in recs["abs_time"].tolist()]
    fhz = [(f / bins_per_tone) * FT8_SYMBOL_FREQ_INTERVAL_HZ for f in recs["abs_freq"].tolist()]
    return tsec, fhz, recs["score"].astype(np.float64 if wf_f64 else np.float32)


def ft4_record_columns(recs: np.ndarray, plan: "Plan", wf_f64: bool):
    """record_columns for FT4 records: time_s = (t_lo + abs_time) hop / fs, the start of symbol 0, and
    freq_hz = (f_lo + abs_freq) fs / nfft, the frequency of tone 0."""
    fs = float(plan.sample_rate)
    tsec = [(plan.t_lo + t) * plan.hop / fs for t in recs["abs_time"].tolist()]
    fhz = [(plan.f_lo + f) * fs / plan.nfft for f in recs["abs_freq"].tolist()]
    return tsec, fhz, recs["score"].astype(np.float64 if wf_f64 else np.float32)


def records_to_results(recs: np.ndarray, sample_rate: int, bins_per_tone: int, wf_f64: bool, protocol="ft8", plan=None):
    """Device records (ok only, candidate order) -> [(FT8Message, FT8DecodeStatus, time_sec,
    freq_hz, score)] exactly as decode_ft8_message returns them (ft8_decode.py:383-391).
    protocol "ft4" (with the decoder's plan): time and frequency are ft4_record_columns'.

    time_sec, freq_hz (Python floats) and score (the waterfall dtype's NumPy scalar) are
    record_columns': columns are converted once per call (the per-record work is only the object
    construction)."""
    n = len(recs)
    if n == 0:
        return []
    payload = recs["payload"].tobytes()
    crc_c = recs["crc_calculated"].tolist()
    crc_e = recs["crc_extracted"].tolist()
    errs = recs["ldpc_errors"].tolist()
    tsec, fhz, sc = record_columns(recs, sample_rate, bins_per_tone, wf_f64)
    from .ft4 import protocol_code
    if protocol_code(protocol) == _lib.FT8_PROTO_FT4:
        tsec, fhz, sc = ft4_record_columns(recs, plan, wf_f64)
    out = []
    for i in range(n):
        msg = FT8Message(payload=bytearray(payload[10 * i: 10 * i + 10]), hash=crc_c[i])
        st = FT8DecodeStatus(ldpc_errors=errs[i], crc_extracted=crc_e[i], crc_calculated=crc_c[i])
        out.append((msg, st, tsec[i], fhz[i], sc[i]))
    return out


def split_slots(raw_u8: np.ndarray, dtype, counts, cap: int) -> list:
    """A host copy of a device buffer of n_slots * cap fixed-size records -> list (per slot) of the
    slot's first min(count, cap) records as a `dtype` array that owns its data."""
    dtype = np.dtype(dtype)
    n_slots = len(counts)
    rows = raw_u8[: n_slots * cap * dtype.itemsize].view(dtype).reshape(n_slots, cap)
    return [rows[s, : min(int(counts[s]), cap)].copy() for s in range(n_slots)]


_PACKAGE_DIR = os.path.dirname(os.path.abspath(__file__)) + os.sep


def warn_truncated(counts: np.ndarray, cap: int) -> None:
    """RuntimeWarning when a slot decoded more messages than its record capacity holds (the device
    keeps the first `cap` in candidate order and counts the rest).  The warning names the first
    frame outside this package: whoever called into it, through however many of its wrappers."""
    over = np.nonzero(counts > cap)[0]
    if over.size:
        import warnings
        level, frame = 2, sys._getframe(1)
        while frame.f_back is not None and os.path.abspath(frame.f_code.co_filename).startswith(_PACKAGE_DIR):
            level, frame = level + 1, frame.f_back
        warnings.warn(f"{over.size} slot(s) decoded more messages than max_results_per_slot={cap} "
                      f"(e.g. slot {int(over[0])}: {int(counts[over[0]])}); the records beyond it were dropped",
                      RuntimeWarning, stacklevel=level)


class SlotDecoder:
    """Batched decode of independent slots on one GPU: [B, N] samples -> per-slot decodes.

    The receive path (STFT -> Costas sync -> selection -> LLR -> BP -> CRC) runs as one
    ft8_decode_batch call on the current stream; outputs are fixed-size device records
    (ft8_result, 40 B) plus per-slot counts, ready for an all-gather across ranks.
    """

    def __init__(self, sample_rate=12000, bins_per_tone=2, steps_per_symbol=2, max_candidates=20,
                 min_score=10, max_iterations=20, freq_min=None, freq_max=None, time_min=None,
                 time_max=None, device=None, flags=0, max_results_per_slot=None, context=None, ap=None,
                 ap_max_hard_errors=None, coherent=None, coherent_drift=None, coherent_nsym=1, subtract=None,
                 coherent_ap=False, osd=None, osd_max_hard_errors=None, protocol="ft8", bp32=False):
        """subtract: True or a pass count in [2, 4] (True: 2) -- sets FT8_FLAG_SUBTRACT: what each pass decodes is
        subtracted and the residual decoded again, that many passes in all, every pass with the ap / coherent
        retries asked for below (ft8_set_subtract(n, 1)); the default capacity holds n * max_candidates rows.
        None / False: off -- a decoder given flags=FT8_FLAG_SUBTRACT instead runs the two plain passes and
        takes neither ap nor coherent.
        ap: a-priori patterns (ap.ap_hypothesis, e.g. ["CQ ? ?", "K1ABC ? ?"], tried in order on every
        candidate BP fails on; at most 8) -- sets FT8_FLAG_AP; None: plain decoding.  ap_max_hard_errors:
        the most hard decisions of an accepted AP decode that may contradict the received LLRs' signs
        (default ap.DEFAULT_MAX_HARD_ERRORS = 36; 174: no limit).
        coherent: True or a count -- sets FT8_FLAG_COHERENT: per slot that many of the best-scoring
        candidates BP fails on (True: 32, 0: every one) are demodulated again coherently from the samples
        (coherent.py) and decoded from those LLRs; None / False: off.
        coherent_drift: True or (max_rate Hz/s, n_rates) -- the coherent pass also searches n_rates (odd,
        <= 33) linear frequency drift rates over +-max_rate (<= 4; True: 1.0, 9) for every listed
        candidate (ft8_set_coherent_drift); needs coherent.  None / False: off.
        coherent_nsym: 1, 2 or 3 -- the coherent pass also decodes joint LLRs over 2 .. coherent_nsym symbols
        for every listed candidate (ft8_set_coherent_nsym); more than 1 needs coherent.  1: off.
        coherent_ap: True -- the candidates the coherent pass listed and left failed are also retried with the
        ap patterns clamped on their coherent LLRs, before the a-priori pass sees the STFT LLRs
        (ft8_set_coherent_ap); needs both ap and coherent.  False: off.
        osd: True, an order in [0, 2] or (order, max_per_slot) -- sets FT8_FLAG_OSD: per slot the first
        max_per_slot candidates (True: order 2 of 32; 0: every one) that every retry above left failed are
        decoded by ordered-statistics decoding of their STFT LLRs (osd.py; ft8_set_osd); None / False: off.
        osd_max_hard_errors: the most hard decisions of an accepted OSD decode that may contradict the received
        LLRs' signs (default osd.DEFAULT_MAX_HARD_ERRORS = 36; 174: no limit).
        bp32: True -- sets FT8_FLAG_BP_F32: every belief-propagation launch of a batch (main pass, retries,
        subtraction passes, FT4) runs in float32 (bp32.py): faster, and no longer bit-identical to the
        reference's float64 decoder.  False: the reference's arithmetic."""
        from . import ap as _ap
        from . import coherent as _coh
        from . import osd as _osd
        from . import subtract as _sub
        from .ft4 import protocol_code
        # protocol: "ft8" or "ft4" (ft4.py; decode, records, texts, messages, ap= and osd= work for FT4)
        self.protocol = protocol_code(protocol)
        if self.protocol == _lib.FT8_PROTO_FT4:
            off = [n for n, v in (("coherent", coherent), ("subtract", subtract), ("coherent_drift", coherent_drift),
                                  ("coherent_ap", coherent_ap)) if v not in (None, False)]
            if off or coherent_nsym != 1 or flags & (_lib.FT8_FLAG_COHERENT | _lib.FT8_FLAG_SUBTRACT):
                raise NotImplementedError("FT4 has no coherent re-demodulation and no subtraction yet: "
                                          + ", ".join(off or ["flags"]) + " is not available with protocol='ft4'")
        self.bp32 = bool(bp32)
        if self.bp32:
            flags |= _lib.FT8_FLAG_BP_F32
        self.osd = _osd.parse_option(osd)   # ValueError for what the library refuses
        self.osd_max_hard_errors = _osd.check_max_hard_errors(
            _osd.DEFAULT_MAX_HARD_ERRORS if osd_max_hard_errors is None else osd_max_hard_errors)
        if self.osd is not None:
            flags |= _lib.FT8_FLAG_OSD
        self.subtract = _sub.passes_of(subtract)   # ValueError for what the library refuses
        if self.subtract is not None:
            flags |= _lib.FT8_FLAG_SUBTRACT
        self.coherent_nsym = _coh.check_nsym(coherent_nsym)   # ValueError for what the library refuses
        self.coherent_ap = bool(coherent_ap)
        if self.coherent_ap and (ap is None or coherent is None or coherent is False):
            raise ValueError("coherent_ap needs both ap and coherent")
        if self.coherent_nsym > 1 and (coherent is None or coherent is False):
            raise ValueError("coherent_nsym needs coherent")
        if coherent_drift is None or coherent_drift is False:
            self.coherent_drift = None
        else:
            if coherent is None or coherent is False:
                raise ValueError("coherent_drift needs coherent")
            a, r = _coh.DEFAULT_DRIFT if coherent_drift is True else coherent_drift
            _coh.drift_rates(a, r)   # ValueError for what the library refuses
            self.coherent_drift = (float(a), int(r))
        if coherent is None or coherent is False:
            self.coherent = None
        else:
            self.coherent = _coh.DEFAULT_MAX_PER_SLOT if coherent is True else int(coherent)
            if self.coherent < 0:
                raise ValueError("coherent takes True or a count >= 0")
            flags |= _lib.FT8_FLAG_COHERENT
        self.ap_patterns = None if ap is None else tuple(ap)
        self.ap_hyps = None if ap is None else [_ap.ap_hypothesis(p) for p in self.ap_patterns]
        self.ap_max_hard_errors = int(_ap.DEFAULT_MAX_HARD_ERRORS if ap_max_hard_errors is None else ap_max_hard_errors)
        if ap is not None:
            if not 1 <= len(self.ap_hyps) <= _lib.FT8_AP_MAX_HYP:
                raise ValueError(f"ap takes 1..{_lib.FT8_AP_MAX_HYP} patterns")
            flags |= _lib.FT8_FLAG_AP
        self.kw = dict(sample_rate=sample_rate, bins_per_tone=bins_per_tone, steps_per_symbol=steps_per_symbol,
                       freq_min=freq_min, freq_max=freq_max, time_min=time_min, time_max=time_max,
                       protocol=self.protocol)
        self.max_candidates = int(max_candidates)
        self.min_score = min_score
        self.max_iterations = int(max_iterations)
        self.flags = flags
        self.device = _lib.device_index(device)
        # the thread's context for the device, or a dedicated one (_lib.Context(device)): decoders
        # that run concurrently on different streams want one context each (the library orders a
        # shared context's work across streams, which serialises them)
        self.ctx = context if context is not None else _lib.context(self.device)
        # a subtract-and-redecode batch appends up to max_candidates records per further pass after up to
        # max_candidates pass-1 records, so its default capacity holds every pass
        self.n_passes = (self.subtract or 2) if flags & _lib.FT8_FLAG_SUBTRACT else 1
        default_cap = max(self.max_candidates, 1) * self.n_passes
        self.cap = int(max_results_per_slot if max_results_per_slot is not None else default_cap)
        self._plans = {}
        self._bufs = {}
        self._launched = False  # whether the last run() reached ft8_decode_batch (else: nothing to decode)
        self._last_slots = 0    # slots of the last run()

    def plan(self, n_samples) -> Plan:
        if n_samples not in self._plans:
            self._plans[n_samples] = make_plan(n_samples, **self.kw)
        return self._plans[n_samples]

    def _buf(self, name, n, dtype=None):
        """The decoder's device buffer `name`, grown (never shrunk) to at least n elements (uint8
        unless dtype is given); never empty, so its pointer is always valid."""
        import torch
        b = self._bufs.get(name)
        if b is None or b.numel() < n:
            b = self._bufs[name] = torch.empty(max(n, 1), dtype=dtype or torch.uint8,
                                               device=torch.device("cuda", self.device))
        return b

    def _buffers(self, n_slots):
        import torch
        return (self._buf("out", n_slots * self.cap * _lib.RESULT_DTYPE.itemsize),
                self._buf("counts", n_slots, torch.int32))

    def run(self, samples, code=None, int16_is_pcm=True):
        """Asynchronous launch on the current stream.  samples: GPU tensor [B, N] (or [N]).
        Returns (records uint8 tensor [B*cap*40], counts int32 tensor [B])."""
        import torch
        x = samples
        if code is None:
            x, code, _ = device_samples(samples, self.device, int16_is_pcm=int16_is_pcm)
        if x.dim() == 1:
            x = x.unsqueeze(0)
        if x.dim() != 2:
            raise ValueError("samples must be [n_slots, n_samples]")
        if not x.is_contiguous():
            x = x.contiguous()
        n_slots, n = int(x.shape[0]), int(x.shape[1])
        out, counts = self._buffers(n_slots)
        plan = self.plan(n)
        self._launched = False
        self._last_slots = n_slots
        if plan.empty or n_slots == 0:
            counts[:n_slots].zero_()
            return out, counts[:n_slots]
        p = make_params(plan, self.max_candidates, self.min_score, self.max_iterations, self.flags)
        if self.ap_hyps is not None:  # a host-side setting; the context may serve other decoders too
            self.ctx.set_ap(self.ap_hyps, self.ap_max_hard_errors)
        if self.coherent is not None:
            self.ctx.set_coherent(self.coherent)
            self.ctx.set_coherent_drift(*(self.coherent_drift or (0.0, 1)))
            self.ctx.set_coherent_nsym(self.coherent_nsym)
            self.ctx.set_coherent_ap(self.coherent_ap)
        if self.osd is not None:
            self.ctx.set_osd(self.osd[0], self.osd[1], self.osd_max_hard_errors)
        if self.flags & _lib.FT8_FLAG_SUBTRACT:
            # every batch states its own setting, so a shared context never carries the opt-in over to a
            # decoder built with the flag alone (whose two passes refuse the retries)
            self.ctx.set_subtract(self.n_passes, self.subtract is not None)
        rc = _lib.lib().ft8_decode_batch(self.ctx.handle, _lib.ptr(x), int(code), n, n_slots, n,
                                         ctypes.byref(p), _lib.ptr(out), _lib.ptr(counts), self.cap,
                                         _lib.stream_handle(torch.device("cuda", self.device)))
        self.ctx.check(rc, "ft8_decode_batch")
        self._launched = True
        return out, counts[:n_slots]

    def pass_counts(self):
        """Synchronous: ft8_subtract_counts of the last run() (or records() / messages() ...) of a subtract
        decoder -> int32 array [n_slots, n_passes], the uncapped row count of every slot after each pass
        (subtract.pass_of gives a row's pass).  Zeros when that run had nothing to decode."""
        import torch
        if not self.flags & _lib.FT8_FLAG_SUBTRACT:
            raise ValueError("pass_counts needs a subtract decoder")
        n_slots, n = self._last_slots, self.n_passes
        if not self._launched or n_slots == 0:
            return np.zeros((n_slots, n), dtype=np.int32)
        dev = torch.device("cuda", self.device)
        d = self._buf("pass_counts", n_slots * n, torch.int32)
        rc = _lib.lib().ft8_subtract_counts(self.ctx.handle, _lib.ptr(d), n_slots, n, _lib.stream_handle(dev))
        self.ctx.check(rc, "ft8_subtract_counts")
        return d[: n_slots * n].cpu().numpy().reshape(n_slots, n).copy()

    def _snr_last(self, out, counts):
        """ft8_snr_last for the records run() just wrote, on the same stream: -> the device buffer of
        n_slots * cap ft8_snr_rec.  A run() that had nothing to decode (an empty plan: no waterfall)
        gives every record status 3, as the library does for records past a slot's count."""
        import torch
        n_slots = int(counts.shape[0])
        nbytes = n_slots * self.cap * _lib.SNR_DTYPE.itemsize
        d_snr = self._buf("snr", nbytes)
        if not self._launched:
            blank = np.zeros(n_slots * self.cap, dtype=_lib.SNR_DTYPE)
            blank["status"] = 3
            d_snr[:nbytes].copy_(torch.from_numpy(blank.view(np.uint8)))
        elif n_slots and self.cap:
            rc = _lib.lib().ft8_snr_last(self.ctx.handle, _lib.ptr(out), _lib.ptr(counts), n_slots, self.cap,
                                         _lib.ptr(d_snr), _lib.stream_handle(out.device))
            self.ctx.check(rc, "ft8_snr_last")
        return d_snr

    def _fetch(self, samples, code=None, int16_is_pcm=True, records=True, text=False, snr=False):
        """run(), then with text one ft8_unpack77 and with snr one ft8_snr_last, all on the current
        stream with no host sync in between; only then the copies to the host and the truncation
        warning: -> (records, ft8_text records, ft8_snr_rec records), each a list per slot, aligned,
        or None where it was not asked for."""
        if snr and self.protocol == _lib.FT8_PROTO_FT4:
            raise NotImplementedError("the signal report (snr, reports) is not available with protocol='ft4' yet")
        out, counts = self.run(samples, code, int16_is_pcm)
        n_slots = int(counts.shape[0])
        d_text = d_snr = None
        if text:
            d_text = self._buf("text", n_slots * self.cap * _lib.TEXT_DTYPE.itemsize)
            if n_slots and self.cap:
                rc = _lib.lib().ft8_unpack77(self.ctx.handle, _lib.ptr(out), _lib.ptr(counts), n_slots, self.cap,
                                             _lib.ptr(d_text), _lib.stream_handle(out.device))
                self.ctx.check(rc, "ft8_unpack77")
        if snr:
            d_snr = self._snr_last(out, counts)
        c = counts.cpu().numpy()
        warn_truncated(c, self.cap)
        n = n_slots * self.cap
        return tuple(d if d is None else split_slots(d[: n * dt.itemsize].cpu().numpy(), dt, c, self.cap)
                     for d, dt in ((out if records else None, _lib.RESULT_DTYPE), (d_text, _lib.TEXT_DTYPE),
                                   (d_snr, _lib.SNR_DTYPE)))

    def records(self, samples, code=None, int16_is_pcm=True):
        """Synchronous: -> list (per slot) of structured ft8_result arrays (ok decodes, candidate order)."""
        return self._fetch(samples, code, int16_is_pcm)[0]

    def decode(self, samples, int16_is_pcm=True):
        """-> list (per slot) of the reference's 5-tuples."""
        x, code, wf_f64 = device_samples(samples, self.device, int16_is_pcm=int16_is_pcm)
        per_slot = self.records(x, code)
        return [records_to_results(r, self.kw["sample_rate"], self.kw["bins_per_tone"], wf_f64, self.protocol,
                                   self.plan(int(x.shape[-1]))) for r in per_slot]

    def texts(self, samples, code=None, int16_is_pcm=True):
        """Synchronous: -> list (per slot) of ft8_text arrays (_lib.TEXT_DTYPE) aligned with records():
        the message text of every decode, unpacked on the device (ft8_unpack77), and dup_of, the
        slot's first record with the same payload."""
        return self._fetch(samples, code, int16_is_pcm, text=True)[1]

    def snr(self, samples, code=None, int16_is_pcm=True):
        """Synchronous: -> list (per slot) of ft8_snr_rec arrays (_lib.SNR_DTYPE) aligned with records():
        the signal report of every decode (snr_db: SNR in 2500 Hz), measured on the device
        (ft8_snr_last) on the waterfall the decode left there.  Raises NotImplementedError for a
        decoder built with FT8_FLAG_SUBTRACT (that waterfall is the residual's)."""
        return self._fetch(samples, code, int16_is_pcm, records=False, snr=True)[2]

    def _message_rows(self, samples, table, unique, int16_is_pcm, snr):
        from .message import text_of
        from .snr import snr_db_or_nan
        x, code, wf_f64 = device_samples(samples, self.device, int16_is_pcm=int16_is_pcm)
        recs, txts, reps = self._fetch(x, code, text=True, snr=snr)
        out = []
        for s, (r, t) in enumerate(zip(recs, txts)):
            if self.protocol == _lib.FT8_PROTO_FT4:
                tsec, fhz, sc = ft4_record_columns(r, self.plan(int(x.shape[-1])), wf_f64)
            else:
                tsec, fhz, sc = record_columns(r, self.kw["sample_rate"], self.kw["bins_per_tone"], wf_f64)
            db = snr_db_or_nan(reps[s]) if snr else None
            rows = []
            for i in range(len(r)):
                if int(t["status"][i]) != 0 or (unique and int(t["dup_of"][i]) >= 0):
                    continue
                text = table.resolve(t[i]) if table is not None else text_of(t[i])
                rows.append((text,) + ((db[i],) if snr else ()) + (tsec[i], fhz[i], sc[i], r[i]))
            if table is not None:
                table.learn(t)
            out.append(rows)
        return out

    def messages(self, samples, table=None, unique=True, int16_is_pcm=True):
        """-> list (per slot) of (text, time_s, freq_hz, score, record) for every decode whose message
        type is unpacked (ft8_text.status 0), in candidate order; time, frequency and score as decode()
        gives them.  unique drops the records whose payload an earlier record of the slot carries.
        table (message.CallsignTable): hashed callsigns it knows are written <CALL>; slots are
        handled in order, and within a slot every record is resolved before the slot is learned."""
        return self._message_rows(samples, table, unique, int16_is_pcm, snr=False)

    def reports(self, samples, table=None, unique=True, int16_is_pcm=True):
        """messages() with the signal report: -> list (per slot) of (text, snr_db, time_s, freq_hz,
        score, record); snr_db is the SNR in 2500 Hz (a Python float; NaN where the report's status
        is 2).  One ft8_decode_batch, one ft8_unpack77 and one ft8_snr_last on the current stream,
        with no host sync in between.  Raises NotImplementedError for a decoder built with
        FT8_FLAG_SUBTRACT."""
        return self._message_rows(samples, table, unique, int16_is_pcm, snr=True)

    def timing(self, reset=False):
        return self.ctx.timing(reset)


def decode_slots(samples, sample_rate=12000, **kwargs):
    """One-call form of SlotDecoder: samples [B, N] (GPU tensor, float32/int16/...) -> list (per
    slot) of decode_ft8_message's 5-tuples."""
    return SlotDecoder(sample_rate=sample_rate, **kwargs).decode(samples)


def decode_one(x, code, sample_rate, bins_per_tone=2, steps_per_symbol=2, max_candidates=20, min_score=10,
               max_iterations=20, freq_min=None, freq_max=None, time_min=None, time_max=None, *, flags=0, snr=False,
               ap=None, ap_max_hard_errors=None, coherent=None, coherent_drift=None, coherent_nsym=1, subtract=None,
               pass_counts=False, coherent_ap=False, osd=None, osd_max_hard_errors=None, protocol="ft8", bp32=False):
    """One slot, x [N] on the GPU with its ft8 dtype code, through a SlotDecoder of its own:
    -> (decode_ft8_message's 5-tuples, with snr the ft8_snr_rec records aligned with them else None,
    the ft8_result records) and, with pass_counts (a subtract decode), the slot's row of
    SlotDecoder.pass_counts as a fourth entry.  Nothing is launched when the masks leave nothing or
    max_candidates <= 0."""
    recs, reps = np.zeros(0, _lib.RESULT_DTYPE), np.zeros(0, _lib.SNR_DTYPE) if snr else None
    per_pass = np.zeros(0, np.int32)
    plan = make_plan(int(x.shape[0]), sample_rate, bins_per_tone, steps_per_symbol, freq_min, freq_max, time_min,
                     time_max, protocol)
    if not plan.empty and max_candidates > 0:
        dec = SlotDecoder(sample_rate, bins_per_tone, steps_per_symbol, max_candidates, min_score, max_iterations,
                          freq_min, freq_max, time_min, time_max, device=x.device, flags=flags, ap=ap,
                          ap_max_hard_errors=ap_max_hard_errors, coherent=coherent, coherent_drift=coherent_drift,
                          coherent_nsym=coherent_nsym, subtract=subtract, coherent_ap=coherent_ap, osd=osd,
                          osd_max_hard_errors=osd_max_hard_errors, protocol=protocol, bp32=bp32)
        recs, _, reps = (v if v is None else v[0] for v in dec._fetch(x.unsqueeze(0), code, snr=snr))
        if pass_counts:
            per_pass = dec.pass_counts()[0]
    wf_f64 = code in (_lib.FT8_F64, _lib.FT8_C128)
    out = records_to_results(recs, sample_rate, bins_per_tone, wf_f64, protocol, plan), reps, recs
    return out + (per_pass,) if pass_counts else out
