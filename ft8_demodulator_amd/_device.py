"""Device-side helpers shared by the mirror modules (waterfall upload, stage calls)."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib


def waterfall_to_device(wf):
    """FT8Waterfall.mag [freq, time] (NumPy or torch) -> time-major device tensor [T, F].

    float32 stays float32 (the reference's np.float32 score path); every other dtype is scored in
    float64."""
    torch = _lib.require_gpu()
    mag = wf.mag
    if isinstance(mag, torch.Tensor):
        t = mag
        if t.dtype not in (torch.float32, torch.float64):
            t = t.to(torch.float64)
        t = t.t().contiguous().cuda()
    else:
        a = np.asarray(mag)
        if a.dtype not in (np.float32, np.float64):
            a = a.astype(np.float64)
        t = torch.from_numpy(np.ascontiguousarray(a.T)).cuda()
    F, T = int(t.shape[1]), int(t.shape[0])
    return t, t.dtype == torch.float64, T, F


def sync_params(wf, max_candidates, min_score, flags=0):
    from ._pipeline import min_score_is_f64
    p = _lib.Ft8Params()
    p.flags = int(flags)
    p.sample_rate = 1
    p.bins_per_tone = int(wf.freq_osr)
    p.steps_per_symbol = int(wf.time_osr)
    p.max_candidates = int(max_candidates)
    p.max_iterations = 0
    p.min_score_f64 = int(min_score_is_f64(min_score))
    p.min_score = float(min_score)
    return p


def grid_shape(T, F, sps, bpt):
    nb = T // sps
    t0 = -10 * sps
    NT = max(nb * sps - sps * 59 - t0, 0)
    NF = max(F - 7 * bpt, 0)
    return t0, NT, NF


def sync_select(wf, max_candidates, min_score, want_grid=False, flags=0):
    """-> (cands [(abs_time, abs_freq, score)], score grid or None, warning flags)."""
    torch = _lib.require_gpu()
    ctx = _lib.context()
    d, f64, T, F = waterfall_to_device(wf)
    N = max(int(max_candidates), 0)
    sps, bpt = int(wf.time_osr), int(wf.freq_osr)
    t0, NT, NF = grid_shape(T, F, sps, bpt)
    dev = d.device
    cand = torch.zeros(max(N, 1) * 2, dtype=torch.int32, device=dev)
    cs = torch.zeros(max(N, 1), dtype=torch.float64, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    grid = torch.empty(max(NT * NF, 1), dtype=d.dtype, device=dev) if want_grid else None
    p = sync_params(wf, max(N, 1) if want_grid else N, min_score, flags)
    rc = _lib.lib().ft8_sync_select(ctx.handle, _lib.ptr(d), int(f64), 1, T, F, ctypes.byref(p),
                                    _lib.ptr(cand), _lib.ptr(cs), _lib.ptr(cnt),
                                    _lib.ptr(grid) if grid is not None else None, _lib.stream_handle())
    ctx.check(rc, "ft8_sync_select")
    warn = torch.zeros(1, dtype=torch.int32, device=dev)
    if NT > 0 and NF > 0 and p.max_candidates > 0:
        ctx.check(_lib.lib().ft8_select_warnings(ctx.handle, _lib.ptr(warn), 1, _lib.stream_handle()),
                  "ft8_select_warnings")
    n = int(cnt.item()) if N > 0 else 0
    c = cand.cpu().numpy().reshape(-1, 2)
    s = cs.cpu().numpy()
    sc_t = np.float64 if f64 else np.float32
    cands = [(int(c[i, 0]), int(c[i, 1]), sc_t(s[i])) for i in range(n)]
    g = None
    if want_grid:
        g = grid[: NT * NF].cpu().numpy().reshape(NT, NF) if NT * NF else np.zeros((NT, NF), d.cpu().numpy().dtype)
    return cands, g, int(warn.item())


def sync_scores(wf, cand_list):
    """ft8_sync_score of arbitrary (abs_time, abs_freq) pairs (k_score_list) -> (scores in the
    waterfall dtype, IndexError flags)."""
    torch = _lib.require_gpu()
    ctx = _lib.context()
    d, f64, T, F = waterfall_to_device(wf)
    n = len(cand_list)
    c = torch.tensor([[int(a), int(b)] for a, b in cand_list] or [[0, 0]], dtype=torch.int32, device=d.device)
    out = torch.empty(max(n, 1), dtype=d.dtype, device=d.device)
    err = torch.zeros(max(n, 1), dtype=torch.int32, device=d.device)
    rc = _lib.lib().ft8_sync_score(ctx.handle, _lib.ptr(d), int(f64), T, F, int(wf.time_osr), int(wf.freq_osr),
                                   _lib.ptr(c), n, _lib.ptr(out), _lib.ptr(err), _lib.stream_handle())
    ctx.check(rc, "ft8_sync_score")
    return out.cpu().numpy()[:n], err.cpu().numpy()[:n].astype(bool)


def llr(wf, cand_list, normalize):
    """cand_list [(abs_time, abs_freq)] -> LLRs [n, 174] (float64)."""
    torch = _lib.require_gpu()
    ctx = _lib.context()
    d, f64, T, F = waterfall_to_device(wf)
    n = len(cand_list)
    if n == 0:
        return np.zeros((0, 174))
    c = torch.tensor([[0, int(a), int(b)] for a, b in cand_list], dtype=torch.int32, device=d.device)
    out = torch.empty(n, 174, dtype=torch.float64, device=d.device)
    rc = _lib.lib().ft8_llr(ctx.handle, _lib.ptr(d), int(f64), T, F, int(wf.time_osr), int(wf.freq_osr),
                            _lib.ptr(c), n, int(bool(normalize)), _lib.ptr(out), _lib.stream_handle())
    ctx.check(rc, "ft8_llr")
    return out.cpu().numpy()


def _llr_rows(x):
    """LLRs (anything array-like of n * 174 values) -> float64 device tensor [n, 174]."""
    torch = _lib.require_gpu()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1, 174))).cuda()


def normalize(x):
    torch = _lib.require_gpu()
    ctx = _lib.context()
    a = _llr_rows(x)
    out = torch.empty_like(a)
    ctx.check(_lib.lib().ft8_normalize(ctx.handle, _lib.ptr(a), a.shape[0], _lib.ptr(out), _lib.stream_handle()),
              "ft8_normalize")
    return out.cpu().numpy()


def bp(llrs, max_iterations, f32=False):
    """LLRs [n, 174] -> (plain uint8 [n, 174], records structured [n]).  f32: the float32 decoder
    (ft8_bp_f32; bp32.bp32_restate is its restatement) instead of the reference's float64."""
    torch = _lib.require_gpu()
    ctx = _lib.context()
    a = _llr_rows(llrs)
    n = a.shape[0]
    plain = torch.zeros(n, 174, dtype=torch.uint8, device=a.device)
    res = torch.zeros(n * _lib.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=a.device)
    call, name = (_lib.lib().ft8_bp_f32, "ft8_bp_f32") if f32 else (_lib.lib().ft8_bp, "ft8_bp")
    ctx.check(call(ctx.handle, _lib.ptr(a), n, int(max_iterations), _lib.ptr(plain), _lib.ptr(res),
                   _lib.stream_handle()), name)
    return plain.cpu().numpy(), res.cpu().numpy().view(_lib.RESULT_DTYPE)


def ap_decode(llrs, records, max_iterations):
    """ft8_ap_decode: LLRs [n, 174] and the records ft8_bp wrote from them -> (records updated by the
    context's a-priori hypotheses (Context.set_ap), hard int16 [n])."""
    torch = _lib.require_gpu()
    ctx = _lib.context()
    a = _llr_rows(llrs)
    n = a.shape[0]
    rec = np.ascontiguousarray(np.asarray(records, dtype=_lib.RESULT_DTYPE).reshape(-1))
    if len(rec) != n:
        raise ValueError(f"{n} LLR vectors but {len(rec)} records")
    res = torch.from_numpy(np.concatenate([rec.view(np.uint8), np.zeros(8, np.uint8)])).to(a.device)
    hard = torch.zeros(max(n, 1), dtype=torch.int16, device=a.device)
    ctx.check(_lib.lib().ft8_ap_decode(ctx.handle, _lib.ptr(a), _lib.ptr(res), n, int(max_iterations),
                                       _lib.ptr(hard), _lib.stream_handle()), "ft8_ap_decode")
    return res.cpu().numpy()[: n * _lib.RESULT_DTYPE.itemsize].view(_lib.RESULT_DTYPE).copy(), hard.cpu().numpy()[:n]


def osd_decode(llrs, records):
    """ft8_osd_decode: LLRs [n, 174] and the records ft8_bp wrote from them -> (records updated by
    ordered-statistics decoding with the context's setting (Context.set_osd), info _lib.OSD_DTYPE [n],
    codewords uint8 [n, 22])."""
    torch = _lib.require_gpu()
    ctx = _lib.context()
    a = _llr_rows(llrs)
    n = a.shape[0]
    rec = np.ascontiguousarray(np.asarray(records, dtype=_lib.RESULT_DTYPE).reshape(-1))
    if len(rec) != n:
        raise ValueError(f"{n} LLR vectors but {len(rec)} records")
    res = torch.from_numpy(np.concatenate([rec.view(np.uint8), np.zeros(8, np.uint8)])).to(a.device)
    info = torch.zeros(max(n, 1) * _lib.OSD_DTYPE.itemsize, dtype=torch.uint8, device=a.device)
    cw = torch.zeros(max(n, 1), 22, dtype=torch.uint8, device=a.device)
    ctx.check(_lib.lib().ft8_osd_decode(ctx.handle, _lib.ptr(a), _lib.ptr(res), n, _lib.ptr(info), _lib.ptr(cw),
                                        _lib.stream_handle()), "ft8_osd_decode")
    return (res.cpu().numpy()[: n * _lib.RESULT_DTYPE.itemsize].view(_lib.RESULT_DTYPE).copy(),
            info.cpu().numpy()[: n * _lib.OSD_DTYPE.itemsize].view(_lib.OSD_DTYPE).copy(), cw.cpu().numpy()[:n])


def coherent_ap_decode(llrs, records, max_iterations, valid=None):
    """ft8_coherent_ap_decode: coherent LLRs [n, 174] or [n, S, 174], the records ft8_bp left and the validity
    bytes uint8 [n] (None: every set usable) -> (records updated by the context's a-priori hypotheses
    (Context.set_ap) on those LLRs, hard int16 [n])."""
    torch = _lib.require_gpu()
    ctx = _lib.context()
    L = np.asarray(llrs, dtype=np.float64)
    if L.ndim == 2:
        L = L[:, None, :]
    if L.ndim != 3 or L.shape[2] != 174:
        raise ValueError("llrs must be [n, 174] or [n, S, 174]")
    n, S = int(L.shape[0]), int(L.shape[1])
    rec = np.ascontiguousarray(np.asarray(records, dtype=_lib.RESULT_DTYPE).reshape(-1))
    if len(rec) != n:
        raise ValueError(f"{n} LLR vectors but {len(rec)} records")
    a = torch.from_numpy(np.concatenate([np.ascontiguousarray(L).reshape(-1), np.zeros(1)])).cuda()
    res = torch.from_numpy(np.concatenate([rec.view(np.uint8), np.zeros(8, np.uint8)])).to(a.device)
    hard = torch.zeros(max(n, 1), dtype=torch.int16, device=a.device)
    d_v = None
    if valid is not None:
        v = np.ascontiguousarray(np.asarray(valid, dtype=np.uint8).reshape(-1))
        if len(v) != n:
            raise ValueError(f"{n} LLR vectors but {len(v)} validity bytes")
        d_v = torch.from_numpy(np.concatenate([v, np.zeros(1, np.uint8)])).to(a.device)
    ctx.check(_lib.lib().ft8_coherent_ap_decode(ctx.handle, _lib.ptr(a), S, None if d_v is None else _lib.ptr(d_v),
                                                _lib.ptr(res), n, int(max_iterations), _lib.ptr(hard),
                                                _lib.stream_handle()), "ft8_coherent_ap_decode")
    return res.cpu().numpy()[: n * _lib.RESULT_DTYPE.itemsize].view(_lib.RESULT_DTYPE).copy(), hard.cpu().numpy()[:n]


def coherent_llr(samples, cand, slot_of, sample_rate=12000, bins_per_tone=2, steps_per_symbol=2, t_lo=0, f_lo=0,
                 code=None, drift=None, nsym=1):
    """ft8_coherent_llr: samples [n_slots, n_samples] (float32, or int16 PCM; NumPy or a GPU tensor with
    its ft8 dtype `code`), candidates cand [n, 2] = (abs_time, abs_freq) of the slots slot_of [n]
    -> (LLRs float64 [n, 174], fits coherent.FIT_DTYPE [n]).  drift = (max_rate, n_rates):
    ft8_coherent_drift_llr -> (LLRs, fits, drifts coherent.DRIFT_DTYPE [n]).  nsym = S > 1:
    ft8_coherent_nsym_llr -> LLRs [n, S, 174], and the validity bytes uint8 [n] come last."""
    from ._pipeline import device_samples
    from .coherent import DRIFT_DTYPE, FIT_DTYPE, check_nsym
    S = check_nsym(nsym)
    torch = _lib.require_gpu()
    ctx = _lib.context()
    x = samples
    if code is None and isinstance(samples, np.ndarray) and samples.dtype == np.int16:   # raw PCM, as a tensor is
        x, code = torch.from_numpy(np.ascontiguousarray(samples)).cuda(), _lib.FT8_I16
    elif code is None:
        x, code, _ = device_samples(samples, int16_is_pcm=True)
    if x.dim() == 1:
        x = x.unsqueeze(0)
    x = x.contiguous()
    n_slots, ns = int(x.shape[0]), int(x.shape[1])
    c = np.ascontiguousarray(np.asarray(cand, dtype=np.int32).reshape(-1, 2))
    so = np.ascontiguousarray(np.asarray(slot_of, dtype=np.int32).reshape(-1))
    n = len(c)
    if len(so) != n:
        raise ValueError(f"{n} candidates but {len(so)} slot indices")
    p = _lib.Ft8Params()
    fs = _lib.sample_rate_hz(sample_rate)
    p.sample_rate, p.sample_rate_hz = int(fs), fs
    p.bins_per_tone, p.steps_per_symbol = int(bins_per_tone), int(steps_per_symbol)
    p.t_lo, p.f_lo = int(t_lo), int(f_lo)
    d_c = torch.from_numpy(np.concatenate([c.reshape(-1), np.zeros(2, np.int32)])).to(x.device)
    d_so = torch.from_numpy(np.concatenate([so, np.zeros(1, np.int32)])).to(x.device)
    d_llr = torch.zeros(max(n, 1), 174, dtype=torch.float64, device=x.device)
    d_fit = torch.zeros(max(n, 1) * FIT_DTYPE.itemsize, dtype=torch.uint8, device=x.device)
    if S > 1:
        d_llr = torch.zeros(max(n, 1), S, 174, dtype=torch.float64, device=x.device)
        d_dr = torch.zeros(max(n, 1) * DRIFT_DTYPE.itemsize, dtype=torch.uint8, device=x.device)
        d_v = torch.zeros(max(n, 1), dtype=torch.uint8, device=x.device)
        a, r = (0.0, 1) if drift is None else (float(drift[0]), int(drift[1]))
        ctx.check(_lib.lib().ft8_coherent_nsym_llr(ctx.handle, _lib.ptr(x), int(code), ns, n_slots, ns, ctypes.byref(p),
                                                   _lib.ptr(d_c), _lib.ptr(d_so), n, a, r, _lib.ptr(d_llr),
                                                   _lib.ptr(d_fit), _lib.ptr(d_dr), S, _lib.ptr(d_v),
                                                   _lib.stream_handle()), "ft8_coherent_nsym_llr")
        out = (d_llr.cpu().numpy()[:n], d_fit.cpu().numpy()[: n * FIT_DTYPE.itemsize].view(FIT_DTYPE).copy())
        if drift is not None:
            out += (d_dr.cpu().numpy()[: n * DRIFT_DTYPE.itemsize].view(DRIFT_DTYPE).copy(),)
        return out + (d_v.cpu().numpy()[:n].copy(),)
    if drift is not None:
        d_dr = torch.zeros(max(n, 1) * DRIFT_DTYPE.itemsize, dtype=torch.uint8, device=x.device)
        ctx.check(_lib.lib().ft8_coherent_drift_llr(ctx.handle, _lib.ptr(x), int(code), ns, n_slots, ns, ctypes.byref(p),
                                                    _lib.ptr(d_c), _lib.ptr(d_so), n, float(drift[0]), int(drift[1]),
                                                    _lib.ptr(d_llr), _lib.ptr(d_fit), _lib.ptr(d_dr),
                                                    _lib.stream_handle()), "ft8_coherent_drift_llr")
        return (d_llr.cpu().numpy()[:n], d_fit.cpu().numpy()[: n * FIT_DTYPE.itemsize].view(FIT_DTYPE).copy(),
                d_dr.cpu().numpy()[: n * DRIFT_DTYPE.itemsize].view(DRIFT_DTYPE).copy())
    ctx.check(_lib.lib().ft8_coherent_llr(ctx.handle, _lib.ptr(x), int(code), ns, n_slots, ns, ctypes.byref(p),
                                          _lib.ptr(d_c), _lib.ptr(d_so), n, _lib.ptr(d_llr), _lib.ptr(d_fit),
                                          _lib.stream_handle()), "ft8_coherent_llr")
    return d_llr.cpu().numpy()[:n], d_fit.cpu().numpy()[: n * FIT_DTYPE.itemsize].view(FIT_DTYPE).copy()


def crc14(msgs, nbits):
    torch = _lib.require_gpu()
    ctx = _lib.context()
    n = len(msgs)
    buf = np.zeros((max(n, 1), 12), dtype=np.uint8)
    for i, m in enumerate(msgs):
        b = bytes(m)[:12]
        buf[i, :len(b)] = np.frombuffer(b, dtype=np.uint8)
    d = torch.from_numpy(buf).cuda()
    nb = torch.tensor(list(nbits) or [0], dtype=torch.int32, device=d.device)
    out = torch.zeros(max(n, 1), dtype=torch.int16, device=d.device)
    ctx.check(_lib.lib().ft8_crc14(ctx.handle, _lib.ptr(d), _lib.ptr(nb), n, _lib.ptr(out), _lib.stream_handle()),
              "ft8_crc14")
    return [int(v) & 0xFFFF for v in out.cpu().numpy()[:n]]


def ldpc_check(bits):
    torch = _lib.require_gpu()
    ctx = _lib.context()
    b = torch.from_numpy(np.ascontiguousarray((np.asarray(bits).reshape(-1, 174) != 0).astype(np.uint8))).cuda()
    n = b.shape[0]
    out = torch.zeros(n, dtype=torch.int32, device=b.device)
    ctx.check(_lib.lib().ft8_ldpc_check(ctx.handle, _lib.ptr(b), n, _lib.ptr(out), _lib.stream_handle()),
              "ft8_ldpc_check")
    return out.cpu().numpy()


def stft(wave_data, sample_rate, bins_per_tone, steps_per_symbol, f_lo=None, f_hi=None, t_lo=None, t_hi=None,
         device=None):
    """-> (waterfall tensor [T, F] time-major on the device, plan, wf_f64)."""
    torch = _lib.require_gpu()
    from ._pipeline import device_samples, make_plan
    x, code, f64 = device_samples(wave_data, device)
    if x.dim() != 1:
        raise ValueError("wave_data must be one-dimensional")
    n = int(x.shape[0])
    plan = make_plan(n, sample_rate, bins_per_tone, steps_per_symbol)
    if plan.frames == 0:
        return None, plan, f64
    ctx = _lib.context(x.device)
    p = _lib.Ft8Params()
    p.sample_rate_hz = _lib.sample_rate_hz(sample_rate)
    p.sample_rate, p.bins_per_tone, p.steps_per_symbol = int(p.sample_rate_hz), int(bins_per_tone), int(steps_per_symbol)
    p.f_lo = 0 if f_lo is None else int(f_lo)
    p.f_hi = plan.nfft if f_hi is None else int(f_hi)
    p.t_lo = 0 if t_lo is None else int(t_lo)
    p.t_hi = plan.frames if t_hi is None else int(t_hi)
    out = torch.empty(max(p.t_hi - p.t_lo, 0), max(p.f_hi - p.f_lo, 0),
                      dtype=torch.float64 if f64 else torch.float32, device=x.device)
    rc = _lib.lib().ft8_stft(ctx.handle, _lib.ptr(x), int(code), n, 1, n, ctypes.byref(p), _lib.ptr(out),
                             _lib.stream_handle(x.device))
    ctx.check(rc, "ft8_stft")
    return out, plan, f64


# ---- FT4 stage calls (ft4.py restates each of them) ---------------------------------------------------
def _wf_slots(wf):
    """A waterfall [T, F] or [n_slots, T, F] (time-major, NumPy or a GPU tensor) -> (device tensor
    [n_slots, T, F], is float64)."""
    torch = _lib.require_gpu()
    t = wf if isinstance(wf, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(wf))
    if t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float64)
    if t.dim() == 2:
        t = t.unsqueeze(0)
    return t.cuda().contiguous(), t.dtype == torch.float64


def ft4_stft(samples, sample_rate=12000, bins_per_tone=2, steps_per_symbol=2, code=None):
    """ft8_stft with FT8_PROTO_FT4: samples [n_slots, n] (NumPy, or a GPU tensor with its ft8 dtype code) ->
    (waterfall tensor [n_slots, T, F] on the device, plan)."""
    torch = _lib.require_gpu()
    from ._pipeline import device_samples, make_params, make_plan
    x = samples
    if code is None:
        x, code, _ = device_samples(samples, int16_is_pcm=True)
    if x.dim() == 1:
        x = x.unsqueeze(0)
    x = x.contiguous()
    n_slots, n = int(x.shape[0]), int(x.shape[1])
    plan = make_plan(n, sample_rate, bins_per_tone, steps_per_symbol, protocol="ft4")
    ctx = _lib.context(x.device)
    p = make_params(plan, 0, 0, 0)
    f64 = code in (_lib.FT8_F64, _lib.FT8_C128)
    out = torch.empty(n_slots, plan.T, plan.F, dtype=torch.float64 if f64 else torch.float32, device=x.device)
    ctx.check(_lib.lib().ft8_stft(ctx.handle, _lib.ptr(x), int(code), n, n_slots, n, ctypes.byref(p), _lib.ptr(out),
                                  _lib.stream_handle(x.device)), "ft8_stft")
    return out, plan


def ft4_sync_select(wf, sps, bpt, max_candidates, min_score, flags=0, want_grid=False):
    """ft8_sync_select with FT8_PROTO_FT4 on wf [n_slots, T, F] -> (per slot [(abs_time, abs_freq, score)],
    score grids [n_slots, NT, NF] or None, warning flags [n_slots])."""
    torch = _lib.require_gpu()
    from ._pipeline import min_score_is_f64
    from .ft4 import ft4_grid_shape
    ctx = _lib.context()
    d, f64 = _wf_slots(wf)
    S, T, F = (int(v) for v in d.shape)
    N = int(max_candidates)
    _, NT, NF = ft4_grid_shape(T, F, sps, bpt)
    p = _lib.Ft8Params()
    p.protocol, p.flags, p.sample_rate = _lib.FT8_PROTO_FT4, int(flags), 1
    p.bins_per_tone, p.steps_per_symbol, p.max_candidates = int(bpt), int(sps), N
    p.min_score_f64, p.min_score = int(min_score_is_f64(min_score)), float(min_score)
    cand = torch.zeros(S * max(N, 1) * 2, dtype=torch.int32, device=d.device)
    cs = torch.zeros(S * max(N, 1), dtype=torch.float64, device=d.device)
    cnt = torch.zeros(S, dtype=torch.int32, device=d.device)
    grid = torch.empty(max(S * NT * NF, 1), dtype=d.dtype, device=d.device) if want_grid else None
    ctx.check(_lib.lib().ft8_sync_select(ctx.handle, _lib.ptr(d), int(f64), S, T, F, ctypes.byref(p), _lib.ptr(cand),
                                         _lib.ptr(cs), _lib.ptr(cnt), _lib.ptr(grid) if want_grid else None,
                                         _lib.stream_handle()), "ft8_sync_select")
    warn = torch.zeros(S, dtype=torch.int32, device=d.device)
    if NT > 0 and NF > 0 and N > 0:
        ctx.check(_lib.lib().ft8_select_warnings(ctx.handle, _lib.ptr(warn), S, _lib.stream_handle()),
                  "ft8_select_warnings")
    c = cand.cpu().numpy().reshape(S, max(N, 1), 2)
    s = cs.cpu().numpy().reshape(S, max(N, 1))
    k = cnt.cpu().numpy()
    out = [[(int(c[b, i, 0]), int(c[b, i, 1]), float(s[b, i])) for i in range(int(k[b]))] for b in range(S)]
    g = grid[: S * NT * NF].cpu().numpy().reshape(S, NT, NF) if want_grid else None
    return out, g, warn.cpu().numpy()


def ft4_llr(wf, sps, bpt, cand_list, normalize=True):
    """ft8_ft4_llr: wf [n_slots, T, F], cand_list [(slot, abs_time, abs_freq)] -> LLRs [n, 174] (float64)."""
    torch = _lib.require_gpu()
    ctx = _lib.context()
    d, f64 = _wf_slots(wf)
    n = len(cand_list)
    if n == 0:
        return np.zeros((0, 174))
    c = torch.tensor([[int(s), int(a), int(b)] for s, a, b in cand_list], dtype=torch.int32, device=d.device)
    out = torch.empty(n, 174, dtype=torch.float64, device=d.device)
    ctx.check(_lib.lib().ft8_ft4_llr(ctx.handle, _lib.ptr(d), int(f64), int(d.shape[1]), int(d.shape[2]), int(sps),
                                     int(bpt), _lib.ptr(c), n, int(bool(normalize)), _lib.ptr(out),
                                     _lib.stream_handle()), "ft8_ft4_llr")
    return out.cpu().numpy()


def ft4_unscramble(records):
    """ft8_ft4_unscramble on a copy of `records` (_lib.RESULT_DTYPE) -> the updated records."""
    torch = _lib.require_gpu()
    ctx = _lib.context()
    rec = np.ascontiguousarray(np.asarray(records, dtype=_lib.RESULT_DTYPE).reshape(-1))
    n = len(rec)
    res = torch.from_numpy(np.concatenate([rec.view(np.uint8), np.zeros(8, np.uint8)])).cuda()
    ctx.check(_lib.lib().ft8_ft4_unscramble(ctx.handle, _lib.ptr(res), n, _lib.stream_handle()), "ft8_ft4_unscramble")
    return res.cpu().numpy()[: n * _lib.RESULT_DTYPE.itemsize].view(_lib.RESULT_DTYPE).copy()
