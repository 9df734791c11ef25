"""The coherent pass (csrc/coherent.hip k_coherent) and the subtraction (csrc/subtract.hip k_sub_est,
k_sub_apply) on the baseband front end (csrc/baseband.h) beyond bins_per_tone = steps_per_symbol and
Q = 32: every row of tests/baseband_geometry_cases.py against the float64 restatements
(coherent.coherent_restate, oracle/subtract.py), with the bounds of the 12 kHz tests.

tests/test_baseband_geometry_cases.py states, on the CPU, which paths each row reaches and that a
transposed pair of factors or a dropped t_lo / f_lo would fail the comparisons below."""
import ctypes

import numpy as np
import pytest

import baseband_geometry_cases as B
import coherent_cases as C
import subtract_cases as S

pytestmark = pytest.mark.gpu

ROWS = B.ROWS
KEYS = ("f32", "i16")
SENTINEL = np.float32(-7.25e9)


def _L():
    from ft8_demodulator_amd import _lib
    return _lib


def _same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# ---- a. k_coherent against coherent_restate ------------------------------------------------------------
_COH = {}


def _coherent(row, key="f32", **kw):
    """coherent_llr_batch on the row's case, once per (row, key) for the plain call."""
    from ft8_demodulator_amd.ldpc_decoder import coherent_llr_batch
    g, c = B.geo(row), B.coherent_case(row)
    x = np.array(c["x"] if key == "f32" else c["pcm"])
    if kw:
        cand = kw.pop("cand", c["cand"])
        return coherent_llr_batch(x, cand, c["slot_of"], g.fs, g.bpt, g.sps, **kw)
    if (row, key) not in _COH:
        _COH[row, key] = coherent_llr_batch(x, c["cand"], c["slot_of"], g.fs, g.bpt, g.sps)
    return _COH[row, key]


@pytest.mark.parametrize("row", ROWS)
def test_coherent_equals_restatement(gpu, row):
    g = B.geo(row)
    C.check_stage(f"row {row}", _coherent(row), B.coherent_ref(row), g.fs, g.D, g.binw)


@pytest.mark.parametrize("row", B.PCM_ROWS)
def test_coherent_int16_equals_restatement(gpu, row):
    g = B.geo(row)
    C.check_stage(f"row {row} int16", _coherent(row, "i16"), B.coherent_ref(row, "i16"), g.fs, g.D, g.binw)


@pytest.mark.parametrize("row", B.DRIFT_ROWS)
def test_coherent_drift_equals_restatement(gpu, row):
    """9 rates over +-1 Hz/s: row b fills the last of the lane-owned elements of z, row e rotates z in
    rows of 26, row h in rows of 9."""
    g = B.geo(row)
    llr, fits, drifts = _coherent(row, drift=B.DRIFT)
    rllr, rfits, rdrifts, vols = B.coherent_ref(row, "f32", B.DRIFT)
    cmp_, _ = C.check_stage(f"row {row} drift", (llr, fits), (rllr, rfits, vols), g.fs, g.D, g.binw)
    assert np.array_equal(drifts["rate_index"][cmp_], rdrifts["rate_index"][cmp_])
    assert np.array_equal(drifts["rate_hz_per_s"][cmp_], rdrifts["rate_hz_per_s"][cmp_])


@pytest.mark.parametrize("row", B.NSYM_ROWS)
def test_coherent_nsym_equals_restatement(gpu, row):
    """max_nsym 3: the rotated correlations follow 8 rows of Q + 1 (row h: past the plain table's end)."""
    from test_gpu_coherent_multisym import _check_stage
    g = B.geo(row)
    _check_stage(f"row {row} nsym", _coherent(row, nsym=3), B.coherent_ref(row, "f32", None, 3), g.fs, g.D)


# ---- b. k_sub_est / k_sub_apply against oracle/subtract.py ---------------------------------------------
def _plan_params(row, masked=False, positional=False):
    from ft8_demodulator_amd._pipeline import make_params, make_plan
    g = B.geo(row)
    if masked:
        time_min, freq_min = B.mask_plan_args(row)
        plan = make_plan(g.n, g.fs, g.bpt, g.sps, freq_min=freq_min, time_min=time_min)
    elif positional:
        plan = make_plan(g.n, g.fs, g.bpt, g.sps)
    else:
        plan = make_plan(g.n, g.fs, steps_per_symbol=g.sps, bins_per_tone=g.bpt)
    assert (plan.nperseg, plan.hop, plan.nfft) == (g.nsps, g.hop, g.nfft)
    return plan, make_params(plan, 3, 2, 20, _L().FT8_FLAG_TOPK)


def _subtract(row, key="f32", masked=False, positional=False, offset=0):
    """ft8_subtract and ft8_subtract_fits on the row's lists, every list over the same samples -> (residual
    float32 [n_lists, n], fits [n_lists, 3]).  offset: the samples start that many elements into their
    allocation."""
    import torch
    _lib = _L()
    g, r = B.geo(row), B.subtract_row(row)
    recs, counts = B.subtract_records(row, B.T_LO, B.F_LO) if masked else B.subtract_records(row)
    n_lists, cap = recs.shape
    src = r["x"] if key == "f32" else r["pcm"]
    host = np.zeros(offset + n_lists * g.n, dtype=src.dtype)
    host[offset:] = np.tile(src, n_lists)
    x = torch.from_numpy(host).cuda()[offset:]
    assert x.data_ptr() % 8 == (offset * x.element_size()) % 8
    resid = torch.full((n_lists, g.n), float(SENTINEL), dtype=torch.float32, device="cuda")
    d_rec = torch.from_numpy(np.ascontiguousarray(recs).view(np.uint8).reshape(-1).copy()).cuda()
    d_cnt = torch.from_numpy(np.array(counts)).cuda()
    plan, p = _plan_params(row, masked, positional)
    if masked:
        assert (plan.t_lo, plan.f_lo) == (B.T_LO, B.F_LO) and plan.t_lo != 0 and plan.f_lo != 0
    else:
        assert (plan.t_lo, plan.f_lo) == (0, 0)
    ctx, L, st = _lib.context(), _lib.lib(), _lib.stream_handle()
    code = _lib.FT8_F32 if key == "f32" else _lib.FT8_I16
    ctx.check(L.ft8_subtract(ctx.handle, _lib.ptr(x), code, _lib.ptr(resid), g.n, n_lists, g.n, ctypes.byref(p),
                             _lib.ptr(d_rec), _lib.ptr(d_cnt), cap, st), "ft8_subtract")
    fits_d = torch.empty(n_lists * cap * _lib.SUB_FIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    ctx.check(L.ft8_subtract_fits(ctx.handle, _lib.ptr(fits_d), n_lists, cap, st), "ft8_subtract_fits")
    torch.cuda.synchronize()
    return resid.cpu().numpy(), fits_d.cpu().numpy().view(_lib.SUB_FIT_DTYPE).reshape(n_lists, cap)


_SUB = {}


def _sub(row, key="f32"):
    if (row, key) not in _SUB:
        _SUB[row, key] = _subtract(row, key)
    return _SUB[row, key]


def _x32(row, key):
    """The samples as the kernels read them (float32; int16: float32(x) / 32767)."""
    r = B.subtract_row(row)
    return r["x"] if key == "f32" else r["pcm"].astype(np.float32) / np.float32(32767.0)


def _check_subtract(row, key):
    g = B.geo(row)
    res, gfit = _sub(row, key)
    _, counts = B.subtract_records(row)
    ofits = B.subtract_fits(row, key)
    x32 = _x32(row, key)
    for s, ofit in enumerate(ofits):
        n_fits, n_off = S.check_fits(gfit[s], ofit)
        assert n_fits == int(counts[s]) and n_off <= max(1, n_fits // 20), (s, n_fits, n_off)
        # the residual against the oracle's residual of its own fits, to -40 dB of the subtracted energy
        own = B.subtract_residual(row, key, s)
        sub = np.sum((np.asarray(B.sub_host(row, key), dtype=np.float64) - own) ** 2)
        err = np.sum((res[s].astype(np.float64) - own) ** 2)
        print(f"row {row} {key} list {s}: {n_fits} fits, {n_off} with start +-1, residual error "
              f"{10 * np.log10(max(err / sub, 1e-30)):.1f} dB of the subtracted energy (bound -40)")
        assert err <= 1e-4 * sub, (s, err / sub)
        # samples no fit covers are the input's
        hit = np.zeros(g.n, dtype=bool)
        for f in gfit[s, :int(counts[s])]:
            assert f["active"]
            hit[max(int(f["start"]), 0):min(int(f["start"]) + g.L, g.n)] = True
        assert _same_bits(res[s][~hit], x32[~hit]), s
        if s == 1:
            assert (~hit).sum() > 2 * g.nsps and not hit[0] and not hit[-1]
    return gfit


@pytest.mark.parametrize("row", ROWS)
def test_subtract_equals_oracle(gpu, oracle, row):
    gfit = _check_subtract(row, "f32")
    if row == "b":      # the records moved early fit at the last of the 33 start offsets
        g = B.geo(row)
        rec = B.subtract_records(row)[0][2]
        assert [int(f["start"]) - int(q["abs_time"]) * g.hop for f, q in zip(gfit[2], rec)] == [g.Mt * g.D] * 3


@pytest.mark.parametrize("row", B.PCM_ROWS)
def test_subtract_int16_equals_oracle(gpu, oracle, row):
    _check_subtract(row, "i16")


# ---- c. vector loads that are only element-aligned ------------------------------------------------------
@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("row", B.MISALIGNED_ROWS)
def test_misaligned_samples_give_the_same_bits(gpu, row, key):
    """The slot as a view one element into its allocation: every four-sample load of bb_mix_down is
    4-byte aligned (float32) or 2-byte aligned (int16) and no better; LLRs, fits and residual equal the
    aligned upload's bit for bit."""
    from ft8_demodulator_amd.ldpc_decoder import coherent_llr_batch
    _lib = _L()
    g, c = B.geo(row), B.coherent_case(row)
    assert g.D % 4 == 0
    src = c["x"] if key == "f32" else c["pcm"]
    base = gpu.zeros(g.n + 5, dtype=gpu.float32 if key == "f32" else gpu.int16, device="cuda")
    view = base[1:1 + g.n]
    view.copy_(gpu.from_numpy(np.array(src[0])))
    align = 16 if key == "f32" else 8
    assert base.data_ptr() % align == 0 and view.data_ptr() % align == view.element_size()
    code = _lib.FT8_F32 if key == "f32" else _lib.FT8_I16
    llr, fits = coherent_llr_batch(view, c["cand"], c["slot_of"], g.fs, g.bpt, g.sps, code=code)
    want = _coherent(row, key)
    assert (want[1]["status"] == 0).sum() >= 27
    assert _same_bits(llr, want[0]) and _same_bits(fits, want[1])
    res, gfit = _subtract(row, key, offset=1)
    wres, wfit = _sub(row, key)
    assert _same_bits(res, wres)
    _, counts = B.subtract_records(row)
    for s in range(len(counts)):
        for name in gfit.dtype.names:
            assert _same_bits(gfit[s, :counts[s]][name], wfit[s, :counts[s]][name]), (s, name)


# ---- d. the factors by keyword and by position ----------------------------------------------------------
@pytest.mark.parametrize("row", B.TRANSPOSED_ROWS)
def test_factors_by_keyword(gpu, oracle, row):
    from ft8_demodulator_amd.ldpc_decoder import coherent_llr_batch
    g, c = B.geo(row), B.coherent_case(row)
    got = coherent_llr_batch(np.array(c["x"]), c["cand"], c["slot_of"], steps_per_symbol=g.sps, bins_per_tone=g.bpt,
                             sample_rate=g.fs)
    C.check_stage(f"row {row} keywords", got, B.coherent_ref(row), g.fs, g.D, g.binw)
    _check_subtract(row, "f32")                      # make_plan by keyword
    _snr_wrapper(gpu, g, True)


@pytest.mark.parametrize("row", B.TRANSPOSED_ROWS)
def test_factors_by_position(gpu, oracle, row):
    from ft8_demodulator_amd.ldpc_decoder import coherent_llr_batch
    g, c = B.geo(row), B.coherent_case(row)
    got = coherent_llr_batch(np.array(c["x"]), c["cand"], c["slot_of"], g.fs, g.bpt, g.sps)
    C.check_stage(f"row {row} positional", got, B.coherent_ref(row), g.fs, g.D, g.binw)
    _, gfit = _subtract(row, positional=True)
    for s, ofit in enumerate(B.subtract_fits(row)):
        S.check_fits(gfit[s], ofit)
    _snr_wrapper(gpu, g, False)


def _snr_wrapper(gpu, g, by_keyword):
    """snr.snr on a random waterfall against snr_reference at the row's factors."""
    from ft8_demodulator_amd import snr
    rng = np.random.default_rng(12)
    T, F = 100, 200
    wf = rng.normal(-50.0, 10.0, size=(1, T, F)).astype(np.float32)
    recs = np.zeros((1, 6), dtype=_L().RESULT_DTYPE)
    pay = rng.integers(0, 256, size=(6, 10), dtype=np.uint8)
    pay[:, 9] &= 0xF8
    recs["payload"], recs["ok"] = pay, 1
    recs["abs_time"], recs["abs_freq"] = rng.integers(1, 5, 6), rng.integers(1, F - 2 - 7 * max(g.bpt, g.sps), 6)
    d_wf = gpu.from_numpy(wf).cuda()
    if by_keyword:
        got = snr.snr(d_wf, recs, steps_per_symbol=g.sps, bins_per_tone=g.bpt, sample_rate=g.fs)
    else:
        got = snr.snr(d_wf, recs, None, None, g.fs, g.bpt, g.sps)
    want = snr.snr_reference(wf, recs, None, g.fs, g.bpt, g.sps)
    assert np.array_equal(got["status"], want["status"]) and (want["status"] < 2).all()
    np.testing.assert_allclose(got["snr_db"], want["snr_db"], rtol=0, atol=1e-6)
    assert np.array_equal(got["dt"], want["dt"]) and np.array_equal(got["df"], want["df"])


# ---- e. t_lo and f_lo ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", B.MASK_ROWS)
def test_masked_runs_give_the_same_bits(gpu, oracle, row):
    """Candidates and records numbered from frame 3 and bin 41, with t_lo = 3 and f_lo = 41: the window
    and the mix frequency are the same doubles (test_baseband_geometry_cases.py), so LLRs, fits and
    residual equal the unmasked run's bit for bit."""
    llr, fits = _coherent(row, cand=B.masked_cand(row), t_lo=B.T_LO, f_lo=B.F_LO)
    want = _coherent(row)
    assert (want[1]["status"] == 0).sum() >= 27
    assert _same_bits(llr, want[0]) and _same_bits(fits, want[1])
    res, gfit = _subtract(row, masked=True)
    wres, wfit = _sub(row)
    assert _same_bits(res, wres)
    _, counts = B.subtract_records(row)
    for s in range(len(counts)):
        assert gfit[s, :counts[s]]["active"].all()
        for name in gfit.dtype.names:
            assert _same_bits(gfit[s, :counts[s]][name], wfit[s, :counts[s]][name]), (s, name)
