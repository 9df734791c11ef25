"""FT8_FLAG_SUBTRACT with up to four passes and with the AP / coherent retries in every pass
(ft8_set_subtract, ft8_subtract_counts), pinned BY CONSTRUCTION: the expected output of a one-call batch is
rebuilt from the library's own public stage calls -- a SlotDecoder without the subtract flag per pass,
ft8_subtract in place on the rows the pass added -- and the NumPy restatement of the merge
(ft8_demodulator_amd.subtract.merge_restate), and compared byte for byte.  No tolerance anywhere.

Slots: synth.make_slots(6, 50, seed=777), the slots of test_subtract_pass2_matches_oracle (12 kHz, 15 s,
K = 300, top-k selection), chosen on an MI355X because they meet every condition the tests assert
(the docstrings give the counts); no other seed or level had to be tried."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import DATA, ROOT

pytestmark = pytest.mark.gpu

FS, K, MIN_SCORE, ITERS = 12000, 300, 2, 20
N_SLOTS, SIGNALS, SEED = 6, 50, 777
COH = dict(coherent=8)
AP_COH = dict(ap=["CQ ? ?"], coherent=8, coherent_nsym=2)
AP_REFUSED = "FT8_FLAG_AP with FT8_FLAG_SUBTRACT is not supported"
COH_REFUSED = "FT8_FLAG_COHERENT with FT8_FLAG_SUBTRACT is not supported"


def _L():
    from ft8_demodulator_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def slots(gpu):
    from ft8_demodulator_amd import synth
    x, _ = synth.make_slots(N_SLOTS, SIGNALS, seed=SEED, device="cuda")
    return x


def _host_rows(out, counts, n_slots, cap):
    """The raw output of a batch on the host: (rows [n_slots, cap], counts [n_slots])."""
    import torch
    torch.cuda.synchronize()
    dt = _L().RESULT_DTYPE
    rows = out[: n_slots * cap * dt.itemsize].cpu().numpy().view(dt).reshape(n_slots, cap).copy()
    return rows, counts.cpu().numpy().copy()


def _decoder(k=K, flags=None, **kw):
    from ft8_demodulator_amd import SlotDecoder
    lib = _L()
    return SlotDecoder(FS, 2, 2, k, MIN_SCORE, ITERS, flags=lib.FT8_FLAG_TOPK if flags is None else flags, **kw)


def _one_call(x, n, retry=None, code=None, **kw):
    """SlotDecoder(subtract=n).run -> (rows [n_slots, cap], counts, pass_counts [n_slots, n], the decoder)."""
    dec = _decoder(subtract=n, **dict(retry or {}, **kw))
    out, counts = dec.run(x, code)
    pc = dec.pass_counts()
    rows, c = _host_rows(out, counts, int(x.shape[0]), dec.cap)
    return rows, c, pc, dec


def _chain(x, n, retry=None, code=None, k_max=K):
    """n passes by construction.  Pass k: R_k = SlotDecoder(TOPK, the retry settings, no subtract flag).run
    on x_{k-1}; the accumulated list is merge_restate'd; ft8_subtract on the rows the pass added, packed
    per slot, writes x_k over x_{k-1} (d_residual == d_samples; int16 samples: pass 1 writes a float32
    buffer).  -> (acc_by_pass: per pass the list per slot of accumulated rows, counts [n_slots, n],
    fits of pass 1 [n_slots, k_max]); k_max: max_candidates."""
    import torch
    from ft8_demodulator_amd._pipeline import make_params
    from ft8_demodulator_amd.subtract import merge_restate
    lib = _L()
    n_slots, ns = int(x.shape[0]), int(x.shape[1])
    code = lib.FT8_F32 if code is None else code
    dec = _decoder(k=k_max, **(retry or {}))
    p = make_params(dec.plan(ns), k_max, MIN_SCORE, ITERS, lib.FT8_FLAG_TOPK)
    ctx, Lb, st = dec.ctx, lib.lib(), lib.stream_handle()
    cur, cur_code, resid = x, code, None
    acc, by_pass, fits1 = None, [], None
    for k in range(1, n + 1):
        out, counts = dec.run(cur, cur_code)
        rows, c = _host_rows(out, counts, n_slots, dec.cap)
        assert dec.cap == k_max and np.all(c <= k_max)
        rk = [rows[s, :c[s]] for s in range(n_slots)]
        if k == 1:
            acc = tails = rk
        else:
            new = [merge_restate(acc[s], rk[s]) for s in range(n_slots)]
            tails = [new[s][len(acc[s]):] for s in range(n_slots)]
            acc = new
        by_pass.append(acc)
        if k == n:
            break
        packed = np.zeros((n_slots, k_max), dtype=lib.RESULT_DTYPE)
        for s, t in enumerate(tails):
            packed[s, :len(t)] = t
        d_rec = torch.from_numpy(packed.view(np.uint8).reshape(-1)).cuda()
        d_cnt = torch.tensor([len(t) for t in tails], dtype=torch.int32).cuda()
        if resid is None:
            resid = x.clone() if code == lib.FT8_F32 else torch.empty(x.shape, dtype=torch.float32, device="cuda")
            src = resid if code == lib.FT8_F32 else x
        else:
            src = resid
        ctx.check(Lb.ft8_subtract(ctx.handle, lib.ptr(src), cur_code, lib.ptr(resid), ns, n_slots, ns, ctypes.byref(p),
                                  lib.ptr(d_rec), lib.ptr(d_cnt), k_max, st), "ft8_subtract")
        if k == 1:
            d_fit = torch.empty(n_slots * k_max * lib.SUB_FIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
            ctx.check(Lb.ft8_subtract_fits(ctx.handle, lib.ptr(d_fit), n_slots, k_max, st), "ft8_subtract_fits")
            torch.cuda.synchronize()
            fits1 = d_fit.cpu().numpy().view(lib.SUB_FIT_DTYPE).reshape(n_slots, k_max).copy()
        cur, cur_code = resid, lib.FT8_F32
    cum = np.array([[len(a[s]) for a in by_pass] for s in range(n_slots)], dtype=np.int32)
    return by_pass, cum, fits1


_CHAINS = {}


def _chain_of(name, x, n, retry=None):
    """The chain `name`, built once per session and never modified."""
    if name not in _CHAINS:
        _CHAINS[name] = _chain(x, n, retry)
    return _CHAINS[name]


def _same(rows, counts, pc, acc, cum, n):
    """A one-call batch of n passes against the first n passes of a chain."""
    want = acc[n - 1]
    assert pc.shape == (len(want), n) and np.array_equal(pc, cum[:, :n]), (pc.tolist(), cum[:, :n].tolist())
    for s, w in enumerate(want):
        assert int(counts[s]) == len(w) <= rows.shape[1], (s, int(counts[s]), len(w))
        assert rows[s, :len(w)].tobytes() == w.tobytes(), s


def _raw_batch(ctx, x, flags, k=K, cap=None, null_out=False):
    """ft8_decode_batch itself, on `ctx` as it stands -> (rc, rows or None, counts)."""
    import torch
    from ft8_demodulator_amd._pipeline import make_params, make_plan
    lib = _L()
    n_slots, ns = int(x.shape[0]), int(x.shape[1])
    cap = 2 * k if cap is None else cap
    p = make_params(make_plan(ns, FS, 2, 2), k, MIN_SCORE, ITERS, flags)
    out = torch.zeros(max(n_slots * cap * lib.RESULT_DTYPE.itemsize, 8), dtype=torch.uint8, device="cuda")
    counts = torch.full((n_slots,), -1, dtype=torch.int32, device="cuda")
    rc = lib.lib().ft8_decode_batch(ctx.handle, lib.ptr(x), lib.FT8_F32, ns, n_slots, ns, ctypes.byref(p),
                                    ctypes.c_void_p(0) if null_out else lib.ptr(out), lib.ptr(counts), cap,
                                    lib.stream_handle())
    if rc != lib.FT8_OK:
        return rc, None, None
    if null_out or cap == 0:
        torch.cuda.synchronize()
        return rc, None, counts.cpu().numpy().copy()
    rows, c = _host_rows(out, counts, n_slots, cap)
    return rc, rows, c


def _last_error(ctx):
    return _L().lib().ft8_last_error(ctx.handle).decode()


# ---- 1. the defaults are the parent's -------------------------------------------------------------------
def test_defaults_and_refusals(slots):
    """A TOPK | SUBTRACT batch on a context that never called ft8_set_subtract and on one set to (2, 0):
    the same rows and counts, and ft8_subtract_counts' last column is d_counts.  FT8_FLAG_AP and
    FT8_FLAG_COHERENT with FT8_FLAG_SUBTRACT are refused at (2, 0) and at (3, 0) with the message the
    pinned tests read."""
    import torch
    lib = _L()
    x = slots[:2]
    sub = lib.FT8_FLAG_TOPK | lib.FT8_FLAG_SUBTRACT
    fresh, told = lib.Context(lib.device_index()), lib.Context(lib.device_index())
    told.set_subtract(2, False)
    rc0, rows0, c0 = _raw_batch(fresh, x, sub)
    rc1, rows1, c1 = _raw_batch(told, x, sub)
    assert rc0 == rc1 == lib.FT8_OK
    assert np.array_equal(c0, c1) and rows0.tobytes() == rows1.tobytes() and np.all(c0 > 0)
    d_pc = torch.empty(2 * 2, dtype=torch.int32, device="cuda")
    fresh.check(lib.lib().ft8_subtract_counts(fresh.handle, lib.ptr(d_pc), 2, 2, lib.stream_handle()), "counts")
    pc = d_pc.cpu().numpy().reshape(2, 2)
    assert np.array_equal(pc[:, 1], c0) and np.all(pc[:, 0] <= pc[:, 1]) and np.all(pc[:, 0] > 0)
    for s in range(2):
        assert np.all(rows0[s, :pc[s, 0]]["pass_index"] & 1 == 0) and np.all(rows0[s, pc[s, 0]:c0[s]]["pass_index"] & 1 == 1)
    for n in (2, 3):
        told.set_subtract(n, False)
        for flag, text in ((lib.FT8_FLAG_AP, AP_REFUSED), (lib.FT8_FLAG_COHERENT, COH_REFUSED)):
            rc, _, _ = _raw_batch(told, x, sub | flag)
            assert rc == lib.FT8_E_UNSUPPORTED and _last_error(told) == text, (n, flag)


# ---- 2. three and four passes by construction -----------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 4])
def test_passes_by_construction(slots, n):
    """One four-pass chain; the one-call batches of 2, 3 and 4 passes equal its first n passes: raw buffer,
    counts and ft8_subtract_counts.  Rows appended per pass over the six slots of seed 777, measured on an
    MI355X (and printed): 314, 84, 11, 1 -- per slot after each pass [46, 59, 62, 62], [56, 67, 67, 67],
    [47, 60, 61, 62], [53, 70, 75, 75], [62, 79, 79, 79], [50, 63, 65, 65].  Pass 3 must append at least one
    row (it appends 11), so seed 777 stayed."""
    acc, cum, _ = _chain_of("plain4", slots, 4)
    added = np.diff(np.concatenate([np.zeros((N_SLOTS, 1), np.int32), cum], axis=1), axis=1).sum(axis=0)
    print(f"subtract passes: rows added per pass over {N_SLOTS} slots: {added.tolist()}")
    assert added[0] > 0 and added[1] > 0 and added[2] >= 1, added.tolist()
    rows, counts, pc, dec = _one_call(slots, n)
    assert dec.cap == n * K
    _same(rows, counts, pc, acc, cum, n)
    for s in range(N_SLOTS):
        assert np.all(rows[s, :cum[s, 0]]["pass_index"] == 0) and np.all(rows[s, cum[s, 0]:counts[s]]["pass_index"] == 1)


def test_passes_by_construction_int16(gpu, slots):
    """Two of the slots as int16 PCM (x / 8 of full scale): pass 1 reads the PCM, every later pass the
    float32 residual.  Measured: rows after each pass [56, 67, 67] and [47, 60, 61]."""
    import torch
    lib = _L()
    pcm = torch.clamp(torch.round(slots[1:3] / 8.0 * 32767.0), -32767, 32767).to(torch.int16)
    acc, cum, _ = _chain(pcm, 3, code=lib.FT8_I16)
    rows, counts, pc, _ = _one_call(pcm, 3, code=lib.FT8_I16)
    print(f"subtract passes int16: counts per pass {cum.tolist()}")
    assert np.all(cum[:, 0] > 0) and np.any(cum[:, 1] > cum[:, 0])
    _same(rows, counts, pc, acc, cum, 3)


# ---- 3. the retries in every pass, by construction ------------------------------------------------------
@pytest.mark.parametrize("name, retry", [("coh", COH), ("ap_coh", AP_COH)])
@pytest.mark.parametrize("n", [2, 3])
def test_retries_by_construction(slots, name, retry, n):
    """retry = 1: R_k comes from a SlotDecoder with the same retry settings and no subtract flag.  Asserted
    on the chain, i.e. on the device's own stage output: at least one pass-1 row has pass_index bit 1 (a
    coherent rescue), such a row's fit is active after the stage ft8_subtract (ft8_subtract_fits: it was
    subtracted), and at least one appended row has bits 0 and 1 both set (a rescue from a residual).
    Measured on an MI355X with make_slots' default -24 ... -10 dB (no weak signals had to be added), over
    the six slots: 40 pass-1 rows with bit 1, 9 of them the first of their payload and so fitted; rows with
    bits 0 and 1 after three passes: 38 (coherent=8) and 45 (with ap "CQ ? ?" and coherent_nsym=2); rows
    after each pass 354, 448, 473 and 354, 451, 481.  The slots' payloads are random, so "CQ ? ?" rescues
    nothing here: test_ap_rows_by_construction covers a-priori rows."""
    acc, cum, fits1 = _chain_of(name, slots, 3, retry)
    r1 = acc[0]
    coh1 = [(s, j) for s in range(N_SLOTS) for j in np.nonzero(r1[s]["pass_index"] & 2)[0]]
    fitted = [(s, j) for s, j in coh1 if fits1[s, j]["active"]]
    both = sum(int(np.sum((a["pass_index"] & 3) == 3)) for a in acc[2])
    ap_rows = sum(int(np.sum(a["pass_index"] >> 4 != 0)) for a in acc[2])
    print(f"subtract retries {name}: pass-1 coherent rows {len(coh1)} ({len(fitted)} fitted), rows with bits 0 and 1 "
          f"{both}, a-priori rows {ap_rows}, counts per pass {cum.sum(axis=0).tolist()}")
    assert len(coh1) >= 1 and len(fitted) >= 1 and both >= 1
    for s in range(N_SLOTS):   # every listed pass-1 row is active exactly where it is ok and first of its payload
        seen = set()
        for j, r in enumerate(r1[s]):
            first = bool(r["ok"]) and bytes(r["payload"]) not in seen
            seen.add(bytes(r["payload"]))
            assert bool(fits1[s, j]["active"]) == first, (s, j)
    rows, counts, pc, _ = _one_call(slots, n, retry)
    _same(rows, counts, pc, acc, cum, n)


def test_ap_rows_by_construction(gpu):
    """The two slots of test_gpu_ap.py's end-to-end case (K = 40; weak "CQ <call> <grid>" signals around the
    plain threshold) with ap = ["CQ ? ?"] in each of three passes.  test_gpu_ap.py pins that slot 0's pass 1
    holds at least two a-priori decodes; here such a row (high nibble of pass_index set) must be in pass 1,
    its fit must be active after the stage ft8_subtract, and every appended row keeps its nibble next to
    bit 0 (the byte-for-byte comparison).  Measured: 4 a-priori rows among slot 0's 6, none appended later
    (rows after each pass [6, 6, 6] and [0, 0, 0]): the later passes run, and find nothing, on a slot of eight
    signals."""
    import ap_cases as AC
    x = gpu.from_numpy(np.array(AC.e2e_samples())).cuda()
    retry = dict(ap=["CQ ? ?"])
    acc, cum, fits1 = _chain(x, 3, retry, k_max=40)
    ap1 = [(s, j) for s in range(2) for j in np.nonzero(acc[0][s]["pass_index"] >> 4)[0]]
    later = sum(int(np.sum((a["pass_index"] >> 4 != 0) & (a["pass_index"] & 1 == 1))) for a in acc[2])
    print(f"subtract retries ap: pass-1 a-priori rows {len(ap1)}, appended a-priori rows {later}, counts per pass "
          f"{cum.tolist()}")
    assert len(ap1) >= 1 and any(fits1[s, j]["active"] for s, j in ap1)
    rows, counts, pc, _ = _one_call(x, 3, retry, k=40)
    _same(rows, counts, pc, acc, cum, 3)


# ---- 4. pipelining ----------------------------------------------------------------------------------------
def test_pipelined_batch_is_identical(slots):
    """The three-pass coherent batch under ft8_set_pipeline(1, 2, 4) (six chunks over two streams, in
    every pass) on a context of its own: the chain's bytes."""
    lib = _L()
    acc, cum, _ = _chain_of("coh", slots, 3, COH)
    ctx = lib.Context(lib.device_index())
    ctx.set_pipeline(1, 2, 4)
    rows, counts, pc, _ = _one_call(slots, 3, COH, context=ctx)
    _same(rows, counts, pc, acc, cum, 3)


# ---- 5. capacity ------------------------------------------------------------------------------------------
def test_capacity(slots):
    """cap = the pass-1 rows of the slot the later passes add most to, + 1: every slot's rows are the first
    cap of the chain's, the counts stay uncapped (ft8_subtract_counts too).  cap = 0 with a null output:
    the counts alone."""
    lib = _L()
    acc, cum, _ = _chain_of("plain4", slots, 4)
    s0 = int(np.argmax(cum[:, 2] - cum[:, 0]))
    cap = int(cum[s0, 0]) + 1
    assert cum[s0, 2] > cap    # that slot is truncated inside what the later passes appended
    rows, counts, pc, dec = _one_call(slots, 3, max_results_per_slot=cap)
    assert dec.cap == cap and np.array_equal(counts, cum[:, 2]) and np.array_equal(pc, cum[:, :3])
    for s in range(N_SLOTS):
        w = acc[2][s][:cap]
        assert rows[s, :len(w)].tobytes() == w.tobytes(), s
    ctx = lib.Context(lib.device_index())
    ctx.set_subtract(3, False)
    rc, _, c = _raw_batch(ctx, slots, lib.FT8_FLAG_TOPK | lib.FT8_FLAG_SUBTRACT, cap=0, null_out=True)
    assert rc == lib.FT8_OK and np.array_equal(c, cum[:, 2])


# ---- 6. noise -----------------------------------------------------------------------------------------------
def test_noise_decodes_nothing(gpu):
    """8 noise-only slots, K = 40, four passes with coherent = 8: no row in any pass (DESIGN section 12
    measured 0 false decodes in 76 800 coherent attempts on noise, so the expected value is 0)."""
    from ft8_demodulator_amd import synth
    x = synth.make_slots(8, 0, seed=4100)[0].cuda()
    dec = _decoder(k=40, subtract=4, coherent=8)
    out, counts = dec.run(x)
    pc = dec.pass_counts()
    assert pc.shape == (8, 4) and not pc.any() and not counts.cpu().numpy().any()


# ---- 7. errors ----------------------------------------------------------------------------------------------
def test_errors(slots):
    import torch
    lib = _L()
    Lb, st = lib.lib(), lib.stream_handle()
    x = slots[:1]
    sub = lib.FT8_FLAG_TOPK | lib.FT8_FLAG_SUBTRACT
    ctx = lib.Context(lib.device_index())
    ctx.set_subtract(3, True)
    for bad in ((1, 0), (5, 0), (2, 2), (0, 1), (3, -1)):
        assert Lb.ft8_set_subtract(ctx.handle, *bad) == lib.FT8_E_ARG, bad
    with pytest.raises(ValueError):
        ctx.set_subtract(5)
    ctx.set_coherent(8)
    rc, rows, c = _raw_batch(ctx, x, sub | lib.FT8_FLAG_COHERENT, cap=3 * K)   # still (3, 1): not refused
    assert rc == lib.FT8_OK and c[0] > 0
    d_pc = torch.empty(8, dtype=torch.int32, device="cuda")
    assert Lb.ft8_subtract_counts(ctx.handle, lib.ptr(d_pc), 1, 3, st) == lib.FT8_OK   # ... and three passes
    torch.cuda.synchronize()
    assert int(d_pc[2]) == int(c[0])
    for shape in ((1, 2), (2, 3), (1, 4)):
        assert Lb.ft8_subtract_counts(ctx.handle, lib.ptr(d_pc), *shape, st) == lib.FT8_E_ARG, shape
    d_fit = torch.empty(K * lib.SUB_FIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    assert Lb.ft8_subtract_fits(ctx.handle, lib.ptr(d_fit), 1, K, st) == lib.FT8_E_ARG      # after three passes
    assert Lb.ft8_subtract_fits(ctx.handle, lib.ptr(d_fit), 1, 2 * K, st) == lib.FT8_E_ARG
    ctx.set_subtract(2, False)
    rc, _, _ = _raw_batch(ctx, x, sub)
    assert rc == lib.FT8_OK
    assert Lb.ft8_subtract_fits(ctx.handle, lib.ptr(d_fit), 1, K, st) == lib.FT8_OK         # after two: pass 1's
    rc, _, _ = _raw_batch(ctx, x, lib.FT8_FLAG_TOPK)
    assert rc == lib.FT8_OK
    assert Lb.ft8_subtract_counts(ctx.handle, lib.ptr(d_pc), 1, 2, st) == lib.FT8_E_ARG      # after a plain batch
    torch.cuda.synchronize()
    for bad in (5, 1, 2.5):
        with pytest.raises(ValueError):
            _decoder(subtract=bad)
    with pytest.raises(NotImplementedError):
        _decoder(subtract=3).snr(x)


# ---- 8. the Python surface ------------------------------------------------------------------------------------
def test_python_surface(slots):
    """SlotDecoder(subtract=3, coherent=8).messages and .pass_counts agree with the chain; a decoder built
    the old way on the same (shared) context afterwards still refuses the retries; decode_ft8_message
    (subtract=3) gives slot 0's three plain passes."""
    from ft8_demodulator_amd import decode_ft8_message
    from ft8_demodulator_amd.subtract import pass_of, subtract_index
    lib = _L()
    acc, cum, _ = _chain_of("coh", slots, 3, COH)
    dec = _decoder(subtract=3, coherent=8)
    msgs = dec.messages(slots, unique=False)
    pc = dec.pass_counts()
    assert np.array_equal(pc, cum)
    for s in range(N_SLOTS):
        recs = [m[-1] for m in msgs[s]]
        assert len(recs) <= len(acc[2][s])
        want = {r.tobytes() for r in acc[2][s]}
        assert all(r.tobytes() in want for r in recs)
        for i, r in enumerate(acc[2][s]):
            assert (pass_of(pc[s], i) > 1) == bool(subtract_index(r))
    old = _decoder(flags=lib.FT8_FLAG_TOPK | lib.FT8_FLAG_SUBTRACT | lib.FT8_FLAG_COHERENT, context=dec.ctx)
    with pytest.raises(NotImplementedError, match=COH_REFUSED):
        old.run(slots[:1])
    plain, pcum, _ = _chain_of("plain4", slots, 4)
    res = decode_ft8_message(slots[0], FS, 2, 2, K, MIN_SCORE, ITERS, selection="topk", subtract=3)
    assert [bytes(m.payload) for m, *_ in res] == [bytes(r["payload"]) for r in plain[2][0]]


def test_cli_matches_api(gpu):
    """python -m ft8_demodulator_amd.from_wave tests/data/synth_cfg2.wav --selection topk --subtract 3 prints
    the payloads decode_ft8_message(selection="topk", subtract=3) returns for the file, in order."""
    from ft8_demodulator_amd import decode_ft8_message, read_wave_file
    wav = os.path.join(DATA, "synth_cfg2.wav")
    x, fs = read_wave_file(wav)
    api = [bytes(m.payload).hex() for m, *_ in decode_ft8_message(x, fs, selection="topk", subtract=3)]
    assert api
    r = subprocess.run([sys.executable, "-m", "ft8_demodulator_amd.from_wave", wav, "--selection", "topk",
                        "--subtract", "3"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    cli = [line.split()[1] for line in r.stdout.splitlines() if line.startswith("Payload:")]
    assert cli == api
