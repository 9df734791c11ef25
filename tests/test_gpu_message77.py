"""ft8_unpack77 on the device (k_unpack77, csrc/msg.hip) against the host unpacker and NumPy, and
the Python surface on top of it (SlotDecoder.texts / messages)."""
import numpy as np
import pytest

import msg77_cases as C

pytestmark = pytest.mark.gpu


def _records(payloads, ok=None):
    """[n_slots, cap, 10] payloads -> ft8_result records."""
    from ft8_demodulator_amd import _lib
    n_slots, cap = payloads.shape[:2]
    r = np.zeros((n_slots, cap), dtype=_lib.RESULT_DTYPE)
    r["payload"] = payloads
    r["ok"] = 1 if ok is None else ok
    r["slot"] = np.arange(n_slots)[:, None]
    r["cand_index"] = np.arange(cap)[None, :]
    return r


def _gpu_unpack(torch, recs, counts=None, stream=None):
    """ft8_unpack77 on records [n_slots, cap] -> ft8_text [n_slots, cap]; the output buffer starts
    as 0xA5 bytes, so a byte the kernel leaves unwritten shows."""
    from ft8_demodulator_amd import _lib
    n_slots, cap = recs.shape
    ctx = _lib.context(0)
    d_rec = torch.from_numpy(recs.reshape(-1).view(np.uint8).copy()).cuda()
    d_cnt = None if counts is None else torch.as_tensor(np.asarray(counts, dtype=np.int32)).cuda()
    d_out = torch.full((max(n_slots * cap, 1) * 64,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = _lib.lib().ft8_unpack77(ctx.handle, _lib.ptr(d_rec), None if d_cnt is None else _lib.ptr(d_cnt), n_slots, cap,
                                 _lib.ptr(d_out), stream if stream is not None else _lib.stream_handle(0))
    ctx.check(rc, "ft8_unpack77")
    torch.cuda.synchronize()
    return d_out[: n_slots * cap * 64].cpu().numpy().view(_lib.TEXT_DTYPE).reshape(n_slots, cap)


def _first_occurrence(payloads, ok, n):
    """dup_of of one slot's first n records by NumPy: the first ok record with the same 77 bits."""
    p = payloads.copy()
    p[:, 9] &= 0xF8
    dup = np.full(len(p), -1, dtype=np.int64)
    first = {}
    for r in range(n):
        if not ok[r]:
            continue
        k = p[r].tobytes()
        if k in first:
            dup[r] = first[k]
        else:
            first[k] = r
    return dup


def _host(payloads):
    from ft8_demodulator_amd import unpack77
    return unpack77(payloads.reshape(-1, 10)).reshape(payloads.shape[:-1])


# ---- 8. kernel against host ----------------------------------------------------------------------------
def test_kernel_equals_host(gpu):
    n_slots, cap = 80, 256
    fixed = C.fixed_payloads()
    pay = np.concatenate([fixed, C.random_payloads(n_slots * cap - len(fixed), seed=8)]).reshape(n_slots, cap, 10)
    assert n_slots * cap - len(fixed) >= 20000
    # duplicates to find: the tail of every slot repeats its head, and three spare bits of byte 9
    # (outside the 77) differ in some of the copies
    pay[:, 240:, :] = pay[:, :16, :]
    pay[:, 250:, 9] |= 5
    got = _gpu_unpack(gpu, _records(pay))
    want = _host(pay)
    for name in want.dtype.names:
        if name != "dup_of":
            assert np.array_equal(got[name], want[name]), name
    g = got.copy()
    g["dup_of"] = -1
    assert g.tobytes() == want.tobytes()
    # the fixed payloads came out as the CPU tests expect them
    texts = [bytes(t).rstrip(b"\0").decode() for t in got.reshape(-1)["text"][: len(fixed)]]
    assert texts[: len(C.VECTORS)] == [t for _, t in C.VECTORS]
    assert texts[len(C.VECTORS):] == [b[3] for b in C.BOUNDARY]
    ok = np.ones(cap, dtype=bool)
    for s in range(n_slots):
        assert np.array_equal(got["dup_of"][s], _first_occurrence(pay[s], ok, cap)), s
    assert (got["dup_of"][:, 240:] >= 0).all() and (got["dup_of"][:, 16:240] == -1).all()


# ---- 9. counts, ok and duplicates -----------------------------------------------------------------------
def test_counts_ok_and_duplicates(gpu):
    A, B = bytes.fromhex(C.VECTORS[0][0]), bytes.fromhex(C.VECTORS[1][0])
    pay = np.zeros((3, 5, 10), dtype=np.uint8)
    pay[:] = np.frombuffer(bytes.fromhex(C.VECTORS[2][0]), dtype=np.uint8)
    for r, p in enumerate([A, B, A, B, B]):
        pay[2, r] = np.frombuffer(p, dtype=np.uint8)
    ok = np.ones((3, 5), dtype=np.uint8)
    ok[2, 1] = 0
    got = _gpu_unpack(gpu, _records(pay, ok), counts=[0, 2, 9])
    assert got["dup_of"][2].tolist() == [-1, -1, 0, -1, 3]
    assert got["status"][2].tolist() == [0, 3, 0, 0, 0]
    assert [bytes(t).rstrip(b"\0").decode() for t in got["text"][2]] == [
        "CQ K1ABC FN42", "", "CQ K1ABC FN42", "K1ABC W9XYZ -11", "K1ABC W9XYZ -11"]
    # status 3 records: zeros but for the status, and dup_of -1
    blank = np.zeros((), dtype=got.dtype)
    blank["status"], blank["dup_of"] = 3, -1
    for s, r in [(0, r) for r in range(5)] + [(1, 2), (1, 3), (1, 4), (2, 1)]:
        assert got[s, r].tobytes() == blank.tobytes(), (s, r)
    # slot 1's two records are the same payload
    assert got["status"][1, :2].tolist() == [0, 0] and got["dup_of"][1, :2].tolist() == [-1, 0]
    # negative counts read as 0; NULL counts as cap
    got = _gpu_unpack(gpu, _records(pay, ok), counts=[-3, 5, 1])
    assert (got["status"][0] == 3).all() and (got["status"][1] == 0).all()
    assert got["status"][2].tolist() == [0, 3, 3, 3, 3]


@pytest.mark.parametrize("cap", [600, 3072, 3073])
def test_cap_above_workgroup(gpu, cap):
    """cap above the 256-lane workgroup (lanes loop), at the largest cap whose keys are staged in LDS
    (3072) and the first that reads them from the records (3073)."""
    rng = np.random.default_rng(cap)
    distinct = C.random_payloads(40, seed=cap)
    n_slots = 2
    pay = distinct[rng.integers(0, 40, size=(n_slots, cap))]
    ok = (rng.random((n_slots, cap)) < 0.9).astype(np.uint8)
    counts = [cap, cap - 7]
    got = _gpu_unpack(gpu, _records(pay, ok), counts=counts)
    want = _host(pay)
    for s in range(n_slots):
        n = counts[s]
        live = np.zeros(cap, dtype=bool)
        live[:n] = ok[s, :n] != 0
        assert np.array_equal(got["dup_of"][s], _first_occurrence(pay[s], live, n))
        assert np.array_equal(got["status"][s][~live], np.full((~live).sum(), 3))
        assert np.array_equal(got["text"][s][live], want["text"][s][live])
        assert np.array_equal(got["status"][s][live], want["status"][s][live])
        assert (got["text"][s][~live] == b"").all()


def test_unpack77_arguments(gpu):
    from ft8_demodulator_amd import _lib
    ctx = _lib.context(0)
    buf = gpu.zeros(64 * 4, dtype=gpu.uint8, device="cuda")
    L, sh = _lib.lib(), _lib.stream_handle(0)
    assert L.ft8_unpack77(ctx.handle, None, None, 0, 5, None, sh) == _lib.FT8_OK       # nothing to do
    assert L.ft8_unpack77(ctx.handle, _lib.ptr(buf), None, 2, 0, _lib.ptr(buf), sh) == _lib.FT8_OK
    assert L.ft8_unpack77(ctx.handle, None, None, 1, 1, _lib.ptr(buf), sh) == _lib.FT8_E_ARG
    assert L.ft8_unpack77(ctx.handle, _lib.ptr(buf), None, -1, 1, _lib.ptr(buf), sh) == _lib.FT8_E_ARG
    assert L.ft8_unpack77(ctx.handle, _lib.ptr(buf), None, 1, 32768, _lib.ptr(buf), sh) == _lib.FT8_E_RANGE
    assert L.ft8_unpack77(None, _lib.ptr(buf), None, 1, 1, _lib.ptr(buf), sh) == _lib.FT8_E_ARG
    gpu.cuda.synchronize()


# ---- 10. end to end --------------------------------------------------------------------------------------
SLOT_TEXTS = [["CQ PJ4/K1ABC", "CQ K1ABC FN42", "TNX BOB 73 GL"], ["K1ABC <PJ4/K1ABC> 73", "W9XYZ K1ABC R-09"]]


@pytest.fixture(scope="module")
def two_slots(gpu):
    """Two 12 kHz slots carrying SLOT_TEXTS at 600 / 1200 / 1800 Hz, noise 20 dB below each signal."""
    from ft8_demodulator_amd import _lib, pack77
    from ft8_demodulator_amd import ft8_generator as G
    fs, N = 12000, 180000
    pays = [pack77(t) for slot in SLOT_TEXTS for t in slot]
    _, _, tones = G.encode_batch(np.frombuffer(b"".join(pays), dtype=np.uint8).reshape(-1, 10))
    sig = np.zeros(len(pays), dtype=_lib.TX_SIGNAL_DTYPE)
    sig["slot"] = [s for s, slot in enumerate(SLOT_TEXTS) for _ in slot]
    sig["f0"] = [600.0 * (1 + k) for slot in SLOT_TEXTS for k in range(len(slot))]
    sig["amplitude"], sig["start"] = 1.0, fs // 2
    g = gpu.Generator(device="cuda")
    g.manual_seed(10)
    # a unit-amplitude sinusoid has power 1/2: noise 20 dB below it has variance 1/200
    x = gpu.randn((2, N), generator=g, device="cuda", dtype=gpu.float32) * float(np.sqrt(0.5 / 100.0))
    G.synthesize(tones, sig, 2, N, fs, out=x)
    return x, [[p.hex() for p in map(pack77, slot)] for slot in SLOT_TEXTS]


def _decoder():
    """SlotDecoder(12000, max_candidates=50, min_score=2) with FT8_FLAG_TOPK.

    The flag is what the slots need, at any noise level: the reference's selection keeps the first
    50 grid points that pass min_score in scan order (later ones only replace the best one kept),
    the sync score is a difference of dB values and so does not depend on the noise level, and in
    these slots 11 334 (slot 0) and 10 968 (slot 1) of the 167 728 grid points pass min_score = 2,
    the first of them at the earliest time offsets, before any signal.  The oracle's port of the
    reference decoder returns no decode at all from these slots with the noise 20, 40, 60, 80 or
    100 dB below the signals; with the 50 highest scores it returns 11 and 8 decodes of the 3 and
    2 messages."""
    from ft8_demodulator_amd import SlotDecoder, _lib
    return SlotDecoder(12000, max_candidates=50, min_score=2, flags=_lib.FT8_FLAG_TOPK)


def test_end_to_end_messages(gpu, two_slots):
    from ft8_demodulator_amd import CallsignTable
    x, payloads = two_slots
    dec = _decoder()
    # the condition: the decoder returns all five payloads at this noise level
    recs = dec.records(x)
    for s in range(2):
        assert {bytes(p).hex() for p in recs[s]["payload"]} == set(payloads[s])
    uniq = dec.messages(x, table=CallsignTable())
    assert [sorted(m[0] for m in slot) for slot in uniq] == [sorted(t) for t in SLOT_TEXTS]
    # without a table the hash stays unresolved
    plain = dec.messages(x)
    assert sorted(m[0] for m in plain[1]) == sorted(["K1ABC <...> 73", "W9XYZ K1ABC R-09"])
    every = dec.messages(x, table=CallsignTable(), unique=False)
    assert [len(slot) for slot in every] == [len(r) for r in recs]
    assert any(len(a) > len(b) for a, b in zip(every, uniq))
    assert [sorted({m[0] for m in slot}) for slot in every] == [sorted(t) for t in SLOT_TEXTS]
    # the tuples carry decode()'s time, frequency and score, and the record itself
    ref = dec.decode(x)
    for s in range(2):
        for (text, t, f, score, rec), (msg, st, t2, f2, score2) in zip(every[s], ref[s]):
            assert (t, f, score) == (t2, f2, score2) and bytes(rec["payload"]) == bytes(msg.payload)
    # texts() is aligned with records()
    texts = dec.texts(x)
    for s in range(2):
        assert len(texts[s]) == len(recs[s]) and (texts[s]["status"] == 0).all()
        first = {}
        for i, p in enumerate(recs[s]["payload"]):
            assert int(texts[s]["dup_of"][i]) == first.get(bytes(p), -1)
            first.setdefault(bytes(p), i)


# ---- 11. stream order -------------------------------------------------------------------------------------
def test_stream_order(gpu, two_slots):
    """run() then ft8_unpack77 on a non-default stream, one sync at the end, equals the synchronous
    result."""
    from ft8_demodulator_amd import _lib
    x, _ = two_slots
    dec = _decoder()
    want_recs, want_txt = dec.records(x), dec.texts(x)
    gpu.cuda.synchronize()
    dec2 = _decoder()
    side = gpu.cuda.Stream()
    d_txt = gpu.full((2 * dec2.cap * 64,), 0xA5, dtype=gpu.uint8, device="cuda")
    side.wait_stream(gpu.cuda.current_stream())
    with gpu.cuda.stream(side):
        out, counts = dec2.run(x)
        rc = _lib.lib().ft8_unpack77(dec2.ctx.handle, _lib.ptr(out), _lib.ptr(counts), 2, dec2.cap, _lib.ptr(d_txt),
                                     _lib.stream_handle(0))
        dec2.ctx.check(rc, "ft8_unpack77")
        assert _lib.stream_handle(0).value == side.cuda_stream
    side.synchronize()
    c = counts.cpu().numpy()
    txt = d_txt.cpu().numpy().view(_lib.TEXT_DTYPE).reshape(2, dec2.cap)
    rec = out[: 2 * dec2.cap * 40].cpu().numpy().view(_lib.RESULT_DTYPE).reshape(2, dec2.cap)
    for s in range(2):
        n = min(int(c[s]), dec2.cap)
        assert rec[s, :n].tobytes() == want_recs[s].tobytes()
        assert txt[s, :n].tobytes() == want_txt[s].tobytes()
        assert (txt[s, n:]["status"] == 3).all()
