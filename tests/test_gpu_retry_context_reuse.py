"""One context across batches and stage calls whose retry shapes differ (csrc/capi.hip: ApRetry, CoherentRetry,
CoherentApRetry, OsdRetry).  Every pass keeps its scratch in the context, sized and sliced by the last call's
list length M, position count n_all and set count; a chunked batch, the stage calls' "one list of n", a batch
with a larger M, fewer sets and fewer slots, and the first batch again must each return what the same call
returns on a fresh context: exact, every byte."""
import numpy as np
import pytest

import ap_cases as A
import coherent_ap_cases as K
import osd_cases as C
import retry_cases as R

pytestmark = pytest.mark.gpu

FS = K.FS
LATE = dict(max_candidates=100, min_score=2)   # test_gpu_coherent_ap.py's LATE
N_STAGE = 8


def _chunked(ctx):
    """Step 1: every retry, three sets, three one-slot chunks on two streams."""
    ctx.set_pipeline(1, 2, 4)
    return R.decoder(FS, K.E2E, coherent=K.CAP, ap=K.AP, coherent_ap=True, coherent_nsym=3, osd=(2, 4), context=ctx)


def _one_chain(ctx):
    """Step 3: longer lists, one set, no OSD, one chain."""
    ctx.set_pipeline()
    return R.decoder(FS, LATE, coherent=40, coherent_nsym=1, ap=K.AP, coherent_ap=True, context=ctx)


def _batch(dec, x):
    return [r.tobytes() for r in dec.records(x)]


def _stage_calls(ctx):
    """Step 2: one small call each of the three stage calls, on the thread's context -> every returned array."""
    from ft8_demodulator_amd.ldpc_decoder import ap_decode_batch, coherent_ap_decode_batch, osd_decode_batch
    c = A.stage_case()
    idx = list(K.stage_order()[:N_STAGE])
    rec = np.array(c["plain"][idx])
    ctx.set_ap(list(c["hyps"]), 174)
    out = list(ap_decode_batch(np.array(c["llr"])[idx], rec.copy(), K.ITERS))
    out += coherent_ap_decode_batch(np.array(K.stage_llr(2)[idx]), rec.copy(), K.ITERS)
    llr, orec = C.all_vectors()
    ctx.set_osd(2, 0, 36)
    out += osd_decode_batch(np.array(llr[:N_STAGE]), np.array(orec[:N_STAGE]))
    return [np.ascontiguousarray(a).tobytes() for a in out]


def _marks(batches):
    pi = np.concatenate([np.frombuffer(b, dtype=_lib().RESULT_DTYPE)["pass_index"] for b in batches])
    return bool(((pi & 2) != 0).any()), bool(((pi >> 4) != 0).any())


def _lib():
    from ft8_demodulator_amd import _lib
    return _lib


def test_context_reused_across_retry_shapes(gpu, oracle, monkeypatch):
    _l = _lib()
    x = gpu.from_numpy(np.array(K.e2e_slots())).cuda()
    shared = _l.context(0)

    # the same calls, each on a context of its own
    want1 = _batch(_chunked(_l.Context(0)), x)
    with monkeypatch.context() as m:
        m.setitem(_l._tls.ctx, 0, _l.Context(0))     # the stage calls run on the thread's context
        want2 = _stage_calls(_l.context(0))
    want3 = _batch(_one_chain(_l.Context(0)), x[:2])
    assert _l.context(0) is shared
    for want in (want1, want3):                      # not vacuous: coherent marks and a-priori indices
        assert _marks(want) == (True, True)
    assert len(want1) == 3 and len(want3) == 2 and len(want2) == 7

    try:
        assert _batch(_chunked(shared), x) == want1
        assert _stage_calls(shared) == want2
        assert _batch(_one_chain(shared), x[:2]) == want3
        assert _batch(_chunked(shared), x) == want1
    finally:
        shared.set_pipeline()
        shared.set_ap([])
        shared.set_osd(2, 0, 36)
