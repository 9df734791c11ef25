"""The plain benchmark run (`bench.py --gpus 1 --steps K --warmup W`, no --full) end to end on a
small batch: the line's contract fields, nothing of a --full run measured, and --dump-outputs
holding exactly what a SlotDecoder returns for the same seeded slots."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, K, W = 8, 2, 1


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(gpu, tmp_path):
    from ft8_demodulator_amd import SlotDecoder, synth
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", str(W),
           "--slots", str(S), "--settle_max", "0", "--dump-outputs", str(out),
           "--legs-out", str(tmp_path / "legs.json")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["full"] is False and d["steps"] == K and d["warmup"] == W and d["n_gpus"] == 1
    assert d["unit"] == "slots/s" and d["higher_is_better"] is True and d["dtype"].startswith("f32")
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(S / (d["ms_per_step"] * 1e-3), rel=1e-4)
    assert d["cpu_baseline"] is None and d["parity"] is None and d["roofline"].get("launch_ms") is None
    assert d["depth"]["one_chain_value"] is None and "legs_summary" not in d
    with open(tmp_path / "legs.json") as f:
        legs = json.load(f)
    assert len(legs["step_times"]["ms"]) == K          # --steps sets the number of timed steps
    assert "stages_ms" not in legs and "bp_stress" not in legs

    # the same slots (per-slot seeds 100000 + slot, synthesised on the CPU) through a decoder here
    x, _ = synth.make_slots(S, 50, fs=12000, snr_db=(-24.0, -10.0), seeds=[100000 + b for b in range(S)], device="cpu")
    dec = SlotDecoder(12000, 2, 2, max_candidates=300, min_score=2, max_iterations=20, device=gpu.device("cuda", 0))
    recs = dec.records(x.to("cuda:0"))
    got = {n[:-4]: np.load(out / n) for n in os.listdir(out)}
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["counts"].tolist() == [len(r_) for r_ in recs] and d["decodes_per_step"] == sum(len(r_) for r_ in recs)
    assert got["kept_slots"].tolist() == list(range(S))
    for s, r_ in enumerate(recs):
        n = len(r_)
        for name in r_.dtype.names:
            assert np.array_equal(got[name][s, :n], r_[name].astype(np.float64)), (s, name)
            assert not got[name][s, n:].any(), (s, name)
