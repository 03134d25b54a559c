"""bench.py's multi-GPU launcher on CPU: ``--gpus 2`` outside a launcher
starts two rank processes itself (torch.distributed.run, gloo here) and
rank 0 reports the world size it joined.  No engine, no measurement.
Then the plain run's contract: what --full switches, what --dump-outputs
writes, and (on the GPU) the line and files of one short plain run."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                       timeout=240, env=env, cwd="/tmp")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_spawns_n_ranks():
    out = _run(["--gpus", "2", "--selftest-cpu", "--backend", "gloo"])
    assert out["n_gpus"] == 2 and out["rank_sum"] == 1.0


def test_bench_single_rank_no_launcher():
    out = _run(["--gpus", "1", "--selftest-cpu", "--backend", "gloo"])
    assert out["n_gpus"] == 1


LEGS = ("config_legs", "read_shard", "exact", "host_inclusive", "cpu_baseline")


def test_plain_run_measures_the_headline_only(monkeypatch):
    """Without --full every side leg and the roofline stamps are off; with it
    each leg is on again under its own switch."""
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert not a.full and a.steps == 7 and a.warmup == 2 and a.dump_outputs is None
    assert all(getattr(a, k) == 0 for k in LEGS) and a.no_roofline
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--exact", "0"])
    a = bench.parse()
    assert a.full and not a.no_roofline and a.exact == 0
    assert all(getattr(a, k) == 1 for k in LEGS if k != "exact")


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    """A plain run on the GPU: --steps sets the timed calls, the line carries
    the headline fields and none of the --full legs, and --dump-outputs writes
    the last timed call's tokens and scores in float32."""
    import numpy as np
    out = _run(["--gpus", "1", "--steps", "4", "--warmup", "3", "--dump-outputs", str(tmp_path / "o")])
    assert out["steps"] == 4 and out["warmup"] == 3 and out["higher_is_better"] is True
    assert out["ms_per_step"] > 0 and out["unit"] == "samples/s" and out["dtype"].startswith("f32")
    assert abs(out["value"] - 256 * 512 / (out["ms_per_step"] * 1e-3)) <= 1e-3 * out["value"]
    for leg in ("pool_check", "one_call_in_flight", "roofline", "exact_fp32", "config_legs", "cpu_baseline"):
        assert leg not in out
    tok, sc = np.load(tmp_path / "o" / "tokens.npy"), np.load(tmp_path / "o" / "scores.npy")
    assert tok.dtype == np.float32 and tok.shape == (256, 100) and sc.dtype == np.float32 and sc.shape == (256,)
    assert np.isfinite(sc).all() and (tok == np.round(tok)).all() and tok.min() >= 0


def test_dump_outputs_writes_float32_arrays(tmp_path):
    """--dump-outputs: one float32 .npy per tensor of the call's result dict,
    integer ids exact, entries that are not tensors left out."""
    import numpy as np
    import torch

    import bench
    out = {"tokens": torch.arange(12, dtype=torch.int32).reshape(3, 4), "scores": torch.tensor([-1.5, 0.25, 3.0]),
           "logp": None, "overflow": 0}
    d = tmp_path / "dump" / "deep"
    bench.dump_outputs(str(d), out)
    assert sorted(p.name for p in d.iterdir()) == ["scores.npy", "tokens.npy"]
    tok, sc = np.load(d / "tokens.npy"), np.load(d / "scores.npy")
    assert tok.dtype == np.float32 and sc.dtype == np.float32
    assert np.array_equal(tok, np.arange(12).reshape(3, 4)) and np.array_equal(sc, [-1.5, 0.25, 3.0])
