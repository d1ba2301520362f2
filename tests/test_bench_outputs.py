"""bench.py's plain run and --dump-outputs: the plain line carries the headline and nothing that needs runs of its own (those are
behind --full), and the dumped arrays are the state the timed steps computed, identical from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_plain_run_times_once_and_full_keeps_the_repeats():
    a = bench.parse(["--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.repeats, a.full, a.dump_outputs) == (7, 2, 1, False, None)
    a = bench.parse(["--full"])
    assert a.full and a.repeats == 5
    assert bench.parse(["--full", "--repeats", "2"]).repeats == 2


def test_dump_outputs_writes_every_row_below_the_cap(tmp_path):
    st = np.random.default_rng(0).standard_normal((3, 1000, 3)).astype(np.float32)
    assert bench.dump_outputs(str(tmp_path), st) == 1000
    for k, name in enumerate(("pos", "vel", "acc")):
        a = np.load(tmp_path / (name + ".npy"))
        assert a.dtype == np.float32 and np.array_equal(a, st[k])


def test_dump_outputs_samples_the_same_rows_above_the_cap(tmp_path, monkeypatch):
    st = np.arange(3 * 5000 * 3, dtype=np.float32).reshape(3, 5000, 3)
    cap = 50000
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", cap)
    rows = bench.dump_outputs(str(tmp_path / "a"), st, writers=2, suffix=".rank1")
    bench.dump_outputs(str(tmp_path / "b"), st, writers=2, suffix=".rank1")
    assert 0 < rows < 5000
    total = 0
    for name in ("pos", "vel", "acc"):
        a, b = np.load(tmp_path / "a" / (name + ".rank1.npy")), np.load(tmp_path / "b" / (name + ".rank1.npy"))
        assert a.shape == (rows, 3) and np.array_equal(a, b)
        total += os.path.getsize(tmp_path / "a" / (name + ".rank1.npy"))
    assert total <= cap // 2
    idx = (np.load(tmp_path / "a" / "pos.rank1.npy")[:, 0] // 3).astype(np.int64)     # row i of pos holds 3i .. 3i+2
    assert np.all(np.diff(idx) > 0) and np.array_equal(np.load(tmp_path / "a" / "acc.rank1.npy"), st[2][idx])


@pytest.mark.gpu
def test_plain_run_dumps_the_state_of_its_timed_steps(engine_lib, tmp_path):
    """Two plain runs with --dump-outputs write the same arrays, and they are the state the same warm-up + K steps leave through
    the plain ABI, bit for bit.  The line holds the headline keys and none of what --full measures."""
    import torch
    from coulomb_oscillators_amd import Engine, EVAL_FMM_KDTREE, INTEG_LEAPFROG
    n, warm, steps = 65536, 2, 3
    outs = []
    for k in range(2):
        d = tmp_path / ("run%d" % k)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--particles", str(n), "--steps", str(steps), "--warmup", str(warm),
                            "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = r.stdout.strip().splitlines()
        assert len(lines) == 1
        out = json.loads(lines[0])
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in out, key
        assert out["steps"] == steps and out["warmup"] == warm and out["repeats"]["n"] == 1 and out["full"] is False
        assert out["value"] > 0 and out["ms_per_step"] > 0
        assert out["tree_reuse"] is None and out["late_phase"] is None and out["near_field_mutual"] is None
        assert "roofline" not in out and "cpu_baseline" not in out and "cli" not in out and "octree_traceless" not in out
        assert out["dump_outputs"]["rows"] == n
        outs.append([np.load(d / (name + ".npy")) for name in ("pos", "vel", "acc")])
    for a, b in zip(*outs):
        assert a.dtype == np.float32 and a.shape == (n, 3) and np.isfinite(a).all()
        np.testing.assert_array_equal(a, b)

    buf = torch.from_numpy(bench.gaussian_ball(n)).cuda()
    prm = torch.from_numpy(bench.coulomb_params(n)).cuda()
    e = Engine(fmm_order=6, unsort=0, tree_steps=1, sync=0)
    e.compute_force(EVAL_FMM_KDTREE, buf, n, prm)
    e.integrate_steps(INTEG_LEAPFROG, EVAL_FMM_KDTREE, buf, n, prm, 5e-4, warm)
    e.integrate_steps(INTEG_LEAPFROG, EVAL_FMM_KDTREE, buf, n, prm, 5e-4, steps)
    torch.cuda.synchronize()
    want = buf.cpu().numpy()
    e.close()
    for k in range(3):
        np.testing.assert_array_equal(outs[0][k], want[k])
