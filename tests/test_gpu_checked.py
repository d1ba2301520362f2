"""The checked build (libnbco_hip_checked.so: every index a kernel reads from a list is range-checked on the device) under
NBCO_POISON=1 (every new scratch allocation filled with 0x7f bytes, the way a recycled allocation holds stale data).

Background (post-mortem of round 1's abort): a traversal that overflowed a frontier region left the region's tail
unwritten, the next launch read it up to its capacity and classified whatever the recycled buffer held -- node ids of a deeper
tree -- and faulted.  A fresh process gets zero-filled memory, which is why the test passed when it was run alone.  The poisoned
allocations make that situation deterministic, the device-side checks turn any such read into a count instead of a fault.

Part 3 of the script puts the walks of tests/test_gpu_context_reuse.py that aim at stale launch estimates and shared scratch (its
parts A, first alternation, and D) through the same build: a stale index then shows up as a count in one of the eight sites.

test_checked_build_runs_the_snapshot_sequences puts the drivers of tests/test_gpu_snapshots.py and tests/test_gpu_snapshot_series.py
-- every diagnostic on one long-lived context, at an n smaller than one the context has seen -- through the same build: the walks of
the probes, the pair statistics, the bond order and the potential pass report to the site NBCO_CHK_WALK, the slice and aperture
kernels to NBCO_CHK_GROUP, and under NBCO_POISON the block of device scalars (`small`) and the partial-sum buffers of the wave-vector
sums and the time correlations start as 0x7f bytes as well.

Each of the two tests runs once, in a subprocess of its own (the checked library is selected with NBCO_LIB before the package loads)."""
import json
import os
import subprocess
import sys
import textwrap

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECKED = os.path.join(ROOT, "coulomb_oscillators_amd", "libnbco_hip_checked.so")

SCRIPT = textwrap.dedent('''
    import json, sys
    import numpy as np, torch
    sys.path.insert(0, %r)
    from coulomb_oscillators_amd import Engine, EngineError, LoopbackWorld, EVAL_FMM_KDTREE, INTEG_LEAPFROG, lib_path
    from oracle.pyoracle import Oracle
    assert lib_path().endswith("libnbco_hip_checked.so")
    o = Oracle(np.float32)
    out = {}
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()

    # 1. the overflow of round 1: one region of list_factor * nodes / 8 pairs, growth off
    n, p = 65536, 6
    buf, par = o.init_reference(n), dev(o.params(n))
    big = Engine(fmm_order=p, unsort=0)                      # leaves node ids of a deeper tree behind in the allocator's pool
    dbig = dev(o.init_reference(1 << 20))
    big.compute_force(EVAL_FMM_KDTREE, dbig, 1 << 20, dev(o.params(1 << 20)))
    torch.cuda.synchronize()
    big.close(); del dbig
    e = Engine(fmm_order=p, unsort=0, list_factor=1, list_grow=0)
    d = dev(buf[:2]); before = d.clone()
    a = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    try:
        e.fmm_cart3_kdtree(d, a, n, par)
        out["overflow_reported"] = False
    except EngineError as err:
        out["overflow_reported"] = "list capacity" in str(err)
    torch.cuda.synchronize()
    out["state_untouched"] = bool(torch.equal(d, before))
    out["violations_after_overflow"] = e.violations()
    e.set(list_factor=48, list_grow=1)
    e.fmm_cart3_kdtree(d, a, n, par)                          # the context keeps working
    torch.cuda.synchronize()
    _, a_ref = o.fmm_kd(buf[:2], o.params(n), p=p, threads=8, unsort=False)
    mag = np.linalg.norm(a_ref, axis=1)
    out["err_after_recovery"] = float((np.linalg.norm(a.cpu().numpy() - a_ref, axis=1) / (mag + mag.mean())).max())
    e.close()

    # 2. the production paths: both near-field kernels, tree reuse, caller's order, odd sizes, octree, two kd-domains
    for (nn, pp, kw) in ((65536, 6, dict(unsort=0, tree_steps=4, p2p_mutual=1)), (65536, 6, dict(unsort=0, p2p_mutual=0)), (5000, 4, dict(unsort=1)),
                         (30001, 5, dict(unsort=1, p2p_mutual=1)), (100000, 6, dict(unsort=0, p2p_mutual=1)), (4097, 3, dict(unsort=0, tree_steps=2))):
        b, pr = dev(o.init_reference(nn)), dev(o.params(nn))
        en = Engine(fmm_order=pp, **kw)
        en.compute_force(EVAL_FMM_KDTREE, b, nn, pr)
        for _ in range(3):
            en.integrate(INTEG_LEAPFROG, EVAL_FMM_KDTREE, b, nn, pr, 5e-4)
        torch.cuda.synchronize()
        assert torch.isfinite(b).all()
        en.close()
    nn = 20000
    b = dev(o.init_reference(nn, test_mode=True)[:2]); acc = torch.zeros((nn, 3), device="cuda")
    en = Engine(fmm_order=6)
    en.fmm_cart3_traceless(b, acc, nn, dev(o.params(nn)))
    torch.cuda.synchronize()
    assert torch.isfinite(acc).all()
    nn = 32768
    st = o.init_reference(nn)
    w = LoopbackWorld([Engine(fmm_order=6, unsort=0, p2p_mutual=1) for _ in range(2)], nn)
    h = nn // 2
    w.partition([dev(st[0][:h]), dev(st[0][h:])], [dev(st[1][:h]), dev(st[1][h:])])
    w.force(dev(o.params(nn)), elastic=False)
    torch.cuda.synchronize()
    assert all(torch.isfinite(r.acc).all() for r in w.runs)
    out["violations_total"] = en.violations()

    # 3. one long-lived context (tests/test_gpu_context_reuse.py): the launch estimate taken from a small evaluation in front of
    #    each large one, so that the waves of the near-field kernel take later work units through their prefetching hand-off, and
    #    a reuse schedule with other calls of the same context between its steps -- each with that module's own assertions
    sys.path.insert(0, %r)
    import test_gpu_context_reuse as T
    T.run_alternation(o, T.VARIANTS["one_directional"])
    out["interrupted_schedule_identical"] = True
    for mutual in (0, 1):
        opts = dict(T.NBCO3, p2p_mutual=mutual)
        plain = T.run_schedule(o, opts)
        for block, interrupted in ((0, True), (4, False), (4, True)):     # as test_calls_in_between_do_not_disturb_a_schedule
            same = bool(torch.equal(T.run_schedule(o, opts, block=block, interrupted=interrupted), plain))
            out["interrupted_schedule_identical"] = out["interrupted_schedule_identical"] and same
            out["schedule mutual {} block {} interrupted {}".format(mutual, block, interrupted)] = same
    last = Engine()
    out["violations_context_reuse"] = last.violations()
    print(json.dumps(out))
''') % (ROOT, os.path.join(ROOT, "tests"))


def test_checked_build_with_poisoned_allocations():
    if not os.path.exists(CHECKED):
        pytest.fail("libnbco_hip_checked.so is not built (make -C coulomb_oscillators_amd/csrc)")
    env = dict(os.environ, NBCO_LIB=CHECKED, NBCO_POISON="1")
    r = subprocess.run([sys.executable, "-c", SCRIPT], capture_output=True, text=True, env=env, timeout=2400)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["overflow_reported"] and out["state_untouched"]
    assert out["violations_after_overflow"] == [0] * 8, out       # no launch read a slot that nothing had written
    assert out["err_after_recovery"] < 1e-5
    assert out["violations_total"] == [0] * 8, out
    assert out["interrupted_schedule_identical"], out
    assert out["violations_context_reuse"] == [0] * 8, out


SNAPSHOT_SCRIPT = textwrap.dedent('''
    import json, sys
    import numpy as np, torch
    sys.path.insert(0, %r)
    sys.path.insert(0, %r)
    from coulomb_oscillators_amd import Engine, EVAL_FMM_KDTREE, Q_Z, lib_path
    from oracle.pyoracle import Oracle
    assert lib_path().endswith("libnbco_hip_checked.so")
    o = Oracle(np.float32)
    out = {}
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()

    # 1. something in the allocator's pool: node ids and tables of a deeper tree, and of 4096 slices
    n = 1 << 18
    big = Engine(fmm_order=4, unsort=1)
    d, prm = dev(o.init_reference(n)), dev(o.params(n))
    t = d[0][:300] * 1.2
    big.compute_force(EVAL_FMM_KDTREE, d, n, prm)
    big.energy_tree(d, n, prm, torch.zeros(n, dtype=torch.float64, device="cuda"))
    big.probe_tree(d, n, t, 300, prm, torch.zeros((300, 3), dtype=torch.float64, device="cuda"), torch.zeros(300, dtype=torch.float64, device="cuda"))
    big.pair_hist_tree(d, n, 64, 0.0005, nn2=torch.zeros(n, dtype=torch.float64, device="cuda"))
    big.slice_moments(d, n, (Q_Z, 4096, -0.03, 0.03))
    torch.cuda.synchronize()
    out["violations_big"] = big.violations()
    big.close(); del d, t

    # 2. the drivers of tests/test_gpu_snapshots.py and tests/test_gpu_snapshot_series.py, with those modules' own assertions
    import test_gpu_snapshots as T
    T.drive_a(o)
    out["violations_a"] = Engine().violations()
    T.run_size_walk_3d(o)
    T.run_size_walk_2d()
    out["violations_b"] = Engine().violations()
    T.drive_c()
    out["violations_c"] = Engine().violations()
    import test_gpu_snapshot_series as S
    S.drive_series_a(o)
    S.run_shape_walk()

    # 3. the counts of every site, all contexts of the process together
    out["violations"] = Engine().violations()
    print(json.dumps(out))
''') % (ROOT, os.path.join(ROOT, "tests"))


def test_checked_build_runs_the_snapshot_sequences():
    """the snapshot sequences and size walks of tests/test_gpu_snapshots.py and the drivers of tests/test_gpu_snapshot_series.py on the
    checked build with poisoned allocations, behind a context that left a deeper tree's tables in the allocator's pool: every
    assertion of those modules holds and no site has counted"""
    if not os.path.exists(CHECKED):
        pytest.fail("libnbco_hip_checked.so is not built (make -C coulomb_oscillators_amd/csrc)")
    env = dict(os.environ, NBCO_LIB=CHECKED, NBCO_POISON="1")
    r = subprocess.run([sys.executable, "-c", SNAPSHOT_SCRIPT], capture_output=True, text=True, env=env, timeout=1800)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["violations"] == [0] * 8, out


def test_production_build_has_no_checks(engine):
    from coulomb_oscillators_amd import EngineError
    with pytest.raises(EngineError, match="not the checked build"):
        engine.violations()
