"""GPU tests of the 3-D probes: nbco_probe (Engine.probe: the exact sums), nbco_kd_probe (Engine.probe_kd: the walk over the tree of
the last kd-tree evaluation, csrc/kd_probe_kernels.hpp) and nbco_probe_tree (Engine.probe_tree: the same behind a tree of its own
on a private context).  Yardsticks: the fp64 sums and the numpy restatement of the walk (tests/probe3d_numpy.py) fed with the
device tree, which reproduces every acceptance decision, so that the two sides differ by fp64 rounding alone."""
import numpy as np
import pytest

import probe3d_numpy as p3
import shapes3d

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = 2, 4
EPS2 = 1e-18


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def nan_out(m):
    import torch
    return (torch.full((m, 3), float("nan"), dtype=torch.float64, device="cuda"),
            torch.full((m,), float("nan"), dtype=torch.float64, device="cuda"))


@pytest.fixture(scope="module")
def states(oracle32):
    """initial states and parameter packs by n, made once"""
    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = (oracle32.init_reference(n), oracle32.params(n))
        return cache[n][0].copy(), cache[n][1]
    return get


def run(fn, *args, want_a=True, want_psi=True):
    """(a, psi) on the host from fn(*args, a, psi) with NaN-filled outputs: every slot must have been written"""
    m = args[-2]
    a, psi = nan_out(m)
    fn(*args, a if want_a else None, psi if want_psi else None)
    a, psi = a.cpu().numpy(), psi.cpu().numpy()
    assert not want_a or np.isfinite(a).all()
    assert not want_psi or np.isfinite(psi).all()
    return a, psi


# ---- the exact call ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps2", [1e-18, 1e-4])
def test_probe_is_the_exact_sum_at_every_launch_shape(engine, states, eps2):
    """n in {1, 2, 63, 64, 65, 257, 4097} x m in {1, 63, 64, 65, 257}, probes half on sources (where n allows) and half off them:
    field within 1e-12 of max_i sum_j |term|, psi within 1e-12 of max_i psi_i (its terms are positive)"""
    buf, par = states(4097)
    engine.set(eps2=eps2)
    prm = dev(par)
    rng = np.random.default_rng(11)
    R = float(np.abs(buf[0]).max())
    worst = 0.0
    for n in (1, 2, 63, 64, 65, 257, 4097):
        x = buf[0][:n]
        for m in (1, 63, 64, 65, 257):
            t = (R * rng.uniform(-1.5, 1.5, (m, 3))).astype(np.float32)
            on = np.arange(0, m, 2)
            t[on] = x[on % n]
            a, psi = run(engine.probe, dev(x), n, dev(t), m, prm)
            ea, epsi, mag = p3.exact(x, t, eps2, with_abs=True)
            ea, epsi, mag = ea * float(par[0]), epsi * float(par[0]), mag * float(par[0])
            ea_, epsi_ = np.abs(a - ea).max(), np.abs(psi - epsi).max()
            assert ea_ <= 1e-12 * mag.max() and epsi_ <= 1e-12 * epsi.max(), (n, m, ea_, mag.max(), epsi_, epsi.max())
            if mag.max() > 0:                                      # (n = 1 with every probe on the source: nothing to divide by)
                worst = max(worst, ea_ / mag.max(), epsi_ / epsi.max())
    print("eps2 = %g: worst deviation of nbco_probe from the fp64 sums %.2e" % (eps2, worst))


def test_probe_on_duplicated_points(engine, states):
    """sources 16 to a place, probes on them: 16 / sqrt(eps2) in psi from the place, nothing in a"""
    n = 4096
    buf, par = states(n)
    x = np.repeat(buf[0][:n // 16], 16, axis=0)
    prm = dev(par)
    for eps2 in (1e-18, 1e-4):
        engine.set(eps2=eps2)
        t = x[::5].copy()
        m = len(t)
        a, psi = run(engine.probe, dev(x), n, dev(t), m, prm)
        ea, epsi, mag = p3.exact(x, t, eps2, with_abs=True)
        assert np.abs(a - ea * float(par[0])).max() <= 1e-12 * mag.max() * float(par[0])
        assert np.abs(psi - epsi * float(par[0])).max() <= 1e-12 * epsi.max() * float(par[0])
        assert (psi >= 16 * float(par[0]) / np.sqrt(float(np.float32(eps2))) * (1 - 1e-12)).all()


def test_probe_at_the_particles_against_direct3_and_energy_tree(engine, states):
    """t = p at EPS2 = 1e-4: the field is direct3's at fp32 rounding; psi less the self term is energy_tree's phi_dev with
    tree_radius = 1e6 (all near field) to 1e-10"""
    import torch
    n, eps2 = 3000, 1e-4
    buf, par = states(n)
    engine.set(eps2=eps2, fmm_order=4, tree_radius=1e6, unsort=1)
    d, prm = dev(buf), dev(par)
    a, psi = run(engine.probe, d[0], n, d[0], n, prm)
    a3 = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    engine.direct3(d[0], a3, n, prm)
    a3 = a3.cpu().numpy().astype(np.float64)
    # direct3 forms every term in fp32 (three differences, r^2, rsqrt, its cube, the product: under 8 roundings) and sums with
    # compensation: within 8 eps32 of sum_j |term|
    mag = p3.exact(buf[0], buf[0], eps2, with_abs=True)[2] * float(par[0])
    assert np.abs(a - a3).max() <= 8 * np.finfo(np.float32).eps * mag.max()
    phi = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    engine.energy_tree(d, n, prm, phi)
    phi = phi.cpu().numpy()
    self_term = float(par[0]) / np.sqrt(float(np.float32(eps2)))
    assert np.abs((psi - self_term) - phi).max() <= 1e-10 * np.abs(phi).max()


# ---- the walk against the restatement on the device tree ---------------------------------------------------------------------------
WALK_CASES = {
    "n64_p1": dict(n=64, p=1),
    "n4096_p3": dict(n=4096, p=3),
    "n3000_p6": dict(n=3000, p=6),
    "n20000_p6": dict(n=20000, p=6),
    "n30001_p10_fp64": dict(n=30001, p=10, far_fp64=1),            # leaves of ~117: the staging tiles
    "n3000_p6_L2": dict(n=3000, p=6, tree_L=2),                    # 750 per leaf
    "n3000_p6_tree_order": dict(n=3000, p=6, unsort=0),
    "n4096_p3_m2l_first": dict(n=4096, p=3, m2l_first=1),
    "n20000_p6_mutual": dict(n=20000, p=6, p2p_mutual=1, unsort=0),
    "n3000_p6_stale_boxes": dict(n=3000, p=6, unsort=0, tree_steps=8, steps=2),
    "n3000_p6_radius2": dict(n=3000, p=6, tree_radius=2.0),
    "n3000_p6_radius05": dict(n=3000, p=6, tree_radius=0.5),
    "plane": dict(n=8000, p=4, shape="plane"),
    "line": dict(n=8000, p=4, shape="line"),
    "dup16": dict(n=8000, p=4, shape="dup16"),
    "late": dict(n=8000, p=4, shape="late"),
    "two_clumps": dict(n=8000, p=4, shape="two_clumps"),
}


def device_tree(eng):
    t = {k: eng.kd_array(k) for k in ("center", "lbound", "rbound", "mult", "index", "mpole")}
    t["L"] = eng.kd_info().L
    return t


def evaluate_case(eng, states, oracle32, case):
    """the evaluation of WALK_CASES[case] on eng; returns (n, p, radius, param, tree dict, tree-ordered positions)"""
    from coulomb_oscillators_amd import EVAL_FMM_KDTREE, INTEG_LEAPFROG
    import shapes3d
    o = dict(unsort=1, m2l_first=0, coll=1, p2p_mutual=0, tree_steps=1, tree_L=0, far_fp64=0, tree_radius=1.0)
    o.update(WALK_CASES[case])
    n, p, steps, shape = o.pop("n"), o.pop("p"), o.pop("steps", 0), o.pop("shape", None)
    if shape:
        buf, par = shapes3d.state(oracle32, shape, n), oracle32.params(n)
    else:
        buf, par = states(n)
    eng.set(fmm_order=p, eps2=EPS2, **o)
    d, prm = dev(buf), dev(par)
    eng.compute_force(EVAL_FMM_KDTREE, d, n, prm)
    for _ in range(steps):
        eng.integrate(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, 5e-4)
    info = eng.kd_info()
    if steps:
        assert info.rebuilt == 0                                   # the boxes are those of the first evaluation
    if o["far_fp64"]:
        assert info.real_bytes == 8 and info.mlt_max > 64
    if o["tree_L"]:
        assert info.L == o["tree_L"]
    pos = d.cpu().numpy()[0]
    if o["unsort"]:
        pos = pos[eng.kd_array("unsort")]
    return n, p, o["tree_radius"], par, prm, device_tree(eng), pos


def level_of(k):
    return (k + 1).bit_length() - 1


@pytest.mark.parametrize("case", sorted(WALK_CASES))
def test_probe_kd_against_the_restatement_on_the_device_tree(engine, states, oracle32, case):
    """field and potential within 1e-10 of their maxima over the probes of a set -- both sides are fp64 over the same widened floats,
    sums of <= 1e4 terms in the same order (the bound test_gpu_energy3d.py holds for the same kind of sums) -- on the four probe
    sets of the host test, probes on node centres, 65 identical probes and a single one"""
    n, p, radius, par, prm, tree, pos = evaluate_case(engine, states, oracle32, case)
    sets = p3.probe_sets(pos, 3)
    ntot = len(tree["mult"])
    pick = np.unique(np.concatenate([np.arange(min(7, ntot)), np.linspace(0, ntot - 1, 40).astype(np.int64)]))
    sets["centres"] = tree["center"][pick].astype(np.float32)
    names = list(sets)
    t = np.concatenate([sets[k] for k in names])
    m = len(t)
    td = dev(t)
    a, psi = run(engine.probe_kd, td, m, prm)
    wa, wpsi, acc, direct = p3.walk(tree, pos, t, p, radius, EPS2, n)
    wa, wpsi = wa * float(par[0]), wpsi * float(par[0])
    levels = {level_of(k) for s in acc for k in s}
    nacc, ndir = sum(len(s) for s in acc), sum(len(s) for s in direct)
    at = 0
    worst = [0.0, 0.0]
    for k in names:
        sl = slice(at, at + len(sets[k]))
        at += len(sets[k])
        ea = np.abs(a[sl] - wa[sl]).max() / np.linalg.norm(wa[sl], axis=1).max()
        ep = np.abs(psi[sl] - wpsi[sl]).max() / np.abs(wpsi[sl]).max()
        worst = [max(worst[0], ea), max(worst[1], ep)]
        assert ea <= 1e-10 and ep <= 1e-10, (case, k, ea, ep)
    print("%s: %d probes, %d expansions at levels %s, %d direct leaves; worst deviation a %.2e psi %.2e"
          % (case, m, nacc, sorted(levels), ndir, worst[0], worst[1]))
    assert len(levels) >= 2 and ndir > 0, (sorted(levels), ndir)             # the case reaches both branches of the walk
    # a probe on a node's centre opens that node
    off = m - len(sets["centres"])
    for j, k in enumerate(pick):
        assert int(k) not in acc[off + j]
    # 65 identical probes and a single one: the bits of the same probe in the big set (the invariant), on two waves / one lane
    j = len(sets["particles"]) + 3
    one = np.repeat(t[j:j + 1], 65, axis=0)
    a65, psi65 = run(engine.probe_kd, dev(one), 65, prm)
    assert (a65 == a[j]).all() and (psi65 == psi[j]).all()
    a1, psi1 = run(engine.probe_kd, dev(t[j:j + 1]), 1, prm)
    assert (a1[0] == a[j]).all() and psi1[0] == psi[j]


# ---- call properties -----------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def evaluated(states):
    """an engine behind an unsort = 1 evaluation of n = 3000 at p = 6, with a probe set that reaches every branch"""
    from coulomb_oscillators_amd import Engine, EVAL_FMM_KDTREE
    n, p = 3000, 6
    buf, par = states(n)
    eng = Engine(fmm_order=p, unsort=1)
    d, prm = dev(buf), dev(par)
    eng.compute_force(EVAL_FMM_KDTREE, d, n, prm)
    t = np.concatenate(list(p3.probe_sets(buf[0], 4).values()))
    yield eng, d, prm, n, p, buf, par, t
    eng.close()


def test_outputs_inputs_and_repeat_calls(evaluated):
    """p and t byte-identical afterwards; a second call returns the same bits; a alone and psi alone return the bits of the joint
    call; a permuted subset returns the bits of the full set -- for all three calls"""
    import torch
    eng, d, prm, n, p, buf, par, t = evaluated
    m = len(t)
    td = dev(t)
    d0, t0 = d.clone(), td.clone()
    rng = np.random.default_rng(8)
    sub = rng.permutation(m)[:m // 3]
    calls = {"probe": lambda tt, mm, **kw: run(eng.probe, d[0], n, tt, mm, prm, **kw),
             "probe_kd": lambda tt, mm, **kw: run(eng.probe_kd, tt, mm, prm, **kw),
             "probe_tree": lambda tt, mm, **kw: run(eng.probe_tree, d[0], n, tt, mm, prm, **kw)}
    for name, call in calls.items():
        a, psi = call(td, m)
        a2, psi2 = call(td, m)
        assert np.array_equal(a, a2) and np.array_equal(psi, psi2), name
        assert np.array_equal(call(td, m, want_psi=False)[0], a), name
        assert np.array_equal(call(td, m, want_a=False)[1], psi), name
        asub, psisub = call(dev(t[sub]), len(sub))
        assert np.array_equal(asub, a[sub]) and np.array_equal(psisub, psi[sub]), name
        assert torch.equal(d, d0) and torch.equal(td, t0), name
    # t == p
    a, psi = run(eng.probe_kd, d[0], n, prm)
    assert torch.equal(d, d0)


def test_side_stream_without_sync(states):
    """sync = 0 on a side stream: the bits of the synchronising calls on the default stream"""
    import torch
    from coulomb_oscillators_amd import Engine, EVAL_FMM_KDTREE
    n, p = 3000, 6
    buf, par = states(n)
    t = np.concatenate(list(p3.probe_sets(buf[0], 4).values()))
    m = len(t)
    out = []
    side = torch.cuda.Stream()
    for stream, sync in ((None, 1), (side, 0)):
        ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream())
        with ctx:
            eng = Engine(fmm_order=p, unsort=1, sync=sync)
            try:
                d, prm, td = dev(buf), dev(par), dev(t)
                torch.cuda.current_stream().synchronize()
                eng.compute_force(EVAL_FMM_KDTREE, d, n, prm)
                res = []
                for fn, args in ((eng.probe, (d[0], n, td, m, prm)), (eng.probe_kd, (td, m, prm)), (eng.probe_tree, (d[0], n, td, m, prm))):
                    a, psi = nan_out(m)
                    torch.cuda.current_stream().synchronize()
                    fn(*args, a, psi)
                    eng.sync()
                    res += [a.cpu().numpy(), psi.cpu().numpy()]
                out.append(res)
            finally:
                eng.close()
    for x, y in zip(*out):
        assert np.isfinite(x).all() and np.array_equal(x, y)


@pytest.mark.parametrize("opts", [dict(fmm_order=6), dict(fmm_order=4, far_fp64=1, tree_radius=1.5), dict(fmm_order=3, tree_L=5, eps2=1e-6),
                                  dict(fmm_order=4, shape="quant16")])
def test_probe_tree_is_probe_kd_on_a_fresh_context(states, oracle32, opts):
    """in any state of the engine -- here before any evaluation, after nbco_direct and after an unsort = 0 run -- bit for bit what a
    fresh context gives behind its own unsort = 1 evaluation.  shape: the sources are that shape of tests/shapes3d.py instead of the
    ball; quant16's tied coordinates flag the selection builds, so that probe_tree settles its build by demotion"""
    from coulomb_oscillators_amd import Engine, EVAL_FMM_KDTREE, INTEG_PEFRL
    n = 4096
    buf, par = states(n)
    opts = dict(opts)
    shape = opts.pop("shape", None)
    if shape:
        buf = shapes3d.state(oracle32, shape, n)
    t = np.concatenate(list(p3.probe_sets(buf[0], 5).values()))
    m = len(t)
    d, prm, td = dev(buf), dev(par), dev(t)
    fresh = Engine(unsort=1, **opts)
    eng = Engine(unsort=0, tree_steps=8, m2l_first=1, p2p_mutual=1, **opts)
    try:
        fresh.compute_force(EVAL_FMM_KDTREE, d.clone(), n, prm)
        if shape == "quant16":   # the same cold build as probe_tree's: flagged twice, demoted to the sorting build
            assert fresh.kd_info().build_mode == 2
        want = run(fresh.probe_kd, td, m, prm)
        got = run(eng.probe_tree, d[0], n, td, m, prm)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        eng.direct(d[0], d[2], n, prm)
        got = run(eng.probe_tree, d[0], n, td, m, prm)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        # after a run in tree order that ends on a drift: the state has changed, and so has the fresh context's answer
        d2 = d.clone()
        eng.compute_force(EVAL_FMM_KDTREE, d2, n, prm)
        eng.integrate(INTEG_PEFRL, EVAL_FMM_KDTREE, d2, n, prm, 5e-4)
        fresh.compute_force(EVAL_FMM_KDTREE, d2.clone(), n, prm)
        want = run(fresh.probe_kd, td, m, prm)
        got = run(eng.probe_tree, d2[0], n, td, m, prm)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    finally:
        fresh.close()
        eng.close()


def test_probe_tree_between_steps_leaves_the_run_untouched(states):
    """one context with tree_steps = 8, m2l_first = 1, track_order = 1, driven with and without probe_tree calls between
    integrate_steps calls: states, nbco_kd_info and NBCO_KD_ORDER bit-identical, and nbco_energy_fmm behind a probe_tree call is
    accepted with the same bits"""
    from coulomb_oscillators_amd import Engine, EVAL_FMM_KDTREE, INTEG_LEAPFROG
    from coulomb_oscillators_amd.engine import KdInfo
    n = 20000
    buf, par = states(n)
    t = dev(p3.probe_sets(buf[0], 6)["box1.5"])

    def drive(with_probes):
        eng = Engine(fmm_order=4, unsort=0, tree_steps=8, m2l_first=1, track_order=1)
        try:
            d, prm = dev(buf), dev(par)
            log = []

            def look():
                if with_probes:
                    run(eng.probe_tree, d[0], n, t, len(t), prm)
                info = eng.kd_info()
                log.append(tuple(getattr(info, f[0]) for f in KdInfo._fields_))
            eng.compute_force(EVAL_FMM_KDTREE, d, n, prm)
            look()
            for k in (1, 6, 3, 9):                                  # 20 evaluations in all: rebuilds at 8 and 16, warm selects
                eng.integrate_steps(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, 5e-4, k)
                look()
            ef = eng.energy_fmm(d, n, prm)
            if with_probes:
                run(eng.probe_tree, d[0], n, t, len(t), prm)
                assert eng.energy_fmm(d, n, prm) == ef              # still accepted, same bits
            return d.cpu().numpy(), log, eng.kd_array("order"), ef
        finally:
            eng.close()
    a, b = drive(False), drive(True)
    assert np.array_equal(a[0], b[0])
    assert a[1] == b[1]
    assert np.array_equal(a[2], b[2])
    assert a[3] == b[3]


def test_energy_calls_after_probe_kd_return_their_earlier_bits(evaluated):
    import torch
    eng, d, prm, n, p, buf, par, t = evaluated
    phi0 = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    ef, ek = eng.energy_fmm(d, n, prm), eng.energy_kd(d, n, prm, phi0)
    info0 = eng.kd_info()
    run(eng.probe_kd, dev(t), len(t), prm)
    run(eng.probe, d[0], n, dev(t), len(t), prm)
    phi1 = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    assert eng.energy_fmm(d, n, prm) == ef
    assert np.array_equal(eng.energy_kd(d, n, prm, phi1), ek) and torch.equal(phi0, phi1)
    info1 = eng.kd_info()
    assert all(getattr(info0, f[0]) == getattr(info1, f[0]) for f in type(info0)._fields_)


def test_refusals_are_followed_by_a_bit_identical_good_call(evaluated):
    import torch
    from coulomb_oscillators_amd import EngineError
    eng, d, prm, n, p, buf, par, t = evaluated
    m = len(t)
    td = dev(t)
    good = {"probe": run(eng.probe, d[0], n, td, m, prm), "kd": run(eng.probe_kd, td, m, prm), "tree": run(eng.probe_tree, d[0], n, td, m, prm)}

    def still_good():
        for name, got in (("probe", run(eng.probe, d[0], n, td, m, prm)), ("kd", run(eng.probe_kd, td, m, prm)),
                          ("tree", run(eng.probe_tree, d[0], n, td, m, prm))):
            assert np.array_equal(got[0], good[name][0]) and np.array_equal(got[1], good[name][1]), name

    def refused(fn, *args, status=ERR_ARG):
        a, psi = nan_out(m)
        with pytest.raises(EngineError) as e:
            fn(*args, a, psi)
        assert e.value.status == status, e.value
        assert torch.isnan(a).all() and torch.isnan(psi).all()      # the outputs are as they were

    for fn in (eng.probe, eng.probe_tree):
        refused(fn, None, n, td, m, prm)
        refused(fn, d[0], n, None, m, prm)
        refused(fn, d[0], n, td, m, None)
        refused(fn, d[0], 0, td, m, prm)
        refused(fn, d[0], -3, td, m, prm)
        refused(fn, d[0], n, td, 0, prm)
        refused(fn, d[0], n, td, -1, prm)
        refused(fn, d[0], n, td, 1 << 31, prm, status=ERR_UNSUPPORTED)
        refused(fn, d[0], 1 << 29, td, m, prm, status=ERR_UNSUPPORTED)
        with pytest.raises(EngineError) as e:
            fn(d[0], n, td, m, prm, None, None)
        assert e.value.status == ERR_ARG
        still_good()
    refused(eng.probe_kd, None, m, prm)
    refused(eng.probe_kd, td, m, None)
    refused(eng.probe_kd, td, 0, prm)
    refused(eng.probe_kd, td, 1 << 31, prm, status=ERR_UNSUPPORTED)
    with pytest.raises(EngineError) as e:
        eng.probe_kd(td, m, prm, None, None)
    assert e.value.status == ERR_ARG
    assert eng.lib.nbco_kd_probe(None, td.data_ptr(), m, prm.data_ptr(), None, None) == ERR_ARG
    still_good()


def test_probe_kd_needs_the_last_evaluation(states):
    """no evaluation yet, after nbco_direct, after a step that ends on a drift: refused; behind an evaluation: served"""
    from coulomb_oscillators_amd import Engine, EngineError, EVAL_FMM_KDTREE, INTEG_PEFRL, INTEG_LEAPFROG
    n = 3000
    buf, par = states(n)
    t = dev(p3.probe_sets(buf[0], 7)["box"])
    m = len(t)
    eng = Engine(fmm_order=4, unsort=1)
    try:
        d, prm = dev(buf), dev(par)

        def refused():
            a, psi = nan_out(m)
            with pytest.raises(EngineError) as e:
                eng.probe_kd(t, m, prm, a, psi)
            assert e.value.status == ERR_ARG

        refused()
        eng.compute_force(EVAL_FMM_KDTREE, d, n, prm)
        run(eng.probe_kd, t, m, prm)
        eng.direct(d[0], d[2], n, prm)
        refused()
        eng.compute_force(EVAL_FMM_KDTREE, d, n, prm)
        run(eng.probe_kd, t, m, prm)
        eng.integrate(INTEG_PEFRL, EVAL_FMM_KDTREE, d, n, prm, 5e-4)       # ends on a drift
        refused()
        run(eng.probe_tree, d[0], n, t, m, prm)                            # .. which the self-contained call does not mind
        eng.integrate(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, 5e-4)    # ends on an evaluation and a kick
        run(eng.probe_kd, t, m, prm)
    finally:
        eng.close()


def test_probe_kd_after_a_sharded_evaluation_is_unsupported(states):
    import torch
    from coulomb_oscillators_amd import Engine, EngineError, LoopbackWorld
    n2, h = 16384, 8192
    buf2, par2 = states(n2)
    prm2 = dev(par2)
    world = LoopbackWorld([Engine(fmm_order=4, unsort=0, p2p_mutual=0) for _ in range(2)], n2)
    try:
        world.partition([dev(buf2[0][:h]), dev(buf2[0][h:])], [dev(buf2[1][:h]), dev(buf2[1][h:])])
        world.force(prm2, elastic=False)
        torch.cuda.synchronize()
        r = world.runs[0]
        t = dev(buf2[0][:100])
        a, psi = nan_out(100)
        with pytest.raises(EngineError) as e:
            r.eng.probe_kd(t, 100, prm2, a, psi)
        assert e.value.status == ERR_UNSUPPORTED
        run(r.eng.probe_tree, r.buf, h, t, 100, prm2)               # the self-contained call takes the domain's particles as a system
    finally:
        for r in world.runs:
            r.eng.close()


# ---- distance from the exact call ----------------------------------------------------------------------------------------------------
def test_probe_tree_is_as_far_from_probe_as_the_restatement_says(engine, oracle32, oracle64):
    """n = 20000, p = 6, the reference ball in tree order (so that `every 7th particle` is the host test's set): the mean relative
    distance of probe_tree from probe on the four probe sets equals the figure of tests/test_probe3d_host.py (p3.FIGURES, from the
    fp64 oracle's tree) within that figure's third digit"""
    n, p = 20000, 6
    buf = oracle32.init_reference(n).astype(np.float64)
    par = oracle32.params(n)
    pv, _ = oracle64.fmm_kd(buf[:2], par.astype(np.float64), p=p, unsort=False, threads=4)
    pos = pv[0].astype(np.float32)
    assert np.array_equal(pos.astype(np.float64), pv[0])
    engine.set(fmm_order=p, eps2=EPS2)
    x, prm = dev(pos), dev(par)
    sets = p3.probe_sets(pos, 3)
    self_term = float(par[0]) / np.sqrt(float(np.float32(EPS2)))
    for name, t in sets.items():
        m = len(t)
        td = dev(t)
        a, psi = run(engine.probe_tree, x, n, td, m, prm)
        ea, epsi = run(engine.probe, x, n, td, m, prm)
        if name == "particles":
            psi, epsi = psi - self_term, epsi - self_term
        got = (p3.mean_rel(a, ea), p3.mean_rel(psi, epsi))
        want = p3.FIGURES[(n, p)][name]
        print("%s: probe_tree from probe a %.3e psi %.3e; restatement a %.3e psi %.3e" % (name, *got, *want))
        for g, w in zip(got, want):
            assert abs(g - w) <= 1e-2 * w, (name, got, want)
