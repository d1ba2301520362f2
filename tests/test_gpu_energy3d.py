"""GPU tests of the 3-D energy diagnostics: nbco_kd_potential (Engine.energy_kd: the O(N) potential pass over the locals of the last
kd-tree evaluation, csrc/kd_potential_kernels.hpp) and nbco_energy_tree (Engine.energy_tree: the same behind a tree of its own on a
private context).  Yardsticks: the fp64 pair sum, the numpy restatement tests/energy3d_numpy.py fed with the device tree, the
oracle's exact energy, and nbco_energy_fmm (unchanged code, no second truncation) on the same evaluation."""
import numpy as np
import pytest

import energy3d_numpy as e3

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = 2, 4


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def nan_phi(n):
    import torch
    return torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")


@pytest.fixture(scope="module")
def states(oracle32):
    """initial states and parameter packs by n, made once"""
    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = (oracle32.init_reference(n), oracle32.params(n))
        return cache[n][0].copy(), cache[n][1]
    return get


def device_tree(eng):
    t = {k: eng.kd_array(k) for k in ("center", "mult", "index", "mpole", "local", "p2p", "m2l")}
    t["L"] = eng.kd_info().L
    return t


def call_twice(eng, fn, d, n, prm):
    """psi (host) and out3 of fn, after checking that every slot was written, that coulomb = 1/2 sum psi and that a second call
    returns the same bits"""
    import torch
    phi = nan_phi(n)
    out = fn(d, n, prm, phi)
    psi = phi.cpu().numpy()
    assert np.isfinite(psi).all()
    assert abs(0.5 * psi.sum() - out[2]) <= 1e-13 * abs(out[2])
    phi2 = nan_phi(n)
    out2 = fn(d, n, prm, phi2)
    assert np.array_equal(out, out2) and torch.equal(phi, phi2)
    assert np.array_equal(fn(d, n, prm), out)                     # phi_dev = NULL
    return psi, out


# ---- all near field: the tight check ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps2,coincident", [(1e-18, 0), (1e-4, 0), (1e-18, 2), (1e-18, 3)])
def test_all_near_field_psi_is_the_fp64_pair_sum(engine, states, eps2, coincident):
    from coulomb_oscillators_amd import EVAL_FMM_KDTREE
    n, p = 3000, 6
    buf, par = states(n)
    for k in range(1, coincident):
        buf[0][7 * k] = buf[0][0]                                  # two / three particles in one place
    engine.set(fmm_order=p, unsort=1, tree_radius=1e6, eps2=eps2)
    d, prm = dev(buf), dev(par)
    engine.compute_force(EVAL_FMM_KDTREE, d, n, prm)
    info = engine.kd_info()
    assert info.m2l_pairs == 0 and info.p2p_pairs == (1 << info.L) * ((1 << info.L) - 1) // 2      # nothing is left to the far field
    psi, _ = call_twice(engine, engine.energy_kd, d, n, prm)
    want = float(par[0]) * e3.pair_potential(buf[0], np.float32(eps2))
    err = np.abs(psi - want) / want
    print("all near field, eps2 = %g, %d coincident: worst per-particle deviation %.2e" % (eps2, coincident, err.max()))
    assert err.max() <= 1e-12


# ---- far field against the restatement -------------------------------------------------------------------------------------
FAR_CASES = {
    "n64_p1": dict(n=64, p=1),
    "n4096_p3": dict(n=4096, p=3),
    "n3000_p6": dict(n=3000, p=6),
    "n20000_p6": dict(n=20000, p=6),
    "n30001_p10_fp64": dict(n=30001, p=10, far_fp64=1),            # leaves of ~117: more targets than lanes
    "n3000_p6_L2": dict(n=3000, p=6, tree_L=2),                    # 750 per leaf
    "n3000_p6_tree_order": dict(n=3000, p=6, unsort=0),
    "n4096_p3_m2l_first": dict(n=4096, p=3, m2l_first=1),
    "n3000_p6_m2l_first_tree_order": dict(n=3000, p=6, m2l_first=1, unsort=0),
    "n3000_p6_ncoll": dict(n=3000, p=6, coll=0),
    "n20000_p6_mutual": dict(n=20000, p=6, p2p_mutual=1, unsort=0),
    "n3000_p6_stale_boxes": dict(n=3000, p=6, unsort=0, tree_steps=8, steps=2),
}


@pytest.mark.parametrize("case", sorted(FAR_CASES))
def test_psi_against_the_restatement_on_the_device_tree(engine, states, case):
    """psi_i within 1e-10 of max |psi| of tests/energy3d_numpy.py on the tree copied out through nbco_kd_copy: both sides are fp64
    over the same widened floats, sums of <= 1e4 terms"""
    from coulomb_oscillators_amd import EVAL_FMM_KDTREE, INTEG_LEAPFROG
    o = dict(unsort=1, m2l_first=0, coll=1, p2p_mutual=0, tree_steps=1, tree_L=0, far_fp64=0)
    o.update(FAR_CASES[case])
    n, p, steps = o.pop("n"), o.pop("p"), o.pop("steps", 0)
    buf, par = states(n)
    engine.set(fmm_order=p, **o)
    d, prm = dev(buf), dev(par)
    engine.compute_force(EVAL_FMM_KDTREE, d, n, prm)
    for _ in range(steps):
        engine.integrate(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, 5e-4)
    info = engine.kd_info()
    if steps:
        assert info.rebuilt == 0                                   # the boxes are those of the first evaluation
    if "far_fp64" in FAR_CASES[case]:
        assert info.real_bytes == 8 and info.mlt_max > 64
    if o["tree_L"]:
        assert info.L == o["tree_L"]
    if n > 64 and not o["tree_L"]:
        assert info.m2l_pairs > 0                                  # there is a far field to compare
    psi, _ = call_twice(engine, engine.energy_kd, d, n, prm)
    pos = d.cpu().numpy()[0]
    if o["unsort"]:
        perm = engine.kd_array("unsort")
        want_tree = e3.psi(device_tree(engine), pos[perm], p, np.float32(1e-18), par[0], coll=bool(o["coll"]))
        want = np.empty(n)
        want[perm] = want_tree
    else:
        want = e3.psi(device_tree(engine), pos, p, np.float32(1e-18), par[0], coll=bool(o["coll"]))
    err = np.abs(psi - want).max() / np.abs(want).max()
    print("%s: max |psi - restatement| / max |psi| = %.2e" % (case, err))
    assert err <= 1e-10


# ---- against the exact energy ----------------------------------------------------------------------------------------------
# Coulomb energy: the table of test_energy_fmm_against_fp64_direct_energy; the measured errors of this pass are
# under half of it at every entry
ENERGY_TOL = {3: 3e-3, 6: 2e-4, 8: 5e-5, 10: 2e-5}
# mean over the particles of |psi_i - exact_i| / exact_i at p = 6: twice the measured figures 5.47e-5 and 2.03e-4
PSI_MEAN_TOL = {3000: 1.1e-4, 20000: 4.1e-4}


@pytest.fixture(scope="module")
def exact_energy(oracle64):
    cache = {}

    def get(n, buf, par):
        if n not in cache:
            cache[n] = oracle64.energy(buf.astype(np.float64), par.astype(np.float64), threads=8)
        return cache[n]
    return get


def exact_psi(d, n, p0):
    """fp64 pair sum per particle on the device, j != i by index"""
    import torch
    x = d[0].double()
    out = torch.zeros(n, dtype=torch.float64, device="cuda")
    for s in range(0, n, 2048):
        r2 = ((x[s:s + 2048, None, :] - x[None, :, :]) ** 2).sum(-1) + float(np.float32(1e-18))
        w = r2.rsqrt()
        i = torch.arange(s, min(s + 2048, n), device="cuda")
        w[i - s, i] = 0.0
        out[s:s + 2048] = w.sum(1)
    return float(p0) * out.cpu().numpy()


@pytest.mark.parametrize("n,p", [(3000, 6), (20000, 6), (65536, 6), (65536, 8), (30001, 10), (4096, 3)])
def test_energy_kd_against_fp64_direct_energy(engine, states, exact_energy, n, p):
    from coulomb_oscillators_amd import EVAL_FMM_KDTREE
    buf, par = states(n)
    want = exact_energy(n, buf, par)
    for unsort in (1, 0):
        engine.set(fmm_order=p, unsort=unsort)
        d, prm = dev(buf), dev(par)
        engine.compute_force(EVAL_FMM_KDTREE, d, n, prm)
        phi = nan_phi(n)
        got = engine.energy_kd(d, n, prm, phi)
        old = engine.energy_fmm(d, n, prm)                          # the same evaluation, multipoles evaluated at the particles
        assert abs(got[0] - want[0]) <= 1e-6 * want[0] and abs(got[1] - want[1]) <= 1e-6 * want[1]
        err, err_old = abs(got[2] - want[2]) / want[2], abs(old[2] - want[2]) / want[2]
        print("n = %d p = %d unsort = %d: Coulomb energy off by %.3e (energy_kd) %.3e (energy_fmm)" % (n, p, unsort, err, err_old))
        assert err <= ENERGY_TOL[p], (err, err_old)
    if p == 6 and n in PSI_MEAN_TOL:
        ex = exact_psi(d, n, par[0])
        mean = float(np.mean(np.abs(phi.cpu().numpy() - ex) / ex))
        print("n = %d p = %d: mean per-particle |psi - exact| / exact = %.3e" % (n, p, mean))
        assert mean <= PSI_MEAN_TOL[n]


# ---- self-contained and non-interfering ------------------------------------------------------------------------------------
def fresh_energy_kd(state, n, prm, **opts):
    """energy_kd on a fresh context behind one nbco_fmm_kdtree evaluation (unsort = 1, tree_steps = 1) of a copy of the state"""
    import torch
    from coulomb_oscillators_amd import Engine
    eng = Engine(unsort=1, tree_steps=1, **opts)
    try:
        s = state.clone()
        a = torch.empty(3 * n, dtype=torch.float32, device="cuda")
        eng.fmm_cart3_kdtree(s, a, n, prm)
        phi = nan_phi(n)
        out = eng.energy_kd(s, n, prm, phi)
        return out, phi
    finally:
        eng.close()


def assert_tree_equals_fresh(eng, d, n, prm, **opts):
    import torch
    before = d.clone()
    phi = nan_phi(n)
    out = eng.energy_tree(d, n, prm, phi)
    assert torch.equal(d, before)                                   # buf is const
    want, wphi = fresh_energy_kd(d, n, prm, **opts)
    assert np.array_equal(out, want) and torch.equal(phi, wphi), (out, want)
    phi2 = nan_phi(n)
    assert np.array_equal(eng.energy_tree(d, n, prm, phi2), out) and torch.equal(phi, phi2)     # the second call: same bits
    return out


def test_energy_tree_is_energy_kd_on_a_fresh_context_in_any_state(states):
    """before any evaluation, after nbco_direct, after nbco_fmm_traceless, after a PEFRL step (which ends on a drift), after a change
    of fmm_order and of n -- each time bit for bit what a fresh context gives behind its own evaluation"""
    import torch
    from coulomb_oscillators_amd import Engine, EVAL_FMM_KDTREE, INTEG_PEFRL
    n = 4096
    buf, par = states(n)
    eng = Engine(fmm_order=4, unsort=0, tree_steps=8, m2l_first=1, p2p_mutual=1)
    try:
        d, prm = dev(buf), dev(par)
        o4 = dict(fmm_order=4, m2l_first=1)
        assert_tree_equals_fresh(eng, d, n, prm, **o4)
        eng.direct(d[0], d[2], n, prm)
        assert_tree_equals_fresh(eng, d, n, prm, **o4)
        eng.fmm_cart3_traceless(d, d[2], n, prm)
        assert_tree_equals_fresh(eng, d, n, prm, **o4)
        eng.compute_force(EVAL_FMM_KDTREE, d, n, prm)
        eng.integrate(INTEG_PEFRL, EVAL_FMM_KDTREE, d, n, prm, 5e-4)
        e_pefrl = assert_tree_equals_fresh(eng, d, n, prm, **o4)
        # the positions the last evaluation saw are not those of the state: nbco_energy_fmm there is off, this one is not
        x = e3.pair_potential(d[0].cpu().numpy(), np.float32(1e-18)).sum() * 0.5 * float(par[0])
        assert abs(e_pefrl[2] - x) <= 3e-3 * x                      # order 4, held to the order-3 bound of ENERGY_TOL
        eng.set(fmm_order=6, far_fp64=1)
        assert_tree_equals_fresh(eng, d, n, prm, fmm_order=6, m2l_first=1, far_fp64=1)
        n2 = 3000
        buf2, par2 = states(n2)
        d2, prm2 = dev(buf2), dev(par2)
        assert_tree_equals_fresh(eng, d2, n2, prm2, fmm_order=6, m2l_first=1, far_fp64=1)
        eng.set(fmm_order=3, far_fp64=0, tree_radius=1.5, eps2=1e-6)
        assert_tree_equals_fresh(eng, d, n, prm, fmm_order=3, m2l_first=1, tree_radius=1.5, eps2=1e-6)
    finally:
        eng.close()


def test_energy_tree_between_steps_leaves_the_run_untouched(states):
    """one context with tree_steps = 8, m2l_first = 1, track_order = 1, driven with and without energy_tree calls between steps and
    between nbco_integrate_steps calls: states, nbco_kd_info (warm_builds, rebuilt, ..) and NBCO_KD_ORDER bit-identical, and
    nbco_energy_fmm directly behind an energy_tree call is accepted with the same bits"""
    from coulomb_oscillators_amd import Engine, EVAL_FMM_KDTREE, INTEG_LEAPFROG
    from coulomb_oscillators_amd.engine import KdInfo
    n = 20000
    buf, par = states(n)

    def drive(with_energy):
        eng = Engine(fmm_order=4, unsort=0, tree_steps=8, m2l_first=1, track_order=1)
        try:
            d, prm = dev(buf), dev(par)
            log = []

            def look():
                if with_energy:
                    eng.energy_tree(d, n, prm)
                info = eng.kd_info()
                log.append(tuple(getattr(info, f[0]) for f in KdInfo._fields_))
            eng.compute_force(EVAL_FMM_KDTREE, d, n, prm)
            look()
            for _ in range(3):
                eng.integrate(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, 5e-4)
                look()
            for k in (6, 3, 9):                                     # 22 evaluations in all: rebuilds at 8 and 16, warm selects
                eng.integrate_steps(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, 5e-4, k)
                look()
            ef = eng.energy_fmm(d, n, prm)
            if with_energy:
                eng.energy_tree(d, n, prm, nan_phi(n))
                assert eng.energy_fmm(d, n, prm) == ef              # still accepted, same bits
            return d.cpu().numpy(), log, eng.kd_array("order"), ef
        finally:
            eng.close()
    a, b = drive(False), drive(True)
    assert np.array_equal(a[0], b[0])
    assert a[1] == b[1]
    names = [f[0] for f in KdInfo._fields_]
    print("rebuilt per look:", [row[names.index("rebuilt")] for row in a[1]], "warm builds:", a[1][-1][names.index("warm_builds")])
    assert a[1][-1][names.index("warm_builds")] > 0                 # (the top levels of n = 20000 are built by selection)
    assert np.array_equal(a[2], b[2])
    assert a[3] == b[3]


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_are_followed_by_a_bit_identical_good_call(states):
    import torch
    from coulomb_oscillators_amd import Engine, EngineError, EVAL_FMM_KDTREE, LoopbackWorld
    n = 3000
    buf, par = states(n)
    eng = Engine(fmm_order=4, unsort=1)
    try:
        d, prm = dev(buf), dev(par)

        def refused(fn, *args, status=ERR_ARG):
            with pytest.raises(EngineError) as e:
                fn(*args)
            assert e.value.status == status, e.value

        refused(eng.energy_kd, d, n, prm)                           # no evaluation yet
        eng.compute_force(EVAL_FMM_KDTREE, d, n, prm)
        good_kd = call_twice(eng, eng.energy_kd, d, n, prm)
        good_tree = call_twice(eng, eng.energy_tree, d, n, prm)

        def still_good():
            psi, out = call_twice(eng, eng.energy_kd, d, n, prm)
            assert np.array_equal(psi, good_kd[0]) and np.array_equal(out, good_kd[1])
            psi, out = call_twice(eng, eng.energy_tree, d, n, prm)
            assert np.array_equal(psi, good_tree[0]) and np.array_equal(out, good_tree[1])

        for fn in (eng.energy_kd, eng.energy_tree):
            refused(fn, None, n, prm)
            refused(fn, d, n, None)
            refused(fn, d, 0, prm)
            refused(fn, d, -5, prm)
            still_good()
        out = (__import__("ctypes").c_double * 3)()
        for name in ("nbco_kd_potential", "nbco_energy_tree"):
            assert getattr(eng.lib, name)(eng.ctx, d.data_ptr(), n, prm.data_ptr(), None, None) == ERR_ARG      # out3_host = NULL
            assert getattr(eng.lib, name)(None, d.data_ptr(), n, prm.data_ptr(), out, None) == ERR_ARG
        still_good()
        refused(eng.energy_kd, d, n - 1, prm)                       # a different n
        still_good()
        eng.energy(d, n, prm)                                       # nbco_energy repacks the positions: the lists are stale
        refused(eng.energy_kd, d, n, prm)
        psi, out = call_twice(eng, eng.energy_tree, d, n, prm)      # .. which the self-contained call does not mind
        assert np.array_equal(psi, good_tree[0]) and np.array_equal(out, good_tree[1])
        eng.compute_force(EVAL_FMM_KDTREE, d, n, prm)
        still_good()
    finally:
        eng.close()
    # after a sharded evaluation: the tree is the assembled global one, pruned to the domain
    n2, h = 16384, 8192
    buf2, par2 = states(n2)
    prm2 = dev(par2)
    world = LoopbackWorld([Engine(fmm_order=4, unsort=0, p2p_mutual=0) for _ in range(2)], n2)
    try:
        world.partition([dev(buf2[0][:h]), dev(buf2[0][h:])], [dev(buf2[1][:h]), dev(buf2[1][h:])])
        world.force(prm2, elastic=False)
        torch.cuda.synchronize()
        run = world.runs[0]
        with pytest.raises(EngineError) as e:
            run.eng.energy_kd(run.buf, h, prm2)
        assert e.value.status == ERR_UNSUPPORTED
        run.eng.energy_fmm(run.buf, h, prm2)                        # the sharded tool still serves
        call_twice(run.eng, run.eng.energy_tree, run.buf, h, prm2)  # and the self-contained call takes the domain's particles as a system
    finally:
        for r in world.runs:
            r.eng.close()
