"""GPU parity tests of the kd-tree evaluator in the configuration the nbco3 binary runs: the reference's GPU driver, i.e. the
M2L-first traversal order (opts.m2l_first = 1, fmm_cart3_kdtree.cuh:504-542) and tree reuse between rebuilds (opts.tree_steps
= 8, :1619-1645), against the oracle's restatement of both (Oracle.fmm_kd(m2l_first=, reuse=)).

Bars: those of test_gpu_fmm_kd.py -- tree integers, boxes, centres, permutation and both interaction lists (as sets) bit-exact,
multipoles and locals within 2e-5 of the per-component maximum, accelerations within 1e-5 (nbutil.force_err).

Which multipoles are compared.  The multipole of a node near the root is a sum over up to N particles whose odd orders cancel
about the centre of charge, and from N ~ 8000 on the fp32 ORACLE is no longer within 2e-5 of its own REAL = double build there, so
it cannot hold anybody else to that bar.  Measured on fresh builds (largest deviation relative to the column maximum; engine vs
fp32 oracle / engine vs fp64 oracle / fp32 oracle vs fp64 oracle):

    all nodes (worst always at level 0 or 1)           nodes of the M2L list
    N =   8192 p 4   2.2e-5 / 8.8e-6 / 2.4e-5          2.6e-6 / 1.6e-6 / 1.5e-6
    N =  30001 p 5   1.6e-5 / 6.4e-6 / 9.5e-6          2.1e-6 / 2.9e-6 / 3.1e-6
    N =  46000 p 6   5.5e-5 / 5.9e-5 / 2.7e-5          1.3e-6 / 7.6e-6 / 7.6e-6
    N =  65536 p 6   4.0e-5 / 2.9e-5 / 4.1e-5          2.3e-6 / 5.1e-6 / 5.1e-6
    N = 262144 p 6   4.4e-5 / 8.3e-5 / 7.7e-5          6.6e-6 / 6.8e-6 / 6.8e-6

No M2L entry reads those top multipoles (the root has no partner, its children are never admissible); they exist only as the
last steps of the M2M chain.  The bar is therefore applied, unchanged, to the multipoles the evaluation reads -- every node that
occurs in the M2L list -- and to the locals of ALL nodes (engine vs fp32 oracle: 9e-7 .. 3.5e-6 on the rows above); the
accelerations, which are what all of them feed, meet 1e-5 with a factor of ten to spare."""
import numpy as np
import pytest

from nbutil import assert_same_tree, canon_pairs, drive_by_hand, expansion_err, force_err, list_entries_changed

pytestmark = pytest.mark.gpu


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def m2l_nodes(tree):
    """the nodes whose multipoles the far field reads (module docstring)"""
    return np.unique(np.asarray(tree["m2l"]).ravel())


# ---- a. fresh builds with the M2L-first traversal ---------------------------------------------------------------------------
FRESH = [
    dict(n=4096, p=6), dict(n=30001, p=5), dict(n=5000, p=3, cube=True), dict(n=65536, p=6),
    dict(n=262144, p=6),                          # top levels by median selection
    dict(n=1000, p=2), dict(n=300, p=1),
    dict(n=20000, p=3, tree_radius=2.0), dict(n=4096, p=4, dens_inhom=4.0),
    dict(n=8192, p=10, far_fp64=1),               # the wide far-field kernels
    dict(n=46000, p=6, p2p_mutual=1),
]


@pytest.mark.parametrize("case", FRESH, ids=lambda c: "-".join("%s%s" % kv for kv in c.items()))
def test_m2l_first_fresh_build_matches_oracle(oracle32, oracle64, case):
    """One evaluation per case with opts.m2l_first = 1 and unsort = 1.  Every case first shows, from the oracle alone, that the
    M2L-first lists differ from the default order's (322 .. 63832 entries on these rows), so an engine that ignored the option
    fails on the lists.  Measured force_err against the oracle: 1.8e-7 (N = 300) .. 1.04e-6 (N = 262144)."""
    import torch
    from coulomb_oscillators_amd import Engine
    o = oracle32
    n, p = case["n"], case["p"]
    radius, dens, fp64 = case.get("tree_radius", 1.0), case.get("dens_inhom", 1.0), case.get("far_fp64", 0)
    buf = o.init_reference(n, test_mode=case.get("cube", False))
    par = o.params(n)
    okw = dict(p=p, threads=8, unsort=True, radius=radius, dens_inhom=dens)
    o.fmm_kd(buf[:2], par, m2l_first=0, **okw)
    other = o.kd_tree()
    _, want_a = o.fmm_kd(buf[:2], par, m2l_first=1, **okw)
    offM, offL = p * (p + 1) * (p + 2) // 6, (p + 1) ** 2
    want = o.kd_tree(offM=offM, offL=offL)
    perm = o.kd_unsort(n)
    # the case can fail: an evaluator that ignored the option would produce `other`
    moved = list_entries_changed(other, want)
    assert moved >= 20, moved

    def run(**opts):
        e = Engine(fmm_order=p, unsort=1, m2l_first=1, tree_radius=radius, dens_inhom=dens, p2p_mutual=case.get("p2p_mutual", 0), **opts)
        d = dev(buf[:2])
        a = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
        e.fmm_cart3_kdtree(d, a, n, dev(par))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(d.cpu().numpy(), buf[:2])      # b_unsort: positions / velocities untouched
        return e, a.cpu().numpy()

    e, got = run(far_fp64=fp64)
    info = e.kd_info()
    assert info.rebuilt == 1 and info.real_bytes == (8 if fp64 else 4)
    assert_same_tree(e, want, n, perm)
    assert (info.p2p_pairs, info.m2l_pairs) == (len(want["p2p"]), len(want["m2l"]))
    err = force_err(got, want_a)
    print("fresh %s: L %d, lists p2p %d m2l %d (m2l_first=0: %d / %d, %d entries differ), force_err %.3e"
          % (case, want["L"], len(want["p2p"]), len(want["m2l"]), len(other["p2p"]), len(other["m2l"]), moved, err))
    assert err < 1e-5
    mp, lc = e.kd_array("mpole"), e.kd_array("local")
    assert np.isfinite(mp).all() and np.isfinite(lc).all()
    if not fp64:
        assert mp.dtype == np.float32
        assert expansion_err(mp, want["mpole"], m2l_nodes(want)) < 2e-5
        assert expansion_err(lc, want["local"]) < 2e-5
    else:
        # as test_far_fp64_kdtree_against_both_oracles: the tuples are doubles and follow the REAL = double oracle wherever its
        # lists equal the fp32 ones; the accelerations are then no further from it than the all-fp32 evaluation's
        assert mp.dtype == np.float64 and lc.dtype == np.float64
        o64 = oracle64
        _, want64 = o64.fmm_kd(buf[:2].astype(np.float64), par.astype(np.float64), m2l_first=1, **okw)
        tree64 = o64.kd_tree(offM=offM, offL=offL)
        e32, got32 = run(far_fp64=0)
        e32.close()
        if all(np.array_equal(canon_pairs(tree64[k]), canon_pairs(want[k])) for k in ("p2p", "m2l")):
            d64, d32 = force_err(got, want64), force_err(got32, want64)
            assert d64 < 1e-5 and d64 < 1.5 * d32 + 2e-7
            tol = 2e-5 if p <= 6 else 1e-4
            assert expansion_err(mp, tree64["mpole"]) < tol
            assert expansion_err(lc, tree64["local"]) < tol
    e.close()


# ---- b. the reuse schedule, evaluation by evaluation ------------------------------------------------------------------------
#        n, p, tree_steps, m2l_first, dt, evaluations, further engine options
SCHEDULES = [
    (8192, 4, 8, 1, 5e-4, 17, {}),                       # `-test2` / the CLI's defaults, across two rebuilds
    (65536, 6, 8, 1, 5e-3, 10, {}),
    (30001, 5, 3, 0, 2e-2, 7, {}),
    (32768, 6, 4, 1, 5e-3, 6, dict(p2p_mutual=1)),
    (20000, 8, 8, 1, 5e-3, 4, dict(far_fp64=1)),
]
_hand_driven = {}     # final host state of the schedules of (b) that have run in this session, for (c)


@pytest.mark.parametrize("n,p,tree_steps,m2l_first,dt,evals,extra", SCHEDULES, ids=lambda v: str(v).replace(" ", "") if isinstance(v, dict) else None)
def test_reuse_schedule_matches_oracle_at_every_evaluation(oracle32, n, p, tree_steps, m2l_first, dt, evals, extra):
    """Every evaluation of a run with tree reuse against the oracle GIVEN THE SAME INPUT: the oracle evaluates the positions the
    engine is about to evaluate (copied off the device), rebuilding where the engine must rebuild and reusing its previous tree
    where the engine must reuse.  The comparison is on the Coulomb part (fmm_cart3_kdtree, then add_elastic separately): near the
    trap's equilibrium the elastic term cancels much of it.  Measured: worst force_err of a row 5.8e-7 .. 2.9e-6 (the latter at
    k = 7 of N = 65536, dt = 5e-3, where 7053 list entries have changed since the rebuild); list entries changed at the end of
    each rebuild period 135 and 161 / 7053 / 2316 and 3938 / 1217 / 76."""
    import torch
    from coulomb_oscillators_amd import Engine
    o = oracle32
    dt = float(np.float32(dt))                 # dt / 2 is exact
    buf = o.init_reference(n)
    par = o.params(n)
    offM, offL = p * (p + 1) * (p + 2) // 6, (p + 1) ** 2
    eng = Engine(fmm_order=p, unsort=0, tree_steps=tree_steps, m2l_first=m2l_first, **extra)
    d, prm = dev(buf), dev(par)
    built, changed, worst = [None], {}, [0.0]

    def force():
        eng.fmm_cart3_kdtree(d, d[2], n, prm)

    def compare(k, x_in):
        torch.cuda.synchronize()
        reuse = k % tree_steps != 0
        pv, a_ref = o.fmm_kd(x_in, par, p=p, threads=8, unsort=False, m2l_first=m2l_first, reuse=int(reuse))
        want = o.kd_tree(offM=offM, offL=offL)
        info = eng.kd_info()
        assert info.rebuilt == (0 if reuse else 1), k
        try:
            assert_same_tree(eng, want, n, o.kd_unsort(n))
        except AssertionError as ex:
            raise AssertionError("evaluation %d (%s): %s" % (k, "reuse" if reuse else "rebuild", ex)) from None
        if reuse:
            # still the topology and the boxes of the rebuild, and a reuse evaluation leaves the caller's state alone
            for name in ("index", "splitdim", "lbound", "rbound"):
                np.testing.assert_array_equal(want[name], built[0][name], err_msg=name)
            np.testing.assert_array_equal(pv, x_in)
            changed[k] = list_entries_changed(built[0], want)
        else:
            built[0] = want
        got = d.cpu().numpy()
        np.testing.assert_array_equal(got[:2], pv, err_msg="[pos | vel] after evaluation %d" % k)
        err = force_err(got[2], a_ref)
        worst[0] = max(worst[0], err)
        print("schedule n=%d p=%d T=%d M=%d k=%d %s: lists p2p %d m2l %d, %d entries changed since the rebuild, force_err %.3e"
              % (n, p, tree_steps, m2l_first, k, "reuse" if reuse else "REBUILD", len(want["p2p"]), len(want["m2l"]), changed.get(k, 0), err))
        assert err < 1e-5, (k, err)
        if info.real_bytes == 4:
            assert expansion_err(eng.kd_array("mpole"), want["mpole"], m2l_nodes(want)) < 2e-5, k
            assert expansion_err(eng.kd_array("local"), want["local"]) < 2e-5, k
        eng.add_elastic(d[0], d[2], n, prm[3:])

    drive_by_hand(eng, d, n, prm, dt, evals, force, compare)
    torch.cuda.synchronize()
    # an engine that kept the lists of the rebuild would not have passed: by the end of every rebuild period the oracle's own
    # lists have moved on
    last = [k for k in range(evals) if k % tree_steps != 0 and ((k + 1) % tree_steps == 0 or k == evals - 1)]
    assert last and all(changed[k] >= 20 for k in last), (last, changed)
    if n > 4096 and evals > tree_steps:
        assert eng.kd_info().warm_builds >= 1          # the later rebuilds select around the previous tree's pivots
    print("schedule n=%d p=%d T=%d M=%d: worst force_err %.3e, entries changed at the end of each period %s"
          % (n, p, tree_steps, m2l_first, worst[0], [changed[k] for k in last]))
    _hand_driven[(n, p, tree_steps, m2l_first, evals)] = d.cpu().numpy()
    eng.close()


# ---- c. the same schedule through the product's entry points ----------------------------------------------------------------
@pytest.mark.parametrize("n,p,tree_steps,m2l_first,dt,evals,extra", SCHEDULES[:2], ids=lambda v: str(v).replace(" ", "") if isinstance(v, dict) else None)
def test_reuse_schedule_through_compute_force_integrate_and_integrate_steps(oracle32, n, p, tree_steps, m2l_first, dt, evals, extra):
    """nbco_force + hand-driven steps, nbco_force + nbco_integrate per step, nbco_force + one nbco_integrate_steps: the same
    operations with the same roundings (include/nbco.h), so the three final states are equal bit for bit; and they lie within
    the tolerances of test_leapfrog_with_fmm_matches_oracle of the run of (b), whose every evaluation was checked against the
    oracle (that run adds the elastic term in a call of its own, one rounding more per evaluation than nbco_force)."""
    import torch
    from coulomb_oscillators_amd import Engine, EVAL_FMM_KDTREE, INTEG_LEAPFROG
    o = oracle32
    dt = float(np.float32(dt))
    buf = o.init_reference(n)
    prm = dev(o.params(n))
    steps = evals - 1
    finals = []

    def two_calls():          # the force of (b): the evaluator, then the trap
        eng.fmm_cart3_kdtree(d, d[2], n, prm)
        eng.add_elastic(d[0], d[2], n, prm[3:])

    for how in ("hand", "integrate", "integrate_steps", "as (b)"):
        eng = Engine(fmm_order=p, unsort=0, tree_steps=tree_steps, m2l_first=m2l_first, **extra)
        d = dev(buf)
        if how == "hand":
            drive_by_hand(eng, d, n, prm, dt, evals, lambda: eng.compute_force(EVAL_FMM_KDTREE, d, n, prm))
        elif how == "as (b)":
            drive_by_hand(eng, d, n, prm, dt, evals, two_calls)
        else:
            eng.compute_force(EVAL_FMM_KDTREE, d, n, prm)
            if how == "integrate":
                for _ in range(steps):
                    eng.integrate(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, dt)
            else:
                eng.integrate_steps(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, dt, steps)
        torch.cuda.synchronize()
        assert eng.kd_info().rebuilt == (1 if steps % tree_steps == 0 else 0)
        finals.append(d.clone())
        eng.close()
    for name, other in (("integrate", finals[1]), ("integrate_steps", finals[2])):
        for part, what in enumerate(("positions", "velocities", "accelerations")):
            assert torch.equal(finals[0][part], other[part]), "%s: %s differ from the hand-driven run" % (name, what)
    # the run of (b) again, without the comparisons: the evaluator is bit-reproducible, so this IS the state the oracle-checked run
    # ended in (asserted when that test has run in this session)
    got, ref = finals[0].cpu().numpy(), finals[3].cpu().numpy()
    key = (n, p, tree_steps, m2l_first, evals)
    if key in _hand_driven:
        np.testing.assert_array_equal(ref, _hand_driven[key])
    # particle order is the tree order of the last rebuild on both sides, which rounding may have ordered differently
    ka = np.lexsort((got[0][:, 2], got[0][:, 1], got[0][:, 0]))
    kb = np.lexsort((ref[0][:, 2], ref[0][:, 1], ref[0][:, 0]))
    assert np.abs(got[0][ka] - ref[0][kb]).max() <= 2e-6 * np.abs(ref[0]).max()
    assert np.abs(got[1][ka] - ref[1][kb]).max() <= 2e-5 * np.abs(ref[1]).max()
