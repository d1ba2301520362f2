"""One long-lived nbco context driven through sizes, options and evaluators, as nbco3 and every caller of INTEGRATION.md drive it
(host/nbco_reference_api.hpp keeps ONE static context and pushes every option change through nbco_set_opts), where the rest of the
suite gives each case a fresh context.

Two bars, used throughout:

(F) fresh-context equality.  What the long-lived context returns for a call equals, BIT FOR BIT, what a context created for that
    call alone returns for the same input and options: torch.equal on positions, velocities and accelerations, np.array_equal on
    the tree arrays and on canon_pairs of both interaction lists.  include/nbco.h promises it (results are bit-reproducible, the
    trees identical, only the speed differs); it is what finds state that leaked from an earlier call.
(O) the oracle.  The fresh context is still the code under test, so at the steps named in each test the long-lived context is also
    held to the CPU oracle with the suite's existing bars: tree integers, boxes, centres, permutation and both lists bit-exact
    (nbutil.assert_same_tree), accelerations force_err < 1e-5.  The oracle's own threaded sums differ from run to run by 3e-7
    (measured: unsort = False against the permuted unsort = True result at N = 30001), so one oracle evaluation per input, taken
    in the caller's order and permuted with its own permutation for tree-order comparisons, serves both orders.

What is NOT held to (F), by design: nbco_energy_fmm in the middle of a reuse schedule (it sums over the lists of the last
evaluation, csrc/k_fmm_kd.hip kd_energy_fmm; a context created for that call alone has no lists and would build a different tree
from the moved state) -- it is held to the fp64 direct energy with the tolerance of test_energy_fmm_against_fp64_direct_energy; and
kd_info().long_lists / warm_builds / warm_misses / build_mode, which describe HOW a context got to its result (k_fmm_kd.hip:194-199:
"the choice only moves the long ones") and are recorded in the assertion messages only.  For the same reason -- no fresh context
has the tree of the middle of a reuse schedule -- the introspection calls among part D's interlopers (nbco_kd_get_info, the copies
of both lists and of the locals) are held to the tree's own arrays (the pair count equals nbutil.directed_pairs of the copied
mult and P2P list; the lists hold info.p2p_pairs / m2l_pairs distinct node pairs inside the tree; the locals are finite): what
they are there for is that the schedule they interrupt ends in the uninterrupted run's state, bit for bit.  The reference of the
nbco_energy_fmm interloper is nbco_energy of a fresh context on the same state (an O(N^2) fp64 sum on the CPU at N = 65536 in
every run would dominate the module), which test_energy_matches_fp64_direct_sum holds to the oracle.

Every precondition is an assertion computed from the oracle on the CPU before the GPU is touched."""
import numpy as np
import pytest

from nbutil import assert_same_tree, canon_pairs, directed_pairs, drive_by_hand, force_err, list_entries_changed, p2p_work_units

pytestmark = pytest.mark.gpu

THREADS = 16
TREE_ARRAYS = ("index", "mult", "splitdim", "lbound", "rbound", "center", "unsort")
_states, _oracle = {}, {}      # inputs and oracle evaluations shared by the tests of this module (the oracle dominates its running time)


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def zeros3(n):
    import torch
    return torch.zeros((n, 3), dtype=torch.float32, device="cuda")


def state(o, n, kind="ball"):
    """[pos | vel | acc] of the reference's Gaussian ball (or its -test cube), host array"""
    key = (kind, n)
    if key not in _states:
        # (the reference normalises its ball to the sample's own moments, which a single particle does not have: NaN at n = 1;
        #  sizes below 16 take the first particles of the 300-particle state instead)
        _states[key] = o.init_reference(n, test_mode=(kind == "cube")) if n >= 16 else np.ascontiguousarray(o.init_reference(300)[:, :n])
        assert np.isfinite(_states[key]).all(), key
    return _states[key]


class Want:
    """one oracle evaluation: accelerations in the caller's order, the tree dict and the permutation"""

    def __init__(self, o, buf, p, radius, dens, m2l_first=0):
        n = buf.shape[1]
        _, self.a = o.fmm_kd(buf[:2], o.params(n), p=p, threads=THREADS, unsort=True, radius=float(np.float32(radius)),
                             dens_inhom=float(np.float32(dens)), m2l_first=m2l_first)
        self.tree, self.perm, self.n = o.kd_tree(), o.kd_unsort(n), n


def oracle_kd(o, n, p, radius=1.0, dens=1.0, kind="ball", m2l_first=0):
    key = (kind, n, p, float(radius), float(dens), m2l_first)
    if key not in _oracle:
        _oracle[key] = Want(o, state(o, n, kind), p, radius, dens, m2l_first)
    return _oracle[key]


# ---- snapshots of one kd-tree evaluation and the two bars ---------------------------------------------------------------------
def kd_snapshot(e, d, a):
    """everything bar (F) compares, copied off the context that has just evaluated [pos | vel] = d into a"""
    import torch
    torch.cuda.synchronize()
    info = e.kd_info()
    s = dict(a=a.clone(), d=d[:2].clone(), shape=(info.L, info.ntot, info.n, info.order, info.mlt_max, info.real_bytes),
             pairs=(info.p2p_pairs, info.m2l_pairs, info.directed_p2p), halves=info.p2p_halves, rebuilt=info.rebuilt,
             how="build_mode %d long_lists %d warm %d/%d" % (info.build_mode, info.long_lists, info.warm_misses, info.warm_builds))
    for name in TREE_ARRAYS:
        s[name] = e.kd_array(name)
    for name in ("p2p", "m2l"):
        s[name] = canon_pairs(e.kd_array(name))
    return s


def kd_eval(e, src, n, prm):
    """one nbco_fmm_kdtree call of context e on a copy of the device state src"""
    d = src[:2].clone()
    a = zeros3(n)
    e.fmm_cart3_kdtree(d, a, n, prm)
    return kd_snapshot(e, d, a)


def kd_fresh(opts, src, n, prm):
    from coulomb_oscillators_amd import Engine
    e = Engine(**opts)
    try:
        return kd_eval(e, src, n, prm)
    finally:
        e.close()


def assert_fresh_equal(live, fresh, what):
    """bar (F)"""
    import torch
    msg = "%s [long-lived: %s | fresh: %s]" % (what, live["how"], fresh["how"])
    for k in ("shape", "pairs", "halves"):
        assert live[k] == fresh[k], "%s: %s %s != %s" % (msg, k, live[k], fresh[k])
    for k in TREE_ARRAYS + ("p2p", "m2l"):
        assert np.array_equal(live[k], fresh[k]), "%s: kd_array(%s) differs from the fresh context's" % (msg, k)
    assert torch.equal(live["d"][0], fresh["d"][0]), msg + ": positions differ from the fresh context's"
    assert torch.equal(live["d"][1], fresh["d"][1]), msg + ": velocities differ from the fresh context's"
    bad = int((live["a"] != fresh["a"]).any(dim=1).sum())
    assert torch.equal(live["a"], fresh["a"]), "%s: accelerations of %d particles differ from the fresh context's" % (msg, bad)


def assert_oracle(e, snap, want, buf, unsort, what):
    """bar (O) for the evaluation `snap` that context e has just made of the host state buf"""
    try:
        assert_same_tree(e, want.tree, want.n, want.perm)
    except AssertionError as ex:
        raise AssertionError("%s: %s" % (what, ex)) from None
    a_ref, pv = (want.a, buf[:2]) if unsort else (want.a[want.perm], buf[:2][:, want.perm])
    np.testing.assert_array_equal(snap["d"].cpu().numpy(), pv, err_msg=what + ": [pos | vel]")
    err = force_err(snap["a"].cpu().numpy(), a_ref)
    print("%s: force_err %.3e (%s)" % (what, err, snap["how"]))
    assert err < 1e-5, (what, err)
    return err


# ---- A. the launch estimate falls short: later trips of the near-field stride loops ------------------------------------------
SMALL = dict(n=4096, p=6, r=1.0, dens=1.0, mlt=1)
#        n, order, tree_radius, dens_inhom, particles per leaf, p2p_halves under p2p_mutual
ROWS = [dict(n=65536, p=3, r=2.0, dens=1.0, mlt=8, halves=0), dict(n=65536, p=4, r=2.5, dens=1.0, mlt=16, halves=0),
        dict(n=65536, p=6, r=3.0, dens=1.0, mlt=32, halves=1), dict(n=100000, p=8, r=3.0, dens=1.0, mlt=49, halves=2),
        dict(n=100000, p=8, r=3.0, dens=0.5, mlt=98, halves=4)]
VARIANTS = {"one_directional": dict(p2p_mutual=0, unsort=1), "mutual": dict(p2p_mutual=1, unsort=1),
            "tree_order": dict(p2p_mutual=0, unsort=0, tree_steps=1)}


def row_opts(row):
    return dict(fmm_order=row["p"], tree_radius=row["r"], dens_inhom=row["dens"])


def row_want(o, row):
    return oracle_kd(o, row["n"], row["p"], row["r"], row["dens"])


def estimate_preconditions(o, rows):
    """From the oracle's lists alone: every large evaluation that follows the small one has at least 4 x as many near-field work
    units as the launch estimate taken from the small evaluation's list.  Returns the ratios."""
    h_small = len(row_want(o, SMALL).tree["p2p"])
    ratios = []
    for row in rows:
        t = row_want(o, row).tree
        units, estimate, longest = p2p_work_units(t)
        est = estimate(h_small)
        print("n %d p %d r %g dens %g: L %d, %d leaf pairs, longest target list %d, %d work units, estimate %d after %d pairs: %.1f"
              % (row["n"], row["p"], row["r"], row["dens"], t["L"], len(t["p2p"]), longest, units, est, h_small, units / est))
        assert units >= 4 * est, (row, units, est)
        assert (row["n"] - 1) // (1 << t["L"]) + 1 == row["mlt"], row
        ratios.append(units / est)
    return ratios


def run_alternation(o, base, rows=ROWS, oracle=True, descend=True):
    """small, rows[0], small, rows[1], ... on ONE context, each evaluation held to (F) and the large ones to (O); then the rows
    backwards without the small evaluation in between (a live estimate that is about right or too large), (F) only."""
    from coulomb_oscillators_amd import Engine
    ratios = estimate_preconditions(o, rows)
    unsort = base.get("unsort", 1)
    live = Engine(**base)
    fresh, devs = {}, {}

    def evaluate(row, tag, held_to_oracle):
        n = row["n"]
        if n not in devs:
            devs[n] = (dev(state(o, n)), dev(o.params(n)))
        src, prm = devs[n]
        live.set(**row_opts(row))
        got = kd_eval(live, src, n, prm)
        key = (n, row["p"], row["r"], row["dens"])
        if key not in fresh:
            fresh[key] = kd_fresh(dict(base, **row_opts(row)), src, n, prm)
        what = "%s: n %d p %d r %g dens %g %s" % (tag, n, row["p"], row["r"], row["dens"], base)
        assert got["rebuilt"] == 1, what
        assert_fresh_equal(got, fresh[key], what)
        if "halves" in row:
            # the kernel the row was chosen for: p2p_kernel<8|16|32|64> by the leaf size, or the mutual kernel's 1, 2 or 4 halves
            assert got["shape"][4] == row["mlt"], (what, got["shape"])
            assert got["halves"] == (row["halves"] if base.get("p2p_mutual") else 0), (what, got["halves"], got["how"])
        if held_to_oracle:
            assert_oracle(live, got, row_want(o, row), state(o, n), unsort, what)

    for i, row in enumerate(rows):
        evaluate(SMALL, "small before row %d" % (i + 1), False)
        evaluate(row, "row %d after the small evaluation (work units / estimate %.1f)" % (i + 1, ratios[i]), oracle)
    if descend:
        for i in reversed(range(len(rows))):
            evaluate(rows[i], "row %d, descending" % (i + 1), False)
    live.close()


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_near_field_launch_estimate_falls_short(oracle32, variant):
    """Part A.  launch_p2p (k_p2p.hpp) starts one wave per work unit of an estimate taken from the PREVIOUS evaluation's list
    (k_fmm_kd.hip:498-501); a fresh context has none and launches for the full capacity, so only here does a wave take a second
    work unit through the software-pipelined hand-off (ck = nk; pt = npt; dsc = ndsc).  The same estimate sizes list_fill_kernel,
    traverse_init_kernel, p2p_link and, under p2p_mutual, the reaction records, whose overflow repeats the evaluation
    (react_overflow).  Ratios work units / estimate of the five rows after the small evaluation, from the oracle's lists:
    7.5, 19.3, 28.7, 32.6, 21.2."""
    run_alternation(oracle32, VARIANTS[variant])


def test_near_field_launch_estimate_falls_short_far_fp64(oracle32, oracle64):
    """Part A, rows 4 and 5 (p = 8) with the fp64 far field: (F), the fp32 geometry and lists bit-exact, and the bars of
    test_far_fp64_kdtree_against_both_oracles against the REAL = double oracle."""
    from coulomb_oscillators_amd import Engine
    o = oracle32
    rows = ROWS[3:]
    estimate_preconditions(o, rows)
    doubles = []
    for row in rows:
        n = row["n"]
        _, want64 = oracle64.fmm_kd(state(o, n)[:2].astype(np.float64), o.params(n).astype(np.float64), p=row["p"], threads=THREADS, unsort=True,
                                    radius=row["r"], dens_inhom=row["dens"])
        tree64 = oracle64.kd_tree()
        # for these two inputs the double oracle's lists equal the fp32 ones, so its accelerations are comparable
        for k in ("p2p", "m2l"):
            assert np.array_equal(canon_pairs(tree64[k]), canon_pairs(row_want(o, row).tree[k])), (row, k)
        doubles.append(want64)
    live = Engine(far_fp64=1, unsort=1)
    for row, want64 in zip(rows, doubles):
        n = row["n"]
        buf, src, prm = state(o, n), dev(state(o, n)), dev(o.params(n))
        for r in (SMALL, row):
            s, p = (dev(state(o, r["n"])), dev(o.params(r["n"]))) if r is SMALL else (src, prm)
            live.set(**row_opts(r))
            got = kd_eval(live, s, r["n"], p)
            what = "far_fp64 n %d p %d dens %g" % (r["n"], r["p"], r["dens"])
            assert got["shape"][5] == 8, what
            assert_fresh_equal(got, kd_fresh(dict(far_fp64=1, unsort=1, **row_opts(r)), s, r["n"], p), what)
        assert_oracle(live, got, row_want(o, row), buf, 1, what)
        got32 = kd_fresh(dict(far_fp64=0, unsort=1, **row_opts(row)), src, n, prm)
        e64, e32 = force_err(got["a"].cpu().numpy(), want64), force_err(got32["a"].cpu().numpy(), want64)
        print("%s: against the double oracle %.3e (all-fp32 evaluation: %.3e)" % (what, e64, e32))
        assert e64 < 1e-5 and e64 < 1.5 * e32 + 2e-7, (what, e64, e32)
    live.close()


RADII = (1.11, 1.25, 1.43, 1.67, 2.0, 2.5, 3.0)
# grid points of the -accuracy walk at N = 65536 where the near field has more work units than the estimate left by the point before
SHORT_POINTS = {(2.0, 2), (2.5, 1), (2.5, 2), (3.0, 1), (3.0, 2)}


def test_accuracy_walk_of_nbco3_on_one_context(oracle32):
    """Part A.  nbco3 -accuracy (host/nbco3.cpp search_parameters over Session::mean_error) replayed at N = 65536 on one context:
    42 changes of (tree_radius, fmm_order) with coll = 1, unsort = 1, between them nbco_direct3 / nbco_copy (first point only, the
    reference sum is cached) / nbco_fmm_kdtree / nbco_mean_relerr and the evaluations of the timing loop.  (F) at every point, (O) at
    the five points where the estimate left by the point before is too small (ratios 1.09, 1.02, 1.12, 1.40, 1.11), at the first
    and at the last.  Then, as Session::simulate does, the context goes to unsort = 0, sync = 0, tree_steps = 8, m2l_first = 1 at
    the chosen (r, p) and takes 10 leapfrog steps: (F) on the final state."""
    import torch
    from coulomb_oscillators_amd import Engine, EVAL_FMM_KDTREE, INTEG_LEAPFROG
    o = oracle32
    n = 65536
    buf, par = state(o, n), o.params(n)
    grid = [(r, p) for r in RADII for p in range(1, 7)]
    held = SHORT_POINTS | {grid[0], grid[-1]}
    # preconditions, from the oracle alone
    prev, wants = None, {}
    for r, p in grid:
        w = Want(o, buf, p, r, 1.0)
        units, estimate, _ = p2p_work_units(w.tree)
        if prev is not None:
            short = units > estimate(prev)
            assert short == ((r, p) in SHORT_POINTS), (r, p, units, estimate(prev))
        prev = len(w.tree["p2p"])
        if (r, p) in held:
            wants[(r, p)] = w
    src, prm = dev(buf), dev(par)
    live = Engine(fmm_order=3)
    d = src.clone()
    ref_acc = zeros3(n)
    fresh_direct = None
    errs = {}
    for r, p in grid:
        live.set(coll=1, unsort=1, tree_radius=r, fmm_order=p)
        if fresh_direct is None:
            live.direct3(d, d[2], n, prm)
            live.copy(ref_acc, d[2], n)
            f = Engine()
            fresh_direct = zeros3(n)
            f.direct3(src, fresh_direct, n, prm)
            f.close()
            assert torch.equal(ref_acc, fresh_direct), "direct3 / copy on the long-lived context"
        live.fmm_cart3_kdtree(d, d[2], n, prm)
        got = kd_snapshot(live, d, d[2])
        err = live.mean_relerr(d[2], ref_acc, n)
        what = "-accuracy r %g p %d" % (r, p)
        assert_fresh_equal(got, kd_fresh(dict(coll=1, unsort=1, tree_radius=r, fmm_order=p), src, n, prm), what)
        want_err = o.mean_relerr(got["a"].cpu().numpy(), ref_acc.cpu().numpy())
        assert abs(err - want_err) <= 2e-5 * want_err + 1e-12, (what, err, want_err)       # the bar of test_reductions
        errs[(r, p)] = err
        if (r, p) in held:
            assert_oracle(live, got, wants[(r, p)], buf, 1, what)
        for _ in range(2):                                        # seconds_per_evaluation(0): one untimed call, one timed
            live.fmm_cart3_kdtree(d, d[2], n, prm)
        torch.cuda.synchronize()
        assert torch.equal(d[2], got["a"]), what + ": the same evaluation again"
    assert torch.equal(d[:2], src[:2])                              # unsort = 1 throughout: the state was never permuted
    r, p = ([k for k in grid if errs[k] < 1e-4] or grid[-1:])[0]      # (nbco3 takes the fastest admissible point; any will do here)
    final = []
    for e in (live, Engine(coll=1, unsort=1, tree_radius=r, fmm_order=p)):
        e.set(tree_radius=r, fmm_order=p)
        e.set(unsort=0, sync=0, tree_steps=8, m2l_first=1)
        s = src.clone()
        e.compute_force(EVAL_FMM_KDTREE, s, n, prm)
        e.integrate_steps(INTEG_LEAPFROG, EVAL_FMM_KDTREE, s, n, prm, 5e-4, 10)
        torch.cuda.synchronize()
        final.append(s)
        e.close()
    assert torch.equal(final[0], final[1]), "10 leapfrog steps after the walk (r %g, p %d)" % (r, p)


# ---- B. a walk through sizes -------------------------------------------------------------------------------------------------
SIZES = [65536, 4096, 100003, 4097, 65536, 1, 300, 262144, 30001, 8193, 65536]
SIZES_ORACLE = {2: 100003, 3: 4097, 7: 262144, 10: 65536}      # step -> n


@pytest.mark.parametrize("unsort", [1, 0])
def test_walk_through_sizes_kdtree(oracle32, unsort):
    """Part B.  Grow-only scratch (nbco_ctx::reserve) shared between entry points, perm_primed_n (one particle count only), the
    warm select's pivots of a tree of another size, the estimate of another size's list: one context, p = 5, eleven particle counts
    up and down.  (F) at every step, (O) at 100003, 4097, 262144 and the last 65536."""
    from coulomb_oscillators_amd import Engine
    o = oracle32
    p = 5
    for step, n in SIZES_ORACLE.items():
        assert SIZES[step] == n
        oracle_kd(o, n, p)                      # (the oracle evaluates them: before the GPU is touched)
    base = dict(fmm_order=p, unsort=unsort)
    live = Engine(**base)
    fresh = {}
    for step, n in enumerate(SIZES):
        src, prm = dev(state(o, n)), dev(o.params(n))
        got = kd_eval(live, src, n, prm)
        if n not in fresh:
            fresh[n] = kd_fresh(base, src, n, prm)
        what = "size walk step %d: n %d unsort %d" % (step, n, unsort)
        assert_fresh_equal(got, fresh[n], what)
        if step in SIZES_ORACLE:
            assert_oracle(live, got, oracle_kd(o, n, p), state(o, n), unsort, what)
    live.close()


def oct_snapshot(e, d, a):
    import torch
    torch.cuda.synchronize()
    info = e.oct_info()
    s = dict(a=a.clone(), d=d.clone(), shape=(info.L, info.ntot, info.order, info.tpl, info.n, info.m2l_entries, info.p2p_groups, info.p2p_desc,
                                              info.p2p_chunks, info.real_bytes))
    for name in ("keys", "perm"):
        s[name] = e.oct_array(name)
    # what an octree evaluation writes and reads of its cell arrays (test_cells_bit_exact_and_forces compares the same ranges):
    # levels 0 and 1 carry nothing -- every kernel of k_fmm_oct.hip starts at node 9 -- and the particle ranges are those of
    # the leaf level; the slots before them keep whatever the allocation held
    s["mult"] = e.oct_array("mult")[9:]
    s["index"] = e.oct_array("index")[((1 << (3 * info.L)) - 1) // 7:]
    return s


def other_eval(e, which, src, n, prm):
    """one call of the evaluator `which` on a copy of the device state; dict of everything (F) compares"""
    import torch
    d = src[:2].clone()
    a = zeros3(n)
    if which in ("fmm_cart3_traceless", "fmm_cart3"):
        getattr(e, which)(d, a, n, prm)
        return oct_snapshot(e, d, a)
    getattr(e, which)(d[0], a, n, prm)
    torch.cuda.synchronize()
    return dict(a=a, d=d)


def assert_same_dict(live, fresh, what):
    import torch
    assert live.keys() == fresh.keys()
    for k, v in live.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(v, fresh[k]), "%s: %s differs from the fresh context's" % (what, k)
        elif isinstance(v, np.ndarray):
            assert np.array_equal(v, fresh[k]), "%s: %s differs from the fresh context's" % (what, k)
        else:
            assert v == fresh[k], "%s: %s %s != %s" % (what, k, v, fresh[k])


@pytest.mark.parametrize("which", ["fmm_cart3_traceless", "fmm_cart3", "direct", "direct3"])
def test_walk_through_sizes_other_evaluators(oracle32, which):
    """Part B, the octree and direct evaluators on contexts of their own (n <= 100003): pos4 and part are shared by the direct sum,
    the energy reduction, the octree and the kd near field.  (F) at every step: accelerations, the permuted state, and for the
    octree keys, permutation and cell arrays."""
    from coulomb_oscillators_amd import Engine
    o = oracle32
    base = dict(fmm_order=5)
    live = Engine(**base)
    fresh = {}
    for step, n in enumerate([n for n in SIZES if n <= 100003]):
        src, prm = dev(state(o, n)), dev(o.params(n))
        got = other_eval(live, which, src, n, prm)
        if n not in fresh:
            f = Engine(**base)
            fresh[n] = other_eval(f, which, src, n, prm)
            f.close()
        assert_same_dict(got, fresh[n], "%s size walk step %d: n %d" % (which, step, n))
    live.close()


def state2d(n):
    from coulomb_oscillators_amd import init2d
    import fmm2d_numpy as F2
    A, om, xi, om0 = F2.kv_params()
    return init2d(n, "kv", A, om), np.array([xi / n, 0.0, om0[0] ** 2, om0[1] ** 2])


def fmm2d_eval(e, n):
    import torch
    st, par = state2d(n)
    d = torch.from_numpy(st.reshape(-1).copy()).cuda()
    a = torch.zeros((n, 2), dtype=torch.float64, device="cuda")
    e.fmm_2d(d, a, n, torch.from_numpy(par).cuda())
    torch.cuda.synchronize()
    return dict(a=a, d=d)


def test_mixed_walk_of_evaluators_on_one_context(oracle32):
    """Part B.  Consecutive calls of ONE context go to different evaluators at different n: kd, octree traceless, direct3, kd,
    symmetric octree, energy, kd, 2-D FMM on a state of its own, kd.  (F) for each call; the third and the last kd call to (O)."""
    from coulomb_oscillators_amd import Engine
    o = oracle32
    p = 5
    base = dict(fmm_order=p, unsort=1)
    calls = [("kd", 65536), ("fmm_cart3_traceless", 30001), ("direct3", 5000), ("kd", 100003), ("fmm_cart3", 20000), ("energy", 3000),
             ("kd", 4097), ("fmm_2d", 30001), ("kd", 65536)]
    for n in (4097, 65536):
        oracle_kd(o, n, p)
    live = Engine(**base)
    kd_calls = 0
    for step, (which, n) in enumerate(calls):
        what = "mixed walk step %d: %s n %d" % (step, which, n)
        f = Engine(**base)
        if which == "fmm_2d":
            assert_same_dict(fmm2d_eval(live, n), fmm2d_eval(f, n), what)
        elif which == "energy":
            b, prm = dev(state(o, n)), dev(o.params(n))
            assert live.energy(b, n, prm) == f.energy(b, n, prm), what
        elif which == "kd":
            src, prm = dev(state(o, n)), dev(o.params(n))
            got = kd_eval(live, src, n, prm)
            assert_fresh_equal(got, kd_eval(f, src, n, prm), what)
            kd_calls += 1
            if kd_calls in (3, 4):
                assert_oracle(live, got, oracle_kd(o, n, p), state(o, n), 1, what)
        else:
            kind = "cube" if which.startswith("fmm") else "ball"
            src, prm = dev(state(o, n, kind)), dev(o.params(n))
            assert_same_dict(other_eval(live, which, src, n, prm), other_eval(f, which, src, n, prm), what)
        f.close()
    live.close()


# ---- C. options that change under a live tree --------------------------------------------------------------------------------
class Leapfrog:
    """One context taking leapfrog steps by hand (main3.cu:832-846 over integrator.cuh:68-80: force; then per step kick, drift,
    force, kick) on the tree-ordered state, the Coulomb part and the trap in two calls so that every evaluation can be compared
    on its own (near the trap's equilibrium the elastic term cancels much of the Coulomb force)."""

    def __init__(self, o, n, dt=5e-4, **opts):
        from coulomb_oscillators_amd import Engine
        self.o, self.n, self.dt, self.opts = o, n, float(np.float32(dt)), dict(opts)
        self.e = Engine(**opts)
        self.d, self.prm = dev(state(o, n)), dev(o.params(n))
        self.k = 0

    def set(self, **kw):
        self.e.set(**kw)
        self.opts.update(kw)

    def evaluate(self):
        """the next force evaluation: (state that entered it, snapshot taken before the trap is added)"""
        e, d, n, dt = self.e, self.d, self.n, self.dt
        if self.k:
            e.step(d[1], d[2], dt / 2, n)
            e.step(d[0], d[1], dt, n)
        x_in = d.clone()
        e.fmm_cart3_kdtree(d, d[2], n, self.prm)
        snap = kd_snapshot(e, d, d[2])
        e.add_elastic(d[0], d[2], n, self.prm[3:])
        if self.k:
            e.step(d[1], d[2], dt / 2, n)
        self.k += 1
        return x_in, snap

    def fresh(self, x_in):
        return kd_fresh(self.opts, x_in, self.n, self.prm)

    def held_to_oracle(self, x_in, snap, what, oracle64=None):
        """(O) on the state the evaluation received (the oracle follows the GPU's state).  With far_fp64 set it is the bar of
        test_far_fp64_kdtree_against_both_oracles: the fp32 geometry and lists bit-exact and within 1e-5 of the fp32 oracle, and
        against the REAL = double oracle within 1e-5 and no further from it than the all-fp32 evaluation of a fresh context
        (wherever the double oracle's lists equal the fp32 ones: they differ only when a node pair sits within fp32 rounding of
        the opening criterion)."""
        buf = x_in.cpu().numpy()
        p, m2l_first = self.opts["fmm_order"], self.opts.get("m2l_first", 0)
        w = Want(self.o, buf, p, self.opts.get("tree_radius", 1.0), self.opts.get("dens_inhom", 1.0), m2l_first)
        err = assert_oracle(self.e, snap, w, buf, self.opts.get("unsort", 1), what)
        if self.opts.get("far_fp64"):
            assert oracle64 is not None and snap["shape"][5] == 8, what
            _, want64 = oracle64.fmm_kd(buf[:2].astype(np.float64), self.o.params(self.n).astype(np.float64), p=p, threads=THREADS, unsort=True,
                                        m2l_first=m2l_first, radius=self.opts.get("tree_radius", 1.0), dens_inhom=self.opts.get("dens_inhom", 1.0))
            tree64, perm = oracle64.kd_tree(), oracle64.kd_unsort(self.n)
            if all(np.array_equal(canon_pairs(tree64[k]), canon_pairs(w.tree[k])) for k in ("p2p", "m2l")):
                if not self.opts.get("unsort", 1):
                    want64 = want64[perm]
                got32 = kd_fresh(dict(self.opts, far_fp64=0), x_in, self.n, self.prm)
                e64, e32 = force_err(snap["a"].cpu().numpy(), want64), force_err(got32["a"].cpu().numpy(), want64)
                print("%s: against the double oracle %.3e (all-fp32 evaluation: %.3e)" % (what, e64, e32))
                assert e64 < 1e-5 and e64 < 1.5 * e32 + 2e-7, (what, e64, e32)
        return err


def test_option_toggles_rebuild_and_match_a_fresh_context(oracle32, oracle64):
    """Part C1, tree_steps = 1, unsort = 0, N = 65536, leapfrog steps with dt = 5e-4.  Each option of the `topo` rule of nbco_set_opts
    and of the topo_change rule of kd_build is toggled between two evaluations: fmm_order 6 -> 10 -> 6 -> 9 -> 3 (generated
    bodies <-> the workgroup-per-node far field of farfield_wide.hpp), far_fp64, p2p_mutual, track_order, dens_inhom, tree_L,
    list_factor.  The evaluation after each toggle reports rebuilt == 1 and satisfies (F); (O) after the changes of order and of
    far_fp64."""
    run = Leapfrog(oracle32, 65536, fmm_order=6, unsort=0, tree_steps=1)
    x_in, snap = run.evaluate()
    assert_fresh_equal(snap, run.fresh(x_in), "first evaluation")
    toggles = [dict(fmm_order=10), dict(fmm_order=6), dict(fmm_order=9), dict(fmm_order=3), dict(fmm_order=6),
               dict(far_fp64=1), dict(far_fp64=0), dict(p2p_mutual=1), dict(p2p_mutual=0), dict(track_order=1), dict(track_order=0),
               dict(dens_inhom=2.0), dict(dens_inhom=1.0), dict(tree_L=12), dict(tree_L=0), dict(list_factor=24), dict(list_factor=48)]
    for change in toggles:
        run.set(**change)
        x_in, snap = run.evaluate()
        what = "evaluation %d after %s" % (run.k - 1, change)
        assert snap["rebuilt"] == 1, what
        assert_fresh_equal(snap, run.fresh(x_in), what)
        if "fmm_order" in change or "far_fp64" in change:
            run.held_to_oracle(x_in, snap, what, oracle64)
    run.e.close()


def test_unsort_toggles_inside_a_reuse_schedule(oracle32):
    """Part C1, unsort 1 -> 0 -> 1 -> 0 on a context whose tree_steps stays 8.  Each change comes after 3 evaluations with the old
    value, so the schedule's own counter is not at a multiple of 8 and a rebuild can only come from the change itself: a tree built
    for the caller's order must not be reused on a state that is expected in tree order.  The evaluation after each change
    reports rebuilt == 1 and satisfies (F) and (O)."""
    run = Leapfrog(oracle32, 65536, fmm_order=4, unsort=1, tree_steps=8)
    for unsort in (1, 0, 1, 0):
        run.set(unsort=unsort)
        for k in range(3):
            x_in, snap = run.evaluate()
            what = "unsort = %d, evaluation %d with it (%d of the context)" % (unsort, k, run.k - 1)
            assert snap["rebuilt"] == (1 if unsort or k == 0 else 0), what
            if k == 0:
                assert_fresh_equal(snap, run.fresh(x_in), what)
                run.held_to_oracle(x_in, snap, what)
    run.e.close()


TOPO_CHANGES = [dict(fmm_order=6), dict(dens_inhom=2.0), dict(tree_L=13), dict(p2p_mutual=1), dict(track_order=1)]


@pytest.mark.parametrize("change", TOPO_CHANGES, ids=lambda c: "%s=%s" % next(iter(c.items())))
def test_topology_options_restart_a_reuse_schedule(oracle32, change):
    """Part C1, the rule written next to tree_steps in include/nbco.h, option by option: under tree_steps = 8 (where a rebuild
    has to be earned) a change of fmm_order, dens_inhom, tree_L, p2p_mutual or track_order before evaluation 3 makes that
    evaluation rebuild -- (F) -- and restarts the schedule: evaluations 4..10 reuse its tree and evaluation 11 rebuilds."""
    run = Leapfrog(oracle32, 65536, fmm_order=4, unsort=0, tree_steps=8)
    rebuilt = []
    for k in range(13):
        if k == 3:
            run.set(**change)
        x_in, snap = run.evaluate()
        rebuilt.append(snap["rebuilt"])
        if k == 3:
            assert snap["rebuilt"] == 1, change
            assert_fresh_equal(snap, run.fresh(x_in), "evaluation 3, after %s" % change)
    assert rebuilt == [1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0], (change, rebuilt)
    run.e.close()


C2_CHANGES = [dict(tree_radius=1.5), dict(m2l_first=1), dict(coll=0), dict(eps2=1e-8)]


@pytest.mark.parametrize("change", C2_CHANGES, ids=lambda c: "%s=%s" % next(iter(c.items())))
def test_options_outside_the_tree_build_change_inside_a_schedule(oracle32, change):
    """Part C2.  tree_radius, m2l_first, coll and eps2 do not enter the tree build and are not in the `topo` rule of nbco_set_opts:
    changed at evaluation 3 of a tree_steps = 8 schedule they leave the tree alone (rebuilt stays 0 until the schedule's own
    rebuild at evaluation 8, include/nbco.h) and take effect at once on the traversal and the kernels.  A fresh context that made
    the same change would share any mistake, so the bar is (O) alone: every evaluation against the oracle's evaluation of the same
    input, rebuilding at 0 and 8 and reusing its tree (reuse = 1) with the NEW value from evaluation 3 on -- tree and lists
    bit-exact, force_err < 1e-5."""
    import torch
    from coulomb_oscillators_amd import Engine
    o = oracle32
    n, p, tree_steps, evals = 65536, 4, 8, 10
    dt = float(np.float32(5e-4))
    buf, par = state(o, n), o.params(n)
    okw = dict(radius=1.0, m2l_first=0, coll=True, eps2=1e-18)
    count = [0]
    # the change can be seen: from the oracle alone, the old and the new value give different lists (or forces) on the same state
    new = dict(okw, **{{"tree_radius": "radius"}.get(k, k): v for k, v in change.items()})
    _, a_old = o.fmm_kd(buf[:2], par, p=p, threads=THREADS, unsort=False, **okw)
    t_old = o.kd_tree()
    _, a_new = o.fmm_kd(buf[:2], par, p=p, threads=THREADS, unsort=False, **new)
    if "tree_radius" in change or "m2l_first" in change:
        assert list_entries_changed(t_old, o.kd_tree()) >= 1000
    else:
        assert force_err(a_new, a_old) > 1e-4
    eng = Engine(fmm_order=p, unsort=0, tree_steps=tree_steps)
    d, prm = dev(buf), dev(par)

    def force():
        if count[0] == 3:
            eng.set(**change)
            for k, v in change.items():
                okw[{"tree_radius": "radius"}.get(k, k)] = float(np.float32(v)) if isinstance(v, float) else v
        count[0] += 1
        eng.fmm_cart3_kdtree(d, d[2], n, prm)

    def compare(k, x_in):
        torch.cuda.synchronize()
        reuse = k % tree_steps != 0
        pv, a_ref = o.fmm_kd(x_in, par, p=p, threads=THREADS, unsort=False, reuse=int(reuse), **okw)
        want = o.kd_tree()
        info = eng.kd_info()
        what = "evaluation %d (%s) with %s" % (k, "reuse" if reuse else "rebuild", change if k >= 3 else "the old value")
        assert info.rebuilt == (0 if reuse else 1), what
        try:
            if okw["coll"]:
                assert_same_tree(eng, want, n, o.kd_unsort(n))
            else:
                # the traversal does not depend on coll and still writes both lists; only the directed pair count of
                # nbco_kd_get_info is left out: it is taken from the sorted near-field list, which coll = 0 does not build
                for name in ("index", "mult", "splitdim", "lbound", "rbound", "center"):
                    np.testing.assert_array_equal(eng.kd_array(name), want[name], err_msg=name)
                np.testing.assert_array_equal(eng.kd_array("unsort"), o.kd_unsort(n), err_msg="unsort")
                assert (info.p2p_pairs, info.m2l_pairs) == (len(want["p2p"]), len(want["m2l"]))
                for name in ("p2p", "m2l"):
                    np.testing.assert_array_equal(canon_pairs(eng.kd_array(name)), canon_pairs(want[name]), err_msg=name)
        except AssertionError as ex:
            raise AssertionError("%s: %s" % (what, ex)) from None
        got = d.cpu().numpy()
        np.testing.assert_array_equal(got[:2], pv, err_msg=what)
        err = force_err(got[2], a_ref)
        print("%s: lists p2p %d m2l %d, force_err %.3e" % (what, len(want["p2p"]), len(want["m2l"]), err))
        assert err < 1e-5, (what, err)
        eng.add_elastic(d[0], d[2], n, prm[3:])

    drive_by_hand(eng, d, n, prm, dt, evals, force, compare)
    eng.close()


def test_far_fp64_toggle_inside_a_schedule_keeps_the_schedule(oracle32, oracle64):
    """Part C3.  far_fp64 changes the width of the expansions, so kd_build throws the tree away (topo_change): the evaluation
    after the toggle rebuilds.  The schedule itself does not restart (include/nbco.h, far_fp64): the context keeps counting its
    evaluations and the next scheduled rebuild is at the next multiple of tree_steps -- toggled at evaluation 3 of a tree_steps = 8
    schedule, evaluations 4..7 reuse the tree of evaluation 3 and evaluation 8 rebuilds.  (F) and (O) at evaluation 3."""
    run = Leapfrog(oracle32, 65536, fmm_order=8, unsort=0, tree_steps=8)
    rebuilt = []
    for k in range(10):
        if k == 3:
            run.set(far_fp64=1)
        x_in, snap = run.evaluate()
        rebuilt.append(snap["rebuilt"])
        if k == 3:
            assert snap["shape"][5] == 8
            assert_fresh_equal(snap, run.fresh(x_in), "evaluation 3, after far_fp64 = 1")
            run.held_to_oracle(x_in, snap, "evaluation 3, after far_fp64 = 1", oracle64)
    assert rebuilt == [1, 0, 0, 1, 0, 0, 0, 0, 1, 0], rebuilt
    run.e.close()


# ---- D. calls in between must not disturb a schedule -------------------------------------------------------------------------
INTERLOPERS = ["direct3_elsewhere", "energy", "energy_fmm", "reductions", "kd_info", "kd_lists", "kd_local", "traceless_copy", "fmm_2d", "profile"]


class Interlopers:
    """the calls of part D, in rotation, each held to (F) where a fresh context can make the same call"""

    def __init__(self, o, e, d, n, prm, opts):
        from coulomb_oscillators_amd import Engine
        self.o, self.e, self.d, self.n, self.prm, self.opts = o, e, d, n, prm, opts
        self.fresh = Engine(**opts)
        self.turn = 0
        self.profiling = False
        self.other, self.other_prm = dev(state(o, 5000)), dev(o.params(5000))
        self.seen = []

    def next(self):
        import torch
        e, f, d, n, prm = self.e, self.fresh, self.d, self.n, self.prm
        which = INTERLOPERS[self.turn % len(INTERLOPERS)]
        self.turn += 1
        self.seen.append(which)
        what = "interloper %d (%s)" % (self.turn, which)
        if self.profiling:
            times = e.profile_get()               # (ms, launches) per phase of the step that ran with the timers on
            assert all(np.isfinite(ms) and ms >= 0 and cnt >= 0 for ms, cnt in times.values()), (what, times)
            e.profile(False)
            self.profiling = False
        if which == "direct3_elsewhere":
            assert_same_dict(other_eval(e, "direct3", self.other, 5000, self.other_prm), other_eval(f, "direct3", self.other, 5000, self.other_prm), what)
        elif which == "energy":
            assert e.energy(d, n, prm) == f.energy(d, n, prm), what
        elif which == "energy_fmm":
            got = e.energy_fmm(d, n, prm)
            want = f.energy(d, n, prm)                  # fp64 direct sum (held to the oracle by test_energy_matches_fp64_direct_sum)
            assert abs(got[0] - want[0]) <= 1e-6 * want[0] and abs(got[1] - want[1]) <= 1e-6 * want[1], (what, got, want)
            assert abs(got[2] - want[2]) <= 2e-4 * want[2], (what, got, want)       # order 6: test_energy_fmm_against_fp64_direct_energy
        elif which == "reductions":
            assert torch.equal(e.minmax(d[0], n), f.minmax(d[0], n)), what
            assert e.pow_sum(d[1], 2, n) == f.pow_sum(d[1], 2, n), what
            assert e.mean_relerr(d[2], d[1], n) == f.mean_relerr(d[2], d[1], n), what
        elif which == "kd_info":
            info = e.kd_info()              # the pair count is taken on demand from the sorted list, here against the tree's own arrays
            assert info.n == n and info.directed_p2p == directed_pairs(e.kd_array("mult"), e.kd_array("p2p"), info.L), (what, info.directed_p2p)
        elif which == "kd_lists":
            info = e.kd_info()
            for name, cnt in (("p2p", info.p2p_pairs), ("m2l", info.m2l_pairs)):
                pairs = e.kd_array(name)
                assert len(np.unique(canon_pairs(pairs))) == cnt and pairs.min() >= 0 and pairs.max() < info.ntot, (what, name)
        elif which == "kd_local":
            assert np.isfinite(e.kd_array("local")).all(), what
        elif which == "traceless_copy":
            assert_same_dict(other_eval(e, "fmm_cart3_traceless", d, n, prm), other_eval(f, "fmm_cart3_traceless", d, n, prm), what)
        elif which == "fmm_2d":
            assert_same_dict(fmm2d_eval(e, 20000), fmm2d_eval(f, 20000), what)
        elif which == "profile":
            e.profile(True)
            self.profiling = True

    def close(self):
        self.fresh.close()


def run_schedule(o, opts, n=65536, steps=17, dt=5e-4, block=0, interrupted=False, stream=None, switch_stream_at=None):
    """compute_force, then `steps` leapfrog steps (nbco_integrate per step, or nbco_integrate_steps in blocks of `block`), with one
    interloper after every step (two after every block) when `interrupted`; returns the final device state.  stream: a
    torch.cuda.Stream the context is created on and the inputs are produced on; switch_stream_at: the step after which a context
    created on the null stream is moved to it with nbco_set_opts."""
    import contextlib
    import torch
    from coulomb_oscillators_amd import Engine, EVAL_FMM_KDTREE, INTEG_LEAPFROG
    on = stream if (stream is not None and switch_stream_at is None) else None
    with (torch.cuda.stream(on) if on is not None else contextlib.nullcontext()):
        base = dev(state(o, n))
        prm = dev(o.params(n))
        torch.cuda.synchronize()
        e = Engine(stream=on.cuda_stream if on is not None else None, **opts)
        d = base * 1.0                          # produced by a torch operation on the context's stream, right before the call
        e.compute_force(EVAL_FMM_KDTREE, d, n, prm)
        calls = Interlopers(o, e, d, n, prm, opts) if interrupted else None
        done = 0
        moved = contextlib.nullcontext()
        while done < steps:
            if block:
                m = min(block, steps - done)
                e.integrate_steps(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, dt, m)
            else:
                m = 1
                e.integrate(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, dt)
            done += m
            if calls:
                for _ in range(2 if block else 1):
                    calls.next()
            if switch_stream_at is not None and done == switch_stream_at:
                e.set(stream=stream.cuda_stream)            # drains the old stream
                moved = torch.cuda.stream(stream)
                moved.__enter__()
        if on is not None:
            on.synchronize()                    # the one synchronisation of the caller's stream
        elif switch_stream_at is not None:
            stream.synchronize()
            moved.__exit__(None, None, None)
        else:
            torch.cuda.synchronize()
        if calls:
            assert set(calls.seen) == set(INTERLOPERS), calls.seen
            calls.close()
        out = d.clone()
        torch.cuda.synchronize()
        e.close()
    return out


NBCO3 = dict(fmm_order=6, unsort=0, tree_steps=8, m2l_first=1, sync=0)     # what nbco3's simulation runs
_plain = {}


def plain_schedule(o, mutual):
    if mutual not in _plain:
        _plain[mutual] = run_schedule(o, dict(NBCO3, p2p_mutual=mutual))
    return _plain[mutual]


@pytest.mark.parametrize("mutual", [0, 1])
def test_calls_in_between_do_not_disturb_a_schedule(oracle32, mutual):
    """Part D.  N = 65536, p = 6, unsort = 0, tree_steps = 8, m2l_first = 1, sync = 0, 17 leapfrog steps: uninterrupted, and with
    one other call of the same context after every step, in rotation: nbco_direct3 on another array of 5000 particles, nbco_energy,
    nbco_energy_fmm, the reductions, nbco_kd_get_info (the on-demand pair count at counters + 100), the copies of both lists (staged
    through the frontier buffer) and of the locals, the octree evaluator on a copy of the state, the 2-D FMM on a state of its own,
    the per-phase timers.  The final states are bit-identical; so are those of the same two runs taken in nbco_integrate_steps
    blocks of 4 with the calls between the blocks.  The interlopers' own results satisfy (F) (see the module docstring for
    nbco_energy_fmm)."""
    import torch
    o = oracle32
    opts = dict(NBCO3, p2p_mutual=mutual)
    plain = plain_schedule(o, mutual)
    assert torch.isfinite(plain).all()
    for block, interrupted in ((0, True), (4, False), (4, True)):
        got = run_schedule(o, opts, block=block, interrupted=interrupted)
        for part, name in enumerate(("positions", "velocities", "accelerations")):
            assert torch.equal(got[part], plain[part]), "%s differ from the uninterrupted step-by-step run (blocks of %d, interrupted %s)" % (name, block, interrupted)


# ---- E. sticky state ---------------------------------------------------------------------------------------------------------
def tie_inputs(o):
    """the tie-heavy inputs of test_large_tree_bit_exact_selection_build (a few / hundreds of exact ties per pivot) and of
    test_three_pass_select_is_reached_and_succeeds (300 distinct floats inside one bucket of the two-pass key)"""
    n = 65536
    out = []
    for quant in (2e-5, 4e-4):
        buf = state(o, n).copy()
        buf[0] = (np.round(buf[0] / quant) * quant).astype(np.float32)
        out.append(("quant %g" % quant, buf))
    rng = np.random.default_rng(5)
    pos = (rng.random((n, 3), dtype=np.float32) - np.float32(0.5)) * np.array([1.0, 0.8, 0.8], dtype=np.float32)
    k = 300
    half = (n - k) // 2
    x = np.sort(np.abs(pos[:, 0]) + np.float32(1e-3))
    pos[:half, 0] = -x[:half]
    pos[half:n - k, 0] = x[half:n - k]
    pos[n - k:, 0] = (np.arange(k, dtype=np.float64) * 3e-13).astype(np.float32)
    assert len(np.unique(pos[n - k:, 0])) == k
    buf = np.zeros((3, n, 3), dtype=np.float32)
    buf[0] = pos[rng.permutation(n)]
    out.insert(1, ("300 floats in one bucket", buf))
    return out      # a few ties (stays in mode 0), one crowded bucket (mode 1), hundreds of exact ties per pivot (mode 2)


def test_escalated_build_mode_is_sticky_and_harmless(oracle32):
    """Part E1.  sel_three_pass / force_sort_build never go back: one context evaluates tie-heavy inputs until kd_info().build_mode
    has reached 1 and then 2, and then the plain Gaussian ball at N = 65536 and 262144: (F) and (O), whatever build_mode says."""
    from coulomb_oscillators_amd import Engine
    o = oracle32
    p = 5
    ties = tie_inputs(o)
    wants = [Want(o, buf, p, 1.0, 1.0) for _, buf in ties]          # the oracle evaluates these inputs
    for n in (65536, 262144):
        oracle_kd(o, n, p)
    base = dict(fmm_order=p, unsort=1)
    live = Engine(**base)
    modes = []
    for (name, buf), want in zip(ties, wants):
        src, prm = dev(buf), dev(o.params(buf.shape[1]))
        got = kd_eval(live, src, buf.shape[1], prm)
        modes.append(live.kd_info().build_mode)
        assert_fresh_equal(got, kd_fresh(base, src, buf.shape[1], prm), name)
        assert_oracle(live, got, want, buf, 1, name)
    assert modes[1] >= 1 and modes[2] == 2, modes
    for n in (65536, 262144):
        src, prm = dev(state(o, n)), dev(o.params(n))
        got = kd_eval(live, src, n, prm)
        what = "ball n %d after build modes %s" % (n, modes)
        assert live.kd_info().build_mode == 2, what           # it is sticky
        assert_fresh_equal(got, kd_fresh(base, src, n, prm), what)
        assert_oracle(live, got, oracle_kd(o, n, p), state(o, n), 1, what)
    live.close()


def test_warm_select_from_an_unrelated_state(oracle32):
    """Part E2.  tree_steps = 1: ball A, then an unrelated state B of the same N (the uniform cube), then A again.  The warm select
    starts from the previous tree's pivots and a miss repeats the build cold.  (F) each time, (O) for B; warm_misses is recorded
    in the messages, not asserted."""
    from coulomb_oscillators_amd import Engine
    o = oracle32
    n, p = 65536, 5
    want_b = oracle_kd(o, n, p, kind="cube")
    base = dict(fmm_order=p, unsort=0, tree_steps=1)
    live = Engine(**base)
    prm = dev(o.params(n))
    for name, kind in (("A", "ball"), ("B", "cube"), ("A again", "ball")):
        src = dev(state(o, n, kind))
        got = kd_eval(live, src, n, prm)
        assert_fresh_equal(got, kd_fresh(base, src, n, prm), name)
        if kind == "cube":
            assert_oracle(live, got, want_b, state(o, n, kind), 0, name)
    live.close()


def test_refused_calls_and_grown_lists_leave_the_context_sound(oracle32):
    """Part E3.  After each refused call -- nbco_energy_fmm with no evaluation or behind an octree evaluation, nbco_fmm_symmetric at
    order 10, a list overflow with list_factor = 1 and list_grow = 0, n = 0, fmm_order = 11 -- the next valid call satisfies (F).  So do the calls after a GROWN
    list (list_factor = 1, list_grow = 1 leaves list_growth > 1): the same evaluation, a much smaller one, and the first one again
    once list_factor is back at its default."""
    from coulomb_oscillators_amd import Engine, EngineError
    o = oracle32
    n, p = 65536, 6
    base = dict(fmm_order=p, unsort=1)
    live = Engine(**base)
    inputs = {m: (dev(state(o, m)), dev(o.params(m))) for m in (n, 4096, 30001)}
    fresh = {m: kd_fresh(base, inputs[m][0], m, inputs[m][1]) for m in inputs}

    def valid(m, what):
        assert_fresh_equal(kd_eval(live, inputs[m][0], m, inputs[m][1]), fresh[m], what)

    src, prm = inputs[n]
    with pytest.raises(EngineError, match="no kd-tree evaluation"):
        live.energy_fmm(src, n, prm)
    valid(n, "after energy_fmm with no evaluation")
    live.set(fmm_order=10)
    with pytest.raises(EngineError):
        live.fmm_cart3(src[:2].clone(), zeros3(n), n, prm)
    live.set(fmm_order=p)
    valid(30001, "after fmm_cart3 at order 10")
    # the octree evaluators overwrite the positions and the sorted M2L keys that nbco_energy_fmm reads (include/nbco.h)
    live.fmm_cart3_traceless(inputs[4096][0][:2].clone(), zeros3(4096), 4096, inputs[4096][1])
    with pytest.raises(EngineError, match="no kd-tree evaluation"):
        live.energy_fmm(inputs[30001][0], 30001, inputs[30001][1])
    valid(30001, "after energy_fmm behind an octree evaluation")
    assert np.isfinite(live.energy_fmm(inputs[30001][0], 30001, inputs[30001][1])).all()
    live.set(list_factor=1, list_grow=0)
    with pytest.raises(EngineError, match="list capacity"):
        live.fmm_cart3_kdtree(src[:2].clone(), zeros3(n), n, prm)
    live.set(list_factor=48, list_grow=1)
    valid(n, "after a list overflow")
    with pytest.raises(EngineError):
        live.fmm_cart3_kdtree(src[:2].clone(), zeros3(n), 0, prm)
    valid(30001, "after n = 0")
    with pytest.raises(EngineError, match="fmm_order"):
        live.set(fmm_order=11)
    assert live.opts().fmm_order == p
    valid(n, "after fmm_order = 11")
    live.set(list_factor=1, list_grow=1)
    valid(n, "with grown lists")
    valid(4096, "much smaller, after grown lists")
    live.set(list_factor=48)
    valid(n, "list_factor reset")
    live.close()


# ---- F. the caller's stream --------------------------------------------------------------------------------------------------
def test_schedule_on_the_callers_stream(oracle32):
    """Part F.  include/nbco.h: "work is enqueued on opts.stream".  The uninterrupted schedule of part D on a context created on a
    side stream with sync = 0, its input produced by a torch operation on that stream immediately before the call, the result
    read after ONE synchronisation of that stream: (F) against the null-stream run.  And a context moved from the null stream to
    the side stream with nbco_set_opts after step 5 of the schedule (which drains the old stream)."""
    import torch
    o = oracle32
    plain = plain_schedule(o, 0)
    side = torch.cuda.Stream()
    got = run_schedule(o, dict(NBCO3, p2p_mutual=0), stream=side)
    assert torch.equal(got, plain), "schedule on a side stream"
    got = run_schedule(o, dict(NBCO3, p2p_mutual=0), stream=side, switch_stream_at=5)
    assert torch.equal(got, plain), "schedule moved to a side stream after step 5"


def test_short_estimate_on_the_callers_stream(oracle32):
    """Part F.  The first two large steps of part A (small, row 1, small, row 2) on a side-stream context with sync = 0; every
    accumulated result is read after one synchronisation of the stream at the end.  (F) against null-stream contexts."""
    import torch
    from coulomb_oscillators_amd import Engine
    o = oracle32
    rows = [SMALL, ROWS[0], SMALL, ROWS[1]]
    estimate_preconditions(o, ROWS[:2])
    hosts = {r["n"]: (dev(state(o, r["n"])), dev(o.params(r["n"]))) for r in rows}
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    results = []
    with torch.cuda.stream(side):
        live = Engine(stream=side.cuda_stream, sync=0, unsort=1)
        for r in rows:
            src, prm = hosts[r["n"]]
            d = src[:2] * 1.0                       # a torch operation on the side stream, right before the call
            a = torch.zeros((r["n"], 3), dtype=torch.float32, device="cuda")
            live.set(**row_opts(r))
            live.fmm_cart3_kdtree(d, a, r["n"], prm)
            results.append((d, a))
        side.synchronize()
    live.close()
    for r, (d, a) in zip(rows, results):
        src, prm = hosts[r["n"]]
        want = kd_fresh(dict(unsort=1, **row_opts(r)), src, r["n"], prm)
        assert torch.equal(a, want["a"]) and torch.equal(d, src[:2]), "side stream: n %d p %d r %g" % (r["n"], r["p"], r["r"])
