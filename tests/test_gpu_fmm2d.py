"""2-D program on the GPU: nbco_2d_* against the numpy restatement of the reference (tests/fmm2d_numpy.py) and exact sums."""
import os

import numpy as np
import pytest

import fmm2d_numpy as F

pytestmark = pytest.mark.gpu

EPS2_F32 = float(np.float32(1e-18))   # opts.eps2 is a float, widened to double by the 2-D path


def _kv(n):
    from coulomb_oscillators_amd import init2d
    A, om, _xi, _ = F.kv_params()
    return init2d(n, "kv", A, om)


def _ga(n):
    from coulomb_oscillators_amd import init2d
    A, om, _xi, _ = F.kv_params()
    return init2d(n, "ga", tuple(v / 2 for v in A), tuple(o * v / 2 for o, v in zip(om, A)))


def _param(n, torch, p1=0.0):
    _A, _om, xi, om0 = F.kv_params()
    h = np.array([xi / n, p1, om0[0] ** 2, om0[1] ** 2])
    return h, torch.from_numpy(h).cuda()


def _err(a, ref):
    mag = np.linalg.norm(ref, axis=1)
    return float((np.linalg.norm(a - ref, axis=1) / (mag + mag.mean())).max())


DIRECT_N = [1, 2, 63, 64, 65, 255, 256, 257, 512, 1000, 4097, 30001]   # the kernel's tile is 256 sources


def _direct_case(engine, n, eps2, scaled):
    import torch
    engine.set(eps2=eps2)
    e2 = float(np.float32(eps2))
    x = _kv(max(n, 2))[0][:n].copy()
    ph, prm = _param(n, torch)
    exact = F.direct(x, e2, ph[0] if scaled else 1.0)
    d = torch.from_numpy(x).cuda()
    for fn in (engine.direct_2d, engine.direct3_2d):
        a = torch.full((n, 2), float("nan"), dtype=torch.float64, device="cuda")
        fn(d, a, n, prm if scaled else None)
        got = a.cpu().numpy()
        if n == 1:
            assert np.array_equal(got, np.zeros((1, 2)))
        else:
            print("direct n=%d eps2=%g scaled=%d err=%.3e" % (n, eps2, scaled, _err(got, exact)))
            assert _err(got, exact) <= 1e-13


@pytest.mark.parametrize("n", DIRECT_N)
def test_direct_and_direct3_against_exact_sum(engine, n):
    _direct_case(engine, n, 1e-18, False)


@pytest.mark.parametrize("n", DIRECT_N)
def test_direct_sums_with_param_and_softening(engine, n):
    """param given (the sums come back times param[0]) and EPS2 = 1e-4, far above every |d|^2 of the beam"""
    _direct_case(engine, n, 1e-4, True)


@pytest.mark.parametrize("case", ["kv", "ga", "lattice", "coincident", "small", "big"])
def test_tree_order_is_the_stable_key_order(engine, case):
    import torch
    n = {"kv": 30001, "ga": 30001, "lattice": 33 * 33, "coincident": 500, "small": 100, "big": 1 << 20}[case]
    if case == "kv" or case == "big":
        st = _kv(n)
    elif case == "ga":
        st = _ga(n)
    elif case == "lattice":
        st = F.lattice(33)
    elif case == "coincident":
        st = np.stack([np.full((n, 2), 0.25), np.arange(2 * n, dtype=np.float64).reshape(n, 2)])
    else:
        st = _ga(n)
    p = 5
    engine.set(fmm_order=p, eps2=1e-18, tree_radius=1.0, coll=1, dens_inhom=1.0, tree_L=0)
    ph, prm = _param(n, torch)
    d = torch.from_numpy(st.reshape(-1).copy()).cuda()
    a = torch.zeros((n, 2), dtype=torch.float64, device="cuda")
    engine.fmm_2d(d, a, n, prm)
    got = d.cpu().numpy().reshape(2, n, 2)
    order = np.argsort(F.keys(st[0], F.levels(n, p), EPS2_F32), kind="stable")
    assert np.array_equal(got, st[:, order])
    assert np.isfinite(a.cpu().numpy()).all()


def _cfg(**kw):
    c = dict(shape="kv", n=6000, radius=1, coll=1, dens=1.0, L=0, eps2=1e-18, p1=0.0, unit=0)
    c.update(kw)
    return c


CASES = [_cfg(p=p) for p in range(1, 11)] + [
    _cfg(p=5, radius=2), _cfg(p=4, radius=2, dens=2.0), _cfg(p=6, coll=0), _cfg(p=3, dens=0.5), _cfg(p=5, L=5),
    _cfg(p=7, radius=2, coll=0, dens=0.5, L=4)] + F.SHAPE_CASES


def _case_id(c):
    return F.case_id(c) if "reach" in c else "p%(p)d_r%(radius)d_coll%(coll)d_d%(dens)g_L%(L)d" % c


def _fmm_call(eng, cfg, st, a_in, torch):
    """one nbco_2d_fmm on a fresh copy of the input.  With coll = 1 the kernel writes a, so a starts as NaN and an unvisited target
    stays visible; with coll = 0 it reads a, so a starts as a_in."""
    n = cfg["n"]
    eng.set(fmm_order=cfg["p"], eps2=cfg["eps2"], tree_radius=float(cfg["radius"]), coll=cfg["coll"], dens_inhom=cfg["dens"], tree_L=cfg["L"])
    _, prm = _param(n, torch, cfg["p1"])
    d = torch.from_numpy(st.reshape(-1).copy()).cuda()
    a = torch.from_numpy(a_in.copy()).cuda()
    if cfg["coll"]:
        a.fill_(float("nan"))
    eng.fmm_2d(d, a, n, prm)
    return d.cpu().numpy().reshape(2, n, 2), a.cpu().numpy()


@pytest.mark.parametrize("cfg", CASES, ids=_case_id)
def test_fmm_accelerations_match_restatement(engine, cfg):
    """Against the restatement: the state bit for bit, the accelerations within 1e-10 (two fp64 summation orders of the same terms),
    and a second call bit-identical to the first.  Where the restatement's accelerations are all exactly 0 (one particle; every
    particle at one point: each pair term is 0 / EPS2) the relative metric is 0 / 0 and the GPU's must be exactly 0 too.
    Against the exact sum (n > 1, coll = 1): the GPU's mean relative error equals the restatement's to three digits, as in the
    -test table.  A figure at fp64 rounding level (every pair in the near field: n = 2 and 3, one leaf; or r = 2 on the clusters,
    6e-14) has no three digits; there the two figures agree within 1e-13, the bound this file puts on an fp64 all-pairs sum.
    Measured on the MI355X: accelerations within 2.9e-15 of the restatement's in every case (worst: `coincident`); the figures at
    rounding level are 1.6e-16 against 0 (n = 3), 6.3035e-14 against 6.3032e-14 and 1.785e-15 against 1.783e-15."""
    import torch
    n, p, coll = cfg["n"], cfg["p"], cfg["coll"]
    e2 = float(np.float32(cfg["eps2"]))   # opts.eps2 is a float
    st = F.case_state(cfg, _kv)
    ph, _ = _param(n, torch, cfg["p1"])
    a_in = np.random.default_rng(3).normal(size=(n, 2))
    got_state, got = _fmm_call(engine, cfg, st, a_in, torch)
    again_state, again = _fmm_call(engine, cfg, st, a_in, torch)
    assert np.isfinite(got).all()
    assert np.array_equal(again_state, got_state) and np.array_equal(again, got)
    ref_state, ref_a = F.fmm(st, p, e2, ph, radius=cfg["radius"], coll=bool(coll), dens_inhom=cfg["dens"], tree_L=cfg["L"], a_in=a_in)
    assert np.array_equal(got_state, ref_state)
    if ref_a.any():
        print("fmm %s err=%.3e" % (_case_id(cfg), _err(got, ref_a)))
        assert _err(got, ref_a) <= 1e-10
    else:
        assert n == 1 or cfg["shape"] == "all_coincident"
        assert np.array_equal(got, np.zeros((n, 2)))
    if n > 1 and coll:
        exact = F.direct(ref_state[0], e2, ph[0])
        g, r = F.mean_relerr(got, exact), F.mean_relerr(ref_a, exact)
        print("fmm %s figure gpu=%.6e restatement=%.6e" % (_case_id(cfg), g, r))
        assert abs(g - r) <= max(1e-3 * r, 1e-13), (g, r)
        if cfg["radius"] >= 2 and p >= 8:
            # both such cases meet it in the restatement alone (test_fmm2d_host.test_wide_high_order_cases_are_below_1e_6)
            assert r < 1e-6 and g < 1e-6, (g, r)


@pytest.mark.parametrize("p", range(1, 11))
def test_every_order_reaches_its_own_kernels(engine, p):
    """the order is chosen per kernel launch: every order at n = 2000, the smallest n of this file that has L >= 3 at every
    order (L = 5 at p = 1, 3 at p = 10), with the comparison and the bars of test_fmm_accelerations_match_restatement"""
    cfg = _cfg(p=p, n=2000)
    assert F.levels(cfg["n"], p) >= 3
    test_fmm_accelerations_match_restatement(engine, cfg)


# every buffer shrinks and every stride changes between neighbours; the last call is the first again
SEQUENCE = [_cfg(shape="gauss", n=30001, p=10), _cfg(shape="clusters", n=300, p=3, L=2), _cfg(shape="gauss", n=3000, p=2, L=13),
            _cfg(p=5), _cfg(shape="gauss", n=1, p=5), _cfg(shape="lattice", n=4096, p=7, L=6, coll=0, p1=0.37),
            _cfg(shape="gauss", n=30001, p=10)]


def test_one_context_many_shapes_equals_fresh_contexts(engine):
    """reserve() keeps the largest scratch buffers, and the order sets the stride of the multipoles and locals inside one
    allocation: a call after a larger one reads what that one left wherever a kernel forgets to write.  Every result must be
    bit-identical to the same call on a fresh context."""
    import torch
    from coulomb_oscillators_amd import Engine
    results = []
    for cfg in SEQUENCE:
        st = F.case_state(cfg, _kv)
        a_in = np.random.default_rng(3).normal(size=(cfg["n"], 2))
        got = _fmm_call(engine, cfg, st, a_in, torch)
        fresh = Engine()
        try:
            want = _fmm_call(fresh, cfg, st, a_in, torch)
        finally:
            fresh.close()
        assert np.isfinite(got[1]).all(), F.case_id(cfg)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), F.case_id(cfg)
        results.append(got)
    assert np.array_equal(results[0][0], results[-1][0]) and np.array_equal(results[0][1], results[-1][1])


def test_test_mode_figure_falls_with_p_and_matches_restatement(engine):
    """main.cu -test: mean relative error of fmm_cart against direct3, p = 1..10"""
    import torch
    n = 4096
    st = _kv(n)
    ph, prm = _param(n, torch)
    figs, refs = [], []
    for p in range(1, 11):
        engine.set(fmm_order=p, eps2=1e-18, tree_radius=1.0, coll=1, dens_inhom=1.0, tree_L=0)
        buf = torch.zeros(6 * n, dtype=torch.float64, device="cuda")
        buf[:4 * n] = torch.from_numpy(st.reshape(-1).copy()).cuda()
        engine.compute_force_2d(2, buf, n, prm, elastic=False)
        fm = buf[4 * n:].clone()
        engine.compute_force_2d(1, buf, n, prm, elastic=False)
        figs.append(engine.mean_relerr_2d(fm, buf[4 * n:], n))
        out, a = F.fmm(st, p, EPS2_F32, ph)
        refs.append(F.mean_relerr(a, F.direct(out[0], EPS2_F32, ph[0])))
    assert all(b < a for a, b in zip(figs, figs[1:])), figs
    # 3 significant digits at every p
    for p, (g, r) in enumerate(zip(figs, refs), 1):
        assert abs(g - r) <= 1e-3 * r, (p, g, r)


def _integrator_case(engine, scheme, kind, scale, elastic):
    import torch
    n, p, dt, steps = 2048, 5, 5e-4, 3
    engine.set(fmm_order=p, eps2=1e-18, tree_radius=1.0, coll=1, dens_inhom=1.0, tree_L=0)
    st = _kv(n)
    ph, prm = _param(n, torch)
    buf0 = np.concatenate([st.reshape(-1), np.zeros(2 * n)])
    k = np.array(ph[2:])

    def f(b):
        if kind < 2:   # kind 1 is the compensated sum of the same terms
            b[2] = F.direct(b[0], EPS2_F32, ph[0])
        else:
            out, a = F.fmm(b[:2].copy(), p, EPS2_F32, ph)
            b[:2] = out
            b[2] = a
        if elastic:
            b[2] -= k * b[0]
    ref = F.integrate(scheme, buf0.copy().reshape(3, n, 2), f, dt, scale=scale, steps=steps)
    d = torch.from_numpy(buf0.copy()).cuda()
    for _ in range(steps):
        engine.integrate_2d(scheme, kind, d, n, prm, dt, scale=scale, elastic=elastic)
    got = d.cpu().numpy().reshape(3, n, 2)
    for q in range(3):
        assert _err(got[q], ref[q]) <= 1e-10, q
    # integrate_steps(K) == K calls, and a second run is bit-identical
    d2 = torch.from_numpy(buf0.copy()).cuda()
    engine.integrate_steps_2d(scheme, kind, d2, n, prm, dt, steps, scale=scale, elastic=elastic)
    assert torch.equal(d, d2)


@pytest.mark.parametrize("scheme", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_integrators_match_restatement(engine, scheme, kind):
    _integrator_case(engine, scheme, kind, 1.0, True)


@pytest.mark.parametrize("scheme", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("scale,elastic", [(0.5, True), (1.0, False), (0.5, False)])
def test_integrators_scale_and_elastic_match_restatement(engine, scheme, kind, scale, elastic):
    """the kick scale (velocity steps only) and the evaluation without the elastic term"""
    _integrator_case(engine, scheme, kind, scale, elastic)


def test_integrators_have_their_orders_and_reverse(engine):
    """The integrators by their own properties (direct force, n = 64, EPS2 = 1e-6; see fmm2d_numpy.CONV_*), with the numpy
    integrator's run at the same step counts as the yardstick, which test_fmm2d_host holds to 2^order: the GPU's ratios of the
    errors at 16 / 32 / 64 steps lie within 25 % of numpy's, and after K steps, v -> -v, K steps, leapfrog, Forest-Ruth and PEFRL
    are back at the start within ten times the distance numpy's run returns to.  A coefficient mis-copied into both the kernels'
    host sequence and its restatement lowers the order or breaks the reversal."""
    import torch
    n = F.CONV_N
    engine.set(eps2=1e-6)
    ph, prm = _param(n, torch)
    buf0 = F.conv_start(_kv(n), ph, F.CONV_EPS2)
    f = F.conv_force(ph, F.CONV_EPS2)

    def np_run(scheme, b, dt, steps):
        return F.integrate(scheme, b, f, dt, steps=steps)

    def gpu_run(scheme, b, dt, steps):
        d = torch.from_numpy(b.reshape(-1).copy()).cuda()
        engine.integrate_steps_2d(scheme, 0, d, n, prm, dt, steps)
        return d.cpu().numpy().reshape(3, n, 2)

    def negate(b):
        return np.stack([b[0], -b[1], b[2]])
    fine = np_run(4, buf0.copy(), F.CONV_T / F.CONV_FINE, F.CONV_FINE)
    want, got = F.conv_ratios(np_run, buf0, fine), F.conv_ratios(gpu_run, buf0, fine)
    for scheme in range(5):
        print("scheme %d ratios gpu=%s numpy=%s" % (scheme, got[scheme][1], want[scheme][1]))
        for g, w in zip(got[scheme][1], want[scheme][1]):
            assert abs(g - w) <= 0.25 * w, (scheme, got[scheme], want[scheme])
    for scheme in F.REVERSIBLE:
        g, w = F.conv_return(gpu_run, negate, buf0, scheme), F.conv_return(np_run, negate, buf0, scheme)
        print("scheme %d return gpu=%.3e numpy=%.3e" % (scheme, g, w))
        assert g <= 10 * w, (scheme, g, w)


RELERR_N = [1, 255, 256, 257, 131072, 131073, 300001]   # one block, the block edge, the 512 x 256 grid and its grid-stride path


@pytest.mark.parametrize("n", RELERR_N)
def test_mean_relerr_against_numpy(engine, n):
    """nbco_2d_mean_relerr against fmm2d_numpy.mean_relerr.  The two sum the same n non-negative fp64 terms in different orders:
    at most n x 1.1e-16 = 3.3e-11 relative apart at n = 3e5, typically sqrt(n) x 1.1e-16 = 6e-14.  Bound 1e-12: the worst value
    measured over these cases on the MI355X is 2.2e-16 (n = 257, random pairs), so 1e-12 is kept (more than ten times that)."""
    import torch
    rng = np.random.default_rng(n)
    ref = rng.normal(size=(n, 2))
    cases = {"random": (rng.normal(size=(n, 2)), ref), "equal": (ref.copy(), ref)}
    zref = ref.copy()
    zref[::3] = 0.0            # rows with ref == 0: the 1e-18 offset is the whole denominator
    zx = zref + 1e-9 * rng.normal(size=(n, 2))
    cases["zero_ref"] = (zx, zref)
    for name, (x, r) in cases.items():
        got = engine.mean_relerr_2d(torch.from_numpy(x).cuda(), torch.from_numpy(r).cuda(), n)
        want = F.mean_relerr(x, r)
        print("relerr n=%d %s gpu=%.17g numpy=%.17g rel=%.3e" % (n, name, got, want, abs(got - want) / want if want else 0.0))
        if name == "equal":
            assert got == 0.0 and want == 0.0
        else:
            assert want > 0 and abs(got - want) <= 1e-12 * want, (name, got, want)


def test_big_kv_is_finite_and_sampled_rows_are_close(engine):
    """N = 2^22, KV, p = 5: all finite; 256 rows against exact sums.  Bound: the restatement's worst of the same 256-row sample is
    1.8e-4 at N = 2^14 and 2.1e-4 at N = 2^16 (p = 5, KV); at 2^22 the rows must stay within 2.5 x that, 5e-4."""
    import torch
    n, p = 1 << 22, 5
    engine.set(fmm_order=p, eps2=1e-18, tree_radius=1.0, coll=1, dens_inhom=1.0, tree_L=0)
    st = _kv(n)
    ph, prm = _param(n, torch)
    d = torch.from_numpy(st.reshape(-1).copy()).cuda()
    a = torch.zeros((n, 2), dtype=torch.float64, device="cuda")
    engine.fmm_2d(d, a, n, prm)
    got = a.cpu().numpy()
    assert np.isfinite(got).all()
    x = d.cpu().numpy().reshape(2, n, 2)[0]
    rows = np.random.default_rng(5).choice(n, 256, replace=False)
    exact = F.direct_rows(x, rows, EPS2_F32, ph[0])
    mag = np.linalg.norm(exact, axis=1)
    err = (np.linalg.norm(got[rows] - exact, axis=1) / (mag + mag.mean())).max()
    assert err < 5e-4, err


def test_orders_above_ten_are_refused(engine):
    """orders above 10 are a documented deviation: NBCO_ERR_ARG.  The refusal comes from the options check that 2-D and 3-D
    share (nbco_set_opts / nbco_create), so no context ever reaches nbco_2d_fmm with such an order."""
    import torch
    from coulomb_oscillators_amd import EngineError
    n = 256
    d = torch.from_numpy(_kv(n).reshape(-1).copy()).cuda()
    a = torch.zeros((n, 2), dtype=torch.float64, device="cuda")
    _, prm = _param(n, torch)
    with pytest.raises(EngineError) as e:
        engine.set(fmm_order=11)
        engine.fmm_2d(d, a, n, prm)
    assert e.value.status == 2


def _refuse_tree_l(v):
    def go(e, t):
        e.set(tree_L=v)
        e.fmm_2d(t["d"], t["a"], t["n"], t["prm"])
    return go


REFUSALS = {
    "tree_L_1": _refuse_tree_l(1), "tree_L_16": _refuse_tree_l(16), "tree_L_neg": _refuse_tree_l(-1),
    "radius_half": lambda e, t: (e.set(tree_radius=0.5), e.fmm_2d(t["d"], t["a"], t["n"], t["prm"])),
    "order_11": lambda e, t: (e.set(fmm_order=11), e.fmm_2d(t["d"], t["a"], t["n"], t["prm"])),
    "n_0": lambda e, t: e.fmm_2d(t["d"], t["a"], 0, t["prm"]),
    "n_neg": lambda e, t: e.fmm_2d(t["d"], t["a"], -1, t["prm"]),
    "fmm_no_param": lambda e, t: e.fmm_2d(t["d"], t["a"], t["n"], None),
    "force_no_param": lambda e, t: e.compute_force_2d(2, t["buf"], t["n"], None),
    "kind_3": lambda e, t: e.compute_force_2d(3, t["buf"], t["n"], t["prm"]),
    "integrate_kind_3": lambda e, t: e.integrate_2d(2, 3, t["buf"], t["n"], t["prm"], 5e-4),
    # the integrators ask what nbco_2d_fmm asks before their first kick or drift: a refused step moves nothing
    "integrate_tree_L_1": lambda e, t: (e.set(tree_L=1), e.integrate_2d(2, 2, t["buf"], t["n"], t["prm"], 5e-4)),
    "integrate_steps_radius_half": lambda e, t: (e.set(tree_radius=0.5), e.integrate_steps_2d(0, 2, t["buf"], t["n"], t["prm"], 5e-4, 2)),
    "scheme_5": lambda e, t: e.integrate_2d(5, 0, t["buf"], t["n"], t["prm"], 5e-4),
    "steps_neg": lambda e, t: e.integrate_steps_2d(2, 0, t["buf"], t["n"], t["prm"], 5e-4, -1),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_bad_arguments_are_refused_and_leave_nothing_behind(engine, case):
    """NBCO_ERR_ARG with a message, from nbco_set_opts or from the entry point, before any launch (f2d_fmm, nbco_2d_force and
    nbco_2d_integrate* check their arguments and options first; an unknown kind or scheme is the switch's default).  The buffers
    are untouched, and the same context, options restored, evaluates the KV beam bit-identically to a fresh one."""
    import torch
    from coulomb_oscillators_amd import Engine, EngineError
    n = 256
    cfg = _cfg(p=5)
    base = dict(fmm_order=5, eps2=1e-18, tree_radius=1.0, coll=1, dens_inhom=1.0, tree_L=0)
    engine.set(**base)
    st = _kv(n)
    buf0 = np.concatenate([st.reshape(-1), np.full(2 * n, 7.0)])
    t = dict(n=n, d=torch.from_numpy(buf0[:4 * n].copy()).cuda(), a=torch.full((n, 2), 7.0, dtype=torch.float64, device="cuda"),
             buf=torch.from_numpy(buf0.copy()).cuda(), prm=_param(n, torch)[1])
    with pytest.raises(EngineError) as e:
        REFUSALS[case](engine, t)
    assert e.value.status == 2
    msg = str(e.value).split(":", 1)[1].strip()
    assert msg, str(e.value)
    assert np.array_equal(t["d"].cpu().numpy(), buf0[:4 * n]) and np.array_equal(t["buf"].cpu().numpy(), buf0)
    assert (t["a"].cpu().numpy() == 7.0).all()
    engine.set(**base)
    st = _kv(cfg["n"])
    a_in = np.zeros((cfg["n"], 2))
    got = _fmm_call(engine, cfg, st, a_in, torch)
    fresh = Engine()
    try:
        want = _fmm_call(fresh, cfg, st, a_in, torch)
    finally:
        fresh.close()
    assert np.isfinite(got[1]).all()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_direct3_compensation_beats_the_plain_sum(engine):
    """n = 2^17: against long-double sums of 64 sampled rows, the compensated sum's error is well below the plain one's"""
    import torch
    n = 1 << 17
    engine.set(eps2=1e-18)
    x = _kv(n)[0].copy()
    d = torch.from_numpy(x).cuda()
    a1 = torch.empty((n, 2), dtype=torch.float64, device="cuda")
    a3 = torch.empty((n, 2), dtype=torch.float64, device="cuda")
    engine.direct_2d(d, a1, n)
    engine.direct3_2d(d, a3, n)
    rows = np.random.default_rng(11).choice(n, 64, replace=False)
    xl = x.astype(np.longdouble)
    ref = np.zeros((64, 2), dtype=np.longdouble)
    for s in range(0, 64, 4):
        dd = xl[rows[s:s + 4]][:, None, :] - xl[None, :, :]
        ref[s:s + 4] = (dd / ((dd * dd).sum(-1) + np.longdouble(EPS2_F32))[..., None]).sum(1)
    mag = np.linalg.norm(ref.astype(np.float64), axis=1)
    e1 = np.mean(np.linalg.norm((a1.cpu().numpy()[rows] - ref).astype(np.float64), axis=1) / mag)
    e3 = np.mean(np.linalg.norm((a3.cpu().numpy()[rows] - ref).astype(np.float64), axis=1) / mag)
    assert e3 < 0.5 * e1, (e3, e1)


def test_deep_forced_tree_reaches_every_leaf(engine):
    """tree_L = 13: 4^13 leaves, more blocks than one dispatch can hold if the near field took one block per leaf.  a starts as
    NaN, so a leaf the near-field kernel never visits leaves NaN behind; the state must be in key order at L = 13."""
    import torch
    n = 3000
    st = _ga(n)
    engine.set(fmm_order=2, eps2=1e-18, tree_radius=1.0, coll=1, dens_inhom=1.0, tree_L=13)
    ph, prm = _param(n, torch)
    d = torch.from_numpy(st.reshape(-1).copy()).cuda()
    a = torch.full((n, 2), float("nan"), dtype=torch.float64, device="cuda")
    engine.fmm_2d(d, a, n, prm)
    got = a.cpu().numpy()
    assert np.isfinite(got).all()
    order = np.argsort(F.keys(st[0], 13, EPS2_F32), kind="stable")
    assert np.array_equal(d.cpu().numpy().reshape(2, n, 2), st[:, order])
    exact = F.direct(st[0][order], EPS2_F32, ph[0])
    assert F.mean_relerr(got, exact) < 0.2   # a sanity bound at p = 2


NEW_KERNELS_NO_SCRATCH = ["f2d_near_kernel", "f2d_m2l_kernel"]


def test_new_kernels_use_no_scratch_and_keys_are_not_contracted():
    import test_source_rules as R
    lib = os.path.join(R.ROOT, "coulomb_oscillators_amd", "libnbco_hip.so")
    blob = open(lib, "rb").read()
    found, bad = set(), []
    for base in R._device_elfs(blob):
        for name, _props, scratch in R._kernel_descriptors(blob, base):
            for k in NEW_KERNELS_NO_SCRATCH:
                if k in name:
                    found.add(k)
                    if scratch:
                        bad.append((name, scratch))
    assert found == set(NEW_KERNELS_NO_SCRATCH)
    assert not bad, bad
    got = R._state_at_definitions(os.path.join(R.CSRC, "k_fmm2d.hip"), ["f2d_keys_kernel", "f2d_scalars_kernel"])
    assert got == {"f2d_keys_kernel": "off", "f2d_scalars_kernel": "off"}
