"""2-D probes on the GPU: nbco_2d_probe against the exact numpy sums, nbco_2d_probe_fmm against the numpy restatement of the
multipole-to-probe pass (tests/probe2d_numpy.py), the invariants of both calls, refusals, one long-lived context, `nbco -probes`."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import fmm2d_numpy as F
import probe2d_numpy as PR
from test_gpu_fmm2d import _err
from test_probe2d_host import probe_sets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NBCO = os.path.join(ROOT, "coulomb_oscillators_amd", "host", "nbco")
BASE = dict(fmm_order=5, eps2=1e-18, tree_radius=1.0, coll=1, dens_inhom=1.0, tree_L=0)
EPS2_F32 = float(np.float32(1e-18))


@functools.lru_cache(maxsize=None)
def _kv(n):
    from coulomb_oscillators_amd import init2d
    A, om, _xi, _ = F.kv_params()
    st = init2d(n, "kv", A, om)
    st.setflags(write=False)
    return st


def _param(n):
    _A, _om, xi, om0 = F.kv_params()
    return np.array([xi / n, 0.0, om0[0] ** 2, om0[1] ** 2])


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).reshape(-1).copy()).cuda()


def _around_beam(m, scale=1.5, seed=0):
    """m points uniform in a square `scale` times the KV beam's larger semi-axis about its centre"""
    half = scale * max(F.kv_params()[0])
    return np.random.default_rng([seed, m]).uniform(-half, half, size=(m, 2))


def _call(fn, x, t, ph, want_a=True, want_psi=True, same=False):
    """one probe call on fresh copies of the sources x [n, 2] and the probes t [m, 2] (same: t is the very array p): (a, psi), each
    None if not asked for.  The outputs start as NaN, and p and t must come back byte-identical."""
    import torch
    n, m = len(x), len(t)
    hx, ht = np.ascontiguousarray(x, dtype=np.float64).reshape(-1), np.ascontiguousarray(t, dtype=np.float64).reshape(-1)
    dx = _dev(hx)
    dt = dx if same else _dev(ht)
    a = torch.full((m, 2), float("nan"), dtype=torch.float64, device="cuda") if want_a else None
    psi = torch.full((m,), float("nan"), dtype=torch.float64, device="cuda") if want_psi else None
    fn(dx, n, dt, m, _dev(ph), a, psi)
    assert np.array_equal(dx.cpu().numpy(), hx), "the sources were modified"
    assert np.array_equal(dt.cpu().numpy(), ht), "the probes were modified"
    return (a.cpu().numpy() if want_a else None), (psi.cpu().numpy() if want_psi else None)


# ---- 1. the exact call ----------------------------------------------------------------------------------------------------------
def _check_exact(got, want, what):
    (a, psi), (wa, wpsi, ab) = got, want
    ea, ep = _err(a, wa), np.abs(psi - wpsi).max() / ab.max()
    print("probe_2d %s: field err %.3e, psi err %.3e of max_i sum_j |term|" % (what, ea, ep))
    assert np.isfinite(a).all() and np.isfinite(psi).all()
    assert ea <= 1e-13
    assert np.abs(psi - wpsi).max() <= 1e-11 * ab.max()


@pytest.mark.parametrize("m", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 4097])
def test_probe_2d_against_exact_sum(engine, n, m):
    """KV sources, probes uniform in 1.5 x the beam's box: field _err <= 1e-13 (the bound test_gpu_fmm2d holds an fp64 all-pairs sum
    to) and every psi within 1e-11 x max_i sum_j |term| (the bound of test_energy_2d_against_exact_sum).  The kernel's tile is 256
    sources and its block 256 probes."""
    x, t, ph = np.ascontiguousarray(_kv(max(n, 2))[0][:n]), _around_beam(m), _param(n)
    engine.set(**BASE)
    _check_exact(_call(engine.probe_2d, x, t, ph), PR.exact(x, t, EPS2_F32, ph[0]), "n=%d m=%d" % (n, m))


def test_probe_2d_at_the_particles_is_the_direct_sum_and_the_energy_psi(engine):
    """t = p (the same array) at n = 1000: a against nbco_2d_direct at 1e-13, psi + param[0] 1/2 log EPS2 against nbco_2d_energy's
    psi at its 1e-11 bound -- the probe counts the source it sits on, with nothing in a and -param[0] 1/2 log EPS2 in psi"""
    import torch
    n = 1000
    st, ph = _kv(n), _param(n)
    x = st[0]
    engine.set(**BASE)
    want = PR.exact(x, x, EPS2_F32, ph[0])
    a, psi = _call(engine.probe_2d, x, x, ph, same=True)
    _check_exact((a, psi), want, "t=p n=1000")
    d, ad = _dev(x), torch.full((n, 2), float("nan"), dtype=torch.float64, device="cuda")
    engine.direct_2d(d, ad, n, _dev(ph))
    assert _err(a, ad.cpu().numpy()) <= 1e-13
    phi = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    engine.energy_2d(_dev(st), n, _dev(ph), phi)
    diff = np.abs(psi + ph[0] * 0.5 * math.log(EPS2_F32) - phi.cpu().numpy()).max()
    print("t=p: psi + param[0] 1/2 log EPS2 against energy_2d's psi: %.3e of max row" % (diff / want[2].max()))
    assert diff <= 1e-11 * want[2].max()


def test_probe_2d_on_duplicated_points(engine):
    """coincident400 (300 particles at one point), probes on every particle, the duplicated point included"""
    x, ph = F.shape("coincident", 400)[0], _param(400)
    engine.set(**BASE)
    _check_exact(_call(engine.probe_2d, x, x.copy(), ph), PR.exact(x, x, EPS2_F32, ph[0]), "coincident400")


# ---- 2. the FMM call against its restatement ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _kv6000_sets():
    sets = probe_sets(_kv(6000)[0])
    return sets, np.concatenate(list(sets.values()))


def _one_leaf(x, p, m=200):
    """m points inside the leaf that holds the beam's centre"""
    L = F.levels(len(x), p)
    mn, mx = x.min(0), x.max(0)
    delta = (mx - mn).max() / (1 << L)
    ij = np.floor((0.0 - mn) / delta)
    return mn + (ij + np.random.default_rng(3).uniform(0.05, 0.95, size=(m, 2))) * delta


def _fmm_case(name):
    """(sources, probes, options)"""
    kv, (sets, allsets) = _kv(6000)[0], _kv6000_sets()
    if name.startswith("kv6000_p"):
        return kv, allsets, dict(fmm_order=int(name[8:]))
    if name.startswith("radius"):
        return kv, allsets, dict(tree_radius=float(name[6:]))
    if name.startswith("dens"):
        return kv, allsets, dict(dens_inhom=float(name[4:]))
    if name == "sparse_L7":          # most leaves are empty, and probes sit in them
        x = _kv(3000)[0]
        return x, np.concatenate(list(probe_sets(x).values())), dict(tree_L=7)
    if name == "deep_L12":           # 4^12 leaves: the grid-stride loop
        x = _kv(3000)[0]
        return x, _around_beam(500, 1.2), dict(fmm_order=1, tree_L=12)
    if name == "one_leaf200":        # more than one lane chunk
        return kv, _one_leaf(kv, 5), {}
    if name == "rows_L2":            # a neighbour row with more than 64 sources
        return kv, allsets, dict(tree_L=2)
    if name in ("n1", "n2"):
        return np.ascontiguousarray(_kv(2)[0][:int(name[1:])]), _around_beam(100, 3.0), {}
    if name == "m1":
        return kv, sets["x1.5"][:1], {}
    assert name == "n140000_m70000"
    x = _kv(140000)[0]
    return x, np.concatenate([x[::4], _around_beam(35000)]), {}


FMM_CASES = (["kv6000_p%d" % p for p in range(1, 11)] + ["radius2", "radius3", "dens0.5", "dens2", "sparse_L7", "deep_L12", "one_leaf200", "rows_L2",
                                                          "n1", "n2", "m1", "n140000_m70000"])


@functools.lru_cache(maxsize=None)
def _kv6000_restated(p):
    return PR.fmm(_kv(6000)[0], _kv6000_sets()[1], p, EPS2_F32, _param(6000)[0])


def _check_fmm(got, want, what):
    (a, psi), (wa, wpsi) = got, want
    ea, ep = _err(a, wa), np.abs(psi - wpsi).max() / np.abs(wpsi).max()
    print("probe_fmm_2d %s: field err %.3e, psi err %.3e of max |psi|" % (what, ea, ep))
    assert np.isfinite(a).all() and np.isfinite(psi).all()
    assert ea <= 1e-10
    assert np.abs(psi - wpsi).max() <= 1e-10 * np.abs(wpsi).max()


@pytest.mark.parametrize("name", FMM_CASES)
def test_probe_fmm_2d_matches_restatement(engine, name):
    """field _err <= 1e-10 and every psi within 1e-10 max |psi|: the tolerances test_gpu_fmm2d and test_gpu_energy2d hold their
    restatements to.  The KV 6000 cases take the four probe sets of test_probe2d_host in one call: every 10th particle, the box,
    1.5 x and 10 x the box."""
    x, t, opt = _fmm_case(name)
    o = dict(BASE, **opt)
    ph = _param(len(x))
    if name.startswith("kv6000_p"):
        want = _kv6000_restated(o["fmm_order"])
    else:
        want = PR.fmm(x, t, o["fmm_order"], EPS2_F32, ph[0], radius=int(o["tree_radius"]), dens_inhom=o["dens_inhom"], tree_L=o["tree_L"])
    engine.set(**o)
    _check_fmm(_call(engine.probe_fmm_2d, x, t, ph), want, name)


def test_probe_fmm_2d_coincident_sources_give_the_closed_form(engine):
    """all_coincident300 with EPS2 = 1e-6, which clamps the cell size: n times the pair law at 1e-12, at probes on the point, next
    to it, across the cells and far outside them; and the restatement at its tolerance"""
    n, eps2 = 300, 1e-6
    e2 = float(np.float32(eps2))
    x = F.shape("all_coincident", n)[0]
    rng = np.random.default_rng(1)
    t = np.concatenate([x[:3], x[0] + 1e-3 * rng.normal(size=(50, 2)), x[0] + rng.uniform(0, 0.03, size=(50, 2)), x[0] + rng.normal(size=(20, 2))])
    ph = np.array([1.0 / n, 0.0, 1.0, 1.5])
    d = t - x[0]
    r2 = (d * d).sum(1) + e2
    wa, wpsi = d / r2[:, None], -0.5 * np.log(r2)
    for p in (1, 5, 10):
        engine.set(**dict(BASE, fmm_order=p, eps2=eps2))
        a, psi = _call(engine.probe_fmm_2d, x, t, ph)
        print("all_coincident300 p=%d: field %.3e psi %.3e" % (p, np.abs(a - wa).max() / np.abs(wa).max(), np.abs(psi - wpsi).max() / np.abs(wpsi).max()))
        assert np.abs(a - wa).max() <= 1e-12 * np.abs(wa).max() and np.abs(psi - wpsi).max() <= 1e-12 * np.abs(wpsi).max()
        assert np.array_equal(a[:3], np.zeros((3, 2)))
        _check_fmm((a, psi), PR.fmm(x, t, p, e2, ph[0]), "all_coincident300 p=%d" % p)


# ---- 3. invariants --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["probe_2d", "probe_fmm_2d"])
def test_probe_calls_are_reproducible_and_depend_on_the_probe_alone(engine, which):
    """KV 6000 and the four probe sets: outputs prefilled with NaN come back finite (and p, t byte-identical: _call); a second call,
    a alone, psi alone, and coll = 0 give the same bits; a permuted subset of the probes gives every probe the bits it got in
    the full set; sync = 0 on a side stream followed by engine.sync() gives the same numbers"""
    import torch
    from coulomb_oscillators_amd import Engine
    x, t, ph = _kv(6000)[0], _kv6000_sets()[1], _param(6000)
    engine.set(**BASE)
    fn = getattr(engine, which)
    a, psi = _call(fn, x, t, ph)
    assert np.isfinite(a).all() and np.isfinite(psi).all()
    a2, psi2 = _call(fn, x, t, ph)
    assert np.array_equal(a, a2) and np.array_equal(psi, psi2), "second call"
    a3, none = _call(fn, x, t, ph, want_psi=False)
    assert none is None and np.array_equal(a, a3), "a alone"
    none, psi3 = _call(fn, x, t, ph, want_a=False)
    assert none is None and np.array_equal(psi, psi3), "psi alone"
    engine.set(**dict(BASE, coll=0))
    a4, psi4 = _call(fn, x, t, ph)
    assert np.array_equal(a, a4) and np.array_equal(psi, psi4), "coll = 0"
    engine.set(**BASE)
    sub = np.random.default_rng(5).permutation(len(t))[:700]
    a5, psi5 = _call(fn, x, t[sub], ph)
    assert np.array_equal(a5, a[sub]) and np.array_equal(psi5, psi[sub]), "permuted subset"
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        live = Engine(stream=side.cuda_stream, **dict(BASE, sync=0))
        try:
            dx, dt, prm = _dev(x) * 1.0, _dev(t) * 1.0, _dev(ph) * 1.0     # produced on the side stream, right before the call
            a6 = torch.full((len(t), 2), float("nan"), dtype=torch.float64, device="cuda")
            psi6 = torch.full((len(t),), float("nan"), dtype=torch.float64, device="cuda")
            getattr(live, which)(dx, len(x), dt, len(t), prm, a6, psi6)
            live.sync()
            assert np.array_equal(a6.cpu().numpy(), a) and np.array_equal(psi6.cpu().numpy(), psi), "sync = 0 on a side stream"
        finally:
            live.close()


# ---- 4. the method's error is the restatement's ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _kv6000_exact():
    return PR.exact(_kv(6000)[0], _kv6000_sets()[1], EPS2_F32, _param(6000)[0])


@pytest.mark.parametrize("p", [3, 5, 7, 10])
def test_distance_from_exact_sum_is_the_restatements(engine, p):
    """KV 6000, the four probe sets: _err(probe_fmm_2d, probe_2d) equals _err(restatement, exact numpy sum) within 1e-10"""
    x, t, ph = _kv(6000)[0], _kv6000_sets()[1], _param(6000)
    engine.set(**dict(BASE, fmm_order=p))
    g_exact, _ = _call(engine.probe_2d, x, t, ph, want_psi=False)
    g_fmm, _ = _call(engine.probe_fmm_2d, x, t, ph, want_psi=False)
    dg, dr = _err(g_fmm, g_exact), _err(_kv6000_restated(p)[0], _kv6000_exact()[0])
    print("p=%d distance from the exact sum: gpu %.6e restatement %.6e" % (p, dg, dr))
    assert abs(dg - dr) <= 1e-10, (dg, dr)


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------
def _raw(eng, name, p, n, t, m, prm, a, psi):
    from coulomb_oscillators_amd.engine import _ptr
    return getattr(eng.lib, name)(eng.ctx, _ptr(p), n, _ptr(t), m, _ptr(prm), _ptr(a), _ptr(psi))


ARG_REFUSALS = {
    "null_p": lambda s: (None, s["n"], s["t"], s["m"], s["prm"], s["a"], s["psi"]),
    "null_t": lambda s: (s["p"], s["n"], None, s["m"], s["prm"], s["a"], s["psi"]),
    "null_param": lambda s: (s["p"], s["n"], s["t"], s["m"], None, s["a"], s["psi"]),
    "n_0": lambda s: (s["p"], 0, s["t"], s["m"], s["prm"], s["a"], s["psi"]),
    "n_neg": lambda s: (s["p"], -1, s["t"], s["m"], s["prm"], s["a"], s["psi"]),
    "m_0": lambda s: (s["p"], s["n"], s["t"], 0, s["prm"], s["a"], s["psi"]),
    "m_neg": lambda s: (s["p"], s["n"], s["t"], -1, s["prm"], s["a"], s["psi"]),
    "n_2^31": lambda s: (s["p"], 1 << 31, s["t"], s["m"], s["prm"], s["a"], s["psi"]),
    "m_2^31": lambda s: (s["p"], s["n"], s["t"], 1 << 31, s["prm"], s["a"], s["psi"]),
    "no_output": lambda s: (s["p"], s["n"], s["t"], s["m"], s["prm"], None, None),
}
OPT_REFUSALS = {"order_0": dict(fmm_order=0), "order_11": dict(fmm_order=11), "radius_half": dict(tree_radius=0.5), "tree_L_1": dict(tree_L=1),
                "tree_L_16": dict(tree_L=16)}


@pytest.mark.parametrize("case", sorted(ARG_REFUSALS) + sorted(OPT_REFUSALS))
def test_bad_arguments_are_refused_and_leave_nothing_behind(engine, case):
    """NBCO_ERR_ARG (2) before any launch: a and psi keep their NaN, p and t their contents, and the same context, options restored,
    returns what a fresh context returns, bit for bit.  The argument cases are asked of both entry points, the option cases --
    what nbco_2d_fmm refuses -- of nbco_2d_probe_fmm (from nbco_set_opts or from the entry point, whichever refuses first)."""
    import torch
    from coulomb_oscillators_amd import Engine, EngineError
    n, m = 256, 100
    x, t, ph = _kv(n)[0], _around_beam(m), _param(n)
    engine.set(**BASE)
    s = dict(n=n, m=m, p=_dev(x), t=_dev(t), prm=_dev(ph), a=torch.full((m, 2), float("nan"), dtype=torch.float64, device="cuda"),
             psi=torch.full((m,), float("nan"), dtype=torch.float64, device="cuda"))
    if case in ARG_REFUSALS:
        for name in ("nbco_2d_probe", "nbco_2d_probe_fmm"):
            assert _raw(engine, name, *ARG_REFUSALS[case](s)) == 2, name
            assert engine.lib.nbco_last_error(engine.ctx).decode().startswith(name + ":")
    else:
        with pytest.raises(EngineError) as e:
            engine.set(**OPT_REFUSALS[case])
            engine._chk(_raw(engine, "nbco_2d_probe_fmm", s["p"], n, s["t"], m, s["prm"], s["a"], s["psi"]))
        assert e.value.status == 2
    engine.sync()
    assert np.isnan(s["a"].cpu().numpy()).all() and np.isnan(s["psi"].cpu().numpy()).all()
    assert np.array_equal(s["p"].cpu().numpy(), x.reshape(-1)) and np.array_equal(s["t"].cpu().numpy(), t.reshape(-1))
    engine.set(**BASE)
    big, bt, bph = _kv(6000)[0], _kv6000_sets()[1], _param(6000)
    got = _call(engine.probe_fmm_2d, big, bt, bph), _call(engine.probe_2d, x, t, ph)
    fresh = Engine(**BASE)
    try:
        want = _call(fresh.probe_fmm_2d, big, bt, bph), _call(fresh.probe_2d, x, t, ph)
    finally:
        fresh.close()
    for g, w in zip(got, want):
        assert np.isfinite(g[0]).all() and np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1])


def test_one_context_serves_probes_between_energy_calls(engine, oracle32):
    """a 3-D energy_tree call and a 2-D energy_fmm_2d call, each made between two probe calls, return what they return without
    them; and the probe calls around them return the same bits"""
    import torch
    from coulomb_oscillators_amd import Engine
    n3 = 4096
    b3 = torch.from_numpy(oracle32.init_reference(n3).copy()).cuda()
    p3 = torch.from_numpy(oracle32.params(n3)).cuda()
    st, t, ph = _kv(6000), _kv6000_sets()[1], _param(6000)
    o = dict(BASE, fmm_order=4)
    fresh = Engine(**o)
    try:
        want3, want2 = fresh.energy_tree(b3, n3, p3), fresh.energy_fmm_2d(_dev(st), 6000, _dev(ph))
    finally:
        fresh.close()
    engine.set(**o)
    first = _call(engine.probe_fmm_2d, st[0], t, ph)
    got3 = engine.energy_tree(b3, n3, p3)
    second = _call(engine.probe_2d, st[0], t[:300], ph)
    got2 = engine.energy_fmm_2d(_dev(st), 6000, _dev(ph))
    third = _call(engine.probe_fmm_2d, st[0], t, ph)
    fourth = _call(engine.probe_2d, st[0], t[:300], ph)
    assert np.isfinite(got3).all() and np.array_equal(got3, want3)
    assert np.isfinite(got2).all() and np.array_equal(got2, want2)
    assert np.array_equal(first[0], third[0]) and np.array_equal(first[1], third[1])
    assert np.array_equal(second[0], fourth[0]) and np.array_equal(second[1], fourth[1])


def test_one_context_interleaves_the_three_tree_users(engine):
    """nbco_2d_fmm, nbco_2d_probe_fmm and nbco_2d_energy_fmm lay the same scratch buffers out in three ways (with locals; without; with
    locals and the potential's constants).  One context serves them in turn at changing n, order and depth: every result --
    accelerations and reordered state, the three energies and psi, field and potential -- is finite and bit for bit a fresh context's"""
    import torch
    from coulomb_oscillators_amd import Engine

    def fmm(e, n, m):
        d, a = _dev(_kv(n)), torch.full((2 * n,), float("nan"), dtype=torch.float64, device="cuda")
        e.fmm_2d(d, a, n, _dev(_param(n)))
        return a.cpu().numpy(), d.cpu().numpy()

    def energy(e, n, m):
        psi = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
        return e.energy_fmm_2d(_dev(_kv(n)), n, _dev(_param(n)), psi), psi.cpu().numpy()

    def probe(e, n, m):
        return _call(e.probe_fmm_2d, _kv(n)[0], _around_beam(m), _param(n))

    small = dict(fmm_order=7, tree_L=2)
    steps = [(fmm, 3000, 0, dict(fmm_order=3)), (probe, 300, 65, small), (energy, 6000, 0, dict(fmm_order=5)), (fmm, 300, 0, small),
             (energy, 3000, 0, dict(fmm_order=3)), (probe, 6000, 257, dict(fmm_order=5))]
    got = []
    for call, n, m, o in steps:
        engine.set(**dict(BASE, **o))
        got.append(call(engine, n, m))
    for (call, n, m, o), g in zip(steps, got):
        fresh = Engine(**dict(BASE, **o))
        try:
            want = call(fresh, n, m)
        finally:
            fresh.close()
        for x, y in zip(g, want):
            assert np.isfinite(x).all() and np.array_equal(x, y), (call.__name__, n, m, o)


# ---- 6. the command line --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nbco(engine_lib):
    if not os.path.exists(NBCO):
        subprocess.check_call(["make", "-C", os.path.dirname(NBCO), "-s", "nbco"])
    return NBCO


def _run(exe, *args):
    return subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=600)


def test_cli_probes_files_match_the_engine_on_the_snapshots(nbco, engine, tmp_path):
    n, m = 3000, 257
    out = tmp_path / "out"
    out.mkdir()
    t = _around_beam(m)
    t.tofile(tmp_path / "probes.bin")
    r = _run(nbco, "-n", n, "-iters", 2, "-steps", 1, "-probes", tmp_path / "probes.bin", "-o", out)
    assert r.returncode == 0, r.stderr
    snaps = ["out%d_0.000500.bin" % i for i in range(3)]
    files = ["probes%d_0.000500.bin" % i for i in range(3)]
    assert sorted(os.listdir(out)) == sorted(["args.txt"] + snaps + files)
    engine.set(**dict(BASE, eps2=EPS2_F32))
    ph = _param(n)
    for snap, f in zip(snaps, files):
        st = np.fromfile(out / snap, dtype=np.float64).reshape(2, n, 2)
        a, psi = _call(engine.probe_fmm_2d, st[0], t, ph)
        got = np.fromfile(out / f, dtype=np.float64)
        assert got.shape == (3 * m,)
        assert np.array_equal(got[:2 * m].reshape(m, 2), a) and np.array_equal(got[2 * m:], psi)


def test_cli_refuses_a_probes_file_that_holds_no_pairs(nbco, tmp_path):
    out = tmp_path / "out"
    out.mkdir()
    (tmp_path / "bad.bin").write_bytes(b"\0" * 15)
    (tmp_path / "empty.bin").write_bytes(b"")
    for f in ("bad.bin", "empty.bin", "missing.bin"):
        r = _run(nbco, "-n", 1024, "-iters", 1, "-steps", 1, "-probes", tmp_path / f, "-o", out)
        assert r.returncode != 0 and "probes file" in r.stderr, f
        assert os.listdir(out) == []


def test_cli_probes_with_test_mode_has_no_effect(nbco, tmp_path):
    out = tmp_path / "out"
    out.mkdir()
    _around_beam(64).tofile(tmp_path / "probes.bin")
    r = _run(nbco, "-test", "-probes", tmp_path / "probes.bin", "-n", 1024, "-o", out)
    assert r.returncode == 0, r.stderr
    assert sum(": Relative error: " in l for l in r.stdout.splitlines()) == 10
    assert os.listdir(out) == []
