"""CPU tests of the 3-D potential pass: the generated operator lpot_body (csrc/gen_ops.py, built for the host by csrc/genops_host.cpp)
against the generated L2P and against exact pair sums, and the numpy restatement tests/energy3d_numpy.py -- what the device kernels
are held to in tests/test_gpu_energy3d.py -- on trees built by the oracle.  No GPU involved."""
import ctypes as C

import numpy as np
import pytest

import energy3d_numpy as e3

sym_off = lambda n: n * (n + 1) * (n + 2) // 6
tl_off = lambda n: n * n


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def gen(engine_lib):
    from coulomb_oscillators_amd.engine import genops_lib
    G = genops_lib()
    V = C.c_void_p
    G.nbco_genop_p2m_f64.argtypes = [C.c_int, V, C.c_int, V, V]
    G.nbco_genop_p2m_f32.argtypes = [C.c_int, V, C.c_int, V, V]
    G.nbco_genop_m2l_f64.argtypes = [C.c_int, V, V, C.c_double, V]
    G.nbco_genop_m2l_f32.argtypes = [C.c_int, V, V, C.c_float, V]
    G.nbco_genop_l2p_f64.argtypes = [C.c_int, V, V, V]
    return G


def cluster_locals(gen, p, rng, radius, sep, dt=np.float64):
    """a random source cluster of `radius` about its centroid, and the order-p locals it induces at a centre `sep` away"""
    pts = rng.uniform(-1, 1, (40, 3))
    pts *= radius * rng.uniform(0.2, 1.0, (40, 1)) / np.linalg.norm(pts, axis=1, keepdims=True)
    pts = pts.astype(dt)
    c = pts.mean(axis=0).astype(dt)
    sfx = "f64" if dt == np.float64 else "f32"
    M = np.zeros(max(sym_off(p), 1), dtype=dt)
    assert getattr(gen, "nbco_genop_p2m_" + sfx)(p, ptr(pts), len(pts), ptr(c), ptr(M)) == 0
    u = rng.standard_normal(3)
    D = (sep * u / np.linalg.norm(u)).astype(dt)          # target centre - source centre
    Lc = np.zeros(tl_off(p + 1), dtype=dt)
    assert getattr(gen, "nbco_genop_m2l_" + sfx)(p, ptr(M), ptr(D), 0.0, ptr(Lc)) == 0
    return pts, c, M, D, Lc


def lpot64(gen, p, Lc, d):
    out = np.zeros(1)
    d = np.ascontiguousarray(d, dtype=np.float64)
    assert gen.nbco_genop_lpot_f64(p, ptr(Lc), ptr(d), ptr(out)) == 0
    return float(out[0])


@pytest.mark.parametrize("p", range(1, 11))
def test_lpot_gradient_is_minus_l2p(gen, p):
    """central difference of nbco_genop_lpot_f64 (h = 1e-4 |d|: truncation O(h^2) ~ 1e-8) against -nbco_genop_l2p_f64 within 1e-6 |a|"""
    rng = np.random.default_rng(900 + p)
    _, _, _, _, Lc = cluster_locals(gen, p, rng, 0.3, 2.0)
    assert lpot64(gen, p, Lc, np.zeros(3)) == 0.0
    for _ in range(4):
        d = rng.standard_normal(3) * 0.15
        a = np.zeros(3)
        assert gen.nbco_genop_l2p_f64(p, ptr(Lc), ptr(d), ptr(a)) == 0
        h = 1e-4 * np.linalg.norm(d)
        g = np.array([(lpot64(gen, p, Lc, d + h * e) - lpot64(gen, p, Lc, d - h * e)) / (2 * h) for e in np.eye(3)])
        assert np.linalg.norm(g + a) <= 1e-6 * np.linalg.norm(a), (p, g, a)


def test_lpot_plus_centre_potential_converges_to_the_exact_potential(gen):
    """source cluster of radius R, targets within R / 2 of a centre 8 R away: m2p at the centre + lpot(d) against sum 1/r; the error
    falls strictly with the order, and the f32 export follows the f64 one to 1e-5"""
    R = 0.25
    errs = []
    for p in range(1, 9):
        rng = np.random.default_rng(77)               # the same cluster and targets at every order
        pts, c, M, D, Lc = cluster_locals(gen, p, rng, R, 8 * R)
        tg = rng.uniform(-1, 1, (16, 3))
        tg *= (R / 2) * rng.uniform(0.3, 1.0, (16, 1)) / np.linalg.norm(tg, axis=1, keepdims=True)
        c0 = float(e3.m2p(M, D, 0.0, p))
        got = np.array([c0 + lpot64(gen, p, Lc, d) for d in tg])
        want = np.array([(1.0 / np.linalg.norm((c + D + d)[None, :] - pts, axis=1)).sum() for d in tg])
        errs.append(float(np.abs(got - want).max() / np.abs(want).max()))
        # the restatement's lpot on the same locals: the generated body to rounding
        mine = e3.lpot(e3.expand_traceless(Lc, p), tg, p)
        assert np.abs(mine - (got - c0)).max() <= 1e-13 * np.abs(got - c0).max() + 1e-300
        # f32 export on f32 inputs
        rng = np.random.default_rng(77)
        _, _, _, _, L32 = cluster_locals(gen, p, rng, R, 8 * R, np.float32)
        g32 = np.zeros(len(tg), dtype=np.float32)
        for k, d in enumerate(tg.astype(np.float32)):
            assert gen.nbco_genop_lpot_f32(p, ptr(L32), ptr(d), ptr(g32[k:k + 1])) == 0
        assert np.abs(g32 - (got - c0)).max() <= 1e-5 * np.abs(got - c0).max(), p
    print("lpot + c0 against the exact potential, orders 1..8:", " ".join("%.2e" % e for e in errs))
    assert all(b < a for a, b in zip(errs, errs[1:])), errs
    assert errs[-1] < 1e-6 < errs[0]


# ---- the restatement on oracle-built trees ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_case(oracle32, oracle64):
    """n = 3000: the fp32 initial state, evaluated by the fp64 oracle at p = 4 and 6 (tree order), with its exact energy"""
    n = 3000
    buf = oracle32.init_reference(n).astype(np.float64)
    par = oracle32.params(n).astype(np.float64)
    want = oracle64.energy(buf, par, threads=8)
    out = {}
    for p in (4, 6):
        pv, acc = oracle64.fmm_kd(buf[:2], par, p=p, unsort=False, threads=4)
        out[p] = (pv, acc, oracle64.kd_tree(sym_off(p), tl_off(p + 1)))
    return n, par, want, out


# the table of test_energy_fmm_against_fp64_direct_energy (3e-3 at order 3, 2e-4 at order 6); order 4 is held to the order-3 bound
ENERGY_TOL = {4: 3e-3, 6: 2e-4}


@pytest.mark.parametrize("p", [4, 6])
def test_restatement_gradient_is_the_oracle_acceleration(oracle_case, p):
    """-grad psi_i by central differences (tree and expansions held fixed) against the oracle's near + far acceleration, 1e-5"""
    n, par, _, out = oracle_case
    pv, acc, tree = out[p]
    pot = e3.Potential(tree, pv[0], p, 1e-18)
    first = (1 << tree["L"]) - 1
    rng = np.random.default_rng(p)
    worst = 0.0
    for lf in rng.choice(first + 1, 6, replace=False):
        i0, m = tree["index"][first + lf], tree["mult"][first + lf]
        idx = np.arange(i0, i0 + m)
        X = pv[0][idx]
        # step: well below the distance to the nearest neighbour, so that the pair terms stay smooth
        src = pot.sources(lf)
        dist = np.linalg.norm(X[:, None, :] - pv[0][src][None, :, :], axis=-1)
        dist[idx[:, None] == src[None, :]] = np.inf
        h = 1e-3 * dist.min(axis=1)
        g = np.zeros_like(X)
        for a in range(3):
            e = np.zeros(3); e[a] = 1.0
            g[:, a] = (pot.at(lf, X + h[:, None] * e, idx) - pot.at(lf, X - h[:, None] * e, idx)) / (2 * h)
        got = -par[0] * g
        err = np.linalg.norm(got - acc[idx], axis=1) / np.linalg.norm(acc[idx], axis=1)
        worst = max(worst, float(err.max()))
    print("p = %d: -grad psi against the oracle's acceleration, worst relative deviation %.2e" % (p, worst))
    assert worst <= 1e-5


@pytest.mark.parametrize("p", [4, 6])
def test_restatement_energy_is_within_the_truncation_of_the_exact_energy(oracle_case, p):
    n, par, want, out = oracle_case
    pv, _, tree = out[p]
    ps = e3.psi(tree, pv[0], p, 1e-18, par[0])
    exact = par[0] * e3.pair_potential(pv[0], 1e-18)
    assert abs(0.5 * exact.sum() - want[2]) <= 1e-12 * want[2]           # the yardstick agrees with the oracle's energy
    err = abs(0.5 * ps.sum() - want[2]) / want[2]
    per = float(np.mean(np.abs(ps - exact) / exact))
    print("n = %d p = %d: restated Coulomb energy off by %.2e, mean per-particle |psi - exact| / exact %.2e" % (n, p, err, per))
    assert err <= ENERGY_TOL[p], (err, ENERGY_TOL[p])
    assert (ps > 0).all()
