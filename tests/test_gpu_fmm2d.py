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


def _param(n, torch):
    _A, _om, xi, om0 = F.kv_params()
    h = np.array([xi / n, 0.0, om0[0] ** 2, om0[1] ** 2])
    return h, torch.from_numpy(h).cuda()


def _err(a, ref):
    mag = np.linalg.norm(ref, axis=1)
    return float((np.linalg.norm(a - ref, axis=1) / (mag + mag.mean())).max())


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000, 4097, 30001])
def test_direct_and_direct3_against_exact_sum(engine, n):
    import torch
    engine.set(eps2=1e-18)
    x = _kv(max(n, 2))[0][:n].copy()
    exact = F.direct(x, EPS2_F32)
    d = torch.from_numpy(x).cuda()
    for fn in (engine.direct_2d, engine.direct3_2d):
        a = torch.full((n, 2), float("nan"), dtype=torch.float64, device="cuda")
        fn(d, a, n)
        got = a.cpu().numpy()
        if n == 1:
            assert np.array_equal(got, np.zeros((1, 2)))
        else:
            assert _err(got, exact) <= 1e-13


def _lattice(n_side):
    g = np.arange(n_side, dtype=np.float64) / (n_side - 1)
    X, Y = np.meshgrid(g, g, indexing="ij")
    x = np.stack([X.ravel(), Y.ravel()], 1)
    return np.stack([x, x[::-1] * 0.5])


@pytest.mark.parametrize("case", ["kv", "ga", "lattice", "coincident", "small", "big"])
def test_tree_order_is_the_stable_key_order(engine, case):
    import torch
    n = {"kv": 30001, "ga": 30001, "lattice": 33 * 33, "coincident": 500, "small": 100, "big": 1 << 20}[case]
    if case == "kv" or case == "big":
        st = _kv(n)
    elif case == "ga":
        st = _ga(n)
    elif case == "lattice":
        st = _lattice(33)
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


CASES = [dict(p=p, radius=1, coll=1, dens=1.0, L=0) for p in range(1, 11)] + [
    dict(p=5, radius=2, coll=1, dens=1.0, L=0), dict(p=4, radius=2, coll=1, dens=2.0, L=0),
    dict(p=6, radius=1, coll=0, dens=1.0, L=0), dict(p=3, radius=1, coll=1, dens=0.5, L=0),
    dict(p=5, radius=1, coll=1, dens=1.0, L=5), dict(p=7, radius=2, coll=0, dens=0.5, L=4)]


@pytest.mark.parametrize("cfg", CASES, ids=lambda c: "p%(p)d_r%(radius)d_coll%(coll)d_d%(dens)g_L%(L)d" % c)
def test_fmm_accelerations_match_restatement(engine, cfg):
    import torch
    n = 6000
    st = _kv(n)
    engine.set(fmm_order=cfg["p"], eps2=1e-18, tree_radius=float(cfg["radius"]), coll=cfg["coll"], dens_inhom=cfg["dens"], tree_L=cfg["L"])
    ph, prm = _param(n, torch)
    a_in = np.random.default_rng(3).normal(size=(n, 2))
    d = torch.from_numpy(st.reshape(-1).copy()).cuda()
    a = torch.from_numpy(a_in.copy()).cuda()
    engine.fmm_2d(d, a, n, prm)
    ref_state, ref_a = F.fmm(st, cfg["p"], EPS2_F32, ph, radius=cfg["radius"], coll=bool(cfg["coll"]), dens_inhom=cfg["dens"],
                             tree_L=cfg["L"], a_in=a_in)
    assert np.array_equal(d.cpu().numpy().reshape(2, n, 2), ref_state)
    assert _err(a.cpu().numpy(), ref_a) <= 1e-10


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


@pytest.mark.parametrize("scheme", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("kind", [0, 2])
def test_integrators_match_restatement(engine, scheme, kind):
    import torch
    n, p, dt, steps = 2048, 5, 5e-4, 3
    engine.set(fmm_order=p, eps2=1e-18, tree_radius=1.0, coll=1, dens_inhom=1.0, tree_L=0)
    st = _kv(n)
    ph, prm = _param(n, torch)
    buf0 = np.concatenate([st.reshape(-1), np.zeros(2 * n)])
    k = np.array(ph[2:])

    def f(b):
        if kind == 0:
            b[2] = F.direct(b[0], EPS2_F32, ph[0])
        else:
            out, a = F.fmm(b[:2].copy(), p, EPS2_F32, ph)
            b[:2] = out
            b[2] = a
        b[2] -= k * b[0]
    ref = F.integrate(scheme, buf0.copy().reshape(3, n, 2), f, dt, steps=steps)
    d = torch.from_numpy(buf0.copy()).cuda()
    for _ in range(steps):
        engine.integrate_2d(scheme, kind, d, n, prm, dt)
    got = d.cpu().numpy().reshape(3, n, 2)
    for q in range(3):
        assert _err(got[q], ref[q]) <= 1e-10, q
    # integrate_steps(K) == K calls, and a second run is bit-identical
    d2 = torch.from_numpy(buf0.copy()).cuda()
    engine.integrate_steps_2d(scheme, kind, d2, n, prm, dt, steps)
    assert torch.equal(d, d2)


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
