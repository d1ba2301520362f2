"""GPU tests of the 3-D energy diagnostics on the degenerate shapes of shapes3d.ENERGY_SHAPE_CASES: nbco_kd_potential (Engine.energy_kd),
nbco_energy_fmm (Engine.energy_fmm) and nbco_energy_tree (Engine.energy_tree) on flat, collinear, tied, duplicated, stretched and
late-run states, where test_gpu_energy3d.py has the Gaussian ball.

The sharp yardsticks are restatements on the DEVICE tree (tests/energy3d_numpy.py): psi per particle against psi_parts, the Coulomb
energy of nbco_energy_fmm against restated_energy_fmm, which finds a particle's leaf in index / mult and walks the ancestors itself.
The truth (the fp64 pair sum, the fp64 oracle's energy) is a sanity bound only: the method's own error on these shapes is up to 7 %,
and the bound is twice the floor that test_energy_shapes_host.py measures on the fp32 oracle's tree, never anything the device gave."""
import numpy as np
import pytest

import energy3d_numpy as e3
import shapes3d as S
from test_gpu_energy3d import ENERGY_TOL, assert_tree_equals_fresh, call_twice, dev, device_tree

pytestmark = pytest.mark.gpu

RESTATED = [r for r in S.ENERGY_SHAPE_CASES if not S.energy_all_near(r)]


def energy_tol(p):
    """ENERGY_TOL names the orders 3, 6, 8, 10; an order between two of them is held to the bound of the lower one (the error falls
    with the order), as test_energy_tree_is_energy_kd_on_a_fresh_context_in_any_state holds order 4 to the order-3 bound"""
    return ENERGY_TOL[max(k for k in ENERGY_TOL if k <= p)]


def exact_psi(d, n, p0, eps2):
    """fp64 pair sum per particle on the device (torch), j != i by index, in d's order"""
    import torch
    x = d[0].double()
    out = torch.zeros(n, dtype=torch.float64, device="cuda")
    for s in range(0, n, 2048):
        r2 = ((x[s:s + 2048, None, :] - x[None, :, :]) ** 2).sum(-1) + float(eps2)
        w = 1.0 / r2.sqrt()
        i = torch.arange(s, min(s + 2048, n), device="cuda")
        w[i - s, i] = 0.0
        out[s:s + 2048] = w.sum(1)
    return float(p0) * out.cpu().numpy()


def evaluate(engine, row, buf, par):
    """one kd-tree evaluation of the row on `engine`; (d, prm, options, info)"""
    from coulomb_oscillators_amd import EVAL_FMM_KDTREE
    o = S.energy_opts(row)
    engine.set(**o)
    d, prm = dev(buf), dev(par)
    engine.compute_force(EVAL_FMM_KDTREE, d, row[1], prm)
    return d, prm, o, engine.kd_info()


@pytest.mark.parametrize("row", RESTATED, ids=S.energy_id)
def test_energy_diagnostics_on_a_shape(engine, oracle32, oracle64, row):
    """One evaluation per row, then:
    energy_kd: every slot of phi written, a second call the same bits, coulomb = 1/2 sum psi (call_twice); per particle
        |psi_i - want_i| <= 1e-12 near_i + 1e-10 max_j |far_j| against the restatement on the device tree -- 1e-10 of the far field is
        the bound of test_psi_against_the_restatement_on_the_device_tree, 1e-12 of the particle's own near field is 1e4 positive fp64
        terms at one rounding each, so that a twin at distance 0 loosens nobody else's bound;
    energy_fmm: its Coulomb energy within 1e-10 of restated_energy_fmm on the same tree;
    energy_tree (rows with default options): the bits of energy_kd on a fresh context;
    and, as a sanity bound, the Coulomb energy within max(ENERGY_TOL, 2 floor) of the fp64 oracle's and the mean per-particle
    deviation from the fp64 pair sum within 2 floor, the floors being those of the fp32 oracle's tree."""
    from coulomb_oscillators_amd import Engine
    shape, n, p, opts = row
    fl = S.energy_floor(oracle32, oracle64, row)
    buf, par = fl["buf"], fl["par"]
    d, prm, o, info = evaluate(engine, row, buf, par)
    eps2 = np.float32(o["eps2"])
    assert info.m2l_pairs > 0 and info.order == p
    if o["far_fp64"]:
        assert info.real_bytes == 8
    if o["tree_L"]:
        assert info.L == o["tree_L"]
    if row in S.ENERGY_WIDE_LEAVES:
        assert info.mlt_max > 64
    psi, out = call_twice(engine, engine.energy_kd, d, n, prm)
    fmm = engine.energy_fmm(d, n, prm)

    # ---- the restatements on the device tree
    tree = device_tree(engine)
    pos = d.cpu().numpy()[0]
    perm = engine.kd_array("unsort") if o["unsort"] else np.arange(n)
    near_t, far_t = e3.psi_parts(tree, pos[perm], p, eps2, par[0], coll=bool(o["coll"]))
    near, far = np.empty(n), np.empty(n)
    near[perm], far[perm] = near_t, far_t
    bound = 1e-12 * near + 1e-10 * np.abs(far).max()
    dev_psi = np.abs(psi - (near + far))
    want_fmm = e3.restated_energy_fmm(tree, pos[perm], p, eps2, par[0], coll=bool(o["coll"]))
    err_fmm = abs(fmm[2] - want_fmm) / abs(want_fmm)
    print("%s: worst |psi - restatement| = %.2e of its bound, %.2e of max |psi|; energy_fmm off its restatement by %.2e"
          % (S.energy_id(row), (dev_psi / bound).max(), dev_psi.max() / np.abs(near + far).max(), err_fmm))
    assert (dev_psi <= bound).all(), np.flatnonzero(dev_psi > bound)[:8]
    assert err_fmm <= 1e-10

    # ---- the truth, within the method's own error on this shape
    E = fl["energy"]
    assert abs(out[0] - E[0]) <= 1e-6 * E[0] and abs(out[1] - E[1]) <= 1e-6 * E[1]
    assert abs(fmm[0] - E[0]) <= 1e-6 * E[0] and abs(fmm[1] - E[1]) <= 1e-6 * E[1]
    err = abs(out[2] - E[2]) / E[2]
    ex = exact_psi(d, n, par[0], eps2)
    mean = float(np.mean(np.abs(psi - ex) / ex))
    print("%s: Coulomb energy off exact by %.3e (floor %.3e), mean per-particle deviation %.3e (floor %.3e)"
          % (S.energy_id(row), err, fl["floor_energy"], mean, fl["floor_mean"]))
    assert err <= max(energy_tol(p), 2 * fl["floor_energy"])
    assert mean <= 2 * fl["floor_mean"]

    # ---- the self-contained call
    if not opts:
        eng = Engine(**o)
        try:
            assert_tree_equals_fresh(eng, dev(buf), n, prm, fmm_order=p)
        finally:
            eng.close()


def test_all_near_field_on_64_copies_per_point(engine, oracle32, oracle64):
    """dup64 with tree_radius = 1e6: no M2L pair, every leaf in every leaf's P2P range, 63 twins at distance 0 per particle -- psi is
    the fp64 pair sum to 1e-12 per particle, and energy_fmm half its total"""
    (row,) = [r for r in S.ENERGY_SHAPE_CASES if S.energy_all_near(r)]
    n = row[1]
    fl = S.energy_floor(oracle32, oracle64, row)
    buf, par = fl["buf"], fl["par"]
    d, prm, o, info = evaluate(engine, row, buf, par)
    assert info.m2l_pairs == 0 and info.p2p_pairs == (1 << info.L) * ((1 << info.L) - 1) // 2
    psi, out = call_twice(engine, engine.energy_kd, d, n, prm)
    want = float(par[0]) * e3.pair_potential(buf[0], np.float32(o["eps2"]))
    err = np.abs(psi - want) / want
    fmm = engine.energy_fmm(d, n, prm)
    print("%s: worst per-particle deviation %.2e, energy_fmm off by %.2e" % (S.energy_id(row), err.max(), abs(fmm[2] - 0.5 * want.sum()) / (0.5 * want.sum())))
    assert err.max() <= 1e-12
    assert abs(fmm[2] - 0.5 * want.sum()) <= 1e-10 * 0.5 * want.sum()
    E = fl["energy"]
    assert abs(out[0] - E[0]) <= 1e-6 * E[0] and abs(out[1] - E[1]) <= 1e-6 * E[1]
