"""CPU tests: the rows of shapes3d.ENERGY_SHAPE_CASES and the radii of shapes3d.BOND_SHAPE_RMAX are what their tables say, asserted on
the oracles and the numpy models before any GPU is involved (test_gpu_energy_shapes3d.py, test_gpu_bond_order.py).

An energy row is a test of the far-field pass only where the far field is a visible part of psi, of the wide-leaf path only where a
leaf holds more than a wave of targets, and its sanity bound against the exact sum is only as good as the method's own error on the
shape (the floor, printed here and tabled in DESIGN section 4).  A bond row keeps the premise of bond_numpy.TOL2 (nb <= 256) and has
linked, isolated and -- where the shape has them -- coincident particles."""
import numpy as np
import pytest

import energy3d_numpy as e3
import shapes3d as S

RESTATED = [r for r in S.ENERGY_SHAPE_CASES if not S.energy_all_near(r)]


def test_the_energy_table_covers_what_it_has_to():
    rows = S.ENERGY_SHAPE_CASES
    assert len({S.energy_id(r) for r in rows}) == len(rows)
    plain = {s for s, n, p, o in rows if (n, p, o) == (4096, 4, {})}
    assert plain == {"gauss", "plane", "plane_off", "line", "lattice", "late", "ejected", "two_clumps", "zeros", "offset"}
    tied = {s for s, n, p, o in rows if (n, p, o) == (4096, 4, dict(eps2=S.EPS2_TIED))}
    assert tied == {"dup2", "dup8", "dup16", "quant16"}
    assert {s for s, n, p, o in rows if p == 10 and o.get("far_fp64") == 1} == {"plane", "late"}
    assert {(s, o.get("eps2", 1e-18)) for s, n, p, o in rows if (n, p) == (8000, 6)} == {("line", 1e-18), ("dup8", S.EPS2_TIED)}
    assert {"plane", "dup16"} <= {r[0] for r in S.ENERGY_WIDE_LEAVES} and any(r[1] % 64 for r in S.ENERGY_WIDE_LEAVES)
    for opt in (dict(unsort=0), dict(p2p_mutual=1, unsort=0), dict(m2l_first=1), dict(coll=0)):
        assert [s for s, _, _, o in rows if o == opt and s != "gauss"], opt
    assert [r for r in rows if S.energy_all_near(r)] == [("dup64", 4096, 4, dict(tree_radius=1e6))]
    # every shape with coincident points runs softened (or all near field), nothing else does
    for s, _, _, o in rows:
        assert (o.get("eps2") == S.EPS2_TIED) == (s in ("dup2", "dup8", "dup16", "quant16")), s


@pytest.mark.parametrize("row", RESTATED, ids=S.energy_id)
def test_an_energy_row_has_a_far_field_and_a_floor(oracle32, oracle64, row):
    """On the fp32 oracle's tree: the restated psi is finite; the far part c0[leaf] + lpot reaches 10 % of max |psi| on at least half
    the particles (line: 10 % of the particle's OWN psi -- the largest psi of a line belongs to a pair 1e-6 of the length apart and
    says nothing about the rest); the rows that claim more than 64 targets per leaf have them.  The floors are printed."""
    shape, n, p, opts = row
    r = S.energy_floor(oracle32, oracle64, row)
    t = r["tree"]
    psi = r["near"] + r["far"]
    assert np.isfinite(psi).all() and np.isfinite(r["exact"]).all()
    scale = np.abs(psi) if shape == "line" else np.abs(psi).max()
    visible = float((np.abs(r["far"]) >= 0.1 * scale).mean())
    leaves = t["mult"][(1 << t["L"]) - 1:]
    print("%-40s L = %d, %d..%d per leaf, far part visible on %.3f, floor: energy %.2e, mean per particle %.2e"
          % (S.energy_id(row), t["L"], leaves.min(), leaves.max(), visible, r["floor_energy"], r["floor_mean"]))
    assert visible >= 0.5
    if opts.get("tree_L"):
        assert t["L"] == opts["tree_L"]
    if row in S.ENERGY_WIDE_LEAVES:
        assert leaves.min() > 64
    assert len(t["m2l"]) > 0


def test_the_all_near_row_has_no_far_field_and_a_finite_pair_sum(oracle32, oracle64):
    (row,) = [r for r in S.ENERGY_SHAPE_CASES if S.energy_all_near(r)]
    r = S.energy_floor(oracle32, oracle64, row)
    L = r["tree"]["L"]
    assert len(r["tree"]["m2l"]) == 0 and len(r["tree"]["p2p"]) == (1 << L) * ((1 << L) - 1) // 2
    assert np.isfinite(r["exact"]).all() and r["near"] is None
    # 63 twins at distance 0: each particle's psi holds 63 / sqrt(eps2) = 6.3e10 param0, and the sum is still the oracle's energy
    assert abs(0.5 * r["exact"].sum() - r["energy"][2]) <= 1e-12 * r["energy"][2]


def test_restated_energy_fmm_on_the_ball(oracle32, oracle64):
    """restated_energy_fmm on the fp64 oracle's gauss tree at p = 10: within 2e-5 of the exact energy (what ENERGY_TOL asks of the
    device at that order), and within twice the floor of psi on this tree of psi's total -- psi truncates the same far field a
    second time, and the floor (its total's distance from the exact energy, 2.5e-7 here) is what that costs"""
    n, p = 4096, 10
    buf, par = S.state(oracle32, "gauss", n), oracle32.params(n)
    _, _, t = S.run_oracle(oracle64, "kd", buf, par, p)
    pos = buf[0][t["perm"]]
    eps2 = np.float32(1e-18)
    got = e3.restated_energy_fmm(t, pos, p, eps2, par[0])
    exact = oracle64.energy(buf.astype(np.float64), par.astype(np.float64), threads=S.THREADS)[2]
    total = 0.5 * e3.psi(t, pos, p, eps2, par[0]).sum()
    floor = abs(total - exact) / exact
    print("restated energy_fmm off exact by %.3e, off psi's total by %.3e; floor of psi on this tree %.3e" % (abs(got - exact) / exact, abs(got - total) / exact, floor))
    assert abs(got - exact) <= 2e-5 * exact
    assert abs(got - total) <= 2 * floor * exact
    # all near field: the restatement is the pair sum
    (near_row,) = [r for r in S.ENERGY_SHAPE_CASES if S.energy_all_near(r)]
    r = S.energy_floor(oracle32, oracle64, near_row)
    near = e3.restated_energy_fmm(r["tree"], r["pos"], 4, np.float32(1e-18), r["par"][0])
    assert abs(near - 0.5 * r["exact"].sum()) <= 1e-12 * 0.5 * r["exact"].sum()


def test_the_bond_table_names_every_shape():
    assert set(S.BOND_SHAPE_RMAX) == set(S.SHAPES)
    assert all(f > 0 and length in ("box", "ball", "grid") for f, length in S.BOND_SHAPE_RMAX.values())


@pytest.mark.parametrize("shape", S.SHAPES)
def test_a_bond_row_keeps_the_premises(oracle32, shape):
    """nb_max <= 256 (bond_numpy.TOL2 is derived for that); a quarter of the particles have a neighbour; somebody has none (not on
    the lattice, whose every point has three); and where the shape has coincident points some pair inside is at r2 = 0 -- the pairs
    that `0 < r2` keeps out and `j != s` would not"""
    pos, rmax, m, inside, zero = S.bond_model(oracle32, shape)
    n = len(pos)
    print("%-10s n = %d, rmax = %.4e (%g %s): nb_max %d, %d linked, %d isolated, %d pairs inside, %d at r2 = 0"
          % ((shape, n, rmax) + S.BOND_SHAPE_RMAX[shape] + (m["nb_max"], n - m["isolated"], m["isolated"], inside, zero)))
    assert 0 < m["nb_max"] <= 256
    assert n - m["isolated"] >= n / 4
    assert (m["isolated"] > 0) == (shape != "lattice")
    assert (zero > 0) == (shape in S.BOND_COINCIDENT)
    assert m["nb"].sum() == 2 * (inside - zero)
