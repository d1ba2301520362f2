"""CPU tests of the 3-D probe restatement tests/probe3d_numpy.py -- what the device calls are held to in tests/test_gpu_probe3d.py -- on
trees built by the oracle: closed forms, the walk against the exact sums, the field as the gradient of the potential, and the
accuracy figures quoted in DESIGN.md section 4.  Also the source rule for kd_probe_admissible and the help text.  No GPU involved."""
import os
import re
import subprocess

import numpy as np
import pytest

import probe3d_numpy as p3
from energy3d_numpy import sym_off

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "coulomb_oscillators_amd", "csrc")
HOST = os.path.join(ROOT, "coulomb_oscillators_amd", "host")
EPS2 = 1e-18


# ---- closed forms -----------------------------------------------------------------------------------------------------------------
def test_exact_one_source():
    x = np.array([[0.25, -0.5, 0.125]], dtype=np.float32)
    t = np.array([[0.25, -0.5, 0.125], [1.25, -0.5, 0.125], [0.25, 1.5, 2.125]], dtype=np.float32)
    a, psi = p3.exact(x, t, 1e-4)
    e = float(np.float32(1e-4))
    d = t.astype(np.float64) - x.astype(np.float64)
    r2 = (d * d).sum(1) + e
    assert np.abs(psi - r2 ** -0.5).max() <= 1e-13 * psi.max()
    assert np.abs(a - d * (r2 ** -1.5)[:, None]).max() <= 1e-13 * np.abs(a).max()
    assert (a[0] == 0).all() and abs(psi[0] - e ** -0.5) <= 1e-13 * psi[0]        # on the source: nothing in a, 1 / sqrt(eps2) in psi


@pytest.mark.parametrize("eps2", [1e-18, 1e-4])
def test_exact_coincident_sources(eps2):
    """300 sources on one point: 300 times one source, on the point and off it"""
    x = np.tile(np.array([[0.5, 0.25, -1.0]], dtype=np.float32), (300, 1))
    t = np.array([[0.5, 0.25, -1.0], [0.0, 0.0, 0.0]], dtype=np.float32)
    a, psi = p3.exact(x, t, eps2)
    e = float(np.float32(eps2))
    d = t[1].astype(np.float64) - x[0].astype(np.float64)
    r2 = float(d @ d) + e
    assert (a[0] == 0).all()
    assert abs(psi[0] - 300 / np.sqrt(e)) <= 1e-13 * psi[0]
    assert abs(psi[1] - 300 / np.sqrt(r2)) <= 1e-13 * psi[1]
    assert np.abs(a[1] - 300 * d * r2 ** -1.5).max() <= 1e-13 * np.abs(a[1]).max()


def test_taylor_table_is_taylor_inv_r():
    """the order-at-a-time recurrence of the restatement against the component-at-a-time one of energy3d_numpy, orders 0..10"""
    rng = np.random.default_rng(5)
    d = rng.standard_normal((7, 3))
    B = p3.taylor_table(d, 1e-3, 10)
    b = p3.taylor_inv_r(d, 1e-3, 10)
    for k in range(11):
        for i, K in enumerate(p3.comps(k)):
            assert np.abs(B[k][i] - b[K]).max() <= 1e-13 * np.abs(b[K]).max() + 1e-300, K


# ---- the walk on oracle-built trees -------------------------------------------------------------------------------------------------
def oracle_tree(oracle32, oracle64, n, p, radius=1.0):
    """the fp32 reference ball evaluated by the fp64 oracle in tree order: (tree-ordered positions, tree dict, oracle acceleration)"""
    buf = oracle32.init_reference(n).astype(np.float64)
    par = oracle32.params(n).astype(np.float64)
    pv, acc = oracle64.fmm_kd(buf[:2], par, p=p, radius=radius, unsort=False, threads=4)
    return pv[0], oracle64.kd_tree(sym_off(p)), acc, par


@pytest.fixture(scope="module")
def case3000(oracle32, oracle64):
    return {p: oracle_tree(oracle32, oracle64, 3000, p) for p in (2, 4)}


def test_walk_with_a_huge_radius_is_the_exact_sum(case3000):
    pos, tree, _, _ = case3000[4]
    probes = np.concatenate(list(p3.probe_sets(pos, 1).values()))
    a, psi, acc, direct = p3.walk(tree, pos, probes, 4, 1e6, EPS2, 3000)
    ea, epsi = p3.exact(pos, probes, EPS2)
    assert all(len(s) == 0 for s in acc) and all(len(s) == 1 << tree["L"] for s in direct)
    assert np.abs(psi - epsi).max() <= 1e-13 * epsi.max()
    assert np.abs(a - ea).max() <= 1e-13 * np.abs(ea).max()


@pytest.mark.parametrize("p", [2, 4])
def test_a_distant_probe_takes_the_root_alone(case3000, p):
    """1000 box diagonals away: one expansion, off the exact sum by the series' remainder.  With the sources within s of the centre
    and the probe at D, psi's remainder is below (s/D)^p / (1 - s/D) of psi and the field's below (p + 1) (s/D)^p / (1 - s/D)^2."""
    pos, tree, _, _ = case3000[p]
    diag = float(np.sqrt(p3.node_sizes(tree)[0]))
    u = np.array([[1.0, 2.0, -2.0], [-2.0, 1.0, 2.0]]) / 3.0
    probes = (tree["center"][0][None, :] + 1000 * diag * u).astype(np.float32)
    a, psi, acc, direct = p3.walk(tree, pos, probes, p, 1.0, EPS2, 3000)
    assert acc == [[0], [0]] and direct == [[], []]
    ea, epsi = p3.exact(pos, probes, EPS2)
    q = 1e-3
    assert np.abs(psi - epsi).max() <= (q ** p / (1 - q) + 1e-13) * epsi.max()
    assert np.abs(a - ea).max() <= ((p + 1) * q ** p / (1 - q) ** 2 + 1e-13) * np.linalg.norm(ea, axis=1).max()


def test_field_is_minus_the_gradient_of_the_potential(case3000):
    """central differences of the walk's potential with h = 1e-6 box sizes, at the probes whose node sets are the same at t and at
    all six t +- h e.  The quotient's own error: rounding 2 x (a few eps psi) / 2h -- 64 eps psi / h is taken -- plus the truncation
    h^2 / 6 |psi'''|, bounded by h^2 / 6 sum_j 15 / r_j^4 over all sources (a third derivative of 1/r is at most 15 / r^4)."""
    p = 4
    pos, tree, _, _ = case3000[p]
    sets = p3.probe_sets(pos, 2)
    probes = np.concatenate([sets["box"][:60], sets["box1.5"][:60], sets["box10"][:40]]).astype(np.float64)
    box = float(np.sqrt(p3.node_sizes(tree)[0]))
    h = 1e-6 * box
    # (the walk takes float32 probes: the shifted points must be float32 numbers, so the step is taken on the float32 grid)
    base = probes.astype(np.float32)
    a, psi, acc, direct = p3.walk(tree, pos, base, p, 1.0, EPS2, 3000)
    grad = np.zeros_like(a)
    same = np.ones(len(base), dtype=bool)
    for c in range(3):
        e = np.zeros(3); e[c] = h
        tp, tm = (base.astype(np.float64) + e).astype(np.float32), (base.astype(np.float64) - e).astype(np.float32)
        _, pp, ap, dp = p3.walk(tree, pos, tp, p, 1.0, EPS2, 3000)
        _, pm, am, dm = p3.walk(tree, pos, tm, p, 1.0, EPS2, 3000)
        step = tp.astype(np.float64)[:, c] - tm.astype(np.float64)[:, c]
        grad[:, c] = (pp - pm) / step
        same &= np.array([ap[i] == acc[i] == am[i] and dp[i] == direct[i] == dm[i] for i in range(len(base))])
        same &= step > 0
    assert same.sum() >= 100, same.sum()
    x = p3.widen(pos)
    r2 = ((base.astype(np.float64)[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    # float32 steps: h is only approximately the step (the quotient uses the true one); the truncation term takes (2h)^2 to cover it
    tol = 64 * np.finfo(np.float64).eps * psi / (0.5 * h) + (2 * h) ** 2 / 6 * (15 / r2 ** 2).sum(1)
    err = np.linalg.norm(grad + a, axis=1)
    print("field + grad psi: worst %.2e of its bound, worst relative %.2e" % ((err / tol)[same].max(), (err / np.linalg.norm(a, axis=1))[same].max()))
    assert (err[same] <= tol[same]).all()


# ---- accuracy figures -----------------------------------------------------------------------------------------
ORDERS = [2, 4, 6, 8, 10]
SETS = ["particles", "box", "box1.5", "box10"]


@pytest.fixture(scope="module")
def accuracy(oracle32, oracle64):
    """mean relative distance of the walk from the exact sums, field and potential, per probe set; and the oracle's fmm_kd error at the
    particles (its field against the exact field, same measure)"""
    out = {}
    for n in (4096, 20000):
        for p in ORDERS:
            pos, tree, acc, par = oracle_tree(oracle32, oracle64, n, p)
            sets = p3.probe_sets(pos, 3)
            row = {}
            for name in SETS:
                a, psi, _, _ = p3.walk(tree, pos, sets[name], p, 1.0, EPS2, n)
                ea, epsi = p3.exact(pos, sets[name], EPS2)
                if name == "particles":
                    epsi = epsi - 1.0 / np.sqrt(float(np.float32(EPS2)))      # the self term, 1e9, is in both: compare what is left
                    psi = psi - 1.0 / np.sqrt(float(np.float32(EPS2)))
                row[name] = (p3.mean_rel(a, ea), p3.mean_rel(psi, epsi))
            ea, _ = p3.exact(pos, pos[::7], EPS2)
            row["fmm_kd"] = p3.mean_rel(acc[::7] / par[0], ea)     # (the evaluator's output is param[0] x the Coulomb sum, tree order)
            out[(n, p)] = row
            print("n = %5d p = %2d:" % (n, p), " ".join("%s a %.2e psi %.2e" % (k, *row[k]) for k in SETS), "fmm_kd a %.2e" % row["fmm_kd"])
    return out


def test_accuracy_figures_are_the_recorded_ones(accuracy):
    """the measurement against p3.FIGURES (what DESIGN.md quotes and the GPU test holds the device to): the same arithmetic on the
    same inputs, so only the libm in use can move them -- a part in a thousand is allowed"""
    for key, row in accuracy.items():
        for name in SETS:
            for got, want in zip(row[name], p3.FIGURES[key][name]):
                assert abs(got - want) <= 1e-3 * want, (key, name, got, want)
        assert abs(row["fmm_kd"] - p3.FIGURES[key]["fmm_kd"]) <= 1e-3 * row["fmm_kd"], key


def test_error_falls_from_order_to_order(accuracy):
    """field and potential, on every probe set and at both sizes, from each of the orders 2, 4, 6, 8, 10 to the next: the recorded
    figures fall by 2.49 at the least, so a factor 2 is asserted"""
    for n in (4096, 20000):
        for name in SETS:
            for lo, hi in zip(ORDERS, ORDERS[1:]):
                for q in (0, 1):
                    assert 2 * accuracy[(n, hi)][name][q] <= accuracy[(n, lo)][name][q], (n, name, lo, hi, q)


def test_probes_at_the_particles_are_closer_than_the_evaluator(accuracy):
    """the walk's field at every 7th particle against the oracle's fmm_kd field there: one truncation (the multipole series at the
    probe) instead of two (multipole and local).  The recorded figures are 2.9 to 290 times smaller: a factor 2 is asserted."""
    for key, row in accuracy.items():
        assert 2 * row["particles"][0] <= row["fmm_kd"], (key, row["particles"][0], row["fmm_kd"])


# ---- source rule and help text ----------------------------------------------------------------------------------------------------
def _state_at_definitions(path, names):
    """the parser of tests/test_source_rules.py: the fp-contract state in force where each function is defined"""
    state, out = "default", {}
    for line in open(path):
        m = re.search(r"#pragma clang fp contract\((\w+)\)", line)
        if m:
            state = m.group(1)
        for n in names:
            if n not in out and re.search(r"\b%s\s*\(" % re.escape(n), line) and ("__device__" in line or "__global__" in line):
                out[n] = state
    return out


def test_probe_acceptance_is_compiled_without_contraction():
    got = _state_at_definitions(os.path.join(CSRC, "kd_probe_kernels.hpp"), ["kd_probe_admissible"])
    assert got.get("kd_probe_admissible") == "off", got


def test_help_names_the_flag(engine_lib):
    subprocess.check_call(["make", "-C", HOST, "-s", "nbco3"])
    r = subprocess.run([os.path.join(HOST, "nbco3"), "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "-probes" in r.stdout and "probes<iter>" in r.stdout
