"""2-D program, host side (no GPU): the initial states of main.cu and the numpy restatement of fmm_cart that the GPU tests use."""
import os
import subprocess
import textwrap

import numpy as np
import pytest

import fmm2d_numpy as F

SEED, DISCARD = 5351550349027530206, 1248

# a short C++ restatement of main.cu:96-170 (centerDist, adjustRMS, initKV, initGA) over the same libstdc++ distributions, built as
# the reference's documented build compiles its host code (GCC, -O2: the sin / cos pair of one angle becomes one sincos call)
CPP = textwrap.dedent(r"""
    #include <cmath>
    #include <cstdio>
    #include <cstdlib>
    #include <random>
    #include <vector>
    struct V { double x, y; };
    static void center(V *d, long n) { V s{0, 0}; for (long i = 0; i < n; ++i) { s.x += d[i].x; s.y += d[i].y; }
        s.x /= (double)n; s.y /= (double)n; for (long i = 0; i < n; ++i) { d[i].x -= s.x; d[i].y -= s.y; } }
    static void rms(V *d, long n, V a) { V s{0, 0}; for (long i = 0; i < n; ++i) { s.x += d[i].x * d[i].x; s.y += d[i].y * d[i].y; }
        s.x /= (double)n; s.y /= (double)n; s.x = std::sqrt(s.x); s.y = std::sqrt(s.y);
        for (long i = 0; i < n; ++i) { d[i].x *= a.x / s.x; d[i].y *= a.y / s.y; } }
    int main(int argc, char **argv) {
        long n = atol(argv[1]); int ga = atoi(argv[2]); V a{atof(argv[3]), atof(argv[4])}, b{atof(argv[5]), atof(argv[6])};
        std::vector<V> d(2 * n);
        std::mt19937_64 gen(5351550349027530206ULL); gen.discard(624 * 2);
        if (!ga) {
            std::uniform_real_distribution<double> dist(0.0, 1.0);
            const double twopi = 6.283185307179586476925286766559;
            for (long i = 0; i < n; ++i) {
                double eta = dist(gen), etax = twopi * dist(gen), etay = twopi * dist(gen);
                double rt = std::sqrt(eta), rt1 = std::sqrt(1 - eta);
                d[i].x = a.x * rt * std::cos(etax); d[i].y = a.y * rt1 * std::cos(etay);
                d[i + n].x = a.x * b.x * rt * std::sin(etax); d[i + n].y = a.y * b.y * rt1 * std::sin(etay);
            }
            center(d.data(), n); rms(d.data(), n, V{a.x / 2, a.y / 2});
            center(d.data() + n, n); rms(d.data() + n, n, V{b.x * a.x / 2, b.y * a.y / 2});
        } else {
            std::normal_distribution<double> dist(0.0, 1.0);
            double *s = (double *)d.data();
            for (long i = 0; i < 4 * n; ++i) s[i] = dist(gen);
            for (long i = 0; i < n; ++i) { d[i].x *= a.x; d[i].y *= a.y; }
            for (long i = n; i < 2 * n; ++i) { d[i].x *= b.x; d[i].y *= b.y; }
            center(d.data(), n); rms(d.data(), n, a);
            center(d.data() + n, n); rms(d.data() + n, n, b);
        }
        fwrite(d.data(), sizeof(V), 2 * n, stdout);
        return 0;
    }
""")


@pytest.fixture(scope="module")
def init_ref(tmp_path_factory):
    d = tmp_path_factory.mktemp("init2d")
    src, exe = d / "init.cpp", d / "init"
    src.write_text(CPP)
    subprocess.check_call(["g++", "-O2", "-std=c++17", str(src), "-o", str(exe)])

    def run(n, ga, a, b):
        out = subprocess.run([str(exe), str(n), str(int(ga))] + ["%.17g" % v for v in (*a, *b)], check=True, capture_output=True).stdout
        return np.frombuffer(out, dtype=np.float64).reshape(2, n, 2)
    return run


@pytest.fixture(scope="module")
def lib(engine_lib):
    from coulomb_oscillators_amd import init2d
    return init2d


@pytest.mark.parametrize("n", [1000, 30001])
def test_init_kv_matches_restatement_bit_for_bit(init_ref, lib, n):
    A, om, _xi, _om0 = F.kv_params()
    got = lib(n, "kv", A, om)
    ref = init_ref(n, False, A, om)
    assert np.array_equal(got, ref)
    # centred, with RMS A/2 and omega A/2 per axis
    assert np.abs(got.mean(axis=1)).max() < 1e-15
    np.testing.assert_allclose(np.sqrt((got[0] ** 2).mean(axis=0)), np.array(A) / 2, rtol=1e-13)
    np.testing.assert_allclose(np.sqrt((got[1] ** 2).mean(axis=0)), np.array(om) * np.array(A) / 2, rtol=1e-13)


def test_init_gaussian_matches_restatement_bit_for_bit(init_ref, lib):
    A, om, _xi, _om0 = F.kv_params()
    x, u = tuple(v / 2 for v in A), tuple(o * v / 2 for o, v in zip(om, A))
    got = lib(4096, "ga", x, u)
    assert np.array_equal(got, init_ref(4096, True, x, u))
    np.testing.assert_allclose(np.sqrt((got[0] ** 2).mean(axis=0)), x, rtol=1e-13)
    np.testing.assert_allclose(np.sqrt((got[1] ** 2).mean(axis=0)), u, rtol=1e-13)


def test_init_seed_and_discard_matter(lib):
    A, om, _xi, _om0 = F.kv_params()
    a = lib(256, "kv", A, om)
    assert not np.array_equal(a, lib(256, "kv", A, om, discard=0))
    assert not np.array_equal(a, lib(256, "kv", A, om, seed=1))


def test_restatement_converges_to_the_exact_sum():
    A, om, xi, _ = F.kv_params()
    rng = np.random.default_rng(7)
    n = 2000
    st = np.stack([rng.normal(size=(n, 2)) * A, rng.normal(size=(n, 2))])
    errs = []
    for p in (1, 3, 5, 8):
        out, a = F.fmm(st, p, 1e-18, [1.0, 0.0], tree_L=4)
        exact = F.direct(out[0], 1e-18)
        errs.append(F.mean_relerr(a, exact))
    assert all(e2 < e1 for e1, e2 in zip(errs, errs[1:])), errs
    assert errs[-1] < 1e-5, errs
    # coll = 0: the near field is replaced by a * param[1]; the far field alone stays finite
    _, a0 = F.fmm(st, 5, 1e-18, [1.0, 0.0], coll=False, tree_L=4)
    assert np.isfinite(a0).all()


def _kv(lib):
    A, om, _xi, _ = F.kv_params()
    return lambda n: lib(n, "kv", A, om)


@pytest.mark.parametrize("cfg", F.SHAPE_CASES, ids=F.case_id)
def test_shape_cases_reach_their_paths(lib, cfg):
    """every input of the GPU value test has the property it is there for, from levels() and keys() alone"""
    e2 = float(np.float32(cfg["eps2"]))
    x = F.case_state(cfg, _kv(lib))[0]
    n, radius = len(x), cfg["radius"]
    assert n == cfg["n"]
    L = F.levels(n, cfg["p"], cfg["dens"], cfg["L"])
    side = 1 << L
    k = F.keys(x, L, e2)
    cnt = np.bincount(k, minlength=side * side)
    clamped = (x.max(axis=0) - x.min(axis=0)).max() / side < np.sqrt(e2)
    reach = cfg["reach"]
    if reach == "leaf>64":          # the second target tile of the near-field kernel
        assert cnt.max() > 64
    elif reach == "leaf>256":       # more than four target tiles, and a neighbour row of more than sixteen source tiles
        assert cnt.max() > 4 * 64
        rows = cnt.reshape(side, side)
        assert max(rows[:, max(j - radius, 0):j + radius + 1].sum(axis=1).max() for j in range(side)) > 16 * 64
    elif reach == "rows>100":       # a neighbour row of more than a hundred source tiles, its last one partial
        rows = cnt.reshape(side, side)
        longest = max(rows[:, max(j - radius, 0):j + radius + 1].sum(axis=1).max() for j in range(side))
        assert longest > 100 * 64 and longest % 64 != 0 and cnt.max() > 4 * 64
    elif reach == "flat":
        assert (k % side == 0).all() and (cnt > 64).any()
    elif reach == "empty>0.9":
        assert (cnt == 0).mean() > 0.9
        top = cnt.reshape(4, side // 4, 4, side // 4).sum(axis=(1, 3))   # level 2: two blobs share a cell
        assert (top > 0).sum() == 2
    elif reach == "hollow":         # the cell that holds the ring's centre is empty, and so is most of the tree
        mid = (x.max(axis=0) + x.min(axis=0)) / 2
        assert F.keys(np.vstack([x, mid]), L, e2)[-1] not in set(k.tolist())
        assert (cnt == 0).mean() > 0.5
    elif reach == "full":           # no empty leaf; with 65 points a side at L = 6 every point lies on a cell face
        assert (cnt > 0).all()
        if cfg["n"] == 65 * 65 and L == 6:
            assert np.array_equal(x * 64, np.round(x * 64)) and cnt.max() == 4
    elif reach == "pile":
        assert cnt.max() >= 3 * n // 4 and (cnt > 0).sum() > 16
    elif reach == "one_leaf":       # zero extent: the cell size is the clamp sqrt(EPS2)
        assert clamped and (k == 0).all()
    elif reach == "stencil":        # edge cells are clipped, interior cells see the whole (4r+2)^2 block
        assert side > 4 * radius + 2 and (cnt > 0).mean() > 0.5
    elif reach == "tiny":
        assert n <= 129 and 2 <= L <= 4
    elif reach == "clamp":          # spread-out particles, yet sqrt(EPS2) exceeds the leaf size
        assert clamped and x.std(axis=0).min() > 0
    elif reach == "soft_m2l":       # EPS2 is 1e-4 .. 1 of a leaf's area, and the tree is the unclamped one
        assert not clamped and (cnt > 0).mean() > 0.5
        assert e2 * side * side / (x.max(axis=0) - x.min(axis=0)).max() ** 2 > 1e-5
    elif reach == "nocoll":
        assert cfg["coll"] == 0 and cfg["p1"] != 0
    else:
        raise AssertionError(reach)


def test_chunked_near_field_keeps_every_targets_sum(lib):
    """slabs over the targets of a leaf: bit-equal to one slab per leaf, at a slab of a few targets and at the default"""
    st = F.shape("gauss", 1500)
    ph = [1.0, 0.0]
    whole = F.fmm(st, 4, 1e-18, ph, tree_L=2, near_chunk=None)
    for chunk in (1, 5000, F.NEAR_CHUNK):
        got = F.fmm(st, 4, 1e-18, ph, tree_L=2, near_chunk=chunk)
        assert np.array_equal(got[0], whole[0]) and np.array_equal(got[1], whole[1])


def test_generators_are_fixed_and_distinct():
    for kind in F.SHAPES:
        n = 4096 if kind == "lattice" else 1000
        a = F.shape(kind, n)
        assert a.shape == (2, n, 2) and np.isfinite(a).all()
        assert np.array_equal(a, F.shape(kind, n))
        if kind not in ("lattice", "all_coincident"):
            assert not np.array_equal(a, F.shape(kind, n, seed=1))
    assert np.ptp(F.shape("all_coincident", 50)[0], axis=0).max() == 0
    assert np.ptp(F.shape("line", 50)[0][:, 1]) == 0


@pytest.mark.parametrize("cfg", [c for c in F.SHAPE_CASES if c["reach"] == "soft_m2l"], ids=F.case_id)
def test_m2l_softening_is_visible_to_the_value_test(lib, cfg):
    """what the GPU comparison at 1e-10 can see: the restatement without `+ EPS2` in its M2L is 3e-6 (EPS2 = 1e-6) to 5e-4 (1e-4)
    away from the unmodified one in the GPU test's metric, so a kernel that dropped the term would be far outside the bound"""
    e2 = float(np.float32(cfg["eps2"]))
    st = F.case_state(cfg, _kv(lib))
    _A, _om, xi, _ = F.kv_params()
    ph = [xi / cfg["n"], 0.0]
    _, a = F.fmm(st, cfg["p"], e2, ph)
    _, b = F.fmm(st, cfg["p"], e2, ph, m2l_eps2=0.0)
    mag = np.linalg.norm(a, axis=1)
    err = (np.linalg.norm(b - a, axis=1) / (mag + mag.mean())).max()
    assert err > 1e4 * 1e-10, err


@pytest.mark.parametrize("cfg", [c for c in F.SHAPE_CASES if c["radius"] >= 2 and c["p"] >= 8], ids=F.case_id)
def test_wide_high_order_cases_are_below_1e_6(lib, cfg):
    """radius >= 2 and p >= 8: the restatement's own figure against the exact sum (1.6e-8 and 1.1e-9), which the GPU test then
    asks of the kernels"""
    e2 = float(np.float32(cfg["eps2"]))
    st = F.case_state(cfg, _kv(lib))
    _A, _om, xi, _ = F.kv_params()
    ph = [xi / cfg["n"], 0.0]
    out, a = F.fmm(st, cfg["p"], e2, ph, radius=cfg["radius"], tree_L=cfg["L"])
    assert F.mean_relerr(a, F.direct(out[0], e2, ph[0])) < 1e-6


def test_numpy_integrators_have_their_orders_and_reverse(lib):
    """direct force, n = 64, T = 0.04, 16 / 32 / 64 steps: the error against a 4096-step PEFRL solution falls by 2^order per
    halving (measured ratios / 2^order: 1.00-1.01 for all five), and leapfrog, Forest-Ruth and PEFRL return to the start after a
    velocity reversal to rounding (1.3e-16 .. 3e-16).  The GPU test takes these runs as its yardstick."""
    _A, _om, xi, om0 = F.kv_params()
    n = F.CONV_N
    ph = np.array([xi / n, 0.0, om0[0] ** 2, om0[1] ** 2])
    buf0 = F.conv_start(_kv(lib)(n), ph, F.CONV_EPS2)
    f = F.conv_force(ph, F.CONV_EPS2)

    def run(scheme, b, dt, steps):
        return F.integrate(scheme, b, f, dt, steps=steps)
    fine = run(4, buf0.copy(), F.CONV_T / F.CONV_FINE, F.CONV_FINE)
    # the yardstick is itself converged: Forest-Ruth at twice the steps agrees far below the smallest error measured
    res = F.conv_ratios(run, buf0, fine)
    floor = F.conv_dist(run(3, buf0.copy(), F.CONV_T / (2 * F.CONV_FINE), 2 * F.CONV_FINE), fine)
    for scheme, (errs, ratios) in res.items():
        assert min(errs) > 1e3 * floor, (scheme, errs, floor)
        for r in ratios:
            assert 0.6 <= r / 2 ** F.ORDERS[scheme] <= 1.6, (scheme, ratios)
    for scheme in F.REVERSIBLE:
        assert F.conv_return(run, lambda b: np.stack([b[0], -b[1], b[2]]), buf0, scheme) < 1e-14


def test_restatement_keys_follow_the_reference_formula():
    x = np.array([[0.0, 0.0], [1.0, 1.0], [0.5, 0.25], [0.999, 0.0]])
    k = F.keys(x, 2, 1e-18)
    # delta = 1/4: (0,0) -> 0; (1,1) clipped to (3,3) -> 15; (2,1) -> 9; (3,0) -> 12
    assert list(k) == [0, 15, 9, 12]
    assert F.levels(30001, 5) == 6 and F.levels(1 << 20, 5) == 8 and F.levels(10, 10) == 2
