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


def test_restatement_keys_follow_the_reference_formula():
    x = np.array([[0.0, 0.0], [1.0, 1.0], [0.5, 0.25], [0.999, 0.0]])
    k = F.keys(x, 2, 1e-18)
    # delta = 1/4: (0,0) -> 0; (1,1) clipped to (3,3) -> 15; (2,1) -> 9; (3,0) -> 12
    assert list(k) == [0, 15, 9, 12]
    assert F.levels(30001, 5) == 6 and F.levels(1 << 20, 5) == 8 and F.levels(10, 10) == 2
