"""GPU parity tests (through the C ABI) for the direct evaluator, the HBM-bound particle kernels,
the reductions and the integrators, against the CPU oracle on the same seeded inputs."""
import numpy as np
import pytest

from nbutil import force_err

pytestmark = pytest.mark.gpu


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


@pytest.mark.parametrize("n", [1, 2, 255, 1000, 4096, 5000])
def test_direct_matches_oracle(engine, oracle32, n):
    """direct / direct3 vs the oracle's Kahan direct sum (direct.cuh:192-256); tolerance 1e-5
    (north_star) on the regularised per-particle relative error."""
    import torch
    o = oracle32
    buf = o.init_reference(max(n, 2))[:, :n]
    par = o.params(n)
    ref = o.direct3(buf[0], par, threads=4)
    p, prm = dev(buf[0]), dev(par)
    a = torch.empty_like(p)
    engine.direct(p, a, n, prm)
    assert force_err(a.cpu().numpy(), ref) < 1e-5
    a3 = torch.empty_like(p)
    engine.direct3(p, a3, n, prm)
    assert force_err(a3.cpu().numpy(), ref) < 1e-5
    # bit-reproducible across calls (fixed-order combination of the j splits)
    a_again = torch.empty_like(p)
    engine.direct(p, a_again, n, prm)
    assert torch.equal(a, a_again)
    # param == nullptr means k = 1 (direct.cuh:148-150)
    a1 = torch.empty_like(p)
    engine.direct(p, a1, n, None)
    assert force_err(a1.cpu().numpy() * par[0], ref) < 1e-5


def test_direct_config2_size_properties(engine, oracle32):
    """BASELINE config 2 (N = 262144): a sampled subset against the fp32 oracle, zero net force
    (Newton III: sum_i a_i = 0 up to rounding) and softening behaviour at a duplicated point."""
    import torch
    o = oracle32
    n = 262144
    buf = o.init_reference(n)
    par = o.params(n)
    dup = (0, 200001)                   # one point twice, in different target blocks and lanes: the pair's r^2 is the softening alone
    buf[0][dup[1]] = buf[0][dup[0]]
    p, prm = dev(buf[0]), dev(par)
    a = torch.empty_like(p)
    engine.direct3(p, a, n, prm)
    assert torch.isfinite(a).all()
    assert torch.equal(a[dup[0]].view(torch.int32), a[dup[1]].view(torch.int32))      # the same sources in the same order: the same bits
    a_h = a.cpu().numpy().astype(np.float64)
    scale = np.linalg.norm(a_h, axis=1).mean()
    assert np.abs(a_h.sum(axis=0)).max() / (n * scale) < 1e-6
    # sampled rows vs oracle (full row sums over all n sources)
    rows = np.random.default_rng(5).choice(n, 64, replace=False)
    pos64 = buf[0].astype(np.float64)
    d = pos64[rows, None, :] - pos64[None, :, :]
    r2 = (d ** 2).sum(-1) + 1e-18
    want = (d / r2[..., None] ** 1.5).sum(1) * float(par[0])
    got = a_h[rows]
    assert (np.linalg.norm(got - want, axis=1) / (np.linalg.norm(want, axis=1) + scale)).max() < 1e-5
    # and the two copies themselves, to which the pair contributes exactly zero
    d = pos64[list(dup), None, :] - pos64[None, :, :]
    r2 = (d ** 2).sum(-1) + 1e-18
    want = (d / r2[..., None] ** 1.5).sum(1) * float(par[0])
    assert (np.linalg.norm(a_h[list(dup)] - want, axis=1) / (np.linalg.norm(want, axis=1) + scale)).max() < 1e-5


@pytest.mark.parametrize("n", [1, 3, 4, 1001, 4096, 30001])
def test_step_elastic_rescale(engine, oracle32, n):
    import torch
    o = oracle32
    rng = np.random.default_rng(n)
    b = rng.standard_normal((n, 3)).astype(np.float32)
    a = rng.standard_normal((n, 3)).astype(np.float32)
    k = np.array([1.2, 0.9, 1.1], dtype=np.float32)
    par = np.array([0.37, 0, 0, 1.2, 0.9, 1.1], dtype=np.float32)
    # step: b += a*ds  (kernel.cuh:85-117); the device uses fma, the oracle mul+add
    bd, ad = dev(b), dev(a)
    engine.step(bd, ad, 0.125, n)
    want = b.copy(); o.step(want, a, 0.125)
    np.testing.assert_allclose(bd.cpu().numpy(), want, rtol=0, atol=2e-7 * np.abs(want).max())
    # add_elastic with and without constants (kernel.cuh:119-173)
    for kk in (k, None):
        pd, ad2 = dev(b), dev(a)
        engine.add_elastic(pd, ad2, n, dev(kk) if kk is not None else None)
        want = a.copy(); o.add_elastic(b, want, kk)
        np.testing.assert_allclose(ad2.cpu().numpy(), want, rtol=0, atol=4e-7 * np.abs(want).max())
    # elastic: a = -k o p (kernel.cuh:175-226)
    pd, ad3 = dev(b), dev(a)
    engine.elastic(pd, ad3, n, dev(k))
    np.testing.assert_allclose(ad3.cpu().numpy(), -b * k, rtol=1e-7)
    # rescale (appel.cuh:506-527)
    ad4 = dev(a)
    engine.rescale(ad4, n, dev(par))
    np.testing.assert_array_equal(ad4.cpu().numpy(), a * np.float32(0.37))
    # misaligned views exercise the scalar paths
    if n >= 4:
        big = dev(np.concatenate([np.zeros(1, np.float32), b.ravel()]))
        biga = dev(np.concatenate([np.zeros(1, np.float32), a.ravel()]))
        engine.step(big[1:], biga[1:], 0.125, n)
        want = b.copy(); o.step(want, a, 0.125)
        np.testing.assert_allclose(big[1:].cpu().numpy().reshape(n, 3), want, rtol=0, atol=2e-7 * np.abs(want).max())


def test_gather_copy(engine):
    import torch
    n = 10007
    rng = np.random.default_rng(0)
    src = rng.standard_normal((n, 3)).astype(np.float32)
    perm = rng.permutation(n).astype(np.int32)
    s, m = dev(src), dev(perm)
    d = torch.empty_like(s)
    engine.gather(d, s, m, n)                      # dst[i] = src[map[i]] (kernel.cuh:229)
    np.testing.assert_array_equal(d.cpu().numpy(), src[perm])
    d2 = torch.empty_like(s)
    engine.gather_inverse(d2, d, m, n)             # dst[map[i]] = src[i] (kernel.cuh:255)
    np.testing.assert_array_equal(d2.cpu().numpy(), src)
    d3 = torch.empty_like(s)
    engine.copy(d3, s, n)
    np.testing.assert_array_equal(d3.cpu().numpy(), src)


@pytest.mark.parametrize("n", [1, 77, 4096, 100003])
def test_reductions(engine, oracle32, n):
    o = oracle32
    rng = np.random.default_rng(n)
    x = rng.standard_normal((n, 3)).astype(np.float32)
    ref = (x + 1e-3 * rng.standard_normal((n, 3))).astype(np.float32)
    mm = engine.minmax(dev(x), n).cpu().numpy()
    np.testing.assert_array_equal(mm, o.minmax(x))                       # exact (reductions.cuh:67-80)
    got = engine.mean_relerr(dev(x), dev(ref), n)
    assert abs(got - o.mean_relerr(x, ref)) <= 2e-5 * o.mean_relerr(x, ref) + 1e-12
    for expo in (1, 2, 3):
        np.testing.assert_allclose(engine.pow_sum(dev(x), expo, n), o.pow_sum(x, expo), rtol=1e-10, atol=1e-9)


def test_energy_matches_fp64_direct_sum(engine, oracle32):
    o = oracle32
    n = 3000
    buf = o.init_reference(n)
    par = o.params(n)
    want = o.energy(buf, par, threads=4)
    got = engine.energy(dev(buf), n, dev(par))
    np.testing.assert_allclose(got[:2], want[:2], rtol=1e-12)
    np.testing.assert_allclose(got[2], want[2], rtol=2e-6)


@pytest.mark.parametrize("scheme", [0, 1, 2, 3, 4])
def test_integrators_with_direct_force(engine, oracle32, scheme):
    """integrator.cuh:32-167 driven with coulombOscillatorDirect (main3.cu:47-51): 5 steps vs the oracle."""
    from coulomb_oscillators_amd import EVAL_DIRECT_KAHAN
    from oracle import pyoracle as po
    o = oracle32
    n = 2048
    buf = o.init_reference(n)
    par = o.params(n)
    o.compute_force(po.KIND_DIRECT3, buf, par, threads=4)
    d = dev(buf)
    dt = 5e-4
    for _ in range(5):
        o.integrate(scheme, po.KIND_DIRECT3, buf, par, dt, threads=4)
        engine.integrate(scheme, EVAL_DIRECT_KAHAN, d, n, dev(par), dt)
    got = d.cpu().numpy()
    for k, name in enumerate(("pos", "vel")):
        scale = np.abs(buf[k]).max()
        assert np.abs(got[k] - buf[k]).max() <= 1e-6 * scale, name
    assert force_err(got[2], buf[2]) < 1e-5


@pytest.mark.parametrize("n,p", [(3000, 6), (20000, 6), (65536, 6), (65536, 8), (30001, 10), (4096, 3)])
def test_energy_fmm_against_fp64_direct_energy(engine, oracle32, oracle64, n, p):
    """nbco_energy_fmm: Coulomb energy from the lists and multipoles of the last kd-tree evaluation (P2P potential + multipole
    expansions evaluated at the particles) against the fp64 direct sum over the same fp32 positions.  The far field carries the
    truncation error of order-p multipoles at the reference's opening radius; what is asserted is what it measures at."""
    import torch
    from coulomb_oscillators_amd import EVAL_FMM_KDTREE
    buf = oracle32.init_reference(n)
    par = oracle32.params(n)
    want = oracle64.energy(buf.astype(np.float64), par.astype(np.float64), threads=8)
    for unsort in (1, 0):
        engine.set(fmm_order=p, unsort=unsort)
        d = dev(buf.copy())
        engine.compute_force(EVAL_FMM_KDTREE, d, n, dev(par))
        got = engine.energy_fmm(d, n, dev(par))
        assert abs(got[0] - want[0]) <= 1e-6 * want[0] and abs(got[1] - want[1]) <= 1e-6 * want[1]
        tol = {3: 3e-3, 6: 2e-4, 8: 5e-5, 10: 2e-5}[p]
        assert abs(got[2] - want[2]) <= tol * want[2], (got[2], want[2], abs(got[2] - want[2]) / want[2])
    # the O(N^2) reduction agrees with the oracle to fp32 pair rounding; the FMM one must not be further from it than its tolerance
    if n <= 20000:
        ref = engine.energy(d, n, dev(par))
        assert abs(ref[2] - want[2]) <= 1e-5 * want[2]
        from coulomb_oscillators_amd import EngineError
        with pytest.raises(EngineError, match="no kd-tree evaluation"):     # nbco_energy repacked the positions: the lists are stale
            engine.energy_fmm(d, n, dev(par))


def test_energy_fmm_large_system_against_sampled_direct_sum(engine, oracle32):
    """N = 1M: the FMM potential energy against a direct fp64 sum over a sample of the particles (the O(N^2) reduction takes
    seconds here and is the thing this entry point replaces)"""
    import torch
    from coulomb_oscillators_amd import EVAL_FMM_KDTREE
    n, p, m = 1 << 20, 6, 2048
    buf = oracle32.init_reference(n)
    par = oracle32.params(n)
    engine.set(fmm_order=p, unsort=0)
    d = dev(buf.copy())
    engine.compute_force(EVAL_FMM_KDTREE, d, n, dev(par))
    got = engine.energy_fmm(d, n, dev(par))
    x = d[0].double()
    idx = torch.randperm(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))[:m]
    phi = torch.zeros(m, dtype=torch.float64, device="cuda")
    for s in range(0, n, 1 << 16):
        r2 = ((x[idx][:, None, :] - x[None, s:s + (1 << 16), :]) ** 2).sum(-1) + 1e-18
        w = r2.rsqrt()
        w[r2 < 1e-17] = 0.0                    # the particle itself
        phi += w.sum(1)
    est = float(par[0]) * 0.5 * float(phi.mean()) * n
    sem = float(par[0]) * 0.5 * float(phi.std()) / np.sqrt(m) * n
    assert abs(got[2] - est) < 5 * sem + 3e-4 * est, (got[2], est, sem)
