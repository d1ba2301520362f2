"""nbco_structure_factor / nbco_2d_structure_factor on the GPU against the long double model of tests/sk_numpy.py.

The bound is derived, not tuned (sk_numpy.bound): |rho_k - model_k| <= n u (8 (hx + hy + hz + 1) + n), u = 2^-53 -- the base phases
(4 u), one complex product per power step and axis join, and the worst case of any summation order over n terms of modulus <= 1.
It is loose next to an error of order 1 from a dropped or doubled particle, a wrong sign, conjugate or index.

The kernel's paths: a tile holds min(256, 3072 / (1 + (hy+1) + (hz+1) + chunks)) particles; a lane keeps a run of L <= 17 indices ix
in a template step of 1, 2, 3, 5, 9, 13 or 17 sums, hx > 16 is cut into chunks; a workgroup owns up to 256 (chunk, iy, iz) items, and
where they are 128 or fewer several copies of them over interleaved particles; the particles are cut into ranges of at least 512, whose
sums are added in 16 slices."""
import functools

import numpy as np
import pytest

import sk_numpy as SK

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = 2, 4
POISON = -123.456
K3 = (2.3, 3.1, 1.4)   # rad per unit length: phases of many turns over a cloud of unit width


@pytest.fixture(scope="module")
def eng(engine_lib):
    import torch
    from coulomb_oscillators_amd import Engine
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible (there is no CPU fallback)")
    e = Engine()
    yield e
    e.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def run(e, x, h, kstep, count=True):
    """one call into a poisoned buffer: (rho as complex128 numpy, n_used); every entry must have been overwritten"""
    import torch
    dim = x.shape[1]
    K = SK.count(h[:dim])
    rho = torch.full((K,), complex(POISON, POISON), dtype=torch.complex128, device="cuda")
    fn = e.structure_factor if dim == 3 else e.structure_factor_2d
    out, used = fn(dev(x), len(x), h, kstep, rho=rho, count=count)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got.shape == (K,) and (got.real != POISON).all() and (got.imag != POISON).all()
    return got, used


@functools.lru_cache(maxsize=None)
def case(n, h, dim=3, centre=0.0, seed=0):
    """(x, model re, model im, n_used) of a Gaussian ball with unequal axes, read-only"""
    x = SK.cloud(n, 1000 + n + seed, centre=(centre, 0.0, 0.0), dim=dim)
    x.setflags(write=False)
    re, im, used = SK.structure_factor(x, h[:dim], K3[:dim])
    return x, re, im, used


def check(eng, n, h, dim=3, centre=0.0):
    x, re, im, used = case(n, tuple(h), dim, centre)
    got, n_used = run(eng, x, h, K3)
    err, lim = SK.error(got, re, im), SK.bound(n, h[:dim])
    print("n %d h %s dim %d: error %.3g, bound %.3g" % (n, h, dim, err, lim))
    assert n_used == used == n
    assert err <= lim
    k0 = SK.index(h[:dim], 0, 0, 0)
    assert got[k0] == complex(n, 0.0)


# ---- closed forms ------------------------------------------------------------------------------------------------------------------
def test_one_particle_at_a_dyadic_position(eng):
    """x = (1/4, -1/8, 3/8) with kstep = 2 pi: every rho_k is a power of exp(2 pi i / 8)"""
    x = np.array([[0.25, -0.125, 0.375]], dtype=np.float32)
    h = (4, 3, 2)
    got, used = run(eng, x, h, (SK.TWO_PI_D,) * 3)
    assert used == 1
    s = np.sqrt(0.5)
    eighth = [(1, 0), (s, s), (0, 1), (-s, s), (-1, 0), (-s, -s), (0, -1), (s, -s)]
    for ix in range(h[0] + 1):
        for iy in range(-h[1], h[1] + 1):
            for iz in range(-h[2], h[2] + 1):
                want = complex(*eighth[(2 * ix - iy + 3 * iz) % 8])
                assert abs(got[SK.index(h, ix, iy, iz)] - want) <= SK.bound(1, h), (ix, iy, iz)
    assert got[SK.index(h, 0, 0, 0)] == 1.0 and got[SK.index(h, 1, 0, 0)] == 1j and got[SK.index(h, 2, 0, 0)] == -1.0   # exact quarter turns


def test_two_particles(eng):
    """x1 = -x2: rho_k = 2 cos(k . x1), real"""
    x = np.array([[0.3, 0.7, -0.2], [-0.3, -0.7, 0.2]], dtype=np.float32)
    h = (3, 2, 2)
    got, used = run(eng, x, h, K3)
    re, im, _ = SK.structure_factor(x, h, K3)
    assert used == 2 and SK.error(got, re, im) <= SK.bound(2, h)
    assert np.abs(got.imag).max() <= SK.bound(2, h) and np.abs(got.real).max() > 1.0


@pytest.mark.parametrize("n", [1, 257, 4097])
def test_the_zero_vector_alone(eng, n):
    x = case(n, (0, 0, 0))[0]
    got, used = run(eng, x, (0, 0, 0), K3)
    assert got.shape == (1,) and got[0] == complex(n, 0.0) and used == n


def test_simple_cubic_lattice(eng):
    """8^3 particles at j/8 - 1/2, kstep = 2 pi, h = (8, 8, 8): 512 on the 18 vectors with every index a multiple of 8, 0 elsewhere"""
    j = np.arange(8) / 8.0 - 0.5
    x = np.stack(np.meshgrid(j, j, j, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    h = (8, 8, 8)
    got, used = run(eng, x, h, (SK.TWO_PI_D,) * 3)
    lim = SK.bound(512, h)
    peaks = 0
    want = np.zeros(SK.count(h), dtype=np.complex128)
    for ix in (0, 8):
        for iy in (-8, 0, 8):
            for iz in (-8, 0, 8):
                want[SK.index(h, ix, iy, iz)] = 512.0
                peaks += 1
    err = np.abs(got - want).max()
    print("lattice: error %.3g, bound %.3g" % (err, lim))
    assert used == 512 and peaks == 18 and err <= lim


# ---- parity with the model ---------------------------------------------------------------------------------------------------------
SIZES = [1, 63, 64, 65, 255, 256, 257, 1025, 4097]
GRIDS = [(1, 0, 0), (0, 3, 0), (3, 0, 5), (4, 4, 4), (8, 2, 5), (64, 0, 0), (0, 0, 64),
         (1, 8, 8)]   # (1, 8, 8): 289 columns, two workgroups of items


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("h", [(3, 0, 5), (8, 2, 5)])
def test_parity_over_the_sizes(eng, n, h):
    check(eng, n, h)


@pytest.mark.parametrize("h", GRIDS)
@pytest.mark.parametrize("n", [257, 1025])
def test_parity_over_the_grids(eng, n, h):
    check(eng, n, h)


@pytest.mark.parametrize("hx", [0, 1, 2, 3, 4, 5, 8, 9, 12, 13, 16, 17, 25, 33, 34, 51, 64])
def test_parity_across_the_template_steps_of_hx(eng, hx):
    """run lengths 1, 2, 3 | 4, 5 | 6, 9 | 10, 13 | 14, 17 sums, then two (17: 9 + 9, 25: 13 + 13, 33: 17 + 17), three (34, 51) and four chunks"""
    check(eng, 257, (hx, 1, 1))


@pytest.mark.parametrize("n", [44, 45, 46, 91])
def test_parity_around_a_short_tile(eng, n):
    """h = (0, 0, 64): 67 complex numbers per particle, a tile of 45"""
    check(eng, n, (0, 0, 64))


def test_parity_on_the_largest_grid(eng):
    """h = 64 on every axis: 66564 items, a tile of 22 (23 particles: two tiles), 1.08 million wave vectors, all of them written and every
    37th of them, the zero vector and the last one held to the model"""
    n, h = 23, (64, 64, 64)
    x = SK.cloud(n, 77)
    got, used = run(eng, x, h, K3)
    only = np.unique(np.concatenate([np.arange(0, SK.count(h), 37), [SK.index(h, 0, 0, 0), SK.count(h) - 1]]))
    re, im, want_used = SK.structure_factor(x, h, K3, only=only)
    assert used == want_used == n and SK.error(got[only], re, im) <= SK.bound(n, h)
    assert got[SK.index(h, 0, 0, 0)] == complex(n, 0.0)


def test_parity_with_many_ranges(eng):
    check(eng, 65537, (2, 2, 2))


def test_parity_far_from_the_origin(eng):
    """a cloud centred at x = 1000: t of several hundred turns"""
    check(eng, 1025, (4, 4, 4), centre=1000.0)


def test_rows_that_are_not_finite_do_not_count(eng):
    n, h = 1025, (3, 2, 2)
    x = case(n, h)[0].copy()
    bad = [(0, 0, np.nan), (5, 1, np.inf), (63, 2, -np.inf), (64, 0, np.inf), (511, 1, np.nan), (512, 2, np.nan), (1024, 0, -np.inf), (700, 1, np.nan)]
    for row, axis, v in bad:
        x[row, axis] = v
    x[700, 2] = np.inf
    got, used = run(eng, x, h, K3)
    re, im, want_used = SK.structure_factor(x, h, K3)
    assert used == want_used == n - len(bad)
    assert np.isfinite(got.real).all() and np.isfinite(got.imag).all()
    assert SK.error(got, re, im) <= SK.bound(n, h)
    assert got[SK.index(h, 0, 0, 0)] == complex(used, 0.0)


# ---- determinism ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [3, 2])
def test_the_same_bytes_on_every_call(engine_lib, eng, dim):
    """a second call, a call on another stream and a call with opts.sync flipped"""
    import torch
    from coulomb_oscillators_amd import Engine
    n, h = 4097, (5, 3, 2)
    x = case(n, h, dim)[0]
    first, used = run(eng, x, h, K3)
    again, _ = run(eng, x, h, K3)
    assert first.tobytes() == again.tobytes()
    nocount, none = run(eng, x, h, K3, count=False)
    assert none is None and first.tobytes() == nocount.tobytes()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        e2 = Engine(stream=side.cuda_stream)
        try:
            other, used2 = run(e2, x, h, K3)
        finally:
            e2.close()
    assert first.tobytes() == other.tobytes() and used2 == used
    flipped = 0 if eng.opts().sync else 1
    e3 = Engine(sync=flipped)
    try:
        assert e3.opts().sync == flipped
        third, _ = run(e3, x, h, K3, count=False)
    finally:
        e3.close()
    assert first.tobytes() == third.tobytes()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [3, 2])
def test_refusals_leave_the_outputs_alone(eng, dim):
    import ctypes as C
    import torch
    from coulomb_oscillators_amd.engine import SkGrid, _ptr
    n, h = 255, (2, 1, 1)
    d = dev(case(n, h, dim)[0])
    K = SK.count(h[:dim])
    rho = torch.full((K,), complex(POISON, POISON), dtype=torch.complex128, device="cuda")
    used = C.c_longlong(-5)
    fn = eng.lib.nbco_structure_factor if dim == 3 else eng.lib.nbco_2d_structure_factor

    def grid(h=h, kstep=K3):
        g = SkGrid()
        for a in range(3):
            g.h[a], g.kstep[a] = h[a], kstep[a]
        return g

    def call(ctx=eng.ctx, p=d, n=n, g=grid(), r=rho):
        return fn(ctx, _ptr(p), n, C.byref(g) if g is not None else None, _ptr(r), C.byref(used))
    bad = [dict(ctx=None), dict(p=None), dict(g=None), dict(r=None), dict(n=0), dict(n=-3)]
    for a in range(dim):
        for v in (-1, 65):
            bad.append(dict(g=grid(h=tuple(v if b == a else h[b] for b in range(3)))))
        for v in (0.0, -1.0, float("inf"), float("nan")):
            bad.append(dict(g=grid(kstep=tuple(v if b == a else K3[b] for b in range(3)))))
    for kw in bad:
        assert call(**kw) == ERR_ARG, kw
    assert call(n=1 << 31) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    got = rho.cpu().numpy()
    assert (got.real == POISON).all() and (got.imag == POISON).all() and used.value == -5
    if dim == 2:   # the 2-D form reads [0..1] only
        assert call(g=grid(h=(2, 1, -9), kstep=(K3[0], K3[1], float("nan")))) == 0 and used.value == n
        used.value = -5
    assert call() == 0 and used.value == n     # a good call afterwards
    torch.cuda.synchronize()
    assert rho[SK.index(h[:dim], 0, 0, 0)].item() == complex(n, 0.0)


# ---- two dimensions ----------------------------------------------------------------------------------------------------------------------
def test_2d_one_and_two_particles(eng):
    x = np.array([[0.25, -0.125]], dtype=np.float64)
    h = (4, 3)
    got, used = run(eng, x, h, (SK.TWO_PI_D,) * 2)
    s = np.sqrt(0.5)
    eighth = [(1, 0), (s, s), (0, 1), (-s, s), (-1, 0), (-s, -s), (0, -1), (s, -s)]
    for ix in range(h[0] + 1):
        for iy in range(-h[1], h[1] + 1):
            assert abs(got[SK.index(h, ix, iy)] - complex(*eighth[(2 * ix - iy) % 8])) <= SK.bound(1, h)
    assert used == 1 and got[SK.index(h, 0, 0)] == 1.0 and got[SK.index(h, 2, 0)] == -1.0
    x = np.array([[0.3, 0.7], [-0.3, -0.7]], dtype=np.float64)
    got, used = run(eng, x, h, K3)
    re, im, _ = SK.structure_factor(x, h, K3[:2])
    assert used == 2 and SK.error(got, re, im) <= SK.bound(2, h) and np.abs(got.imag).max() <= SK.bound(2, h)
    got, used = run(eng, x, (0, 0), K3)
    assert got.shape == (1,) and got[0] == 2.0


@pytest.mark.parametrize("n,h", [(1, (3, 5)), (255, (3, 5)), (256, (3, 5)), (257, (3, 5)), (1025, (8, 2)), (4097, (4, 4)), (257, (64, 0)), (257, (0, 64)),
                                 (91, (0, 64)), (257, (17, 64)), (257, (2, 64)), (65537, (2, 2))])
def test_2d_parity(eng, n, h):
    """(0, 64): a tile of 46; (2, 64): 129 items; (17, 64): 258 items in two chunks, two workgroups of items"""
    check(eng, n, h, dim=2)


def test_2d_rows_that_are_not_finite_and_a_far_cloud(eng):
    n, h = 1025, (3, 4)
    check(eng, n, h, dim=2, centre=1000.0)
    x = case(n, h, 2)[0].copy()
    x[0, 0], x[64, 1], x[1024, 0], x[600, 1] = np.nan, np.inf, -np.inf, 1e308   # (1e308 * w overflows: t is not finite)
    got, used = run(eng, x, h, (K3[0], 70.0))
    re, im, want_used = SK.structure_factor(x, h, (K3[0], 70.0))
    assert used == want_used == n - 4 and SK.error(got, re, im) <= SK.bound(n, h)
    assert got[SK.index(h, 0, 0)] == complex(used, 0.0)


# ---- state -------------------------------------------------------------------------------------------------------------------------------
def test_structure_factor_leaves_a_kd_evaluation_and_the_run_as_they_were(oracle32):
    """an nbco_fmm_kdtree evaluation with tree_steps = 8, nbco_kd_potential, then both calls: nbco_kd_get_info is unchanged, and the
    following nbco_kd_potential and nbco_integrate_steps return the bits they return on a context that never made the calls"""
    import torch
    from coulomb_oscillators_amd import Engine, EVAL_FMM_KDTREE, INTEG_LEAPFROG
    n, p = 3000, 4
    buf, par = oracle32.init_reference(n), oracle32.params(n)
    x2 = case(257, (3, 5), 2)[0]

    def drive(with_sk):
        e = Engine(fmm_order=p, tree_steps=8, unsort=0)
        try:
            d, prm = torch.from_numpy(buf.copy()).cuda(), torch.from_numpy(par).cuda()
            e.compute_force(EVAL_FMM_KDTREE, d, n, prm)
            phi = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
            out = np.asarray(e.energy_kd(d, n, prm, phi)).tobytes() + phi.cpu().numpy().tobytes()
            if with_sk:
                info = bytes(e.kd_info())
                rho, used = e.structure_factor(d, n, (4, 4, 4), (900.0, 900.0, 900.0))
                assert used == n and rho[SK.index((4, 4, 4), 0, 0, 0)].item() == complex(n, 0.0)
                rho, used = e.structure_factor_2d(dev(x2), 257, (3, 5), K3)
                assert used == 257 and bytes(e.kd_info()) == info
            phi.fill_(float("nan"))
            out += np.asarray(e.energy_kd(d, n, prm, phi)).tobytes() + phi.cpu().numpy().tobytes()
            e.integrate_steps(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, 5e-4, 10)
            return out + d.cpu().numpy().tobytes() + bytes(e.kd_info())
        finally:
            e.close()
    assert drive(True) == drive(False)
