"""nbco_modes_record / nbco_mode_corr on the GPU against the long double model of tests/modes_numpy.py and against nbco_mode_corr_ref.

The bounds are derived, not tuned (modes_numpy): rho within sk_numpy.bound(n, h); j_c within u V_c (8 (H + 1) + 2 n + 2); the
correlation sums within (m pairs + 2) u sum|products| (rr, jj), pairs u sum|terms| (s0, s1) and (2 pairs + 8) u sum M M (ll) of the
model -- and, for the same series, THE BYTES of nbco_mode_corr_ref.

The recording kernel's paths: the tiles, items, copies and ranges of nbco_structure_factor, with runs of at most 4 indices ix in
template steps of 1, 2, 3, 4 sums (hx > 3 is cut into chunks).  The correlation kernel's: one lag per lane up to 64 lags, pairs of lags in
steps of 2 (up to 512 lags) and 4; up to four k per workgroup where a k needs 128 lanes or fewer and the LDS holds them."""
import ctypes as C
import functools

import numpy as np
import pytest

import modes_numpy as MN
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


def state(x, v):
    """[pos n | vel n] as one float32 array"""
    return np.concatenate([np.asarray(x, dtype=np.float32).reshape(-1), np.asarray(v, dtype=np.float32).reshape(-1)])


def record(e, x, v, h, kstep, count=True, cap=3, frame=1):
    """one call into a poisoned series: (the K records of the frame as float64 (K, 8), n_used); the other frames must keep the poison"""
    import torch
    K = SK.count(h)
    series = torch.full((K, cap, 8), POISON, dtype=torch.float64, device="cuda")
    out, used = e.modes_record(dev(state(x, v)), len(x), h, kstep, series=series, frame=frame, count=count)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got.shape == (K, cap, 8) and (got[:, frame, :] != POISON).all()
    assert (np.delete(got, frame, axis=1) == POISON).all()
    return got[:, frame, :].copy(), used


def velocities(n, seed):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray((rng.standard_normal((n, 3)) * np.array([0.7, 1.9, 0.3]) + np.array([0.2, 0.0, -1.0])).astype(np.float32))


@functools.lru_cache(maxsize=None)
def case(n, h, centre=0.0):
    """(x, v, model records, n_used, V) of a Gaussian ball with unequal axes and a drifting velocity distribution, read-only"""
    x = SK.cloud(n, 2000 + n, centre=(centre, 0.0, 0.0))
    v = velocities(n, 3000 + n)
    x.setflags(write=False)
    v.setflags(write=False)
    rec, used, V = MN.records(x, v, h, K3)
    return x, v, rec, used, V


WORST = {"rho": 0.0, "j": 0.0}


def hold(got, rec, n, h, V, what):
    err_r, err_j = MN.record_errors(got, rec)
    lim_r, lim_j = SK.bound(n, h), MN.j_bound(n, h, V)
    fr = [err_r / lim_r] + [err_j[c] / lim_j[c] if lim_j[c] > 0 else (0.0 if err_j[c] == 0 else np.inf) for c in range(3)]
    WORST["rho"], WORST["j"] = max(WORST["rho"], fr[0]), max(WORST["j"], *fr[1:])
    print("%s: fractions of the bounds rho %.3g, j %.3g %.3g %.3g (worst so far rho %.3g, j %.3g)" % (what, *fr, WORST["rho"], WORST["j"]))
    assert max(fr) <= 1.0


def check(eng, n, h, centre=0.0):
    x, v, rec, used, V = case(n, tuple(h), centre)
    got, n_used = record(eng, x, v, h, K3)
    assert n_used == used == n
    hold(got, rec, n, h, V, "n %d h %s" % (n, h))
    k0 = SK.index(h, 0, 0, 0)
    assert got[k0, 0] == n and got[k0, 1] == 0.0 and (got[k0, 3::2] == 0.0).all()


# ---- recording: parity with the model ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025, 4097])
@pytest.mark.parametrize("h", [(3, 0, 5), (8, 2, 5)])
def test_parity_over_the_sizes(eng, n, h):
    check(eng, n, h)


@pytest.mark.parametrize("h", [(1, 0, 0), (0, 3, 0), (4, 4, 4), (17, 1, 1), (64, 0, 0), (0, 0, 64), (1, 8, 8)])
def test_parity_over_the_grids(eng, h):
    """run lengths of 2, 1, 3 (two chunks), 4 (five chunks: 18 = 5 x 4 - 2), 4 (seventeen), 1, 2; (1, 8, 8): 289 columns, two workgroups"""
    check(eng, 1025, h)


def test_parity_with_many_ranges(eng):
    check(eng, 65537, (2, 2, 2))


def test_parity_far_from_the_origin(eng):
    """a cloud centred at x = 1000: t of several hundred turns"""
    check(eng, 1025, (4, 4, 4), centre=1000.0)


def test_rows_that_are_not_finite_do_not_count(eng):
    n, h = 1025, (3, 2, 2)
    x, v = case(n, h)[0].copy(), case(n, h)[1].copy()
    bad_x = [(0, 0, np.nan), (5, 1, np.inf), (63, 2, -np.inf), (64, 0, np.inf), (512, 2, np.nan), (1024, 0, -np.inf)]
    bad_v = [(1, 0, np.nan), (7, 2, np.inf), (65, 1, -np.inf), (511, 0, np.nan), (1023, 2, np.inf), (700, 1, np.nan)]
    for row, axis, q in bad_x:
        x[row, axis] = q
    for row, axis, q in bad_v:
        v[row, axis] = q
    x[700, 2] = np.inf   # (both at once is still one row)
    got, used = record(eng, x, v, h, K3)
    rec, want_used, V = MN.records(x, v, h, K3)
    assert used == want_used == n - len(bad_x) - len(bad_v)
    assert np.isfinite(got).all()
    hold(got, rec, n, h, V, "rows that do not count")
    k0 = SK.index(h, 0, 0, 0)
    assert got[k0, 0] == used and got[k0, 1] == 0.0 and (got[k0, 3::2] == 0.0).all()


# ---- recording: closed forms ---------------------------------------------------------------------------------------------------------
def test_one_particle_at_a_dyadic_position(eng):
    """x = (1/4, -1/8, 3/8) with kstep = 2 pi: every rho_k is a power of exp(2 pi i / 8), and j_k = v rho_k"""
    x = np.array([[0.25, -0.125, 0.375]], dtype=np.float32)
    v = np.array([[1.5, -2.0, 0.25]], dtype=np.float32)
    h = (4, 3, 2)
    got, used = record(eng, x, v, h, (SK.TWO_PI_D,) * 3)
    assert used == 1
    s = np.sqrt(0.5)
    eighth = [(1, 0), (s, s), (0, 1), (-s, s), (-1, 0), (-s, -s), (0, -1), (s, -s)]
    lim_j = MN.j_bound(1, h, [1.5, 2.0, 0.25])
    for ix in range(h[0] + 1):
        for iy in range(-h[1], h[1] + 1):
            for iz in range(-h[2], h[2] + 1):
                want = complex(*eighth[(2 * ix - iy + 3 * iz) % 8])
                g = got[SK.index(h, ix, iy, iz)]
                assert abs(complex(g[0], g[1]) - want) <= SK.bound(1, h), (ix, iy, iz)
                for c in range(3):
                    assert abs(complex(g[2 + 2 * c], g[3 + 2 * c]) - float(v[0, c]) * want) <= lim_j[c], (ix, iy, iz, c)
    # exact quarter turns
    assert got[SK.index(h, 0, 0, 0)].tolist() == [1.0, 0.0, 1.5, 0.0, -2.0, 0.0, 0.25, 0.0]
    assert got[SK.index(h, 1, 0, 0)].tolist() == [0.0, 1.0, 0.0, 1.5, 0.0, -2.0, 0.0, 0.25]
    assert got[SK.index(h, 2, 0, 0)].tolist() == [-1.0, 0.0, -1.5, 0.0, 2.0, 0.0, -0.25, 0.0]


def test_two_mirrored_particles(eng):
    """x1 = -x2, v1 = -v2: rho_k = 2 cos(k . x1) is real, j_k = 2 i v1 sin(k . x1) imaginary"""
    x = np.array([[0.3, 0.7, -0.2], [-0.3, -0.7, 0.2]], dtype=np.float32)
    v = np.array([[1.0, -0.5, 2.0], [-1.0, 0.5, -2.0]], dtype=np.float32)
    h = (3, 2, 2)
    got, used = record(eng, x, v, h, K3)
    rec, _, V = MN.records(x, v, h, K3)
    assert used == 2
    hold(got, rec, 2, h, V, "two particles")
    lim_j = MN.j_bound(2, h, V)
    assert np.abs(got[:, 1]).max() <= SK.bound(2, h) and np.abs(got[:, 0]).max() > 1.0
    for c in range(3):
        assert np.abs(got[:, 2 + 2 * c]).max() <= lim_j[c] and np.abs(got[:, 3 + 2 * c]).max() > 0.5


def test_a_plain_snapshot_is_frames_cap_one(eng):
    n, h = 257, (3, 0, 5)
    x, v, rec, used, V = case(n, h)
    out, n_used = eng.modes_record(dev(state(x, v)), n, h, K3)
    assert tuple(out.shape) == (SK.count(h), 1, 8) and n_used == n
    hold(out.cpu().numpy()[:, 0, :], rec, n, h, V, "snapshot")


# ---- recording: determinism ----------------------------------------------------------------------------------------------------------
def test_the_same_bytes_on_every_call(engine_lib, eng):
    """a second call, a call on another stream and a call with opts.sync flipped"""
    import torch
    from coulomb_oscillators_amd import Engine
    n, h = 4097, (5, 3, 2)
    x, v = case(n, h)[:2]
    first, used = record(eng, x, v, h, K3)
    again, _ = record(eng, x, v, h, K3)
    assert first.tobytes() == again.tobytes()
    nocount, none = record(eng, x, v, h, K3, count=False)
    assert none is None and first.tobytes() == nocount.tobytes()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        e2 = Engine(stream=side.cuda_stream)
        try:
            other, used2 = record(e2, x, v, h, K3)
        finally:
            e2.close()
    assert first.tobytes() == other.tobytes() and used2 == used
    flipped = 0 if eng.opts().sync else 1
    e3 = Engine(sync=flipped)
    try:
        assert e3.opts().sync == flipped
        third, _ = record(e3, x, v, h, K3, count=False)
    finally:
        e3.close()
    assert first.tobytes() == third.tobytes()


# ---- correlation ---------------------------------------------------------------------------------------------------------------------
def correlate(e, series, h, frames, lags):
    """one call into a poisoned output with room behind it: the K x lags records as MODE_LAG; what lies behind must keep the poison"""
    import torch
    from coulomb_oscillators_amd import MODE_LAG
    K = SK.count(h)
    out = torch.full((K * lags + 5, 8), POISON, dtype=torch.float64, device="cuda")
    e.mode_corr(dev(series), h, K3, frames, lags, out=out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[K * lags:] == POISON).all()
    return np.ascontiguousarray(got[:K * lags]).view(MODE_LAG).reshape(K, lags)


HOST_SHAPES = sorted({(f, l) for f in (1, 2, 63, 64, 65, 257) for l in (1, f, min(f, 64))})
# (300, 129): pairs of lags on 128 lanes, two k per workgroup; (600, 513): four lags per lane, the odd one out
MORE_SHAPES = [(300, 129), (600, 513)]


@pytest.mark.parametrize("h", [(0, 0, 0), (1, 1, 1), (2, 3, 1)])
@pytest.mark.parametrize("frames,lags", HOST_SHAPES + MORE_SHAPES)
def test_corr_has_the_bytes_of_the_host_rule(eng, h, frames, lags):
    from coulomb_oscillators_amd import mode_corr_ref
    K, cap = SK.count(h), frames + 3
    series = MN.random_series(K, cap, 100 * frames + lags + sum(h))
    series[:, frames:, :] = np.nan   # beyond `frames`: never read
    got = correlate(eng, series, h, frames, lags)
    want = mode_corr_ref(series, h, K3, frames, lags)
    assert (got["pairs"] == (frames - np.arange(lags))[None, :]).all()
    assert got.tobytes() == want.tobytes()
    lag_list = list(range(lags)) if lags <= 65 else sorted(set(range(0, lags, 23)) | {lags - 1, lags // 2, lags // 2 + 1})
    frac = MN.corr_fractions(got[:, lag_list], MN.correlate(series, h, K3, frames, lag_list=lag_list))
    print("h %s frames %d lags %d: worst fractions of the bounds %s" % (h, frames, lags, frac))
    assert max(frac.values()) <= 1.0


def test_corr_at_the_longest_series(eng):
    """frames = lags = 1024 at K = 18: the 64 KiB of LDS, four lags per lane"""
    from coulomb_oscillators_amd import mode_corr_ref
    h, frames = (1, 1, 1), 1024
    series = MN.random_series(SK.count(h), frames, 9)
    got = correlate(eng, series, h, frames, frames)
    assert got.tobytes() == mode_corr_ref(series, h, K3, frames, frames).tobytes()
    lag_list = [0, 1, 255, 256, 511, 512, 513, 767, 768, 1022, 1023]
    frac = MN.corr_fractions(got[:, lag_list], MN.correlate(series, h, K3, frames, lag_list=lag_list))
    print("frames 1024: worst fractions of the bounds %s" % frac)
    assert max(frac.values()) <= 1.0


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def test_a_drifting_lattice(eng):
    """4^3 particles at j / 4 drifting by d = (1, -2, 3) / 64 per frame (every position exact in fp32), kstep = 2 pi 4: every k of the grid
    is a reciprocal lattice vector, rho_k(t) = n exp(i k . d t) and rr(k, tau) = pairs n^2 cos(k . d tau).  A record is within
    B = sk_numpy.bound(n, h) of that, so a product of two within 2 n B + B^2 and the sum of `pairs` of them within pairs times that; the
    correlation adds (2 pairs + 2) u sum|products| <= (2 pairs + 2) u pairs (n + B)^2."""
    import torch
    h, frames, n = (2, 2, 2), 9, 64
    j = np.arange(4) / 4.0
    x0 = np.stack(np.meshgrid(j, j, j, indexing="ij"), axis=-1).reshape(-1, 3)
    d = np.array([1.0, -2.0, 3.0]) / 64.0
    kstep = (4.0 * SK.TWO_PI_D,) * 3
    K = SK.count(h)
    series = torch.full((K, frames, 8), POISON, dtype=torch.float64, device="cuda")
    for t in range(frames):
        x = (x0 + d[None, :] * t).astype(np.float32)
        assert np.array_equal(x.astype(np.float64), x0 + d[None, :] * t)
        _, used = eng.modes_record(dev(state(x, np.broadcast_to(d, x.shape))), n, h, kstep, series=series, frame=t)
        assert used == n
    from coulomb_oscillators_amd import MODE_LAG
    out = eng.mode_corr(series, h, kstep, frames, frames)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(MODE_LAG).reshape(K, frames)
    idx = MN.wave_vectors(h, (1.0, 1.0, 1.0))          # the integer indices
    turns = (idx @ np.array([1.0, -2.0, 3.0])) / 16.0  # k . d / 2 pi = 4 (ix - 2 iy + 3 iz) / 64, exact
    tau = np.arange(frames)
    pairs = (frames - tau).astype(np.float64)
    cyc = np.outer(turns, tau)
    want = pairs[None, :] * n * n * np.asarray(np.cos(SK.TWO_PI * (cyc - np.rint(cyc)).astype(SK.L)), dtype=np.float64)
    B = SK.bound(n, h)
    lim = pairs * (2 * n * B + B * B) + (2 * pairs + 2) * MN.U * pairs * (n + B) ** 2 + MN.U * pairs * n * n   # (the last: `want` in fp64)
    err = np.abs(got["rr"] - want)
    print("drifting lattice: worst fraction of the bound %.3g" % float((err / lim[None, :]).max()))
    assert (err <= lim[None, :]).all()
    assert (got["pairs"] == (frames - tau)[None, :]).all()


# ---- state ---------------------------------------------------------------------------------------------------------------------------
def test_the_modes_calls_leave_a_kd_evaluation_and_the_run_as_they_were(oracle32):
    """an nbco_fmm_kdtree evaluation with tree_steps = 8, nbco_kd_potential and nbco_kd_probe, then both calls: nbco_kd_get_info is
    unchanged, and the following nbco_kd_potential, nbco_kd_probe and nbco_integrate_steps return the bits they return on a context
    that never made the calls"""
    import torch
    from coulomb_oscillators_amd import Engine, EVAL_FMM_KDTREE, INTEG_LEAPFROG
    n, p, m = 3000, 4, 64
    buf, par = oracle32.init_reference(n), oracle32.params(n)
    probes = np.ascontiguousarray(buf[0][:m] * 1.5)
    h, kstep = (4, 4, 4), (900.0, 900.0, 900.0)

    def drive(with_modes):
        e = Engine(fmm_order=p, tree_steps=8, unsort=0)
        try:
            d, prm, t = torch.from_numpy(buf.copy()).cuda(), torch.from_numpy(par).cuda(), dev(probes)

            def diagnostics():
                phi = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
                a = torch.full((m, 3), float("nan"), dtype=torch.float64, device="cuda")
                psi = torch.full((m,), float("nan"), dtype=torch.float64, device="cuda")
                en = np.asarray(e.energy_kd(d, n, prm, phi)).tobytes()
                e.probe_kd(t, m, prm, a, psi)
                torch.cuda.synchronize()
                return en + phi.cpu().numpy().tobytes() + a.cpu().numpy().tobytes() + psi.cpu().numpy().tobytes()
            e.compute_force(EVAL_FMM_KDTREE, d, n, prm)
            out = diagnostics()
            if with_modes:
                info = bytes(e.kd_info())
                series, used = e.modes_record(d, n, h, kstep, frames_cap=2, frame=0)
                assert used == n and series[SK.index(h, 0, 0, 0), 0, 0].item() == n
                e.modes_record(d, n, h, kstep, series=series, frame=1, count=False)
                e.mode_corr(series, h, kstep, 2, 2)
                torch.cuda.synchronize()
                assert bytes(e.kd_info()) == info
            out += diagnostics()
            e.integrate_steps(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, 5e-4, 10)
            return out + d.cpu().numpy().tobytes() + bytes(e.kd_info())
        finally:
            e.close()
    assert drive(True) == drive(False)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def grid(h, kstep=K3):
    from coulomb_oscillators_amd.engine import SkGrid
    g = SkGrid()
    for a in range(3):
        g.h[a], g.kstep[a] = h[a], kstep[a]
    return g


def bad_grids(h):
    out = []
    for a in range(3):
        for q in (-1, 65):
            out.append(grid(tuple(q if b == a else h[b] for b in range(3))))
        for q in (0.0, -1.0, float("inf"), float("nan")):
            out.append(grid(h, tuple(q if b == a else K3[b] for b in range(3))))
    return out


def test_record_refusals_leave_the_outputs_alone(eng):
    import torch
    from coulomb_oscillators_amd.engine import _ptr
    n, h, cap = 255, (2, 1, 1), 3
    x, v = case(n, h)[:2]
    d = dev(state(x, v))
    K = SK.count(h)
    series = torch.full((K, cap, 8), POISON, dtype=torch.float64, device="cuda")
    used = C.c_longlong(-5)

    def call(ctx=eng.ctx, p=d, n=n, g=grid(h), s=series, cap=cap, frame=1):
        return eng.lib.nbco_modes_record(ctx, _ptr(p), n, C.byref(g) if g is not None else None, _ptr(s), cap, frame, C.byref(used))
    bad = [dict(ctx=None), dict(p=None), dict(g=None), dict(s=None), dict(n=0), dict(n=-3), dict(cap=0, frame=0), dict(cap=-1, frame=0),
           dict(frame=-1), dict(frame=cap), dict(frame=cap + 7)] + [dict(g=g) for g in bad_grids(h)]
    for kw in bad:
        assert call(**kw) == ERR_ARG, kw
    assert call(n=1 << 31) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (series.cpu().numpy() == POISON).all() and used.value == -5
    assert call() == 0 and used.value == n     # a good call afterwards
    torch.cuda.synchronize()
    assert series[SK.index(h, 0, 0, 0), 1, 0].item() == n


def test_corr_refusals_leave_the_outputs_alone(eng):
    import torch
    from coulomb_oscillators_amd.engine import _ptr
    h, cap = (1, 1, 1), 8
    K = SK.count(h)
    series = dev(MN.random_series(K, cap, 1))
    out = torch.full((K * 8, 8), POISON, dtype=torch.float64, device="cuda")

    def call(ctx=eng.ctx, s=series, g=grid(h), cap=cap, frames=8, lags=8, o=out):
        return eng.lib.nbco_mode_corr(ctx, _ptr(s), C.byref(g) if g is not None else None, cap, frames, lags, _ptr(o))
    bad = [dict(ctx=None), dict(s=None), dict(g=None), dict(o=None), dict(lags=0), dict(lags=-1), dict(lags=9), dict(frames=9, lags=1),
           dict(frames=0, lags=0), dict(cap=2048, frames=1025, lags=1)] + [dict(g=g) for g in bad_grids(h)]
    for kw in bad:
        assert call(**kw) == ERR_ARG, kw
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == POISON).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() != POISON).all()
