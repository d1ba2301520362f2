"""GPU tests of the aperture: nbco_aperture_count / nbco_aperture_apply and their nbco_2d_ forms (Engine.aperture_count, aperture,
aperture_count_2d, aperture_2d) against the fp64 numpy model tests/aperture_numpy.py.  The rule has no square root, no division on
the device and no fused multiply-add, and a compaction moves bits: every comparison in this file is on BYTES, there is no tolerance."""
import ctypes as C

import numpy as np
import pytest

import aperture_numpy as AP

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_CAPACITY, ERR_UNSUPPORTED = 2, 3, 4
# the wave edge, the workgroup edge, one group of 64 workgroup counts (4097 rows: 17 counts), a second level of the scan (65 537 rows:
# 257 counts in 5 groups) and a third (1 048 833 rows: 4098 counts, 65 group sums, 2 sums of those)
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 4097, 65537, 300001)
THREE_LEVELS = 1048833
PATTERNS = ("nobody", "everybody", "first", "last", "alternating", "random", "nonfinite")
GUARD = 5                              # records behind lost_cap that must stay as they were
HALF = (0.0075, 0.0025, 0.025)         # 2.5 rms radii of the reference Gaussian
FAR = (3.0, 1.0, 10.0)
GEOM = {3: dict(half=(0.7, 0.5, 0.9), centre=(0.1, -0.2, 0.05)), 2: dict(half=(0.7, 0.5), centre=(0.1, -0.2))}


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


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def make_state(dim, shape, n, pattern, seed):
    """(state (3, n, dim), mask of the rows meant to be lost): rows inside reach up to 0.999 of the surface, rows outside start at
    1.001 of it -- or hold a NaN or an infinity"""
    rng = np.random.default_rng(seed)
    dtype = np.float32 if dim == 3 else np.float64
    half, centre = np.array(GEOM[dim]["half"]), np.array(GEOM[dim]["centre"])
    out = {"nobody": np.zeros(n, bool), "everybody": np.ones(n, bool), "first": np.arange(n) == 0, "last": np.arange(n) == n - 1,
           "alternating": np.arange(n) % 2 == 1, "random": rng.random(n) < 0.1, "nonfinite": rng.random(n) < 0.05}[pattern]
    if shape == AP.ELLIPSOID:
        v = rng.standard_normal((n, dim))
        v /= np.sqrt((v * v).sum(axis=1))[:, None]
        r = np.where(out, rng.uniform(1.001, 3.0, n), 0.999 * rng.random(n) ** (1.0 / dim))
        u = v * r[:, None]
    else:
        u = rng.uniform(-0.999, 0.999, (n, dim))
        axis = rng.integers(0, dim, n)
        far = rng.uniform(1.001, 3.0, n) * rng.choice([-1.0, 1.0], n)
        u[out, axis[out]] = far[out]
    pos = (centre + u * half).astype(dtype)
    if pattern == "nonfinite":
        bad = np.nonzero(out)[0]
        pos[bad] = (centre + 0.1 * half).astype(dtype)                           # inside but for one coordinate
        pos[bad, rng.integers(0, dim, len(bad))] = rng.choice([np.nan, np.inf, -np.inf], len(bad))
    state = rng.standard_normal((3, n, dim)).astype(dtype)
    state[0] = pos
    return state, out


def lost_buffers(dim, cap):
    import torch
    dtype = torch.float32 if dim == 3 else torch.float64
    lost = torch.full(((cap + GUARD) * 2 * dim,), -7.25, dtype=dtype, device="cuda")
    rows = torch.full((cap + GUARD,), -77, dtype=torch.int32, device="cuda")
    return lost, rows


def fns(e, dim):
    return (e.aperture_count, e.aperture) if dim == 3 else (e.aperture_count_2d, e.aperture_2d)


def check_case(e, dim, shape, n, pattern, seed):
    from coulomb_oscillators_amd import EngineError
    count, apply = fns(e, dim)
    g = GEOM[dim]
    state, meant = make_state(dim, shape, n, pattern, seed)
    want_state, want_lost, want_rows = AP.apply(state, shape, g["half"], g["centre"])
    k = len(want_rows)
    assert np.array_equal(np.nonzero(meant)[0], want_rows), "the pattern is not what the model loses"
    d = dev(state.reshape(-1))
    # _count: n - n_kept, and p is left alone
    assert count(d, n, shape, g["half"], g["centre"]) == k
    assert same(d.cpu().numpy(), state.reshape(-1))
    # too small a record: refused, nothing moved, n_kept right
    if k:
        lost, rows = lost_buffers(dim, k - 1)
        with pytest.raises(EngineError) as err:
            apply(d, n, shape, g["half"], g["centre"], lost=lost[:(k - 1) * 2 * dim], lost_row=rows[:k - 1])
        assert err.value.status == ERR_CAPACITY and err.value.n_kept == n - k
        assert same(d.cpu().numpy(), state.reshape(-1))
        assert (lost == -7.25).all() and (rows == -77).all()
    # the call itself, with a record of exactly k (at least 1) and guard records behind it
    cap = max(k, 1)
    lost, rows = lost_buffers(dim, cap)
    kept = apply(d, n, shape, g["half"], g["centre"], lost=lost[:cap * 2 * dim], lost_row=rows[:cap])
    assert kept == n - k
    got = d.cpu().numpy()
    assert same(got[:3 * dim * kept].reshape(3, kept, dim), want_state)
    got_lost, got_rows = lost.cpu().numpy().reshape(-1, 2 * dim), rows.cpu().numpy()
    assert same(got_lost[:k], want_lost) and same(got_rows[:k], want_rows)
    assert (got_lost[k:] == -7.25).all() and (got_rows[k:] == -77).all()
    if k == 0:
        assert same(got, state.reshape(-1))                      # nobody lost: not a byte has moved
    # a second call on the result loses nobody and changes no byte, here or in the record
    if kept:
        assert apply(d, kept, shape, g["half"], g["centre"], lost=lost[:cap * 2 * dim], lost_row=rows[:cap]) == kept
        assert same(d.cpu().numpy(), got) and same(lost.cpu().numpy().reshape(-1, 2 * dim), got_lost) and same(rows.cpu().numpy(), got_rows)
        assert count(d, kept, shape, g["half"], g["centre"]) == 0
    # no record at all, and one output only
    if k:
        d2 = dev(state.reshape(-1))
        assert apply(d2, n, shape, g["half"], g["centre"]) == kept
        assert same(d2.cpu().numpy()[:3 * dim * kept], got[:3 * dim * kept])
        d3 = dev(state.reshape(-1))
        assert apply(d3, n, shape, g["half"], g["centre"], lost_row=rows[:cap]) == kept
        assert same(rows.cpu().numpy()[:k], want_rows) and same(d3.cpu().numpy()[:3 * dim * kept], got[:3 * dim * kept])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("shape", [AP.ELLIPSOID, AP.BOX], ids=["ellipsoid", "box"])
@pytest.mark.parametrize("dim", [3, 2])
def test_bytes_against_the_model(eng, dim, shape, n):
    for i, pattern in enumerate(PATTERNS):
        try:
            check_case(eng, dim, shape, n, pattern, seed=1000 * n + 10 * i + dim)
        except AssertionError as err:
            raise AssertionError("pattern %s: %s" % (pattern, err)) from err


@pytest.mark.parametrize("dim", [3, 2])
def test_three_levels_of_the_scan(eng, dim):
    check_case(eng, dim, AP.ELLIPSOID, THREE_LEVELS, "random", seed=dim)


@pytest.mark.parametrize("dim", [3, 2])
def test_open_axis_and_surface_points(eng, dim):
    """the hand-made points of test_aperture_host.py on the device: exactly on the surface, one ulp beyond, an open axis"""
    dtype = np.float32 if dim == 3 else np.float64
    count, _ = fns(eng, dim)
    half, centre = [2.0, 0.5, 4.0][:dim], [8.0, -2.0, 16.0][:dim]
    pts = []
    for a in range(dim):
        for sign in (-1.0, 1.0):
            on = np.array(centre, dtype=dtype)
            on[a] += sign * half[a]
            beyond = on.copy()
            beyond[a] = np.nextafter(beyond[a], dtype(sign * np.inf))
            pts += [on, beyond]
    e = np.float32(1.2 * 2.0 ** -27)
    pts = np.array(pts, dtype=dtype)
    for shape in (AP.ELLIPSOID, AP.BOX):
        want = AP.inside(pts, shape, half, centre)
        assert want.tolist() == [True, False] * (2 * dim)
        assert count(dev(pts.reshape(-1)), len(pts), shape, half, centre) == dim * 2
        for i in range(len(pts)):
            assert count(dev(pts[i]), 1, shape, half, centre) == int(not want[i]), (shape, i)
    if dim == 3:   # the summation order: (xx + yy) + zz
        p = np.array([[e, e, 1.0], [1.0, e, e]], dtype=np.float32)
        assert AP.inside(p, AP.ELLIPSOID, [1.0] * 3).tolist() == [False, True]
        assert [count(dev(p[i]), 1, AP.ELLIPSOID, [1.0] * 3) for i in range(2)] == [1, 0]
    big = dtype(1e30)
    z = [0.0] * (dim - 2)
    pipe = np.array([[0.0, big] + z, [0.0, -big] + z, [2.0, big] + z, [np.nextafter(dtype(2.0), dtype(3.0)), 0.0] + z,
                     [0.0, np.inf] + z, [0.0, np.nan] + z, [np.nan, 0.0] + z], dtype=dtype)
    open_half = [2.0, np.inf, 4.0][:dim]
    for shape in (AP.ELLIPSOID, AP.BOX):
        want = AP.inside(pipe, shape, open_half)
        assert want.tolist() == [True, True, True, False, False, False, False]
        for i in range(len(pipe)):
            assert count(dev(pipe[i]), 1, shape, open_half) == int(not want[i]), (shape, i)


@pytest.mark.parametrize("dim", [3, 2])
def test_refused_calls_leave_everything_untouched(eng, dim):
    import torch
    from coulomb_oscillators_amd.engine import Aperture
    lib, ctx = eng.lib, eng.ctx
    n = 300
    state, _ = make_state(dim, AP.ELLIPSOID, n, "random", 5)
    d = dev(state.reshape(-1))
    lost, rows = lost_buffers(dim, n)
    count_fn, apply_fn = (lib.nbco_aperture_count, lib.nbco_aperture_apply) if dim == 3 else (lib.nbco_2d_aperture_count, lib.nbco_2d_aperture_apply)
    P = lambda t: C.c_void_p(t.data_ptr())

    def ap(shape=0, centre=(0.0, 0.0, 0.0), half=(0.7, 0.5, 0.9)):
        return Aperture(shape, (C.c_double * 3)(*centre), (C.c_double * 3)(*half))

    good, out = ap(), C.c_longlong(-5)
    bad_aps = [ap(shape=2), ap(shape=-1), ap(centre=(np.nan, 0, 0)), ap(centre=(0, np.inf, 0)), ap(half=(np.nan, 0.5, 0.9)), ap(half=(0.7, 0.0, 0.9)),
               ap(half=(-0.7, 0.5, 0.9))]
    calls = [(None, P(d), n, C.byref(good), C.byref(out)), (ctx, None, n, C.byref(good), C.byref(out)), (ctx, P(d), n, None, C.byref(out)),
             (ctx, P(d), n, C.byref(good), None), (ctx, P(d), 0, C.byref(good), C.byref(out)), (ctx, P(d), -3, C.byref(good), C.byref(out))]
    calls += [(ctx, P(d), n, C.byref(b), C.byref(out)) for b in bad_aps]
    for args in calls:
        assert count_fn(*args) == ERR_ARG, args
        assert apply_fn(*args, P(lost), P(rows), n) == ERR_ARG, args
    assert apply_fn(ctx, P(d), n, C.byref(good), C.byref(out), P(lost), P(rows), -1) == ERR_ARG
    assert count_fn(ctx, P(d), 1 << 31, C.byref(good), C.byref(out)) == ERR_UNSUPPORTED
    assert apply_fn(ctx, P(d), 1 << 31, C.byref(good), C.byref(out), P(lost), P(rows), n) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert out.value == -5
    assert same(d.cpu().numpy(), state.reshape(-1)) and (lost == -7.25).all() and (rows == -77).all()
    if dim == 2:   # the third axis of the structure is not read by the 2-D calls
        odd = ap(centre=(0.0, 0.0, np.nan), half=(0.7, 0.5, -1.0))
        assert count_fn(ctx, P(d), n, C.byref(odd), C.byref(out)) == 0 and 0 < out.value < n


# ---- the context ---------------------------------------------------------------------------------------------------------------------
REF = dict(tree_steps=1, m2l_first=0)                    # the reference configuration (unsort = 1)
DRIVER = dict(tree_steps=8, m2l_first=1, unsort=0)       # what nbco3 runs
DT = float(np.float32(5e-4))


def test_a_call_that_loses_nobody_is_not_noticed(oracle32):
    """n = 4096, p = 4, the driver configuration: 20 nbco_integrate_steps with a no-loss call behind each give the final state and the
    sequence of kd_info.rebuilt of the run without the calls, bit for bit; nbco_energy_fmm right behind one returns the same bits"""
    import torch
    from coulomb_oscillators_amd import AP_ELLIPSOID, EVAL_FMM_KDTREE, INTEG_LEAPFROG, Engine
    n = 4096
    buf, par = oracle32.init_reference(n), oracle32.params(n)

    def run(with_calls):
        e = Engine(fmm_order=4, **DRIVER)
        try:
            d, prm = dev(buf.reshape(-1)), dev(par)
            e.compute_force(EVAL_FMM_KDTREE, d, n, prm)
            if with_calls:
                assert e.aperture(d, n, AP_ELLIPSOID, FAR) == n
            energy = e.energy_fmm(d, n, prm)
            rebuilt = []
            for _ in range(20):
                e.integrate_steps(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, DT, 2)
                if with_calls:
                    assert e.aperture(d, n, AP_ELLIPSOID, FAR) == n
                    assert e.aperture_count(d, n, AP_ELLIPSOID, FAR) == 0
                rebuilt.append(e.kd_info().rebuilt)
            e.compute_force(EVAL_FMM_KDTREE, d, n, prm)
            if with_calls:
                assert e.aperture(d, n, AP_ELLIPSOID, FAR) == n
            energy += e.energy_fmm(d, n, prm)
            return d.cpu().numpy(), rebuilt, np.array(energy)
        finally:
            e.close()

    s0, r0, e0 = run(False)
    s1, r1, e1 = run(True)
    assert 0 < sum(r0) < 20 and r0 == r1
    assert same(s0, s1) and same(e0, e1)


@pytest.mark.parametrize("config", [REF, DRIVER], ids=["reference", "driver"])
def test_a_lossy_call_leaves_a_context_as_good_as_new(oracle32, config):
    """the reference Gaussian at n = 4096 and the 2.5-rms ellipsoid, on a context with some history (6 evaluations: the rebuild
    schedule of the driver configuration is in mid-cycle): energy_fmm / probe_kd refuse right behind the call, and 8
    nbco_integrate_steps equal those of a fresh context that is given the compacted state"""
    import torch
    from coulomb_oscillators_amd import AP_ELLIPSOID, EVAL_FMM_KDTREE, INTEG_LEAPFROG, Engine, EngineError
    n = 4096
    buf, par = oracle32.init_reference(n), oracle32.params(n)
    old, new = Engine(fmm_order=4, **config), Engine(fmm_order=4, **config)
    try:
        d, prm = dev(buf.reshape(-1)), dev(par)
        old.compute_force(EVAL_FMM_KDTREE, d, n, prm)
        for _ in range(2):
            old.integrate_steps(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, DT, 2)
        old.compute_force(EVAL_FMM_KDTREE, d, n, prm)
        old.energy_fmm(d, n, prm)                                   # (valid here)
        kept = old.aperture(d, n, AP_ELLIPSOID, HALF)
        assert 0 < kept < n
        probe, psi = dev(np.zeros(3, dtype=np.float32)), torch.zeros(1, dtype=torch.float64, device="cuda")
        for call in (lambda: old.energy_fmm(d, kept, prm), lambda: old.energy_kd(d, kept, prm), lambda: old.probe_kd(probe, 1, prm, psi=psi)):
            with pytest.raises(EngineError) as err:
                call()
            assert err.value.status == ERR_ARG
        f = d[:9 * kept].clone()
        for _ in range(8):
            old.integrate_steps(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, kept, prm, DT, 2)
            new.integrate_steps(INTEG_LEAPFROG, EVAL_FMM_KDTREE, f, kept, prm, DT, 2)
            assert old.kd_info().rebuilt == new.kd_info().rebuilt
        assert same(d[:9 * kept].cpu().numpy(), f.cpu().numpy())
        old.compute_force(EVAL_FMM_KDTREE, d, kept, prm)
        new.compute_force(EVAL_FMM_KDTREE, f, kept, prm)
        assert same(np.array(old.energy_fmm(d, kept, prm)), np.array(new.energy_fmm(f, kept, prm)))
    finally:
        old.close()
        new.close()


def test_a_lossy_call_behind_the_direct_sum(oracle32):
    import torch
    from coulomb_oscillators_amd import AP_ELLIPSOID, EVAL_DIRECT, INTEG_LEAPFROG, Engine
    n = 4096
    buf, par = oracle32.init_reference(n), oracle32.params(n)
    old, new = Engine(), Engine()
    try:
        d, prm = dev(buf.reshape(-1)), dev(par)
        old.compute_force(EVAL_DIRECT, d, n, prm)
        kept = old.aperture(d, n, AP_ELLIPSOID, HALF)
        assert 0 < kept < n
        f = d[:9 * kept].clone()
        for _ in range(8):
            old.integrate_steps(INTEG_LEAPFROG, EVAL_DIRECT, d, kept, prm, DT, 1)
            new.integrate_steps(INTEG_LEAPFROG, EVAL_DIRECT, f, kept, prm, DT, 1)
        assert same(d[:9 * kept].cpu().numpy(), f.cpu().numpy())
    finally:
        old.close()
        new.close()


def test_a_lossy_call_behind_the_2d_fmm(oracle32):
    import torch
    from coulomb_oscillators_amd import AP_ELLIPSOID, EVAL2D_FMM, INTEG_LEAPFROG, Engine
    n = 4096
    ref = oracle32.init_reference(n)
    state = np.zeros((3, n, 2))
    state[:2] = ref[:2, :, :2]
    par = np.array([2e-6 / n, 0.0, 1.095 ** 2, 1.0])
    old, new = Engine(fmm_order=5), Engine(fmm_order=5)
    try:
        d, prm = dev(state.reshape(-1)), dev(par)
        old.compute_force_2d(EVAL2D_FMM, d, n, prm)
        kept = old.aperture_2d(d, n, AP_ELLIPSOID, HALF[:2])
        assert 0 < kept < n
        f = d[:6 * kept].clone()
        for _ in range(8):
            old.integrate_steps_2d(INTEG_LEAPFROG, EVAL2D_FMM, d, kept, prm, 5e-4, 1)
            new.integrate_steps_2d(INTEG_LEAPFROG, EVAL2D_FMM, f, kept, prm, 5e-4, 1)
        assert same(d[:6 * kept].cpu().numpy(), f.cpu().numpy())
    finally:
        old.close()
        new.close()


def test_order_tracking_follows_the_state(oracle32):
    """track_order = 1, unsort = 0 and nbco_fmm_kdtree only: positions are permuted and never moved.  Evaluate, lose, evaluate: row i
    of the state is particle order[i] of the first state, and the lost rows, through the order map as it was before the call, are
    exactly the particles of the first state that are outside"""
    import torch
    from coulomb_oscillators_amd import AP_ELLIPSOID, Engine
    n = 4096
    buf, par = oracle32.init_reference(n), oracle32.params(n)
    e = Engine(fmm_order=4, unsort=0, track_order=1)
    try:
        d, prm = dev(buf.reshape(-1)), dev(par)
        e.fmm_cart3_kdtree(d, d[6 * n:], n, prm)
        before = e.kd_array("order")
        assert same(d[:3 * n].cpu().numpy().reshape(n, 3), buf[0][before]) and not np.array_equal(before, np.arange(n))
        rows = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        kept = e.aperture(d, n, AP_ELLIPSOID, HALF, lost_row=rows)
        assert 0 < kept < n
        lost_rows = rows[:n - kept].cpu().numpy()
        outside = np.nonzero(~AP.inside(buf[0], AP.ELLIPSOID, HALF))[0]
        assert np.array_equal(np.sort(before[lost_rows]), outside)
        e.fmm_cart3_kdtree(d, d[6 * kept:], kept, prm)
        order = e.kd_array("order")
        assert order.shape == (kept,) and np.array_equal(np.sort(order), np.setdiff1d(np.arange(n), outside))
        assert same(d[:3 * kept].cpu().numpy().reshape(kept, 3), buf[0][order])
        assert same(d[3 * kept:6 * kept].cpu().numpy().reshape(kept, 3), buf[1][order])
    finally:
        e.close()
