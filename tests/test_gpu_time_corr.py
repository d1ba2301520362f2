"""nbco_traj_record and nbco_time_corr on the GPU against the long double model of tests/corr_numpy.py.

The bounds are derived, not tuned (corr_numpy): with u = 2^-53, dx2 and r4 within (pairs + 8) u of the model, relative; vv within
(pairs + 8) u times the sum of the |terms|; pairs integer for integer.  Every test prints the worst measured fraction of the bound.

The places the kernel can go wrong (time_corr_kernels.hpp), which the parity cases walk:
  * lags per lane: 1 up to 64 lags (lane = lag), then pairs (one lag from the bottom, one from the top): 2 up to 512 lags, 4 up to
    1024, 8 beyond -- the steps 64 | 65, 512 | 513, 1024 | 1025, and 2048;
  * lanes of a row W = 64, 128, 192, 256 by ceil(lags / 2): the steps 128 | 129, 256 | 257, 384 | 385;
  * rows in flight per workgroup S = min(256 / W, 2048 / frames): 4, 3 (frames = 600, lags <= 128), 2, 1 -- rows that are no
    multiple of S leave copies idle in the last round;
  * row ranges: at most 512, so from 512 S rows on a workgroup takes several rounds, and any two rows already give two ranges,
    whose records tc_reduce_kernel adds;
  * an odd number of lags (the top half is one shorter), lags = 1, 2 and frames, frames = 1, frames_cap > frames (the frames
    past `frames` hold finite garbage that must not be read)."""
import functools

import numpy as np
import pytest

import corr_numpy as CN

pytestmark = pytest.mark.gpu

ERR_ARG = 2
POISON = -123.456
WORST = {"fraction": 0.0}


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


def corr(e, traj, frames, lags, rows=None):
    """one call into a poisoned buffer: the records; every one must have been overwritten"""
    import torch
    out = torch.full((lags, 8), POISON, dtype=torch.float64, device="cuda")
    got = e.time_corr(dev(traj) if isinstance(traj, np.ndarray) else traj, traj.shape[0] if rows is None else rows, frames, lags, out=out)
    torch.cuda.synchronize()
    raw = got.cpu().numpy()
    assert raw.shape == (lags, 8) and not (raw == POISON).any()
    return CN.records(raw)


def walk(rows, frames, cap, seed, offset=0.0, step=0.05):
    """a random walk per row around `offset` with random velocities; the frames past `frames` are finite garbage"""
    rng = np.random.default_rng(seed)
    t = np.empty((rows, cap, 6), dtype=np.float32)
    t[..., :3] = (offset + rng.normal(0.0, 1.0, (rows, 1, 3)) * (step * 20) + np.cumsum(rng.normal(0.0, step, (rows, cap, 3)), axis=1)).astype(np.float32)
    t[..., 3:] = rng.normal(0.0, 1.0, (rows, cap, 3)).astype(np.float32)
    t[:, frames:] = rng.normal(0.0, 100.0, (rows, cap - frames, 6)).astype(np.float32)
    return t


@functools.lru_cache(maxsize=None)
def case(rows, frames, cap):
    t = walk(rows, frames, cap, 7 * rows + 13 * frames + cap)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def ref(rows, frames, cap, lags):
    return CN.model(case(rows, frames, cap), frames, lags)


def parity(e, t, frames, lags, model=None, what=""):
    got = corr(e, t, frames, lags)
    frac = CN.check(got, CN.model(t, frames, lags) if model is None else model, what)
    WORST["fraction"] = max(WORST["fraction"], frac)
    print("%s rows %d frames %d lags %d: worst fraction of the bound %.3g" % (what, t.shape[0], frames, lags, frac))
    return got


# ---- closed forms, exact ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames,lags", [(16, 16), (100, 70), (300, 300)])
def test_uniform_motion_on_a_dyadic_grid(eng, frames, lags):
    """x = x0 + v t with dyadic x0 and v: D = v tau exactly, dx2 = (v tau)^2 (frames - tau), r4 = |v tau|^4 (frames - tau),
    vv = v^2 (frames - tau), all of them integers times powers of two far below 2^53"""
    x0 = np.array([0.5, -1.25, 3.0])
    v = np.array([0.25, -0.5, 0.125])
    t = np.zeros((1, frames + 2, 6), dtype=np.float32)
    t[0, :, :3] = x0 + v * np.arange(frames + 2)[:, None]
    t[0, :, 3:] = v
    got = corr(eng, t, frames, lags)
    tau = np.arange(lags, dtype=np.float64)
    cnt = frames - tau
    assert np.array_equal(got["pairs"], cnt.astype(np.uint64))
    assert np.array_equal(got["dx2"], (v[None, :] * tau[:, None]) ** 2 * cnt[:, None])
    assert np.array_equal(got["r4"], ((v ** 2).sum() * tau ** 2) ** 2 * cnt)
    assert np.array_equal(got["vv"], (v ** 2)[None, :] * cnt[:, None])


def test_one_row_one_frame_one_lag(eng):
    t = np.array([[[1.5, -2.0, 0.25, 3.0, 0.0, -1.0]]], dtype=np.float32)
    got = corr(eng, t, 1, 1)
    assert got["pairs"][0] == 1 and not got["dx2"].any() and got["r4"][0] == 0
    assert np.array_equal(got["vv"][0], [9.0, 0.0, 1.0])
    t[0, 0, 3:] = 0
    got = corr(eng, t, 1, 1)
    assert got["pairs"][0] == 1 and got.tobytes()[:56] == bytes(56)


# ---- parity -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 2, 3, 4, 5, 63, 64, 65, 257, 1025, 2049])
def test_rows_around_the_rows_in_flight_and_the_ranges(eng, rows):
    """frames = 20, lags = 20: four rows in flight, 512 ranges from 2048 rows on, a second round at 2049"""
    parity(eng, case(rows, 20, 23), 20, 20, ref(rows, 20, 23, 20), "rows")


@pytest.mark.parametrize("frames", [1, 2, 63, 64, 65, 130, 257])
def test_frames_with_one_two_and_all_lags(eng, frames):
    for lags in sorted({1, min(2, frames), frames}):
        parity(eng, case(5, frames, frames + 3), frames, lags, ref(5, frames, frames + 3, lags), "frames")


@pytest.mark.parametrize("frames,lags", [(70, 64), (130, 65), (128, 128), (129, 129), (256, 256), (257, 257), (384, 384), (385, 385), (512, 512), (513, 513),
                                         (1024, 1024), (1025, 1025), (600, 64), (600, 128), (2048, 2), (2048, 130)])
def test_every_step_of_the_lags_per_lane_and_of_the_lanes_per_row(eng, frames, lags):
    parity(eng, case(7, frames, frames + 1), frames, lags, ref(7, frames, frames + 1, lags), "steps")


def test_2048_frames_of_three_rows(eng):
    parity(eng, case(3, 2048, 2048), 2048, 2048, ref(3, 2048, 2048, 2048), "longest")


def test_the_first_rows_of_a_larger_buffer(eng):
    """rows smaller than the buffer: the rows behind are not read (they hold other data)"""
    t = case(65, 20, 23)
    got = corr(eng, dev(t), 20, 20, rows=33)
    CN.check(got, CN.model(t[:33], 20, 20), "head")


# ---- rows that are not finite ---------------------------------------------------------------------------------------------------------
def test_frames_that_are_not_finite_count_for_nothing(eng):
    """a row NaN from frame 9 on (a lost particle), a gap in the middle, one infinite velocity, one NaN coordinate, a row never
    written; pairs equals the model and the sums stay within the bound"""
    t = walk(9, 40, 44, 5).copy()
    t[1, 9:] = np.nan
    t[2, 15:22] = np.nan
    t[3, 7, 4] = np.inf
    t[4, 30, 0] = np.nan
    t[5, 0, 5] = -np.inf
    t[6] = np.nan
    m = CN.model(t, 40, 40)
    assert m["pairs"][0] == 9 * 40 - (31 + 7 + 1 + 1 + 1 + 40) and m["pairs"][39] < 9
    parity(eng, t, 40, 40, m, "nonfinite")
    parity(eng, t, 40, 7, None, "nonfinite")


def test_a_buffer_of_nan_gives_zeros(eng):
    t = np.full((5, 70, 6), np.nan, dtype=np.float32)
    got = corr(eng, t, 70, 70)
    assert got.tobytes() == bytes(64 * 70)


# ---- a cloud far from the origin --------------------------------------------------------------------------------------------------
def test_small_displacements_far_from_the_origin(eng):
    """positions near 1000 that move by 1e-3 per frame: the differences are exact in double, and the bound holds as it stands"""
    t = walk(33, 100, 100, 11, offset=1000.0, step=1e-3)
    m = CN.model(t, 100, 100)
    assert 0 < float(m["dx2"][1].max()) < 1e-2 * 33 * 99
    parity(eng, t, 100, 100, m, "offset")


# ---- reproducibility and refusals -------------------------------------------------------------------------------------------------
def test_the_same_bytes_on_every_call_and_stream(eng):
    import torch
    from coulomb_oscillators_amd import Engine
    t = dev(case(257, 20, 23))
    u = dev(case(7, 513, 514))
    a, b = corr(eng, t, 20, 20), corr(eng, u, 513, 513)
    assert corr(eng, t, 20, 20).tobytes() == a.tobytes() and corr(eng, u, 513, 513).tobytes() == b.tobytes()
    s = torch.cuda.Stream()
    other = Engine(stream=s.cuda_stream)
    try:
        with torch.cuda.stream(s):
            assert corr(other, t, 20, 20).tobytes() == a.tobytes() and corr(other, u, 513, 513).tobytes() == b.tobytes()
    finally:
        other.close()


def test_refusals_leave_the_output_alone(eng):
    import torch
    t = dev(case(5, 20, 23))
    out = torch.full((20, 8), POISON, dtype=torch.float64, device="cuda")
    P = lambda x: None if x is None else x.data_ptr()
    for traj, rows, cap, frames, lags, o in ((None, 5, 23, 20, 20, out), (t, 5, 23, 20, 20, None), (t, 0, 23, 20, 20, out), (t, -1, 23, 20, 20, out),
                                             (t, 5, 23, 20, 0, out), (t, 5, 23, 20, 21, out), (t, 5, 23, 24, 20, out), (t, 5, 19, 20, 20, out),
                                             (t, 5, 4096, 2049, 20, out)):
        rc = eng.lib.nbco_time_corr(eng.ctx, P(traj), rows, cap, frames, lags, P(o))
        assert rc == ERR_ARG, (rows, cap, frames, lags)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == POISON).all()
    assert eng.lib.nbco_time_corr(None, P(t), 5, 23, 20, 20, P(out)) == ERR_ARG
    CN.check(corr(eng, t, 20, 20), ref(5, 20, 23, 20), "after refusals")


# ---- nbco_traj_record against a numpy scatter, bit for bit ------------------------------------------------------------------------
def state_of(n, seed):
    rng = np.random.default_rng(seed)
    s = rng.normal(0.0, 1.0, 9 * n).astype(np.float32)
    s[::7] = -0.0
    s[3::11] = np.float32(1e-42)      # a subnormal
    s[5::13] = np.inf
    return s


def record(e, state, n, rows, cap, frame, stride=1, ids=None):
    """one call into a poisoned trajectory buffer: the buffer as numpy"""
    import torch
    traj = torch.full((rows, cap, 6), POISON, dtype=torch.float32, device="cuda")
    e.traj_record(dev(state), n, traj, frame, stride=stride, ids=None if ids is None else dev(np.asarray(ids, dtype=np.int32)))
    torch.cuda.synchronize()
    return traj.cpu().numpy()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4097])
@pytest.mark.parametrize("stride", [1, 3])
def test_record_is_the_numpy_scatter(eng, n, stride):
    s = state_of(n, n)
    perm = np.random.default_rng(n + 1).permutation(n)
    full = (n + stride - 1) // stride
    for ids in (None, perm):
        for rows in sorted({full, max(1, full // 2), full + 5}):
            got = record(eng, s, n, rows, 4, 2, stride, ids)
            assert (got[:, [0, 1, 3]] == np.float32(POISON)).all()
            want = CN.scatter(s, n, ids, rows, stride)
            assert same(got[:, 2], want), (n, stride, rows, ids is None)
            if rows > full:
                assert np.isnan(got[full:, 2]).all()


def test_record_skips_ids_that_are_out_of_range(eng):
    n = 300
    s = state_of(n, 3)
    ids = np.arange(n) * 5 - 20          # negative numbers, numbers past the rows, numbers off the stride
    got = record(eng, s, n, 100, 1, 0, 2, ids)
    assert same(got[:, 0], CN.scatter(s, n, ids, 100, 2))


def test_record_refusals_leave_the_buffer_alone(eng):
    import torch
    n = 64
    st = dev(state_of(n, 1))
    traj = torch.full((n, 4, 6), POISON, dtype=torch.float32, device="cuda")
    P = lambda x: None if x is None else x.data_ptr()
    for buf, nn, tr, rows, cap, frame, stride in ((None, n, traj, n, 4, 0, 1), (st, n, None, n, 4, 0, 1), (st, 0, traj, n, 4, 0, 1), (st, n, traj, 0, 4, 0, 1),
                                                  (st, n, traj, n, 4, 0, 0), (st, n, traj, n, 4, -1, 1), (st, n, traj, n, 4, 4, 1)):
        assert eng.lib.nbco_traj_record(eng.ctx, P(buf), nn, None, P(tr), rows, cap, frame, stride) == ERR_ARG, (nn, rows, cap, frame, stride)
    torch.cuda.synchronize()
    assert (traj.cpu().numpy() == np.float32(POISON)).all()


# ---- live tracking ----------------------------------------------------------------------------------------------------------------
HALF = (0.0075, 0.0025, 0.025)         # 2.5 rms radii of the reference Gaussian
STEPS = 10


def drive(oracle32, tree_steps, recording, aperture_at=()):
    """n = 5001 (velocities and accelerations off the 16-byte grid) on one context with unsort = 0, track_order = 1: an evaluation,
    then STEPS leapfrog steps, a frame after each.  Returns state, kd_info log, order maps, the trajectory buffer and n per frame."""
    import torch
    from coulomb_oscillators_amd import AP_ELLIPSOID, EVAL_FMM_KDTREE, INTEG_LEAPFROG, Engine
    from coulomb_oscillators_amd.engine import KdInfo
    n = n0 = 5001
    e = Engine(fmm_order=4, unsort=0, tree_steps=tree_steps, track_order=1)
    try:
        d = dev(oracle32.init_reference(n).reshape(-1))
        prm = dev(oracle32.params(n))
        traj = torch.full((n0, STEPS + 1, 6), POISON, dtype=torch.float32, device="cuda")
        log, orders, states = [], [], []

        def look(frame, order):
            if recording:
                e.traj_record(d, n, traj, frame)
            info = e.kd_info()
            log.append(tuple(getattr(info, f[0]) for f in KdInfo._fields_))
            orders.append(order)
            states.append(d[:9 * n].cpu().numpy())
        e.compute_force(EVAL_FMM_KDTREE, d, n, prm)
        look(0, e.kd_array("order"))
        for k in range(1, STEPS + 1):
            e.integrate(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, 5e-4)
            order = e.kd_array("order")
            if k in aperture_at:
                # (the tree is dropped with the lost particles: the compacted map is worked out here, from the lost rows)
                rows = torch.full((n,), -1, dtype=torch.int32, device="cuda")
                kept = e.aperture(d, n, AP_ELLIPSOID, HALF, lost_row=rows)
                gone = np.zeros(n, dtype=bool)
                gone[rows[:n - kept].cpu().numpy()] = True
                order, n = order[~gone], kept
            look(k, order)
        torch.cuda.synchronize()
        return states, log, orders, traj.cpu().numpy()
    finally:
        e.close()


@pytest.mark.parametrize("tree_steps", [1, 8])
def test_frames_follow_the_order_map_and_the_run_does_not_notice(eng, oracle32, tree_steps):
    plain = drive(oracle32, tree_steps, False)
    rec = drive(oracle32, tree_steps, True)
    for a, b in zip(plain[0], rec[0]):
        assert same(a, b)                                  # positions, velocities and accelerations, every step
    assert plain[1] == rec[1]
    assert all(np.array_equal(a, b) for a, b in zip(plain[2], rec[2]))
    assert (plain[3] == np.float32(POISON)).all()
    n = 5001
    assert any(not np.array_equal(o, np.arange(n)) for o in rec[2])
    for f in range(STEPS + 1):
        assert same(rec[3][:, f], CN.scatter(rec[0][f], n, rec[2][f], n, 1)), f
    got = corr(eng, rec[3], STEPS + 1, STEPS + 1)
    frac = CN.check(got, CN.model(rec[3], STEPS + 1, STEPS + 1), "live")
    print("live tracking, tree_steps %d: worst fraction of the bound %.3g" % (tree_steps, frac))
    assert got["pairs"][0] == n * (STEPS + 1)


def test_particles_lost_to_an_aperture_stay_nan(eng, oracle32):
    states, log, orders, traj = drive(oracle32, 8, True, aperture_at=(3, 6))
    n0 = 5001
    counts = [len(o) for o in orders]
    assert counts[2] == n0 and counts[3] < n0 and counts[6] <= counts[3] and counts[-1] > 0
    alive = np.ones(n0, dtype=bool)
    for f in range(STEPS + 1):
        n = counts[f]
        assert same(traj[:, f], CN.scatter(states[f], n, orders[f], n0, 1)), f
        here = np.zeros(n0, dtype=bool)
        here[orders[f]] = True
        assert not (here & ~alive).any()                   # nobody comes back
        alive = here
        assert np.isnan(traj[~here, f]).all() and np.isfinite(traj[here, f]).all()
    m = CN.model(traj, STEPS + 1, STEPS + 1)
    assert m["pairs"][0] == sum(counts) and m["pairs"][STEPS] == counts[-1]
    got = corr(eng, traj, STEPS + 1, STEPS + 1)
    print("aperture: worst fraction of the bound %.3g" % CN.check(got, m, "aperture"))


def test_track_order_without_a_tracked_evaluation_is_refused(oracle32):
    import torch
    from coulomb_oscillators_amd import EVAL_FMM_KDTREE, Engine, EngineError
    n = 1000
    e = Engine(fmm_order=4, unsort=0, track_order=1)
    try:
        d = dev(oracle32.init_reference(n).reshape(-1))
        prm = dev(oracle32.params(n))
        traj = torch.full((n, 2, 6), POISON, dtype=torch.float32, device="cuda")
        with pytest.raises(EngineError) as err:
            e.traj_record(d, n, traj, 0)
        assert err.value.status == ERR_ARG
        torch.cuda.synchronize()
        assert (traj.cpu().numpy() == np.float32(POISON)).all()
        ids = np.arange(n, dtype=np.int32)[::-1]
        e.traj_record(d, n, traj, 0, ids=dev(ids))         # the caller's own numbers are accepted
        e.compute_force(EVAL_FMM_KDTREE, d, n, prm)
        with pytest.raises(EngineError):
            e.traj_record(d, n - 1, traj, 1)               # the map describes n particles, not n - 1
        e.traj_record(d, n, traj, 1)
        torch.cuda.synchronize()
        got = traj.cpu().numpy()
        s = d.cpu().numpy()
        assert same(got[:, 1], CN.scatter(s, n, e.kd_array("order"), n, 1))
    finally:
        e.close()


def test_zz_the_worst_fraction_of_the_bound(eng):
    print("nbco_time_corr: worst measured fraction of the bound over this module %.3g" % WORST["fraction"])
    assert WORST["fraction"] <= 1.0
