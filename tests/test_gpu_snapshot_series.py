"""The series calls on ONE long-lived context: nbco_traj_record / nbco_time_corr and nbco_modes_record / nbco_mode_corr, which keep
caller-owned buffers across the snapshots of a run (host/nbco3.cpp -corr and -modes), beside the one-shot calls that
tests/test_gpu_snapshots.py holds.  The bars are that module's -- (M) the numpy model on what is read back from the device, (F) a
context created for the call alone returns the same bytes, (R) the run does not notice -- and so are its helpers.  No tolerance is
introduced here: (M) is test_gpu_time_corr's byte comparison with corr_numpy.scatter, corr_numpy.check against corr_numpy.model,
test_gpu_modes.hold (sk_numpy.bound and modes_numpy.j_bound against modes_numpy.records) and the bytes of nbco_mode_corr_ref.

Driver (a): the 3-D snapshot sequence of test_gpu_snapshots.run_snapshots_3d (its loop, options, apertures and compute_force points:
SeriesCalls rides it through `extra`).  Behind each snapshot's aperture: traj_record without ids -- the context's order map, which the
aperture has just compacted -- with rows = N0 // 3 + 1 and stride 3 into frame `snapshot`, and modes_record on (3, 2, 2) into frame
`snapshot` of a series of six; behind the last snapshot time_corr and mode_corr over the five frames, all lags.
Driver (b): on one context, time_corr over TC_SHAPES, then modes_record over MODE_SHAPES with a mode_corr on a random series of the same
grid behind each.

Where each scratch path of the library meets a smaller or differently cut user behind a larger one (the one-shot paths are walked in
tests/test_gpu_snapshots.py, this module's in the two drivers here):
  sk_part            run_size_walk_3d: structure_factor_2d and structure_factor alternate on it at every step, each with the grid of its
                     step (GRIDS_B2, GRIDS_B).  17 ranges of K = 2601 (step 0), then one range (step 1: nothing of it is written, the
                     result goes straight to the caller), then 40 ranges of K = 75 inside the bytes of step 0 (step 2), 9 ranges of two
                     chunks of ix (step 5), 40 ranges of K = 578 (step 6), at last 3 ranges of K = 1081665.  The snapshot sequences: the
                     same grid at a shrinking n, 16 ranges down to 8 (2-D: 15 down to 11).  preconditions_walk (tests/test_snapshots_host.py) holds the table.
  md_part            driver (b) here, MODE_SHAPES: 17 ranges of K = 405 records of eight doubles, one range, 40 ranges of K = 75, one,
                     9 ranges of five chunks of ix (17, 1, 1), 40 ranges of K = 578, one.  Driver (a): K = 100 at 16 ranges down to 8.
  tc_part            driver (b) here, TC_SHAPES: 257 ranges of 16 lags, 3 ranges of 300 lags, 257 of 65, one range (nothing of it is
                     written), 65 of 513, 257 of 64, 3 of 2048, one again -- lags x ranges records cut anew at every step, and every
                     lags-per-lane step 1, 2, 4, 8.  Driver (a): 512 ranges of 5 lags.
  c->part            bond_order (exact form) at every snapshot and walk step behind the records of beam_moments, slice_moments and
                     pair_hist of the same snapshot, and behind its own (n + 63) / 64 records of the snapshot or step before, which
                     were more: run_snapshots_3d, run_snapshots_2d (bond_order_2d) and both size walks.
  c->small, kBondOut the same calls: the bond summary is added up in c->small behind the beam moments' block at kBeamOut, written earlier
                     in every snapshot (CALLS3D / CALLS2D order: beam_moments .. bond_order).
  the child context  energy_tree, probe_tree, pair_hist_tree and now bond_order_tree share it in every snapshot of run_snapshots_3d
                     (n shrinking 7962 .. 3905) and at every step of run_size_walk_3d (8193, 300, 20000, 1, ..); hold() asserts the nb of
                     the tree form against the exact form's besides (F) and (M).
  the order map      driver (a) here: traj_record(ids=None) reads the map the aperture compacted (7962, 7960, 7385, 6078, 3905 entries
                     behind 8193), held byte for byte to corr_numpy.scatter with the map worked out on the host from the loss record,
                     and to a fresh context given that map as ids.

tests/test_gpu_checked.py runs both drivers on the checked build with poisoned allocations."""
import numpy as np
import pytest

import corr_numpy as CN
import modes_numpy as MN
import sk_numpy as SK
import test_gpu_modes as MD
import test_gpu_snapshots as T
import test_gpu_time_corr as TC

pytestmark = pytest.mark.gpu

ROWS, STRIDE = T.N0 // 3 + 1, 3
TRAJ_CAP = MODES_CAP = 6               # one frame more than there are snapshots: it keeps its poison
MODES_H = (3, 2, 2)
KSTEP = T.SK_KSTEP
MODEL_MAX = T.MODEL_MAX


def fresh_engine(fn, **opts):
    """fn(a context created for this call alone)"""
    from coulomb_oscillators_amd import Engine
    f = Engine(**opts)
    try:
        return fn(f)
    finally:
        f.close()


def corr_call(e, traj, rows, frames, lags):
    """one time_corr call into a poisoned buffer with room behind it: dict(cmp=(the lags x 8 doubles,))"""
    import torch
    out = torch.full((lags + 3, 8), TC.POISON, dtype=torch.float64, device="cuda")
    e.time_corr(traj, rows, frames, lags, out=out)
    torch.cuda.synchronize()
    raw = out.cpu().numpy()
    assert not (raw[:lags] == TC.POISON).any() and (raw[lags:] == TC.POISON).all()
    return dict(cmp=(np.ascontiguousarray(raw[:lags]),))


def mode_corr_call(e, series, h, kstep, frames, lags):
    """one mode_corr call into a poisoned buffer with room behind it (as test_gpu_modes.correlate): dict(cmp=(K x lags x 8 doubles,))"""
    import torch
    K = SK.count(h)
    out = torch.full((K * lags + 5, 8), MD.POISON, dtype=torch.float64, device="cuda")
    e.mode_corr(series, h, kstep, frames, lags, out=out)
    torch.cuda.synchronize()
    raw = out.cpu().numpy()
    assert (raw[K * lags:] == MD.POISON).all()
    return dict(cmp=(np.ascontiguousarray(raw[:K * lags]),))


def check_mode_corr(got, series_host, h, kstep, frames, lags, what):
    """bar (M) of mode_corr: the bytes of nbco_mode_corr_ref on the same series, and pairs = frames - lag"""
    from coulomb_oscillators_amd import MODE_LAG, mode_corr_ref
    rec = got["cmp"][0].view(MODE_LAG).reshape(SK.count(h), lags)
    assert (rec["pairs"] == (frames - np.arange(lags))[None, :]).all(), what
    assert rec.tobytes() == mode_corr_ref(series_host, h, kstep, frames, lags).tobytes(), what + ": not the bytes of the host rule"


# ---- (a) inside the 3-D snapshot sequence ---------------------------------------------------------------------------------------------
class SeriesCalls:
    """what rides run_snapshots_3d: the trajectory buffer and the mode series, poisoned once, and the bars at every snapshot"""

    def __init__(self):
        import torch
        self.traj = torch.full((ROWS, TRAJ_CAP, 6), TC.POISON, dtype=torch.float32, device="cuda")
        self.series = torch.full((SK.count(MODES_H), MODES_CAP, 8), MD.POISON, dtype=torch.float64, device="cuda")
        self.traj_host, self.series_host = self.traj.cpu().numpy(), self.series.cpu().numpy()
        self.frames = 0
        self.alive = np.ones(ROWS, dtype=bool)

    def snapshot(self, e, snap, view, n, order, what):
        import torch
        assert snap == self.frames and len(order) == n
        host = view.cpu().numpy().copy()
        e.traj_record(view, n, self.traj, snap, stride=STRIDE)                        # ids = None: the context's order map
        _, used = e.modes_record(view, n, MODES_H, KSTEP, series=self.series, frame=snap)
        torch.cuda.synchronize()
        assert np.array_equal(view.cpu().numpy(), host), what + ": a series call wrote the state"
        traj, series = self.traj.cpu().numpy(), self.series.cpu().numpy()
        # (M) the frame is the numpy scatter through the compacted map, byte for byte, and every other frame is as it was
        want = CN.scatter(host, n, order, ROWS, STRIDE)
        assert TC.same(traj[:, snap], want), what + ": traj_record against corr_numpy.scatter"
        self.traj_host[:, snap] = traj[:, snap]
        assert traj.tobytes() == self.traj_host.tobytes(), what + ": traj_record wrote another frame"
        here = np.isfinite(want).all(axis=1)
        assert not (here & ~self.alive).any() and here.sum() == (order % STRIDE == 0).sum(), what     # nobody comes back: lost rows stay NaN
        assert np.isnan(traj[~here, snap]).all(), what
        self.alive = here
        # (M) the mode records against the long double model of the state read back
        pos, vel = host[:3 * n].reshape(n, 3), host[3 * n:6 * n].reshape(n, 3)
        rec, want_used, V = T.model("modes", T.digest(host[:6 * n]) + repr((MODES_H, KSTEP)), lambda: MN.records(pos, vel, MODES_H, KSTEP))
        assert used == want_used == n, (what, used, want_used)
        MD.hold(series[:, snap], rec, n, MODES_H, V, what + ": modes_record")
        k0 = SK.index(MODES_H, 0, 0, 0)
        assert series[k0, snap, 0] == n and series[k0, snap, 1] == 0.0, what
        self.series_host[:, snap] = series[:, snap]
        assert series.tobytes() == self.series_host.tobytes(), what + ": modes_record wrote another frame"

        # (F) a fresh context, given the map as ids, writes the same frame; a fresh context writes the same mode frame
        def fresh(f):
            t2, s2 = torch.full_like(self.traj, TC.POISON), torch.full_like(self.series, MD.POISON)
            f.traj_record(view, n, t2, snap, stride=STRIDE, ids=T.dev(order.astype(np.int32)))
            _, u2 = f.modes_record(view, n, MODES_H, KSTEP, series=s2, frame=snap)
            torch.cuda.synchronize()
            return t2.cpu().numpy(), s2.cpu().numpy(), u2
        t2, s2, u2 = fresh_engine(fresh)
        assert TC.same(t2[:, snap], traj[:, snap]) and (np.delete(t2, snap, axis=1) == np.float32(TC.POISON)).all(), what + ": traj_record (F)"
        assert TC.same(s2[:, snap], series[:, snap]) and (np.delete(s2, snap, axis=1) == MD.POISON).all() and u2 == used, what + ": modes_record (F)"
        self.frames += 1

    def finish(self, e):
        """behind the last snapshot: both correlations over the frames recorded, all lags"""
        F = self.frames
        what = "behind snapshot %d" % F
        got = T.refusal(corr_call, e, self.traj, ROWS, F, F)
        assert got["cmp"][0] is not T.REFUSED, (what, got)
        frac = CN.check(got["cmp"][0], CN.model(self.traj_host, F, F), what + ": time_corr")
        print("%s: time_corr, worst fraction of the bound %.3g" % (what, frac))
        pairs = CN.records(got["cmp"][0])["pairs"]
        assert pairs[0] > pairs[F - 1] == self.alive.sum() > 0, (what, pairs)          # lost particles drop out of the later lags
        T.assert_same_result(got, fresh_engine(lambda f: corr_call(f, self.traj, ROWS, F, F)), what + ": time_corr")
        got = T.refusal(mode_corr_call, e, self.series, MODES_H, KSTEP, F, F)
        assert got["cmp"][0] is not T.REFUSED, (what, got)
        check_mode_corr(got, self.series_host, MODES_H, KSTEP, F, F, what + ": mode_corr")
        T.assert_same_result(got, fresh_engine(lambda f: mode_corr_call(f, self.series, MODES_H, KSTEP, F, F)), what + ": mode_corr")
        assert self.traj.cpu().numpy().tobytes() == self.traj_host.tobytes() and self.series.cpu().numpy().tobytes() == self.series_host.tobytes()


def drive_series_a(o):
    """the series calls inside run_snapshots_3d, (M) and (F) at every snapshot, and (R): the run with them is the run without them"""
    calls = SeriesCalls()
    with_calls = T.run_snapshots_3d(o, False, extra=calls)
    assert calls.frames == len(T.KS) and calls.alive.sum() < ROWS
    plain = T.run_snapshots_3d(o, False)
    T.assert_same_run(with_calls, plain, ("n", "info", "order", "lost", "rows", "state"))
    return with_calls


# ---- (b) a shape walk of the correlations on one context ------------------------------------------------------------------------------
TC_SHAPES = [(2049, 16, 16), (3, 300, 300), (1025, 130, 65), (1, 1, 1), (65, 600, 513), (2049, 64, 64), (3, 2048, 2048), (2, 70, 64)]   # (rows, frames, lags)
MODE_SHAPES = [(8193, (4, 4, 4)), (300, (2, 2, 2)), (20000, (2, 2, 2)), (1, (64, 0, 0)), (4097, (17, 1, 1)), (20000, (1, 8, 8)), (2, (0, 0, 0))]   # (n, h)
# (frames, lags) of the mode_corr behind each modes_record step: one lag per lane, pairs of lags in steps of 2 and of 4, the longest series
MODE_CORR_SHAPES = [(65, 65), (300, 129), (16, 16), (600, 513), (64, 64), (257, 257), (1024, 1024)]


def run_shape_walk():
    """Driver (b): one context over TC_SHAPES, then over MODE_SHAPES; every step to (F), and to (M) (the mode records where n <= 8193)"""
    from coulomb_oscillators_amd import Engine
    assert len(MODE_CORR_SHAPES) == len(MODE_SHAPES)
    live = Engine()
    fresh = {}
    worst = 0.0
    try:
        for step, (rows, frames, lags) in enumerate(TC_SHAPES):
            what = "time_corr walk step %d: rows %d frames %d lags %d" % (step, rows, frames, lags)
            cap = frames + 1 if frames < 2048 else frames
            traj = TC.dev(TC.case(rows, frames, cap))
            got = T.refusal(corr_call, live, traj, rows, frames, lags)
            assert got["cmp"][0] is not T.REFUSED, (what, got)
            key = ("tc", rows, frames, lags)
            if key not in fresh:
                fresh[key] = fresh_engine(lambda f: T.refusal(corr_call, f, traj, rows, frames, lags))
            T.assert_same_result(got, fresh[key], what)
            frac = CN.check(got["cmp"][0], TC.ref(rows, frames, cap, lags), what)
            worst = max(worst, frac)
            print("%s: worst fraction of the bound %.3g" % (what, frac))
        print("time_corr walk: worst fraction of the bound %.3g" % worst)
        for step, ((n, h), (frames, lags)) in enumerate(zip(MODE_SHAPES, MODE_CORR_SHAPES)):
            what = "modes walk step %d: n %d h %s" % (step, n, h)
            x, v = SK.cloud(n, 2000 + n), MD.velocities(n, 3000 + n)
            rec_got, used = MD.record(live, x, v, h, MD.K3)                      # frames_cap = 3, frame = 1; the other two keep their poison
            key = ("md", n, h)
            if key not in fresh:
                fresh[key] = fresh_engine(lambda f: MD.record(f, x, v, h, MD.K3))
            assert TC.same(rec_got, fresh[key][0]) and used == fresh[key][1] == n, what + ": modes_record (F)"
            if n <= MODEL_MAX:
                rec, want_used, V = MN.records(x, v, h, MD.K3)
                assert want_used == n
                MD.hold(rec_got, rec, n, h, V, what)
            k0 = SK.index(h, 0, 0, 0)
            assert rec_got[k0, 0] == n and rec_got[k0, 1] == 0.0 and (rec_got[k0, 3::2] == 0.0).all(), what
            what += ": mode_corr frames %d lags %d" % (frames, lags)
            series_host = MN.random_series(SK.count(h), frames + 1, 100 * frames + lags + sum(h))
            series_host[:, frames:, :] = np.nan                                    # beyond `frames`: never read
            series = T.dev(series_host)
            got = T.refusal(mode_corr_call, live, series, h, MD.K3, frames, lags)
            assert got["cmp"][0] is not T.REFUSED, (what, got)
            check_mode_corr(got, series_host, h, MD.K3, frames, lags, what)
            key = ("mc", h, frames, lags)
            if key not in fresh:
                fresh[key] = fresh_engine(lambda f: mode_corr_call(f, series, h, MD.K3, frames, lags))
            T.assert_same_result(got, fresh[key], what)
    finally:
        live.close()


# ---- the tests: one driver each ---------------------------------------------------------------------------------------------------------
def test_series_calls_inside_the_snapshot_sequence_3d(oracle32):
    drive_series_a(oracle32)


def test_shape_walk_of_the_correlations(engine_lib):
    run_shape_walk()
