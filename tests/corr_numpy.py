"""The numpy model of nbco_time_corr (include/nbco.h), in long double: the terms are formed by the rule of csrc/time_corr.hpp -- every
float widened, D_c one float64 subtraction (the rule's one rounding), then the squares, r2^2 and the velocity products exactly as the
rule's fused operations see them, which long double holds to 2^-64 -- and summed in long double.  Besides the sums it returns the sum
of the |terms| of vv, which the bound of vv is stated in.

The bounds (recursive summation of `pairs` terms in any order, one rounding per fused addition, plus the three roundings of r2 and
their doubling in r2^2), with u = 2^-53:
    dx2, r4:  |got - model| <= (pairs + 8) u model
    vv:       |got - model| <= (pairs + 8) u sum |term|
and pairs integer for integer.  check() asserts them and returns the worst measured fraction of the bound."""
import numpy as np

U = 2.0 ** -53
LAG = np.dtype([("dx2", "<f8", (3,)), ("r4", "<f8"), ("vv", "<f8", (3,)), ("pairs", "<u8")])   # nbco_corr_lag
assert LAG.itemsize == 64


def model(traj, frames, lags):
    """traj: float32 [rows, frames_cap, 6].  Returns dict(pairs uint64 [lags], dx2 [lags, 3], r4 [lags], vv [lags, 3], vv_abs [lags, 3]),
    the sums in long double."""
    traj = np.asarray(traj, dtype=np.float32)
    assert traj.ndim == 3 and traj.shape[2] == 6 and 1 <= lags <= frames <= traj.shape[1]
    t = traj[:, :frames]
    fin = np.isfinite(t).all(axis=2)
    x = np.where(fin[..., None], t[..., :3], np.float32(0)).astype(np.float64)
    v = np.where(fin[..., None], t[..., 3:], np.float32(0)).astype(np.longdouble)
    L = np.longdouble
    out = dict(pairs=np.zeros(lags, np.uint64), dx2=np.zeros((lags, 3), L), r4=np.zeros(lags, L), vv=np.zeros((lags, 3), L), vv_abs=np.zeros((lags, 3), L))
    for tau in range(lags):
        m = frames - tau
        ok = fin[:, :m] & fin[:, tau:frames]
        d = (x[:, tau:frames] - x[:, :m]).astype(L)          # float64 subtraction: the rule's rounding
        d2 = np.where(ok[..., None], d * d, L(0))
        r2 = (d2[..., 0] + d2[..., 1]) + d2[..., 2]
        w = np.where(ok[..., None], v[:, :m] * v[:, tau:frames], L(0))
        out["pairs"][tau] = int(ok.sum())
        out["dx2"][tau] = d2.reshape(-1, 3).sum(axis=0)
        out["r4"][tau] = (r2 * r2).sum()
        out["vv"][tau] = w.reshape(-1, 3).sum(axis=0)
        out["vv_abs"][tau] = np.abs(w).reshape(-1, 3).sum(axis=0)
    return out


def records(raw):
    """the nbco_corr_lag records in a buffer: a numpy array of any dtype holding lags x 64 bytes"""
    return np.ascontiguousarray(raw).view(np.uint8).reshape(-1).view(LAG)


def check(got, ref, what=""):
    """got: LAG records; ref: model().  Asserts pairs and the bounds; returns the worst |got - model| / bound (0 where both are 0)."""
    got = records(got)
    lags = len(ref["pairs"])
    assert len(got) == lags, (what, len(got), lags)
    assert np.array_equal(got["pairs"], ref["pairs"]), (what, "pairs", got["pairs"][:8], ref["pairs"][:8])
    worst = 0.0
    L = np.longdouble
    for tau in range(lags):
        k = L(int(ref["pairs"][tau]) + 8) * L(U)
        items = [("dx2[%d]" % c, got["dx2"][tau, c], ref["dx2"][tau, c], ref["dx2"][tau, c]) for c in range(3)]
        items.append(("r4", got["r4"][tau], ref["r4"][tau], ref["r4"][tau]))
        items += [("vv[%d]" % c, got["vv"][tau, c], ref["vv"][tau, c], ref["vv_abs"][tau, c]) for c in range(3)]
        for name, g, r, scale in items:
            assert np.isfinite(g), (what, tau, name, g)
            err, bound = abs(L(g) - r), k * scale
            assert err <= bound, (what, "lag", tau, name, float(g), float(r), float(err), float(bound))
            if bound > 0:
                worst = max(worst, float(err / bound))
    return worst


def scatter(state, n, ids, rows, stride):
    """the frame nbco_traj_record writes: float32 [rows, 6], NaN where nobody writes.  state: float32 flat [pos n | vel n ..];
    ids: the particle number of every state row (None: the row)."""
    state = np.asarray(state, dtype=np.float32).reshape(-1)
    pos, vel = state[:3 * n].reshape(n, 3), state[3 * n:6 * n].reshape(n, 3)
    p = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    out = np.full((rows, 6), np.nan, dtype=np.float32)
    sel = (p >= 0) & (p % stride == 0) & (p // stride < rows)
    out[p[sel] // stride, :3] = pos[sel]
    out[p[sel] // stride, 3:] = vel[sel]
    return out
