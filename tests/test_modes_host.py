"""The host side of the collective modes, no GPU: nbco_mode_corr_ref against the long double model of tests/modes_numpy.py within the
derived bounds (rr, jj: (m pairs + 2) u sum|products|; s0, s1: pairs u sum|terms|; ll: (2 pairs + 8) u sum M(t) M(t + tau)), a closed
form, nbco_mode_corr_derive bit for bit against the same expressions in numpy, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import modes_numpy as MN
import sk_numpy as SK

ERR_ARG = 2
K3 = (2.3, 3.1, 1.4)
GRIDS = [(0, 0, 0), (1, 1, 1), (2, 3, 1)]
SHAPES = sorted({(f, l) for f in (1, 2, 63, 64, 65, 257) for l in (1, f, min(f, 64))})


@pytest.mark.parametrize("h", GRIDS)
@pytest.mark.parametrize("frames,lags", SHAPES)
def test_ref_against_the_model(engine_lib, h, frames, lags):
    from coulomb_oscillators_amd import mode_corr_ref, MODE_LAG
    assert np.dtype(MODE_LAG).itemsize == 64
    K, cap = SK.count(h), frames + 3
    series = MN.random_series(K, cap, 100 * frames + lags + sum(h))
    series[:, frames:, :] = np.nan   # beyond `frames`: never read
    got = mode_corr_ref(series, h, K3, frames, lags)
    assert got.shape == (K, lags)
    assert (got["pairs"] == (frames - np.arange(lags))[None, :]).all()
    frac = MN.corr_fractions(got, MN.correlate(series, h, K3, frames, lags))
    print("h %s frames %d lags %d: worst fractions of the bounds %s" % (h, frames, lags, frac))
    assert max(frac.values()) <= 1.0


def test_one_free_particle_in_closed_form(engine_lib):
    """rho(t) = exp(i theta t), j = v rho, theta a multiple of 2 pi / 8: rr = pairs cos(theta tau), ll = (k . v)^2 rr"""
    from coulomb_oscillators_amd import mode_corr_ref
    h, frames, lags = (1, 1, 1), 40, 40
    K = SK.count(h)
    kv = MN.wave_vectors(h, K3)
    v = np.array([0.5, -1.25, 2.0])
    t = np.arange(frames)
    series = np.zeros((K, frames + 1, 8))
    r = np.sqrt(0.5)
    cos8 = np.array([1.0, r, 0.0, -r, -1.0, -r, 0.0, r])   # exact but for r, which is within u of 2^-1/2, relative
    sin8 = np.roll(cos8, 2)
    for k in range(K):
        c, s = cos8[(k % 8) * t % 8], sin8[(k % 8) * t % 8]
        series[k, :frames, 0], series[k, :frames, 1] = c, s
        for a in range(3):
            series[k, :frames, 2 + 2 * a], series[k, :frames, 3 + 2 * a] = v[a] * c, v[a] * s
    got = mode_corr_ref(series, h, K3, frames, lags)
    model = MN.correlate(series, h, K3, frames, lags)
    assert max(MN.corr_fractions(got, model).values()) <= 1.0
    tau = np.arange(lags)
    pairs = (frames - tau).astype(np.float64)
    A = lambda name, k: np.asarray(model[name][k], dtype=np.float64)
    for k in range(K):
        want = pairs * cos8[(k % 8) * tau % 8]
        # on top of the rule's bound, the series itself: a rho component is within u of the true one (2 u per product), a j component
        # within 2 u (v c is rounded: 4 u per product); v . v and k . v are fp64 sums of three products (8 u with what scales them)
        assert (np.abs(got["rr"][k] - want) <= (2 * pairs + 2 + 2 * pairs + 1) * MN.U * A("rr_abs", k)).all(), k
        assert (np.abs(got["jj"][k] - float(v @ v) * want) <= (6 * pairs + 2 + 4 * pairs + 8) * MN.U * A("jj_abs", k)).all(), k
        kdotv = float(kv[k] @ v)
        assert (np.abs(got["ll"][k] - kdotv * kdotv * want) <= (2 * pairs + 8 + 4 * pairs + 8) * MN.U * A("ll_abs", k)).all(), k


def test_derive_is_the_written_expressions(engine_lib):
    from coulomb_oscillators_amd import mode_corr_ref, mode_corr_derive, MODE_LAG
    h, frames, lags = (2, 3, 1), 65, 64
    K = SK.count(h)
    series = MN.random_series(K, frames, 5)
    rec = mode_corr_ref(series, h, K3, frames, lags)
    n_norm = 37.25
    out = mode_corr_derive(rec, h, K3, n_norm)
    assert out.shape == (K, lags, 4) and np.isfinite(out).all()
    kv = MN.wave_vectors(h, K3)
    k2 = ((kv[:, 0] * kv[:, 0] + kv[:, 1] * kv[:, 1]) + kv[:, 2] * kv[:, 2])[:, None]
    m = rec["pairs"].astype(np.float64)
    d = m * n_norm
    want = np.zeros((K, lags, 4))
    want[..., 0] = rec["rr"] / d
    want[..., 1] = (rec["rr"] - (rec["s1"][..., 0] * rec["s0"][..., 0] + rec["s1"][..., 1] * rec["s0"][..., 1]) / m) / d
    with np.errstate(divide="ignore", invalid="ignore"):
        want[..., 2] = np.where(k2 == 0.0, 0.0, rec["ll"] / (k2 * d))
        want[..., 3] = np.where(k2 == 0.0, 0.0, (rec["jj"] - rec["ll"] / k2) / (2.0 * d))
    assert out.tobytes() == want.tobytes()
    k0 = SK.index(h, 0, 0, 0)
    assert not out[k0, :, 2:].any() and out[k0, :, :2].any()            # k = 0: no direction to project on
    # a float64 view of the records is taken as well
    assert np.array_equal(mode_corr_derive(rec.view(np.float64).reshape(K, lags, 8), h, K3, n_norm), out)
    # no pairs, and no particles: zeros whatever the sums hold
    empty = rec.copy()
    empty["pairs"][:, ::2] = 0
    o2 = mode_corr_derive(empty, h, K3, n_norm)
    assert not o2[:, ::2].any() and np.array_equal(o2[:, 1::2], out[:, 1::2])
    for n0 in (0.0, -1.0):
        assert not mode_corr_derive(rec, h, K3, n0).any()


def _grid(h, kstep):
    from coulomb_oscillators_amd.engine import SkGrid
    g = SkGrid()
    for a in range(3):
        g.h[a], g.kstep[a] = h[a], kstep[a]
    return g


def test_refusals(engine_lib):
    from coulomb_oscillators_amd.engine import _load
    lib = _load()
    h, cap = (1, 1, 1), 8
    K = SK.count(h)
    series = MN.random_series(K, cap, 1)
    out = np.full((K, 8, 8), -7.0)
    P = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None

    def ref(s=series, g=_grid(h, K3), cap=cap, frames=8, lags=8, o=out):
        return lib.nbco_mode_corr_ref(P(s), C.byref(g) if g is not None else None, cap, frames, lags, P(o))
    bad = [dict(s=None), dict(g=None), dict(o=None), dict(lags=0), dict(lags=-1), dict(lags=9, frames=8), dict(frames=9), dict(frames=0, lags=0),
           dict(cap=1025 + 1, frames=1025, lags=1)]
    for a in range(3):
        for q in (-1, 65):
            bad.append(dict(g=_grid(tuple(q if b == a else h[b] for b in range(3)), K3)))
        for q in (0.0, -1.0, float("inf"), float("nan")):
            bad.append(dict(g=_grid(h, tuple(q if b == a else K3[b] for b in range(3)))))
    for kw in bad:
        assert ref(**kw) == ERR_ARG, kw
    assert (out == -7.0).all()
    assert ref() == 0 and (out != -7.0).all()

    rec, der = np.zeros((K, 2, 8)), np.full((K, 2, 4), -7.0)

    def derive(i=rec, g=_grid(h, K3), lags=2, o=der):
        return lib.nbco_mode_corr_derive(P(i), C.byref(g) if g is not None else None, lags, 1.0, P(o))
    for kw in (dict(i=None), dict(g=None), dict(o=None), dict(lags=-1), dict(g=_grid((1, 65, 1), K3)), dict(g=_grid((-1, 1, 1), K3))):
        assert derive(**kw) == ERR_ARG, kw
    assert (der == -7.0).all()
    assert derive(lags=0) == 0 and (der == -7.0).all()
    assert derive() == 0 and not der.any()
