"""The model of the collective modes (include/nbco.h: nbco_modes_record, nbco_mode_corr) that the tests hold the library to.

Records: r = t - rint(t) is formed in fp64 as the rule forms it (sk_numpy.reduced); a row counts iff its t and its three velocity floats
are finite.  From there on the model is long double: cos / sin of 2 pi (k . r), times v, summed.  Correlations: long double sums
straight from their definitions, Re[rho(t + tau) conj rho(t)], Re[j(t + tau) . conj j(t)], Re[P(t + tau) conj P(t)] with P = k . j, and
the sums of rho(t) and rho(t + tau).  None of the library's products is repeated here, so a wrong sign, conjugate, index, axis or a
dropped row shows as an error of order one, and rounding as one far below the bounds.

The bounds are derived, not tuned; u = 2^-53, H = hx + hy + hz:
  rho        sk_numpy.bound(n, h).
  j_c        u V_c (8 (H + 1) + 2 n + 2), V_c the sum of |v_c| over the counted rows: the phase error of the rho bound (8 (H + 1) u per
             term) times |v|, plus a chain of n fused multiply-adds in any order on each of the two components (n u V_c each; the
             modulus of the two is below twice one of them: 2 n), plus 2 for the rounding of the result.
  rr, jj     (m pairs + 2) u sum|products|, m = 2 and 6 fused multiply-adds per origin, in any order.
  s0, s1     pairs u sum|terms|, per component.
  ll         (2 pairs + 8) u sum_t M(t) M(t + tau), M = sum_c |k_c| (|Re j_c| + |Im j_c|) >= |P|: two fma per origin and the three
             roundings in each of P(t), P(t + tau) (6 u, and 2 u of slack)."""
import numpy as np

import sk_numpy as SK

L = SK.L
U = SK.U


def wave_vectors(h, kstep):
    """(K, 3) float64: k_c = (double) i_c * kstep_c at nbco_structure_factor's index"""
    h = [int(v) for v in h]
    ix = np.arange(0, h[0] + 1)
    iy = np.arange(-h[1], h[1] + 1)
    iz = np.arange(-h[2], h[2] + 1)
    g = np.stack(np.meshgrid(ix, iy, iz, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
    return g * np.array([float(kstep[0]), float(kstep[1]), float(kstep[2])], dtype=np.float64)[None, :]


def records(x, v, h, kstep, only=None, chunk=2048):
    """(rec, n_used, V): rec a long double array (K, 8) {rho.re, rho.im, jx.re, jx.im, ..} -- or over the flat indices `only` --, the
    number of rows that counted, and V[c] = sum |v_c| over them (float)"""
    h = [int(q) for q in h]
    x, v = np.asarray(x), np.asarray(v)
    r_t, used_t = SK.reduced(x, kstep)
    vfin = np.isfinite(v).all(axis=1)
    used = used_t & vfin
    r = r_t[vfin[used_t]].astype(L)
    vl = v[used].astype(L)
    idx = wave_vectors(h, (1.0, 1.0, 1.0)).astype(L)   # the integer indices
    if only is not None:
        idx = idx[only]
    K = len(idx)
    rec = np.zeros((K, 8), dtype=L)
    for j0 in range(0, len(r), chunk):
        b, vb = r[j0:j0 + chunk], vl[j0:j0 + chunk]
        cyc = idx @ b.T
        cyc -= np.rint(cyc)
        ang = SK.TWO_PI * cyc
        c, s = np.cos(ang), np.sin(ang)
        rec[:, 0] += c.sum(axis=1)
        rec[:, 1] += s.sum(axis=1)
        for a in range(3):
            rec[:, 2 + 2 * a] += c @ vb[:, a]
            rec[:, 3 + 2 * a] += s @ vb[:, a]
    return rec, int(used.sum()), [float(np.abs(vl[:, a]).sum()) for a in range(3)]


def record_errors(got, rec):
    """(rho error, [j_c errors]): the largest modulus over k of the complex differences; got float64 (K, 8)"""
    d = got.astype(L) - rec
    out = []
    for a in range(4):
        out.append(float(np.sqrt(d[:, 2 * a] ** 2 + d[:, 2 * a + 1] ** 2).max()))
    return out[0], out[1:]


def j_bound(n, h, V):
    return [U * V[c] * (8.0 * (sum(h) + 1) + 2.0 * n + 2.0) for c in range(3)]


def correlate(series, h, kstep, frames, lags=None, lag_list=None):
    """the model of nbco_mode_corr for the lags of lag_list (default 0 .. lags - 1): a dict of long double arrays (K, len(lag_list)) --
    rr, jj, ll, s0re, s0im, s1re, s1im -- and of the sums of absolute values that scale the bounds -- rr_abs, jj_abs, ll_abs, s0re_abs,
    .. -- and pairs (int64)"""
    ser = np.asarray(series)[:, :frames, :].astype(L)
    K = ser.shape[0]
    kv = wave_vectors(h, kstep).astype(L)
    if lag_list is None:
        lag_list = list(range(lags))
    names = ["rr", "jj", "ll", "s0re", "s0im", "s1re", "s1im"]
    out = {q: np.zeros((K, len(lag_list)), dtype=L) for q in names + [q + "_abs" for q in names]}
    out["pairs"] = np.array([frames - t for t in lag_list], dtype=np.int64)
    P = np.stack([(kv[:, None, :] * ser[:, :, 2::2]).sum(axis=2), (kv[:, None, :] * ser[:, :, 3::2]).sum(axis=2)], axis=-1)   # (K, frames, 2)
    M = (np.abs(kv)[:, None, :] * (np.abs(ser[:, :, 2::2]) + np.abs(ser[:, :, 3::2]))).sum(axis=2)
    for i, tau in enumerate(lag_list):
        a, b = ser[:, :frames - tau, :], ser[:, tau:frames, :]
        prod = a * b
        out["rr"][:, i] = prod[:, :, 0:2].sum(axis=(1, 2))
        out["rr_abs"][:, i] = np.abs(prod[:, :, 0:2]).sum(axis=(1, 2))
        out["jj"][:, i] = prod[:, :, 2:8].sum(axis=(1, 2))
        out["jj_abs"][:, i] = np.abs(prod[:, :, 2:8]).sum(axis=(1, 2))
        out["ll"][:, i] = (P[:, :frames - tau, :] * P[:, tau:frames, :]).sum(axis=(1, 2))
        out["ll_abs"][:, i] = (M[:, :frames - tau] * M[:, tau:frames]).sum(axis=1)
        for q, src, c in (("s0re", a, 0), ("s0im", a, 1), ("s1re", b, 0), ("s1im", b, 1)):
            out[q][:, i] = src[:, :, c].sum(axis=1)
            out[q + "_abs"][:, i] = np.abs(src[:, :, c]).sum(axis=1)
    return out


def corr_fractions(got, model):
    """the worst measured fraction of each bound: got a numpy array (K, len(lag_list)) of MODE_LAG records.  Returns a dict
    {rr, jj, ll, s}; a bound of zero asks for an error of zero (the fraction is then 0 or inf)"""
    pairs = model["pairs"].astype(np.float64)[None, :]
    assert (got["pairs"] == model["pairs"][None, :]).all()

    def frac(val, name, factor):
        err = np.abs(val.astype(L) - model[name]).astype(np.float64)
        lim = (factor * U * model[name + "_abs"]).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            f = np.where(lim > 0, err / lim, np.where(err > 0, np.inf, 0.0))
        return float(f.max())
    s = max(frac(got["s0"][..., 0], "s0re", pairs), frac(got["s0"][..., 1], "s0im", pairs),
            frac(got["s1"][..., 0], "s1re", pairs), frac(got["s1"][..., 1], "s1im", pairs))
    return {"rr": frac(got["rr"], "rr", 2 * pairs + 2), "jj": frac(got["jj"], "jj", 6 * pairs + 2),
            "ll": frac(got["ll"], "ll", 2 * pairs + 8), "s": s}


def propagated(series, E8, h, kstep, frames, lag_list):
    """what an error of at most E8[p] in component p of every record (series: the model's records, long double (K, frames, 8)) moves the
    correlation sums by: a product a b moves by at most |a| E + |b| E + E^2, P = k . j by at most E_P = sum_c |k_c| E_jc per component
    and rho's sums by pairs E.  Returns a dict rr, jj, ll, s of float64 arrays (K, len(lag_list)).  A program that correlates its own
    records is held to the model of the exact records within this plus the rounding bounds, the latter scaled by sum|products| plus
    this (the products of the program's records are that much larger at most)."""
    S = np.abs(np.asarray(series)[:, :frames, :]).astype(L)
    E8 = np.asarray(E8, dtype=np.float64).astype(L)
    kv = np.abs(wave_vectors(h, kstep)).astype(L)
    EP = (kv * E8[2::2][None, :]).sum(axis=1)                                      # (K,)
    Mre = (kv[:, None, :] * S[:, :, 2::2]).sum(axis=2)                             # (K, frames): >= |Re P|
    Mim = (kv[:, None, :] * S[:, :, 3::2]).sum(axis=2)
    out = {q: np.zeros((S.shape[0], len(lag_list))) for q in ("rr", "jj", "ll", "s")}
    for i, tau in enumerate(lag_list):
        a, b = S[:, :frames - tau, :], S[:, tau:frames, :]
        prop = (a + b) * E8[None, None, :] + (E8 * E8)[None, None, :]
        out["rr"][:, i] = prop[:, :, 0:2].sum(axis=(1, 2))
        out["jj"][:, i] = prop[:, :, 2:8].sum(axis=(1, 2))
        pairs = frames - tau
        out["ll"][:, i] = ((Mre[:, :pairs] + Mre[:, tau:frames] + Mim[:, :pairs] + Mim[:, tau:frames]) * EP[:, None]).sum(axis=1) + 2 * pairs * EP * EP
        out["s"][:, i] = pairs * float(E8[0])
    return out


def held_with_records(got, model, prop):
    """the worst fraction of (rounding bound scaled by sum|products| + prop) + prop over rr, jj, ll, s0, s1: got (K, lags) MODE_LAG"""
    pairs = model["pairs"].astype(np.float64)[None, :]
    assert (got["pairs"] == model["pairs"][None, :]).all()
    worst = 0.0

    def frac(val, name, factor, p):
        err = np.abs(val.astype(L) - model[name]).astype(np.float64)
        lim = factor * U * (model[name + "_abs"].astype(np.float64) + p) + p
        with np.errstate(divide="ignore", invalid="ignore"):
            return float(np.where(lim > 0, err / lim, np.where(err > 0, np.inf, 0.0)).max())
    worst = max(frac(got["rr"], "rr", 2 * pairs + 2, prop["rr"]), frac(got["jj"], "jj", 6 * pairs + 2, prop["jj"]),
                frac(got["ll"], "ll", 2 * pairs + 8, prop["ll"]),
                frac(got["s0"][..., 0], "s0re", pairs, prop["s"]), frac(got["s0"][..., 1], "s0im", pairs, prop["s"]),
                frac(got["s1"][..., 0], "s1re", pairs, prop["s"]), frac(got["s1"][..., 1], "s1im", pairs, prop["s"]))
    return worst


def random_series(K, cap, seed):
    """records with a static mean (a trapped cloud's form factor) and a fluctuating part, float64 (K, cap, 8)"""
    rng = np.random.default_rng(seed)
    mean = rng.standard_normal((K, 1, 8)) * np.array([40.0, 40.0, 3.0, 3.0, 3.0, 3.0, 3.0, 3.0])
    return np.ascontiguousarray(mean + rng.standard_normal((K, cap, 8)) * 5.0)
