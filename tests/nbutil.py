"""Shared helpers for the parity tests."""
import numpy as np


def force_err(a, ref):
    """max_i |a_i - ref_i| / (|ref_i| + mean_j |ref_j|).

    The per-particle relative error, regularised by the mean force magnitude so that particles
    near the trap centre (net force ~ 0 by cancellation) do not dominate.
    """
    a = np.asarray(a, dtype=np.float64).reshape(-1, 3)
    ref = np.asarray(ref, dtype=np.float64).reshape(-1, 3)
    mag = np.linalg.norm(ref, axis=1)
    return float((np.linalg.norm(a - ref, axis=1) / (mag + mag.mean() + 1e-300)).max())


def directed_pairs(mult, p2p, L):
    mult = np.asarray(mult, dtype=np.int64)
    leaves = mult[(1 << L) - 1:]
    return int((2 * mult[p2p[:, 0]] * mult[p2p[:, 1]]).sum() + (leaves ** 2).sum())


def canon_pairs(pairs):
    """Order-independent representation of an unordered pair list."""
    p = np.sort(np.asarray(pairs, dtype=np.int64).reshape(-1, 2), axis=1)
    keys = p[:, 0] * (1 << 32) + p[:, 1]
    return np.sort(keys)


def list_entries_changed(t0, t1):
    """number of P2P / M2L list entries (unordered node pairs) that are in one of two trees' lists and not in the other's"""
    return int(sum(len(np.setxor1d(canon_pairs(t0[k]), canon_pairs(t1[k]))) for k in ("p2p", "m2l")))


def leaf_pair_cover(t):
    """nleaf x nleaf matrix: how many times the interaction lists of the tree dict `t` (Oracle.kd_tree) serve each ordered pair of
    leaves.  A node pair of either list stands for all leaf pairs below it, in both directions; every leaf is served with itself
    once (the self P2P).  A correct dual traversal gives ones everywhere, whatever its admissibility rule."""
    L = int(t["L"])
    nleaf = 1 << L
    d = np.zeros((nleaf + 1, nleaf + 1), dtype=np.int64)

    def leaves_below(node):
        node = np.asarray(node, dtype=np.int64)
        lev = np.floor(np.log2(node + 1)).astype(np.int64)
        w = 1 << (L - lev)
        j = node + 1 - (1 << lev)
        return j * w, (j + 1) * w

    for key in ("p2p", "m2l"):
        pairs = np.asarray(t[key], dtype=np.int64).reshape(-1, 2)
        a0, a1 = leaves_below(pairs[:, 0])
        b0, b1 = leaves_below(pairs[:, 1])
        for r0, r1, c0, c1 in ((a0, a1, b0, b1), (b0, b1, a0, a1)):
            np.add.at(d, (r0, c0), 1)
            np.add.at(d, (r0, c1), -1)
            np.add.at(d, (r1, c0), -1)
            np.add.at(d, (r1, c1), 1)
    cover = d.cumsum(axis=0).cumsum(axis=1)[:nleaf, :nleaf]
    cover[np.arange(nleaf), np.arange(nleaf)] += 1
    return cover


def _powf(x, y):
    """the C library's powf, which the opening criterion is written with (numpy's float32 power may be a vector routine that rounds
    differently)"""
    import ctypes
    import ctypes.util
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]
    libm.powf.restype = ctypes.c_float
    return np.float32(libm.powf(float(np.float32(x)), float(np.float32(y))))


def kd_admissible_f32(t, pairs, p, par=1.0):
    """The opening criterion (fmm_cart3_kdtree.cuh:401-414) of the node pairs `pairs`, recomputed in float32 from the tree dict's
    center / lbound / rbound / mult, every product and sum rounded where the scalar code rounds it."""
    f = np.float32
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    n1, n2 = pairs[:, 0], pairs[:, 1]
    c, lb, rb = (np.asarray(t[k], dtype=f) for k in ("center", "lbound", "rbound"))
    mult = np.asarray(t["mult"], dtype=np.int64)

    def dot3(v):
        return (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]

    dist2 = dot3(c[n2] - c[n1])
    sz = np.maximum(dot3(rb[n1] - lb[n1]), dot3(rb[n2] - lb[n2]))
    big = np.maximum(mult[n1], mult[n2])
    expo = f(1) / f(3 * p + 6)
    tab = {int(m): _powf(f(m) / f(mult[0]), expo) for m in np.unique(big)}
    parm = f(par) * np.array([tab[int(m)] for m in big], dtype=f)
    return (parm * parm) * sz < dist2


NBCO_P2P_CHUNK = 16      # csrc/kd_list_kernels.hpp:67: entries of a target leaf's list per near-field work unit


def p2p_work_units(t, coll=True):
    """Work units of the near field of the tree dict `t` and the launch estimate for them, as (units, estimate(h_prev), longest target list).

    units: the sum over leaves of ceil(entries / NBCO_P2P_CHUNK), entries = the leaf's directed P2P entries plus its self entry.
    estimate: what k_fmm_kd.hip:498-501 derives from the PREVIOUS evaluation's list of h_prev leaf pairs for a tree of this one's
    nleaf leaves: (2 (h + h / 4 + 1024) + nleaf) / NBCO_P2P_CHUNK + nleaf in integer arithmetic (its min() with the list capacity
    is left out: the capacity is 48 x the node count and never binds on these inputs).  launch_p2p starts one wave per estimated
    unit; a wave takes a second unit only where units > estimate."""
    L = int(t["L"])
    nleaf, first = 1 << L, (1 << L) - 1
    pairs = np.asarray(t["p2p"], dtype=np.int64).reshape(-1, 2)
    assert (pairs >= first).all(), "the P2P list of a complete kd-tree holds leaf pairs only"
    entries = np.bincount((pairs - first).ravel(), minlength=nleaf) + (1 if coll else 0)
    units = int(((entries + NBCO_P2P_CHUNK - 1) // NBCO_P2P_CHUNK).sum())

    def estimate(h_prev):
        h = int(h_prev)
        return (2 * (h + h // 4 + 1024) + nleaf) // NBCO_P2P_CHUNK + nleaf

    return units, estimate, int(entries.max())


# ---- shared by the kd-driver and the long-lived-context modules -----------------------------------------------------------
def expansion_err(got, want, nodes=None):
    """largest deviation of a multipole / local array, relative to the largest component of its column over the whole tree;
    nodes: the rows looked at (default: all)"""
    scale = np.abs(want).max(axis=0, keepdims=True).clip(1e-30 if want.dtype == np.float32 else 1e-300)
    err = np.abs(got - want) / scale
    return float((err if nodes is None else err[nodes]).max())


def assert_same_tree(engine, want, n, perm):
    info = engine.kd_info()
    assert (info.L, info.ntot, info.n) == (want["L"], want["ntot"], n)
    for name in ("index", "mult", "splitdim", "lbound", "rbound", "center"):
        np.testing.assert_array_equal(engine.kd_array(name), want[name], err_msg=name)
    np.testing.assert_array_equal(engine.kd_array("unsort"), perm, err_msg="unsort")
    for name in ("p2p", "m2l"):
        np.testing.assert_array_equal(canon_pairs(engine.kd_array(name)), canon_pairs(want[name]), err_msg=name)
    assert info.directed_p2p == directed_pairs(want["mult"], want["p2p"], want["L"])


def drive_by_hand(eng, d, n, prm, dt, evals, force, on_eval=None):
    """Leapfrog as the reference's loop runs it (main3.cu:832-846 over integrator.cuh:68-80: force; then per step kick, drift,
    force, kick), spelled out so that the caller sees the state that enters every force evaluation."""
    for k in range(evals):
        if k:
            eng.step(d[1], d[2], dt / 2, n)
            eng.step(d[0], d[1], dt, n)
        x_in = d[:2].cpu().numpy() if on_eval else None
        force()
        if on_eval:
            on_eval(k, x_in)
        if k:
            eng.step(d[1], d[2], dt / 2, n)


def warm_engine(warm, **opts):
    """an Engine whose kd-tree build uses the warm median select (k_kdselect.hip) or never does: NBCO_SEL_WARM is read when the
    context is created, and is put back afterwards"""
    import os
    from coulomb_oscillators_amd import Engine
    old = os.environ.get("NBCO_SEL_WARM")
    os.environ["NBCO_SEL_WARM"] = "1" if warm else "0"
    try:
        return Engine(**opts)
    finally:
        if old is None:
            del os.environ["NBCO_SEL_WARM"]
        else:
            os.environ["NBCO_SEL_WARM"] = old
