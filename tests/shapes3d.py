"""Inputs of the 3-D shape tests (test_shapes3d_host.py, test_gpu_shapes3d.py): the states a run reaches late and the states users
feed in -- flat, collinear, tied, duplicated, stretched -- built from the reference's Gaussian ball so that every one of them has
the ball's particle count, velocities and length scale.  Pure numpy on top of Oracle.init_reference; all arithmetic in float32.

CASES lists (evaluator, shape, n, p, what).  what = "forces": both oracles are finite on the input and agree on the tree, so the
accelerations of a GPU evaluation are compared with them.  what = "lists": the reference's forces mean nothing on the input (fp32
cancellation, lists that differ between fp32 and fp64, NaN in both precisions); only the tree / keys / lists are compared.
test_shapes3d_host.py asserts, without a GPU, that every case is what this table says it is."""
import numpy as np

SHAPES = ("gauss", "plane", "plane_off", "line", "lattice", "quant16", "dup2", "dup8", "dup16", "dup64", "late", "two_clumps", "offset")
DRAWS = ("lattice", "dup2", "dup8", "dup16", "dup64")      # the shapes that take a permutation, in the order they draw it
LATE_ROWS = np.array([[40.0, 0, 0], [0, -55.0, 0], [0, 0, 70.0]], dtype=np.float32)


def lattice_side(n):
    m = int(round(n ** (1.0 / 3.0)))
    assert m ** 3 == n, "a lattice needs n = m^3"
    return m


def state(oracle32, name, n):
    """the (3, n, 3) float32 buffer [pos | vel | acc = 0] of shape `name`; velocities are the Gaussian ball's"""
    f = np.float32
    assert name in SHAPES, name
    buf = oracle32.init_reference(n).copy()
    pos = buf[0]
    R = f(np.abs(pos).max())
    # one generator per call, every permutation drawn in the order of DRAWS: a shape's rows do not depend on which shapes were
    # asked for before it
    rng = np.random.default_rng(7)
    perm = {k: rng.permutation(n) for k in DRAWS}
    if name == "plane":
        pos[:, 2] = 0
    elif name == "plane_off":
        pos[:, 2] = f(0.37) * R
    elif name == "line":
        pos[:, 1:] = 0
    elif name == "lattice":
        m = lattice_side(n)
        g = np.indices((m, m, m)).reshape(3, -1).T.astype(f)
        pos[:] = (((g / f(m)) - f(0.5)) * R)[perm["lattice"]]
    elif name == "quant16":
        pos[:] = np.round(pos / R * f(16)) / f(16) * R
    elif name.startswith("dup"):
        K = int(name[3:])
        pos[:] = np.repeat(pos[:n // K], K, axis=0)[perm[name]]
    elif name == "late":
        pos[:3] = LATE_ROWS * R
    elif name == "two_clumps":
        pos[:n // 2, 0] += f(1000) * R
    elif name == "offset":
        pos += f(300) * R
    assert buf.dtype == f and pos.dtype == f
    return buf


def kd_cases():
    F, T = "forces", "lists"
    rows = [
        ("gauss", 4096, 4, F), ("gauss", 8000, 6, F),
        ("plane", 4096, 4, F), ("plane", 8000, 6, F), ("plane", 4096, 10, F),
        ("plane_off", 4096, 4, F), ("plane_off", 8000, 6, F),
        ("line", 4096, 4, F), ("line", 8000, 6, F), ("line", 4096, 10, T),       # fp32 leaves its range on a line at p = 10
        ("lattice", 4096, 4, F), ("lattice", 2197, 4, T), ("lattice", 8000, 6, T),
        ("quant16", 4096, 10, F), ("quant16", 4096, 4, T), ("quant16", 8000, 6, T),
        ("dup2", 4096, 4, F), ("dup2", 8000, 6, F),
        ("dup8", 4096, 4, F), ("dup8", 8000, 6, F),
        ("dup16", 4096, 4, F), ("dup64", 4096, 4, T),
        ("late", 4096, 4, F), ("late", 8000, 6, F), ("late", 4096, 10, F),
        ("two_clumps", 8000, 6, T), ("offset", 4096, 4, T), ("offset", 8000, 6, T),
    ]
    return [("kd",) + r for r in rows]


def oct_cases():
    F, T = "forces", "lists"
    traceless = [
        ("gauss", 4096, 4, F), ("plane", 8000, 6, F), ("plane", 4096, 10, F), ("plane_off", 4096, 4, F),
        ("line", 8000, 6, F), ("line", 4096, 10, F), ("lattice", 4096, 4, F), ("quant16", 8000, 6, F),
        ("dup2", 4096, 4, F), ("dup8", 8000, 6, F), ("dup16", 4096, 4, F), ("dup64", 4096, 4, F),
        ("late", 4096, 4, F), ("late", 8000, 6, F), ("late", 4096, 10, F),
        ("two_clumps", 4096, 10, F), ("offset", 4096, 4, T),
    ]
    symmetric = [
        ("gauss", 4096, 4, F), ("plane", 8000, 6, F), ("plane_off", 8000, 6, F), ("line", 4096, 4, F),
        ("lattice", 4096, 4, F), ("quant16", 4096, 4, F), ("dup2", 8000, 6, F), ("dup8", 4096, 4, F),
        ("dup16", 8000, 6, F), ("late", 4096, 4, F), ("late", 8000, 6, F), ("late", 4096, 10, F),
        ("two_clumps", 4096, 10, F), ("offset", 8000, 6, T),
    ]
    return [("traceless",) + r for r in traceless] + [("symmetric",) + r for r in symmetric]


CASES = kd_cases() + oct_cases()

# octree "forces" cases on which the fp32 oracle overflows (a stretched tree: few occupied cells far apart, r^-(p+1) (2p-1)!! out
# of the fp32 range) while the fp64 oracle is finite.  There the GPU runs with far_fp64 = 1 and is compared with the fp64 oracle
# alone.  The host module asserts that exactly these cases overflow.
OCT_FP32_OVERFLOWS = {
    ("traceless", "plane", 4096, 10), ("traceless", "line", 4096, 10), ("traceless", "late", 8000, 6), ("traceless", "late", 4096, 10),
    ("traceless", "two_clumps", 4096, 10),
    ("symmetric", "late", 8000, 6), ("symmetric", "late", 4096, 10), ("symmetric", "two_clumps", 4096, 10),
}

LONG_RANGE = dict(n=65536, p=3, radius=2.0)       # the late-run state of test_long_ranges_take_their_own_kernel_when_the_lists_are_long
FLOOR_CASE_OF_LONG_RANGE = ("kd", "late", 8000, 6)


def case_id(case):
    return "%s-%s-%d-p%d-%s" % case


def order_of(case):
    """the order a case runs at: the symmetric evaluator has generated operators up to order 9"""
    ev, _, _, p, _ = case
    return min(p, 9) if ev == "symmetric" else p


def force_bound(floor):
    """how far an fp32 evaluation may be from the fp32 oracle: the project's bar, or four times the distance between the two oracles
    where that is larger (two fp32 summation orders, each about one floor from fp64, doubled because the floor is the maximum over
    a few thousand particles of one draw)"""
    return max(1e-5, 4.0 * floor)


def per_target_entries(tree):
    """entries of every leaf's P2P list, the self entry included"""
    L = int(tree["L"])
    pairs = np.asarray(tree["p2p"], dtype=np.int64).reshape(-1, 2)
    return np.bincount(pairs.ravel() - ((1 << L) - 1), minlength=1 << L) + 1


# why a "lists" case is not a "forces" case (the host module asserts each):
#   nonfinite32    the fp32 oracle's accelerations are not finite, the fp64 oracle's are
#   nonfinite      neither oracle's accelerations are finite
#   lists_differ   the fp32 and fp64 oracles walk different trees or write different lists: their forces differ by truncation
#   cancellation   the lists agree, but the two oracles are more than 5e-5 apart: fp32 rounding of coordinates far from the origin
LISTS_WHY = {
    ("kd", "line", 4096, 10): "nonfinite32", ("kd", "dup64", 4096, 4): "nonfinite",
    ("kd", "lattice", 2197, 4): "lists_differ", ("kd", "lattice", 8000, 6): "lists_differ",
    ("kd", "quant16", 4096, 4): "lists_differ", ("kd", "quant16", 8000, 6): "lists_differ",
    ("kd", "two_clumps", 8000, 6): "lists_differ", ("kd", "offset", 4096, 4): "lists_differ", ("kd", "offset", 8000, 6): "lists_differ",
    ("traceless", "offset", 4096, 4): "cancellation", ("symmetric", "offset", 8000, 6): "cancellation",
}

# octree shapes whose far field is below the force bound: a line's force is its neighbours' (spacing 1e-6 of the length), and three
# far particles (or a second clump) stretch the grid until the ball is one cell.  The accelerations there test the near field and
# the number range of the far field; the far field itself is compared through the locals of the occupied cells.
OCT_NEAR_FIELD_ONLY = ("line", "late", "two_clumps")

THREADS = 8
_cache = {}


def evaluate(oracle32, oracle64, case):
    """both oracles on one case, once per process: dict of buf, par, and per precision (32 / 64) the accelerations a, the state pv
    (octree: cell order), the tree dict t (kd-tree: with mpole / local and the unsort map `perm`; octree: with centre / mpole / local
    under "ex"), plus finite32 / finite64 and floor = force_err(a32, a64) (nan where either is not finite).  Nothing in it is to be
    modified."""
    from nbutil import force_err
    if case in _cache:
        return _cache[case]
    ev, shape, n, _, _ = case
    p = order_of(case)
    buf = state(oracle32, shape, n)
    par = oracle32.params(n)
    r = {"buf": buf, "par": par, "p": p}
    for tag, o in ((32, oracle32), (64, oracle64)):
        a, pv, t = run_oracle(o, ev, buf, par, p)
        r["a%d" % tag], r["pv%d" % tag], r["t%d" % tag] = a, pv, t
        r["finite%d" % tag] = bool(np.isfinite(a).all())
    r["floor"] = force_err(r["a32"], r["a64"]) if r["finite32"] and r["finite64"] else float("nan")
    _cache[case] = r
    return r


def run_oracle(o, ev, buf, par, p, expansions=True, **kw):
    """(a, pv, tree) of one oracle evaluation; kd-tree: accelerations in the caller's order (unsort) unless kw says otherwise"""
    real = o.dtype
    pv_in, par = buf[:2].astype(real), par.astype(real)
    if ev == "kd":
        kw.setdefault("unsort", True)
        pv, a = o.fmm_kd(pv_in, par, p=p, threads=THREADS, **kw)
        t = o.kd_tree(offM=p * (p + 1) * (p + 2) // 6, offL=(p + 1) ** 2) if expansions else o.kd_tree()
        t["perm"] = o.kd_unsort(buf.shape[1])
    else:
        sym = ev == "symmetric"
        pv, a = (o.fmm_oct_symmetric if sym else o.fmm_oct_traceless)(pv_in, par, p=p, threads=THREADS, **kw)
        t = o.oct_tree(buf.shape[1])
        if expansions:
            t["ex"] = o.oct_expansions(p, symmetric=sym)
    return a, pv, t


def same_kd_tree(t0, t1):
    return all(np.array_equal(t0[k], t1[k]) for k in ("index", "mult", "splitdim", "perm"))


def same_kd_lists(t0, t1):
    from nbutil import canon_pairs
    return all(np.array_equal(canon_pairs(t0[k]), canon_pairs(t1[k])) for k in ("p2p", "m2l"))


def long_range_oracle(oracle32, again=False):
    """the 65536-particle late state of the long-range tests under the fp32 oracle, in tree order (unsort = 0), once per process:
    (buf, par, pv, a, tree).  again: the evaluation of the state the first one left behind -- what the second force evaluation of a
    context with tree_steps = 1 is given."""
    key = ("long_range", again)
    if key not in _cache:
        n, p, radius = LONG_RANGE["n"], LONG_RANGE["p"], LONG_RANGE["radius"]
        if again:
            buf = long_range_oracle(oracle32)[0].copy()
            buf[:2] = long_range_oracle(oracle32)[2]
        else:
            buf = state(oracle32, "late", n)
        par = oracle32.params(n)
        a, pv, t = run_oracle(oracle32, "kd", buf, par, p, expansions=False, unsort=False, radius=radius)
        _cache[key] = (buf, par, pv, a, t)
    return _cache[key]


def column_errs(got, want):
    """nbutil.expansion_err column by column: the largest deviation of each column, relative to the column's largest entry in `want`"""
    want = np.asarray(want)
    scale = np.abs(want).max(axis=0).clip(1e-30 if want.dtype == np.float32 else 1e-300)
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.abs(np.asarray(got, dtype=np.float64) - want) / scale).max(axis=0)


def alive_columns(w32, w64):
    """The columns of a multipole / local array that carry information in fp32: those on which the two oracles agree to 1 % of the
    column's scale.  A component that vanishes by symmetry (the z moments of a plane at z = const, the odd moments of a lattice cell)
    is exactly zero in one precision and the rounding of a centroid in the other; the two oracles differ there by 100 % or by 1e290,
    and nothing can be asked of a third evaluation.  (Where both oracles have an exact zero the column stays alive, and the GPU has
    to have an exact zero too.)"""
    return column_errs(np.asarray(w32, dtype=np.float64), w64) < 1e-2
