"""Inputs of the 3-D shape tests (test_shapes3d_host.py, test_gpu_shapes3d.py): the states a run reaches late and the states users
feed in -- flat, collinear, tied, duplicated, stretched -- built from the reference's Gaussian ball so that every one of them has
the ball's particle count, velocities and length scale.  Pure numpy on top of Oracle.init_reference; all arithmetic in float32.

CASES lists (evaluator, shape, n, p, what).  what = "forces": both oracles are finite on the input and agree on the tree, so the
accelerations of a GPU evaluation are compared with them.  what = "lists": the reference's forces mean nothing on the input (fp32
cancellation, lists that differ between fp32 and fp64, NaN in both precisions); only the tree / keys / lists are compared.
test_shapes3d_host.py asserts, without a GPU, that every case is what this table says it is.

SELECT_CASES lists (shape, n, p, what) for the kd-tree at sizes whose top levels are built by selection (test_gpu_select_shapes.py),
and select_nodes / mode_from_nodes / tie_orders restate on the oracle's tree what that build meets there."""
import numpy as np

SHAPES = ("gauss", "plane", "plane_off", "line", "lattice", "quant16", "dup2", "dup8", "dup16", "dup64", "late", "two_clumps", "offset",
          "dup128", "ejected", "zeros", "quant2048")
# the shapes that take a permutation, in the order they draw it (new ones at the end only: the states of the others keep their bytes)
DRAWS = ("lattice", "dup2", "dup8", "dup16", "dup64", "dup128")
ZERO_BLOCK = 4                                              # "zeros": -0.0 on this many particles below the root median, +0.0 on as many above
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
    elif name.startswith("quant"):
        # a grid of K cells per R: 16 puts hundreds of particles on every grid plane; 2048 a dozen, all at different points of it
        K = f(int(name[5:]))
        pos[:] = np.round(pos / R * K) / K * R
    elif name.startswith("dup"):
        K = int(name[3:])
        pos[:] = np.repeat(pos[:n // K], K, axis=0)[perm[name]]
    elif name == "late":
        pos[:3] = LATE_ROWS * R
    elif name == "ejected":
        # the late state a long run reaches (nbco.h, list_grow): a few particles thrown out to 1e6 times the ball's size
        pos[:3] = f(25000) * LATE_ROWS * R
    elif name == "zeros":
        # The root cuts the axis of largest extent into the n // 2 smallest keys and the rest.  The axis is shifted (in fp32) so that
        # exactly n // 2 coordinates are negative, then the ZERO_BLOCK negative ones nearest to zero become -0.0 and the ZERO_BLOCK
        # positive ones nearest to zero +0.0: eight particles that compare equal as floats, that no linear bucket key separates, and
        # that the reference's key (the ordered float bits) orders strictly -- the root pivot is -0.0, the right child begins at +0.0.
        a = int(np.argmax(pos.max(axis=0) - pos.min(axis=0)))
        x = np.sort(pos[:, a])
        k = n // 2
        pos[:, a] -= x[k - 1] + (x[k] - x[k - 1]) / f(2)
        order = np.argsort(pos[:, a], kind="stable")
        assert pos[order[k - 1], a] < 0 < pos[order[k], a], "the shift leaves no coordinate at zero and the median at the sign change"
        pos[order[k - ZERO_BLOCK:k], a] = f(-0.0)
        pos[order[k:k + ZERO_BLOCK], a] = f(0.0)
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

# the shapes that only SELECT_CASES runs (added with it; CASES is pinned by test_the_table_covers_what_it_has_to)
SELECT_ONLY = ("dup128", "ejected", "zeros", "quant2048")


def select_cases():
    """(shape, n, p, what) with the meanings of CASES, kd-tree only, at sizes whose top levels are built by SELECTION (k_kdselect.hip:
    every level whose nodes hold more than 4096 particles).  20480 -> 10240 -> 5120: three selection levels, two with the 1024-thread
    kernels and one with the 256-thread kernels; 65536: four.  The lattice needs a cube: 27^3 = 19683 -> 9841 / 9842 -> 4920 / 4921."""
    F, T = "forces", "lists"
    n = 20480
    rows = [(s, n, 4, F) for s in ("gauss", "plane", "plane_off", "line", "dup2", "dup8", "dup16", "late", "ejected", "zeros")]
    rows += [("lattice", 19683, 4, T), ("quant16", n, 4, T), ("dup64", n, 4, T), ("dup128", n, 4, T), ("two_clumps", n, 4, T), ("offset", n, 4, T),
             ("quant2048", n, 4, T)]
    rows += [("late", n, 6, F), ("dup8", n, 6, F)]
    rows += [("late", 65536, 4, F), ("plane", 65536, 4, F), ("line", 65536, 4, F), ("ejected", 65536, 4, F)]
    return rows


SELECT_CASES = select_cases()
SELECT_MIN = 4096          # kSubS: a node above it is split by selection, the rest of its subtree in one workgroup's LDS
TIE_CAP = 64               # kTieCap of k_kdselect.hip: candidates the exact resolver orders
# why a "lists" row of SELECT_CASES is one (the vocabulary of LISTS_WHY below)
SELECT_LISTS_WHY = {
    ("lattice", 19683, 4): "lists_differ", ("quant16", 20480, 4): "nonfinite", ("dup64", 20480, 4): "nonfinite",
    ("dup128", 20480, 4): "nonfinite", ("two_clumps", 20480, 4): "lists_differ", ("offset", 20480, 4): "lists_differ",
    ("quant2048", 20480, 4): "lists_differ",
}


def kd_of(row):
    """a SELECT_CASES row as a case of evaluate()"""
    return ("kd",) + tuple(row)


def select_id(row):
    return "%s-%d-p%d-%s" % tuple(row)


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


# ---- the selection levels of a kd-tree (k_kdselect.hip), restated on the oracle's tree -----------------------------------------
def ordered_key(x):
    """the reference's sort key of a float32: its bits, ordered (-0.0 strictly before +0.0)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u >> 31, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def lin_bucket(x, lo, hi, bits=22):
    """lin_window / lin_key of k_kdselect.hip in float32 numpy, every subtraction, division and multiplication rounded to fp32:
    the top `bits` bits of the box-linear key of the coordinates x in a node whose box is [lo, hi] along the split axis"""
    f = np.float32
    top = f(4294967040.0)
    span = f(hi) - f(lo)
    scale = top / span if span > 0 else f(0)
    v = (np.asarray(x, dtype=f) - f(lo)) * f(scale)
    assert v.dtype == f
    return np.minimum(np.maximum(v, f(0)), top).astype(np.uint32) >> np.uint32(32 - bits)


def warm_bits(n, level):
    """bits of the warm select's bucket key at a level of a tree over n particles (kd_select_level, before any miss has coarsened
    it): about 1 / 64 element per bucket, between 16 and 22 bits"""
    node = n >> level
    lg = 0
    while (1 << lg) < node:
        lg += 1
    return max(12, min(22, max(16, lg + 6)))


def select_nodes(tree, pos_tree_order):
    """One row per node that the build splits by selection (more than SELECT_MIN particles), from a tree dict of the oracle and the
    positions in that tree's order: (node, ties, bucket, ties_left, near, warm).
      ties       particles of the node whose key along the split axis equals the pivot's (the largest key of the left child)
      bucket     particles of the node in the pivot's 22-bit bucket of the box-linear key (lin_bucket) over the node's own box
      ties_left  how many of the ties are in the left child: ties_left == ties means that the cut falls BEHIND the tied run
      near       particles in the pivot's bucket or one of its two neighbours
      warm       particles in the pivot's bucket of the WARM select, which cuts the same key into warm_bits(level) bits"""
    pos = np.asarray(pos_tree_order, dtype=np.float32)
    rows = []
    for v in np.flatnonzero(np.asarray(tree["mult"]) > SELECT_MIN):
        if 2 * v + 2 >= tree["ntot"]:
            continue
        a, i, m = int(tree["splitdim"][v]), int(tree["index"][v]), int(tree["mult"][v])
        ml = int(tree["mult"][2 * v + 1])
        assert int(tree["index"][2 * v + 1]) == i
        x = pos[i:i + m, a]
        key = ordered_key(x)
        pivot = int(np.argmax(key[:ml]))
        assert key[:ml].max() <= key[ml:].min(), "the oracle's children are the ml smallest keys and the rest"
        tie = key == key[pivot]
        b = lin_bucket(x, tree["lbound"][v, a], tree["rbound"][v, a]).astype(np.int64)
        w = b >> (22 - warm_bits(int(tree["mult"][0]), int(v + 1).bit_length() - 1))
        rows.append((int(v), int(tie.sum()), int((b == b[pivot]).sum()), int(tie[:ml].sum()), int((np.abs(b - b[pivot]) <= 1).sum()),
                     int((w == w[pivot]).sum())))
    return np.array(rows, dtype=np.int64).reshape(-1, 6)


def mode_from_nodes(nodes):
    """What nbco_kd_get_info's build_mode has to be after a first build, from select_nodes' rows; None where the figures do not decide.

    The build starts with the two-pass select: every element of the pivot's 22-bit bucket is a candidate of the exact resolver,
    which takes TIE_CAP of them.  A fuller bucket flags the build and it is repeated with three passes (mode 1), whose candidates
    are the exact ties of the pivot -- and those only where the cut falls INSIDE the tied run (all_left in sel_partition_kernel: a run
    that ends with the left child goes left as a whole and nobody resolves it).  More than TIE_CAP of them flag that build too and
    the sorting build takes over (mode 2).
      2     some node has more than TIE_CAP ties and the cut inside them
      1     not 2, and some node's bucket certainly overflows: more than TIE_CAP ties (equal keys share a bucket however the key is
            cut into digits), or more than 4 x TIE_CAP particles in the restated bucket
      0     every restated bucket holds at most TIE_CAP / 2
    The factors 4 and 1 / 2 keep the expectation independent of how the two radix passes cut the 22 bits and of the last bit of
    this restatement."""
    ties, bucket, left = nodes[:, 1], nodes[:, 2], nodes[:, 3]
    if ((ties > TIE_CAP) & (left < ties)).any():
        return 2
    if (ties > TIE_CAP).any() or (bucket > 4 * TIE_CAP).any():
        return 1
    if (bucket <= TIE_CAP // 2).all():
        return 0
    return None


def expected_mode(oracle32, oracle64, row):
    """mode_from_nodes on the fp32 oracle's tree of a SELECT_CASES row, as a set of admissible modes (None: not asserted).
    dup64: TIE_CAP copies of every point.  The rule is nt > kTieCap, so a bucket that holds exactly one point's copies still fits
    the resolver (mode 0); one neighbour in it and the build goes to three passes, where every cut falls behind a tied run (mode 1).
    Where the pivot's bucket AND its two neighbours hold nothing but the copies at every selection node, rounding cannot add
    one: then it is mode 0."""
    r = evaluate(oracle32, oracle64, kd_of(row))
    nodes = select_nodes(r["t32"], r["buf"][0][r["t32"]["perm"]])
    if row[0] == "dup64":
        return {0} if (nodes[:, 4] == TIE_CAP).all() and (nodes[:, 1] == TIE_CAP).all() else {0, 1}
    mode = mode_from_nodes(nodes)
    return None if mode is None else {mode}


def tie_orders(tree, pos_tree_order):
    """The exact tie resolver's order, restated: inside node v the reference's stable-sort chain orders by (c[a1], c[a2], c[a3],
    original index), a1 = splitdim(v), a2 and a3 the next distinct split axes of v's ancestors, nearest first (k_kdselect.hip, head).
    One row per selection node whose cut falls inside a run of equal c[a1]: (node, chain, blind) -- chain: the tied particles that
    the oracle's tree has in the left child are the first ones of that order; blind: they are ALSO the first ones of the order
    without c[a2], so that a resolver that ignores its second key would not be seen at this node."""
    pos = np.asarray(pos_tree_order, dtype=np.float32)
    org = np.asarray(tree["perm"], dtype=np.int64)
    rows = []
    for v, ties, _, left, _, _ in select_nodes(tree, pos):
        if left == ties:
            continue
        i, m, ml = int(tree["index"][v]), int(tree["mult"][v]), int(tree["mult"][2 * v + 1])
        a1 = int(tree["splitdim"][v])
        rest, u = [], int(v)
        while u > 0 and len(rest) < 2:
            u = (u - 1) // 2
            a = int(tree["splitdim"][u])
            if a != a1 and a not in rest:
                rest.append(a)
        key = ordered_key(pos[i:i + m, a1])
        tied = np.flatnonzero(key == key[:ml].max())
        k23 = [ordered_key(pos[i + tied, a]) if a is not None else np.zeros(len(tied), dtype=np.uint32) for a in (rest + [None, None])[:2]]
        went_left = set(tied[tied < ml].tolist())
        full = tied[np.lexsort((org[i + tied], k23[1], k23[0]))][:left]
        blind = tied[np.lexsort((org[i + tied], k23[1]))][:left]
        rows.append((int(v), set(full.tolist()) == went_left, set(blind.tolist()) == went_left))
    return rows


# ---- the 3-D energy diagnostics and the tree bond order on the shapes (test_energy_shapes_host.py, test_gpu_energy_shapes3d.py,
# test_gpu_bond_order.py) ------------------------------------------------------------------------------------------------------------
# the options a row of ENERGY_SHAPE_CASES runs with unless it says otherwise (Engine.set names)
ENERGY_BASE = dict(unsort=1, m2l_first=0, coll=1, p2p_mutual=0, tree_steps=1, tree_L=0, far_fp64=0, eps2=1e-18, tree_radius=1.0)
# where points coincide the softened near field buries the far field at eps2 = 1e-18: those rows run with a softening length of 1e-4,
# below the ball's median nearest-neighbour distance of 4.5e-4
EPS2_TIED = 1e-8


def energy_shape_cases():
    """(shape, n, p, opts): the rows of the energy diagnostics.  n = 4096 at p = 4 gives 256 leaves of 16; tree_L = 5 gives 32 leaves
    of 128 (two tiles of 64 targets in kd_psi_leaf_kernel), of 125 / 126 at n = 4001 (an uneven last tile); p = 10 gives 32 leaves
    of 128 by the level formula itself.  The last row is all near field (no M2L pair): the only form in which 64 copies per point
    give finite numbers, compared with the pair sum alone.

    Two rows are not the obvious ones, because the obvious ones have no far field (test_energy_shapes_host.py measures it).  Three
    particles at 40..70 R stretch a tree of 32 leaves until the whole ball is one another's near field: late at p = 10 (32 leaves by
    the formula) has a far part of 0 % of max |psi|, late at n = 4001 with tree_L = 5 of 3 %.  So late at p = 10 runs with
    tree_L = 8 (77 % of the particles above the 10 %), and the uneven last tile (125 / 126 per leaf) runs on plane_off (88 %)."""
    tied = dict(eps2=EPS2_TIED)
    rows = [(s, 4096, 4, {}) for s in ("gauss", "plane", "plane_off", "line", "lattice", "late", "ejected", "two_clumps", "zeros", "offset")]
    rows += [(s, 4096, 4, tied) for s in ("dup2", "dup8", "dup16", "quant16")]
    rows += [("plane", 4096, 10, dict(far_fp64=1)), ("late", 4096, 10, dict(far_fp64=1, tree_L=8))]
    rows += [("line", 8000, 6, {}), ("dup8", 8000, 6, tied)]
    rows += [("plane", 4096, 4, dict(tree_L=5)), ("dup16", 4096, 4, dict(tree_L=5, **tied)), ("plane_off", 4001, 4, dict(tree_L=5))]
    rows += [("plane_off", 4096, 4, dict(unsort=0)), ("late", 4096, 4, dict(p2p_mutual=1, unsort=0)), ("line", 4096, 4, dict(m2l_first=1)),
             ("ejected", 4096, 4, dict(coll=0))]
    rows += [("dup64", 4096, 4, dict(tree_radius=1e6))]
    return rows


ENERGY_SHAPE_CASES = energy_shape_cases()
# the rows that claim more than 64 per leaf: tree_L = 5, and plane at p = 10 by the level formula
ENERGY_WIDE_LEAVES = [r for r in ENERGY_SHAPE_CASES if r[3].get("tree_L") == 5 or (r[2] == 10 and not r[3].get("tree_L"))]


def energy_id(row):
    shape, n, p, opts = row
    return "-".join(["%s-%d-p%d" % (shape, n, p)] + ["%s=%g" % kv for kv in sorted(opts.items())])


def energy_all_near(row):
    return row[3].get("tree_radius", 1.0) > 1e3


def energy_opts(row):
    """a row's Engine options, fmm_order included"""
    return dict(ENERGY_BASE, fmm_order=row[2], **row[3])


def energy_oracle_kw(oracle, row):
    """run_oracle's keywords for a row: the oracle has no tree_L, and takes its levels from dens_inhom * n / p^2 -- a power of two
    there moves the level count by whole levels; far_fp64 and p2p_mutual change no tree and no list"""
    _, n, p, _ = row
    o = energy_opts(row)
    kw = dict(radius=o["tree_radius"], eps2=o["eps2"], coll=bool(o["coll"]), unsort=bool(o["unsort"]), m2l_first=o["m2l_first"])
    if o["tree_L"]:
        kw["dens_inhom"] = 2.0 ** (o["tree_L"] - oracle.lib.oracle_kd_levels(n, p, 1.0))
    return kw


def energy_floor(oracle32, oracle64, row):
    """What the METHOD gives on a row, from the fp32 oracle's tree and no device output, once per process: dict of
      tree, pos     the fp32 oracle's tree and the positions in its order
      near, far     the two parts of the restated psi (energy3d_numpy.psi_parts), tree order; None on the all-near-field row
      exact         param0 * the fp64 pair sum, tree order
      energy        oracle64.energy of the state: kinetic, elastic, Coulomb
      floor_energy  |0.5 sum psi - energy[2]| / energy[2]
      floor_mean    mean_i |psi_i - exact_i| / exact_i"""
    import energy3d_numpy as e3
    key = ("energy_floor", energy_id(row))
    if key in _cache:
        return _cache[key]
    shape, n, p, _ = row
    o = energy_opts(row)
    eps2 = np.float32(o["eps2"])
    buf, par = state(oracle32, shape, n), oracle32.params(n)
    kw = energy_oracle_kw(oracle32, row)
    _, pv, t = run_oracle(oracle32, "kd", buf, par, p, **kw)
    pos = buf[0][t["perm"]] if kw["unsort"] else pv[0]
    r = {"tree": t, "pos": pos, "buf": buf, "par": par, "near": None, "far": None}
    r["exact"] = float(par[0]) * e3.pair_potential(pos, eps2)
    r["energy"] = oracle64.energy(buf.astype(np.float64), par.astype(np.float64), eps2=float(eps2), threads=THREADS)
    if not energy_all_near(row):
        with np.errstate(all="ignore"):
            r["near"], r["far"] = e3.psi_parts(t, pos, p, eps2, par[0], coll=kw["coll"])
        psi = r["near"] + r["far"]
        # (a coll = 0 evaluation leaves the near field out: its floors are the near field's share, and its sharp test is the restatement)
        r["floor_energy"] = float(abs(0.5 * psi.sum() - r["energy"][2]) / r["energy"][2])
        r["floor_mean"] = float(np.mean(np.abs(psi - r["exact"]) / r["exact"]))
    _cache[key] = r
    return r


# Bond order: the neighbour radius per shape as (factor, length), at the sizes of bond_shape_n.  Lengths, in the units of the state:
#   "box"   the longest side of the shape's bounding box over the ball's (the scale of test_tree_is_exact_is_reference_on_every_shape)
#   "ball"  1: the ball's own scale, where a few outliers (or a second clump) set the bounding box
#   "grid"  one grid spacing: R / m on the lattice of side m, R / 16 on quant16 (R = the ball's largest |coordinate|)
# 0.002 box is the middle window of the pair statistics.  line: 0.002 gives several hundred neighbours, 0.0006 gives 199.  lattice:
# 1.5 spacings take the 6 + 12 first and second neighbours.  quant16: 1.2 spacings take the 6 face cells only (the 12 edge cells at
# 1.41 spacings bring 698 neighbours at n = 4001), and even those hold 340 particles at n = 4001: the shape runs at n = 2001 (166).
# dup64 / dup128: 64 / 32 distinct points, so nb is a multiple of 64 / 128; 0.002 box links 704 particles of dup64 and no radius
# links a quarter of dup128 with fewer than two other points in reach.
# test_energy_shapes_host.py asserts of every row: nb_max <= 256, a quarter of the particles linked, one isolated (lattice: none).
BOND_SHAPE_RMAX = {
    "gauss": (0.002, "box"), "plane": (0.002, "box"), "plane_off": (0.002, "box"), "line": (0.0006, "box"), "lattice": (1.5, "grid"),
    "quant16": (1.2, "grid"), "dup2": (0.002, "box"), "dup8": (0.002, "box"), "dup16": (0.002, "box"), "dup64": (0.002, "ball"),
    "late": (0.002, "ball"), "two_clumps": (0.002, "ball"), "offset": (0.002, "box"), "dup128": (0.0017, "ball"), "ejected": (0.002, "ball"),
    "zeros": (0.002, "box"), "quant2048": (0.002, "box"),
}
BOND_COINCIDENT = ("quant16", "dup2", "dup8", "dup16", "dup64", "dup128")          # shapes with pairs at r2 = 0


def bond_shape_n(name):
    """the sizes of test_tree_is_exact_is_reference_on_every_shape, but for quant16 (above)"""
    return 3375 if name == "lattice" else 4096 if name.startswith("dup") else 2001 if name == "quant16" else 4001


def bond_rmax(oracle32, name):
    n = bond_shape_n(name)
    factor, length = BOND_SHAPE_RMAX[name]
    gauss = state(oracle32, "gauss", n)[0]
    if length == "box":
        pos = state(oracle32, name, n)[0]
        return factor * float((pos.max(0) - pos.min(0)).max() / (gauss.max(0) - gauss.min(0)).max())
    if length == "ball":
        return factor
    assert length == "grid" and name in ("lattice", "quant16")
    return factor * float(np.abs(gauss).max()) / (lattice_side(n) if name == "lattice" else 16)


def bond_model(oracle32, name):
    """(pos, rmax, bond_numpy.bond_order, pairs inside, pairs at r2 = 0) of a shape, once per process"""
    import bond_numpy as BN
    import pairstat_numpy as PN
    key = ("bond", name)
    if key not in _cache:
        pos = np.ascontiguousarray(state(oracle32, name, bond_shape_n(name))[0])
        rmax = bond_rmax(oracle32, name)
        r2, _ = PN.inside_pairs(pos, rmax)
        _cache[key] = (pos, rmax, BN.bond_order(pos, rmax), len(r2), int((r2 == 0).sum()))
    return _cache[key]
