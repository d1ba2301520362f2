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
