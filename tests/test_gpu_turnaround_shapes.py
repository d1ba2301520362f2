"""kd_turnaround_kernel (csrc/kd_build_kernels.hpp), the fused pass between two force evaluations of nbco_integrate_steps and its _b and _t
forms, at every part of its launch: 128 workgroups of 1024 threads, four rows per thread and trip at i0 + u * 131072, a second trip of the
grid-stride loop above n = 524288.  The other modules hold the fused run to the step-by-step sequence at n <= 100000, where only slot
u = 0 of the first trip holds a row.  Here: slots 1 to 3, a partly filled slot, the second trip, and the benchmark's n = 2^20.

Part 0 (no GPU) pins the sizes to the kernel's constants.  Part 1 compares the fused run with the step-by-step sequence bit for bit: state,
tree and counts.  Part 2 holds what part 1 would not see if both sides were wrong alike: the root box against numpy's min and max, the
bath's rows against the numpy model, the step-by-step side's re-ordering against the permutation it reports."""
import hashlib
import os
import re

import numpy as np
import pytest

import bath_numpy as bn
from test_gpu_bath import BATH, OMEGA, SEED

gpu = pytest.mark.gpu

PREP_GRID, PREP_BLOCK, U = 128, 1024, 4               # kd_build_kernels.hpp: kPrepGrid, kPrepBlock, and U of kd_turnaround_kernel
STRIDE = PREP_GRID * PREP_BLOCK                       # 131072 rows per slot
# n: rows in (trip 0, slots 0..3), rows in (trip 1, slots 0..3)
OCCUPANCY = {
    131073: ((STRIDE, 1, 0, 0), (0, 0, 0, 0)),                        # slot 1, one row; odd n: v and a are off the 16-byte grid
    262148: ((STRIDE, STRIDE, 4, 0), (0, 0, 0, 0)),                   # slot 2, a tail; aligned
    393217: ((STRIDE, STRIDE, STRIDE, 1), (0, 0, 0, 0)),              # slot 3, one row
    524293: ((STRIDE,) * 4, (5, 0, 0, 0)),                            # second trip, slot 0 only
    655367: ((STRIDE,) * 4, (STRIDE, 7, 0, 0)),                       # second trip, tail in slot 1
    1048576: ((STRIDE,) * 4, (STRIDE,) * 4),                          # the benchmark's shape
}
SIZES = tuple(OCCUPANCY)
N_DIST_LOCAL = 600000 // 2                                            # test_gpu_dist.py: test_sharded_turnaround_equals_step_kernels[600000x2-*]
GRID1D_THREADS = 2048 * 256                                           # kd_list_kernels.hpp: grid1d's cap x kBlock (reorder_state_kernel)

VARIANTS = ("plain", "omega", "bath", "omega_bath")
T0 = 2 ** 32 - 3                                                      # the tick's low word wraps inside the run
DT = 5e-4


def rows_per_slot(n):
    """rows of each (trip, slot) of kd_turnaround_kernel's loop `for (i0 = tid; i0 < n; i0 += U * stride)`, row i = i0 + u * stride"""
    trips = max(2, -(-n // (U * STRIDE)))
    return tuple(tuple(min(max(n - (t * U + u) * STRIDE, 0), STRIDE) for u in range(U)) for t in range(trips))


# ---- 0. the sizes still mean what they say ----------------------------------------------------------------------------------------
def test_sizes_reach_the_slots_they_are_named_for():
    """the constants mirrored above are the ones in the kernel's source, and every size used below fills the slots it is there for.
    A retuned launch fails here: choose new sizes then."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "coulomb_oscillators_amd", "csrc", "kd_build_kernels.hpp")).read()
    m = re.search(r"constexpr int kPrepBlock = (\d+), kPrepGrid = (\d+);", src)
    assert m and (int(m.group(1)), int(m.group(2))) == (PREP_BLOCK, PREP_GRID)
    body = src[src.index("void kd_turnaround_kernel("):]
    body = body[:body.index("\n}\n")]
    u = re.findall(r"constexpr int U = (\d+);", body)
    assert u == [str(U)]
    assert "i0 += U * stride" in body and "i0 + u * stride" in body and "gridDim.x * kPrepBlock" in body
    assert STRIDE == 131072
    for n, want in OCCUPANCY.items():
        got = rows_per_slot(n)
        assert got == want, (n, got)
        assert sum(map(sum, got)) == n
    assert rows_per_slot(N_DIST_LOCAL) == ((STRIDE, STRIDE, 37856, 0), (0, 0, 0, 0))
    # what the other modules reach: slot 0 of the first trip alone
    for n in (100000, 65536, 32768):
        assert rows_per_slot(n) == ((n, 0, 0, 0), (0, 0, 0, 0))
    assert 655367 > GRID1D_THREADS and 655367 % 4 != 0 and 131073 % 4 != 0 and 262148 % 4 == 0


# ---- the runs ---------------------------------------------------------------------------------------------------------------------
_HOST = {}


def _host(oracle32, n):
    """the reference's initial state and parameters, once per n, read-only"""
    if n not in _HOST:
        buf, par = oracle32.init_reference(n), oracle32.params(n)
        buf.setflags(write=False)
        par.setflags(write=False)
        _HOST[n] = (buf, par)
    return _HOST[n]


def _dev(x):
    import torch
    return torch.from_numpy(np.array(x)).cuda()


def _single(e, variant, d, n, prm, k, **kw):
    """step number k of the run, one call"""
    from coulomb_oscillators_amd import EVAL_FMM_KDTREE as KD, INTEG_LEAPFROG as LF
    om = OMEGA if "omega" in variant else None
    if "bath" in variant:
        e.integrate_t(LF, KD, d, n, prm, DT, BATH["gamma"], BATH["kT"], T0 + k, seed=SEED, omega=om, **kw)
    elif om:
        e.integrate_b(LF, KD, d, n, prm, DT, om, **kw)
    else:
        e.integrate(LF, KD, d, n, prm, DT, **kw)


def _fused(e, variant, d, n, prm, k, steps, **kw):
    """steps k .. k + steps - 1 of the run in one call"""
    from coulomb_oscillators_amd import EVAL_FMM_KDTREE as KD, INTEG_LEAPFROG as LF
    om = OMEGA if "omega" in variant else None
    if "bath" in variant:
        e.integrate_steps_t(LF, KD, d, n, prm, DT, steps, BATH["gamma"], BATH["kT"], T0 + k, seed=SEED, omega=om, **kw)
    elif om:
        e.integrate_steps_b(LF, KD, d, n, prm, DT, steps, om, **kw)
    else:
        e.integrate_steps(LF, KD, d, n, prm, DT, steps, **kw)


TREE_ARRAYS = ("lbound", "rbound", "splitdim", "index", "center", "unsort")
INFO_FIELDS = ("L", "ntot", "n", "p2p_pairs", "m2l_pairs", "build_mode")


def _run(oracle32, n, p, tree_steps, steps, variant, fused, kw):
    """compute_force, then steps + 3 leapfrog steps: `steps` fused, one single, two fused -- or all of them single.  Returns the state on
    the device, the tree of the last evaluation and its counts."""
    import torch
    from coulomb_oscillators_amd import Engine, EVAL_FMM_KDTREE
    buf, par = _host(oracle32, n)
    e = Engine(fmm_order=p, unsort=0, tree_steps=tree_steps)
    d, prm = _dev(buf), _dev(par)
    e.compute_force(EVAL_FMM_KDTREE, d, n, prm, elastic=kw.get("elastic", True))
    if fused == "whole":
        _fused(e, variant, d, n, prm, 0, steps + 3, **kw)
    elif fused:
        _fused(e, variant, d, n, prm, 0, steps, **kw)
        _single(e, variant, d, n, prm, steps, **kw)
        _fused(e, variant, d, n, prm, steps + 1, 2, **kw)
    else:
        for k in range(steps + 3):
            _single(e, variant, d, n, prm, k, **kw)
    torch.cuda.synchronize()
    info = e.kd_info()
    tree = {name: e.kd_array(name) for name in TREE_ARRAYS}
    counts = {f: int(getattr(info, f)) for f in INFO_FIELDS}
    e.close()
    return d, tree, counts


_ENDS = {}          # (n, p, tree_steps, steps, scale, elastic, variant) -> digest of the velocities after the steps + 3 fused steps


def _digest(v):
    return hashlib.sha256(v.contiguous().cpu().numpy().tobytes()).digest()


def _end_of(oracle32, n, p, tree_steps, steps, variant, kw):
    key = (n, p, tree_steps, steps, kw.get("scale", 1.0), kw.get("elastic", True), variant)
    if key not in _ENDS:
        _ENDS[key] = _digest(_run(oracle32, n, p, tree_steps, steps, variant, "whole", kw)[0][1])
    return _ENDS[key]


def _order(n):
    return 6 if n == 1 << 20 else 4                   # p = 6 at 2^20: the benchmark's configuration


CASES = ([(n, 1, 4, v, {}) for n in SIZES for v in VARIANTS]
         + [(n, 3, 7, v, {}) for n in (262148, 655367) for v in VARIANTS]
         + [(n, 1, 4, v, dict(scale=0.5, elastic=False)) for n in (131073, 655367) for v in ("plain", "omega_bath")])


def _case_id(c):
    n, tree_steps, steps, variant, kw = c
    return "%d-ts%d-%s%s" % (n, tree_steps, variant, "-scaled" if kw else "")


# ---- 1. fused equals step by step -------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_fused_leapfrog_equals_step_by_step(oracle32, case):
    """the pattern of the three modules' test of this name at the sizes of OCCUPANCY: `steps` fused steps, one single step and two more
    fused ones against steps + 3 single calls on a second engine.  tree_steps = 1: GATHER = true and prep = 1 in every pass;
    tree_steps = 3, steps = 7: the passes are (GATHER, prep) = (1, 0), (0, 0), (0, 1), (1, 0), ... -- with tree_steps = 1 all four
    combinations of each instantiation.  scale = 0.5: the kick's ks = dt scale / 2 and the drift's ds = dt are different numbers.
    Positions, velocities, accelerations, the tree of the last evaluation and its counts: the same bytes."""
    import torch
    n, tree_steps, steps, variant, kw = case
    p = _order(n)
    out = [_run(oracle32, n, p, tree_steps, steps, variant, fused, kw) for fused in (False, True)]
    (d0, tree0, counts0), (d1, tree1, counts1) = out
    assert torch.isfinite(d0).all() and torch.isfinite(d1).all()
    for part, name in enumerate(("positions", "velocities", "accelerations")):
        a, b = d0[part].view(torch.int32), d1[part].view(torch.int32)
        assert torch.equal(a, b), "%s differ in %d rows, the first at row %d" % (name, int((a != b).any(1).sum()), int((a != b).any(1).nonzero()[0]))
    assert counts0 == counts1 and counts0["n"] == n
    for name in TREE_ARRAYS:
        assert tree0[name].shape == tree1[name].shape, name
        assert np.array_equal(tree0[name].view(np.int32), tree1[name].view(np.int32)), name + " differs"
    # the variant was in the run: it ends elsewhere than the runs without its parts
    key = (n, p, tree_steps, steps, kw.get("scale", 1.0), kw.get("elastic", True), variant)
    _ENDS.setdefault(key, _digest(d1[1]))
    others = {"plain": (), "omega": ("plain",), "bath": ("plain",), "omega_bath": ("plain", "omega", "bath")}[variant]
    if kw:
        others = others[:1]
    for other in others:
        assert _ENDS[key] != _end_of(oracle32, n, p, tree_steps, steps, other, kw), (variant, other)


# ---- 2. checks that do not compare the GPU with itself ----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n", SIZES)
def test_root_box_is_numpys_min_and_max(oracle32, n, variant):
    """tree_steps = 1: the last evaluation of a fused run rebuilds from the prologue the turnaround wrote -- the bounding-box reduction
    over every slot and trip -- and the positions do not move after it.  lbound[0] / rbound[0] are then numpy's min(0) / max(0) of the final
    positions, as bytes (the oracle's root box is exactly that: checked on the CPU at n = 5000 and 131073), and `unsort`, the
    identity written from every slot and permuted by the build, is a permutation.  In tree order the last rows hold an extreme of the
    root's split axis: a reduction that left a slot out gives another box."""
    d, tree, counts = _run(oracle32, n, _order(n), 1, 4, variant, "whole", {})
    _ENDS.setdefault((n, _order(n), 1, 4, 1.0, True, variant), _digest(d[1]))
    pos = d[0].cpu().numpy()
    assert np.isfinite(pos).all() and counts["n"] == n
    assert tree["lbound"][0].tobytes() == pos.min(0).tobytes(), (tree["lbound"][0], pos.min(0))
    assert tree["rbound"][0].tobytes() == pos.max(0).tobytes(), (tree["rbound"][0], pos.max(0))
    assert int(tree["splitdim"][0]) == int(np.argmax(pos.max(0) - pos.min(0)))
    assert np.array_equal(np.sort(tree["unsort"]), np.arange(n, dtype=np.int32))


@gpu
def test_bath_rows_against_the_numpy_model(oracle32):
    """kd_turnaround_kernel<false, float, Bath3> in every slot and in the second trip against bath_numpy: n = 655367 free particles
    (param[0] = 0, no elastic term), one tree for the whole run (tree_steps = 64), so a row keeps its index and the noise of row i is the
    model's.  The accelerations are 0, the kicks add nothing, and the velocities after three fused steps are the model's two half bath
    steps per step on the tree-ordered initial velocities (as values: a kick may turn a -0 into +0).  gamma dt = 0.2 and 0.75.  This is
    the comparison of test_gpu_bath.py's test_free_particles_reach_the_bath_temperature, which runs over the direct evaluator and never
    enters the fused pass.  Positions: part 1 (numpy has no fused multiply-add to restate them with)."""
    import torch
    from coulomb_oscillators_amd import Engine, EVAL_FMM_KDTREE, INTEG_LEAPFROG, bath_coeffs
    n, steps = 655367, 3
    buf, par = _host(oracle32, n)
    par = par.copy()
    par[0] = 0
    e = Engine(fmm_order=4, unsort=0, tree_steps=64)
    d, prm = _dev(buf), _dev(par)
    e.compute_force(EVAL_FMM_KDTREE, d, n, prm, elastic=False)
    torch.cuda.synchronize()
    start = d.cpu().numpy()
    perm = e.kd_array("unsort")
    assert np.isfinite(start[2]).all() and np.array_equal(start[2], np.zeros((n, 3), dtype=np.float32))
    assert start[1].tobytes() == buf[1][perm].tobytes()                          # tree order
    e.integrate_steps_t(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, DT, steps, BATH["gamma"], BATH["kT"], T0, seed=SEED, elastic=False)
    torch.cuda.synchronize()
    got = d.cpu().numpy()
    assert np.array_equal(e.kd_array("unsort"), perm)                            # no rebuild in between: the rows stayed
    e.close()
    assert np.isfinite(got).all() and np.array_equal(got[2], np.zeros((n, 3), dtype=np.float32))
    want = bn.free_bath_run(start[1], DT, steps, bn.Bath(BATH["gamma"], BATH["kT"], SEED, coeffs=bath_coeffs), tick0=T0)
    bad = (got[1] != want).any(1)
    assert not bad.any(), "%d rows differ from the model, the first at row %d" % (int(bad.sum()), int(np.flatnonzero(bad)[0]))
    assert got[1][:, 1].tobytes() == start[1][:, 1].tobytes()                    # gamma = 0 on y
    assert not np.array_equal(got[1][:, 0], start[1][:, 0]) and not np.array_equal(got[0], start[0])


@gpu
def test_step_by_step_reordering_follows_the_permutation(oracle32):
    """the other side of part 1: reorder_state_kernel above the 2048 x 256 threads of its grid (a second grid-stride pass) puts positions
    AND velocities into the order the tree reports"""
    import torch
    from coulomb_oscillators_amd import Engine, EVAL_FMM_KDTREE
    n = 655367
    buf, par = _host(oracle32, n)
    e = Engine(fmm_order=4, unsort=0, tree_steps=1)
    d, prm = _dev(buf), _dev(par)
    e.compute_force(EVAL_FMM_KDTREE, d, n, prm)
    torch.cuda.synchronize()
    perm = e.kd_array("unsort")
    e.close()
    got = d.cpu().numpy()
    assert np.array_equal(np.sort(perm), np.arange(n, dtype=np.int32))
    assert not np.array_equal(perm, np.arange(n, dtype=np.int32))
    assert got[0].tobytes() == buf[0][perm].tobytes()
    assert got[1].tobytes() == buf[1][perm].tobytes()
