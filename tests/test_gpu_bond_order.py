"""GPU tests of the bond-orientational order: nbco_bond_order / nbco_bond_order_tree / nbco_2d_bond_order (Engine.bond_order,
bond_order_tree, bond_order_2d) against the numpy model of tests/bond_numpy.py, which shares nothing with the kernels' harmonics
(Legendre double sums over the bonds).  nb, bonds, isolated and nb_max compare as integers; q_l^2, psi_l^2 and Q_l^2 with the
absolute tolerance 1e-11 derived for nb <= 256 (|Y_lm| <= 1.02, degree-6 polynomials of about 40 operations on a u good to 3 ulp:
7e-15 per term; a mean over at most 256 terms adds 256 * 2^-53; 13 components).  Every input asserts nb.max() <= 256.  The sizes are
the smallest at which the kernels take another path: the exact form's tiles are 256 wide, the walk's waves 64, its workgroups 1024."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import bond_numpy as BN
import shapes3d

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "coulomb_oscillators_amd", "host")
ERR_ARG, ERR_UNSUPPORTED = 2, 4
POISON_NB, POISON_Q = -7777, -123.456
FORMS3 = ("exact", "tree")


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


def fn_of(e, form):
    return dict(exact=e.bond_order, tree=e.bond_order_tree, exact2d=e.bond_order_2d)[form]


def run(e, form, d, n, rmax, want_nb=True, want_q=True, want_sum=True):
    """one call into poisoned buffers; returns (nb, q, summary) with numpy arrays, None for what was not asked for"""
    import torch
    nb = torch.full((n,), POISON_NB, dtype=torch.int32, device="cuda") if want_nb else False
    q = torch.full((n, 2), POISON_Q, dtype=torch.float64, device="cuda") if want_q else False
    _, _, s = fn_of(e, form)(d, n, rmax, nb=nb, q=q, summary=want_sum)
    torch.cuda.synchronize()
    return (nb.cpu().numpy().astype(np.int64) if want_nb else None), (q.cpu().numpy() if want_q else None), s


@functools.lru_cache(maxsize=None)
def ball(n, dim=3):
    """a Gaussian ball of unit width (fp32 in 3-D, fp64 in 2-D), read-only"""
    x = np.random.default_rng(100 + n).normal(size=(n, dim))
    x = x.astype(np.float32) if dim == 3 else x
    x.setflags(write=False)
    return x


_MODEL = {}


def model(key, pos, rmax):
    """the model of an input, computed once per key and shared; every input of this file has nb <= 256, the tolerance's premise"""
    if key not in _MODEL:
        m = BN.bond_order(pos, rmax)
        assert m["nb_max"] <= 256
        _MODEL[key] = m
    return _MODEL[key]


def check(got, m, what=""):
    """a call's (nb, q, summary) against the model: integers exactly, squares within TOL2"""
    nb, q, s = got
    n = len(m["nb"])
    assert np.array_equal(nb, m["nb"]), (what, "nb", np.flatnonzero(nb != m["nb"])[:8])
    assert np.isfinite(q).all() and not q[m["nb"] == 0].any(), what
    err = np.abs(q * q - m["q2"]).max()
    print(what, "max |dq2|", err)
    assert err < BN.TOL2, (what, err)
    assert (s.n, s.bonds, s.isolated, s.nb_max) == (n, m["bonds"], m["isolated"], m["nb_max"]), what
    Q = np.array(s.Q[:])
    errQ = np.abs(Q * Q - m["Q2"]).max()
    print(what, "max |dQ2|", errQ)
    assert errQ < BN.TOL2, (what, errQ)
    assert np.abs(np.array(s.q_mean[:]) - m["q_mean"]).max() < BN.TOL_MEAN, what


# ---- exact form against the model ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 255, 257, 513])
def test_exact_form_on_a_ball(eng, n):
    """below a tile, across one tile edge and across two; n = 1 has nobody to look at"""
    pos, rmax = ball(n), 1.0
    m = model(("ball", n), pos, rmax)
    d = dev(pos)
    got = run(eng, "exact", d, n, rmax)
    check(got, m, ("exact", n))
    assert got[2].dim == 3 and np.array_equal(d.cpu().numpy(), pos)   # the input is not written
    if n >= 255:
        assert m["nb_max"] >= 20


@pytest.mark.parametrize("name", ["sc", "fcc"])
def test_exact_form_on_a_lattice(eng, name):
    """sc 13^3 = 2197 with first and second neighbours inside (nb = 18 in the bulk), fcc 365 with the 12 nearest"""
    pos, _ = BN.LATTICES[name]()
    rmax = 1.5 if name == "sc" else math.sqrt(3.0)
    assert len(pos) == (2197 if name == "sc" else 365)
    check(run(eng, "exact", dev(pos), len(pos), rmax), model((name, rmax), pos, rmax), name)


# ---- tree form against the model and against the exact form's nb --------------------------------------------------------------------
@pytest.mark.parametrize("n", [63, 64, 65, 1025])
def test_tree_form_on_a_ball(eng, n):
    """a wave less one, a full wave, a wave and one; a second workgroup with one particle"""
    pos, rmax = ball(n), 0.5 if n > 100 else 1.0
    m = model(("ball", n, rmax), pos, rmax)
    d = dev(pos)
    got = run(eng, "tree", d, n, rmax)
    check(got, m, ("tree", n))
    assert np.array_equal(got[0], run(eng, "exact", d, n, rmax)[0])
    assert np.array_equal(d.cpu().numpy(), pos)


def test_tree_form_with_isolated_particles(eng):
    """n = 3001 Gaussian fp32 with rmax = 0.3: particles without a neighbour in the halo, up to a few tens in the core"""
    n, rmax = 3001, 0.3
    pos = ball(n)
    m = model(("ball", n, rmax), pos, rmax)
    assert m["isolated"] > 100 and m["nb_max"] >= 10
    d = dev(pos)
    got = run(eng, "tree", d, n, rmax)
    check(got, m, "tree 3001")
    ex = run(eng, "exact", d, n, rmax)
    check(ex, m, "exact 3001")
    assert np.array_equal(got[0], ex[0])


def test_tree_form_with_leaves_of_several_staging_rounds(engine_lib):
    """the sc lattice, n = 2197, with tree_L = 3: leaves of about 275 particles take five staging rounds of 64"""
    from coulomb_oscillators_amd import Engine
    pos, _ = BN.sc()
    m = model(("sc", 1.5), pos, 1.5)
    e = Engine(tree_L=3)
    try:
        check(run(e, "tree", dev(pos), len(pos), 1.5), m, "sc tree_L=3")
    finally:
        e.close()


@pytest.mark.parametrize("name,opts,rmax", [("ball", {}, 0.5), ("sc", dict(tree_L=3), 1.5)])
def test_tree_form_and_pair_statistics_see_the_same_walk(engine_lib, name, opts, rmax):
    """bond_order_tree and pair_hist_tree(bins=1) are two visitors of one walk: on one engine and one input every bond is a counted
    pair seen from both ends, and a particle has no neighbour exactly where it has no nearest neighbour.  ball(1025): a second
    workgroup with one particle and both sides of a wave; sc with tree_L = 3: leaves of five staging rounds.  The premise -- no two
    particles coincide, or a pair at r2 = 0 would be counted and not be a bond -- and the identities themselves are asserted of the
    numpy models first."""
    import torch
    import pairstat_numpy as PN
    from coulomb_oscillators_amd import Engine
    pos = ball(1025) if name == "ball" else BN.sc()[0]
    n = len(pos)
    m = model((name, n, rmax) if name == "ball" else (name, rmax), pos, rmax)
    r2_inside, nn2_model = PN.inside_pairs(pos, rmax)
    assert len(r2_inside) > 0 and r2_inside.min() > 0.0
    assert m["nb"].sum() == 2 * len(r2_inside) and np.array_equal(m["nb"] == 0, np.isinf(nn2_model)) and m["isolated"] == np.isinf(nn2_model).sum()
    e = Engine(**opts)
    try:
        d = dev(pos)
        nb, _, s = run(e, "tree", d, n, rmax)
        nn2 = torch.full((n,), -1.0, dtype=torch.float64, device="cuda")
        counts = e.pair_hist_tree(d, n, 1, rmax, nn2=nn2)
        torch.cuda.synchronize()
        counts, nn2 = [int(v) for v in counts.cpu().numpy()], nn2.cpu().numpy()
    finally:
        e.close()
    assert int(nb.sum()) == 2 * counts[0] and sum(counts) == n * (n - 1) // 2
    lonely = nn2 == np.inf
    assert np.array_equal(nb == 0, lonely)
    assert s.isolated == lonely.sum() and s.bonds == 2 * counts[0]


@pytest.mark.parametrize("shape", shapes3d.SHAPES)
def test_tree_and_exact_forms_on_every_shape(eng, engine_lib, oracle32, shape):
    """flat, collinear, tied, duplicated, stretched and late-run inputs (the sizes of the pair statistics' shape test, the radii of
    shapes3d.BOND_SHAPE_RMAX, whose premises test_energy_shapes_host.py asserts): both forms against the model, the same nb from
    both, and the tree form once more with tree_L = 3, where a leaf of about 500 particles takes eight staging rounds.  On dup8 and
    quant16 the identity of test_tree_form_and_pair_statistics_see_the_same_walk with coincident points: the pair visitor counts a
    pair at r2 = 0 (j != s), the bond visitor does not (0 < r2), so sum nb = 2 (pairs inside - pairs at r2 = 0), the second count
    from the numpy model."""
    import torch
    from coulomb_oscillators_amd import Engine
    pos, rmax, m, inside, zero = shapes3d.bond_model(oracle32, shape)
    assert m["nb_max"] <= 256
    n = len(pos)
    d = dev(pos)
    ex, tr = run(eng, "exact", d, n, rmax), run(eng, "tree", d, n, rmax)
    check(ex, m, (shape, "exact"))
    check(tr, m, (shape, "tree"))
    assert np.array_equal(ex[0], tr[0])
    e = Engine(tree_L=3)
    try:
        t3 = run(e, "tree", d, n, rmax)
        check(t3, m, (shape, "tree_L=3"))
        if shape in ("dup8", "quant16"):
            assert zero > 0
            counts = e.pair_hist_tree(d, n, 1, rmax)
            torch.cuda.synchronize()
            counts = [int(v) for v in counts.cpu().numpy()]
            assert counts[0] == inside and sum(counts) == n * (n - 1) // 2
            assert int(t3[0].sum()) == 2 * (counts[0] - zero) and t3[2].bonds == 2 * (counts[0] - zero)
    finally:
        e.close()
    assert np.array_equal(d.cpu().numpy(), pos)


def test_tree_form_on_the_bcc_lattice(eng):
    pos, _ = BN.bcc()
    assert len(pos) == 1024
    rmax = math.sqrt(4.5)
    check(run(eng, "tree", dev(pos), len(pos), rmax), model(("bcc", rmax), pos, rmax), "bcc")


def test_tree_form_refuses_leaves_the_build_cannot_hold(engine_lib):
    """tree_L = 2 at n = 20000 asks for 5000 particles per leaf, more than the build's 4096: NBCO_ERR_UNSUPPORTED before any launch,
    the outputs untouched (what nbco_pair_hist_tree refuses)"""
    import torch
    from coulomb_oscillators_amd import Engine, EngineError
    n = 20000
    d = dev(np.random.default_rng(3).normal(size=(n, 3)).astype(np.float32))
    e = Engine(tree_L=2)
    try:
        nb = torch.full((n,), POISON_NB, dtype=torch.int32, device="cuda")
        q = torch.full((n, 2), POISON_Q, dtype=torch.float64, device="cuda")
        with pytest.raises(EngineError) as err:
            e.bond_order_tree(d, n, 0.05, nb=nb, q=q)
        assert err.value.status == ERR_UNSUPPORTED and "per leaf" in str(err.value)
        torch.cuda.synchronize()
        assert (nb == POISON_NB).all() and (q == POISON_Q).all()
    finally:
        e.close()


# ---- ideal-lattice values on the device ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS3)
@pytest.mark.parametrize("name,rmax2,nb,q4,q6", BN.IDEAL)
def test_ideal_lattice_values(eng, form, name, rmax2, nb, q4, q6):
    """the central particle of sc, bcc (both cutoffs) and fcc: Steinhardt's table to 1e-7 (the sc cutoff is rmax^2 = 1.5, see
    tests/test_bond_order_host.py)"""
    pos, centre = BN.LATTICES[name]()
    got_nb, got_q, s = run(eng, form, dev(pos), len(pos), math.sqrt(rmax2))
    assert got_nb[centre] == nb and s.nb_max == nb
    assert abs(got_q[centre, 0] - q4) < 1e-7 and abs(got_q[centre, 1] - q6) < 1e-7


# ---- degenerate shapes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS3 + ("exact2d",))
def test_coincident_particles_have_no_bonds(eng, form):
    n = 1000
    d = dev(np.full((n, 2), -0.5)) if form == "exact2d" else dev(np.full((n, 3), 0.00123, dtype=np.float32))
    nb, q, s = run(eng, form, d, n, 1e-3)
    assert not nb.any() and not q.any()
    assert (s.bonds, s.isolated, s.nb_max) == (0, n, 0) and s.Q[:] == [0.0, 0.0] and s.q_mean[:] == [0.0, 0.0]


@pytest.mark.parametrize("form", FORMS3)
def test_two_coincident_particles_inside_a_lattice(eng, form):
    """a duplicate of a bulk point: the twins are not neighbours of each other, and everybody near them counts both"""
    pos, centre = BN.fcc()
    pos = np.concatenate([pos, pos[centre:centre + 1]])
    rmax = math.sqrt(3.0)
    m = model(("fcc twin", rmax), pos, rmax)
    assert m["nb"][centre] == 12 and m["nb"][-1] == 12 and m["nb_max"] == 13
    check(run(eng, form, dev(pos), len(pos), rmax), m, form)


def test_a_nan_coordinate_is_isolated_and_nobodys_neighbour(eng):
    n, rmax = 513, 1.0
    pos = ball(n).copy()
    pos[300, 1] = np.nan
    m = model(("ball nan", n), pos, rmax)
    keep = np.arange(n) != 300
    rest = model(("ball less one", n), pos[keep], rmax)
    assert m["nb"][300] == 0 and np.array_equal(m["nb"][keep], rest["nb"])
    check(run(eng, "exact", dev(pos), n, rmax), m, "nan")


@pytest.mark.parametrize("form", FORMS3)
def test_rmax_below_the_smallest_spacing(eng, form):
    pos, _ = BN.sc(3)
    nb, q, s = run(eng, form, dev(pos), len(pos), 0.999)
    assert not nb.any() and not q.any() and (s.bonds, s.isolated) == (0, len(pos))


# ---- 2-D exact form ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["square", "triangular", "random"])
def test_exact_form_in_two_dimensions(eng, shape):
    if shape == "random":
        pos, centre, rmax = ball(257, 2), None, 0.7
    else:
        pos, centre = (BN.square2d if shape == "square" else BN.triangular2d)()
        rmax = 1.2
    m = model(("2d", shape), pos, rmax)
    got = run(eng, "exact2d", dev(pos), len(pos), rmax)
    check(got, m, shape)
    assert got[2].dim == 2
    if shape == "square":
        assert got[0][centre] == 4 and abs(got[1][centre, 0] ** 2 - 1.0) < BN.TOL2 and got[1][centre, 1] ** 2 < BN.TOL2
    if shape == "triangular":
        assert got[0][centre] == 6 and abs(got[1][centre, 1] ** 2 - 1.0) < BN.TOL2 and got[1][centre, 0] ** 2 < BN.TOL2


# ---- outputs ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS3 + ("exact2d",))
def test_output_combinations_and_repeatability(eng, form):
    """each NULL combination of the three outputs returns what all three together return, a second call the same bytes; None allocates"""
    n, rmax = 1025, 0.5
    dim = 2 if form == "exact2d" else 3
    d = dev(ball(n, dim))
    nb, q, s = run(eng, form, d, n, rmax)
    assert (nb != POISON_NB).all() and (q != POISON_Q).all()     # poisoned buffers are fully overwritten
    nb2, q2, s2 = run(eng, form, d, n, rmax)
    assert nb2.tobytes() == nb.tobytes() and q2.tobytes() == q.tobytes() and bytes(s2) == bytes(s)
    for want in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)):
        a, b, c = run(eng, form, d, n, rmax, *[bool(w) for w in want])
        assert (a is None) == (not want[0]) and (b is None) == (not want[1]) and (c is None) == (not want[2])
        assert a is None or a.tobytes() == nb.tobytes(), want
        assert b is None or b.tobytes() == q.tobytes(), want
        assert c is None or bytes(c) == bytes(s), want
    made_nb, made_q, made_s = fn_of(eng, form)(d, n, rmax)
    assert made_nb.cpu().numpy().astype(np.int64).tobytes() == nb.tobytes() and made_q.cpu().numpy().tobytes() == q.tobytes()
    assert bytes(made_s) == bytes(s)


@pytest.mark.parametrize("form", FORMS3 + ("exact2d",))
def test_refusals_leave_the_outputs_alone(eng, form):
    import ctypes as C
    import torch
    from coulomb_oscillators_amd import BondSummary
    from coulomb_oscillators_amd.engine import _ptr
    n, rmax = 255, 1.0
    dim = 2 if form == "exact2d" else 3
    d = dev(ball(n, dim))
    nb = torch.full((n,), POISON_NB, dtype=torch.int32, device="cuda")
    q = torch.full((n, 2), POISON_Q, dtype=torch.float64, device="cuda")
    s = BondSummary()
    s.n, s.nb_max, s.Q[0] = -5, -6, -7.0
    fn = getattr(eng.lib, dict(exact="nbco_bond_order", tree="nbco_bond_order_tree", exact2d="nbco_2d_bond_order")[form])

    def call(ctx=eng.ctx, p=d, n=n, rmax=rmax, a=nb, b=q, c=s):
        return fn(ctx, _ptr(p), n, rmax, _ptr(a), _ptr(b), C.byref(c) if c is not None else None)
    bad = [dict(ctx=None), dict(p=None), dict(n=0), dict(n=-3), dict(a=None, b=None, c=None), dict(rmax=0.0), dict(rmax=-1.0),
           dict(rmax=float("inf")), dict(rmax=float("nan"))]
    for kw in bad:
        assert call(**kw) == ERR_ARG, kw
    assert call(n=1 << 31) == ERR_UNSUPPORTED
    if form == "tree":
        assert call(n=(0x7fffffff // 4) + 1) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (nb == POISON_NB).all() and (q == POISON_Q).all() and (s.n, s.nb_max, s.Q[0]) == (-5, -6, -7.0)
    assert call() == 0 and s.n == n     # a good call afterwards


# ---- state ---------------------------------------------------------------------------------------------------------------------------------------
def test_bond_order_leaves_a_kd_evaluation_and_the_run_as_they_were(oracle32):
    """an nbco_fmm_kdtree evaluation with tree_steps = 8, then a call of each form: nbco_kd_get_info is unchanged, and the following
    nbco_kd_potential and nbco_integrate_steps return the bits they return on a context that never made the calls"""
    import torch
    from coulomb_oscillators_amd import Engine, EVAL_FMM_KDTREE, INTEG_LEAPFROG
    n, p = 3000, 4
    buf, par = oracle32.init_reference(n), oracle32.params(n)
    d2 = dev(ball(257, 2))

    def drive(with_bonds):
        e = Engine(fmm_order=p, tree_steps=8, unsort=0)
        try:
            d, prm = torch.from_numpy(buf.copy()).cuda(), torch.from_numpy(par).cuda()
            e.compute_force(EVAL_FMM_KDTREE, d, n, prm)
            if with_bonds:
                info = bytes(e.kd_info())
                for form, dd, nn, rmax in (("exact", d, n, 0.002), ("tree", d, n, 0.002), ("exact2d", d2, 257, 0.7)):
                    nb, _, s = run(e, form, dd, nn, rmax)
                    assert s.bonds == nb.sum() > 0 and bytes(e.kd_info()) == info, form
            phi = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
            out = np.asarray(e.energy_kd(d, n, prm, phi)).tobytes() + phi.cpu().numpy().tobytes()
            e.integrate_steps(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, 5e-4, 10)
            return out + d.cpu().numpy().tobytes() + bytes(e.kd_info())
        finally:
            e.close()
    assert drive(True) == drive(False)


# ---- CLI -------------------------------------------------------------------------------------------------------------------------------------------
def test_cli_gpu_files_agree_with_the_host_twin(engine_lib, tmp_path):
    """`nbco3 -n 2048 -p 4 -iters 2 -steps 2 -bonds 0.0012`: snapshots byte-equal to a run without the flag; every bonds file has the nb
    of `nbco3 -cpu -bonds` on that snapshot byte for byte and its q^2 within the tolerance, in the snapshot's order; bonds.txt agrees"""
    subprocess.check_call(["make", "-C", HOST, "-s"])
    exe = os.path.join(HOST, "nbco3")
    n, rmax = 2048, 0.0012

    def nbco3(folder, *args):
        folder.mkdir()
        r = subprocess.run([exe, *[str(a) for a in args], "-o", str(folder)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        return folder
    common = ["-n", n, "-p", 4, "-iters", 2, "-steps", 2]
    plain, logged = nbco3(tmp_path / "plain", *common), nbco3(tmp_path / "logged", *common, "-bonds", rmax)
    snaps = sorted(f for f in os.listdir(logged) if f.startswith("out") and f.endswith(".bin"))
    assert snaps == ["out0_0.000500.bin", "out2_0.000500.bin"]
    assert not [f for f in os.listdir(plain) if f.startswith("bonds")]
    lines = (logged / "bonds.txt").read_text().splitlines()
    assert len(lines) == len(snaps)
    for k, name in enumerate(snaps):
        assert (plain / name).read_bytes() == (logged / name).read_bytes(), name
        # the host twin on this very snapshot: the program steps once before its first snapshot, and a step of 1e-30 moves no fp32 position
        twin = nbco3(tmp_path / ("twin%d" % k), "-cpu", "-cpu-threads", 4, "-iters", 0, "-ds", 1e-30, "-bonds", rmax, logged / name)
        assert (twin / "out0_0.000000.bin").read_bytes()[:12 * n] == (logged / name).read_bytes()[:12 * n]
        raw_g, raw_c = (logged / name.replace("out", "bonds")).read_bytes(), (twin / "bonds0_0.000000.bin").read_bytes()
        assert len(raw_g) == len(raw_c) == 20 * n
        assert raw_g[:4 * n] == raw_c[:4 * n], name
        nb = np.frombuffer(raw_g, dtype=np.int32, count=n)
        assert 0 < (nb == 0).sum() < n and 2 <= nb.max() <= 256
        qg, qc = np.frombuffer(raw_g, dtype=np.float64, offset=4 * n), np.frombuffer(raw_c, dtype=np.float64, offset=4 * n)
        assert np.abs(qg * qg - qc * qc).max() < BN.TOL2, name
        g, c = lines[k].split(), (twin / "bonds.txt").read_text().split()
        assert len(g) == 8 and int(g[0]) == (0, 2)[k] and g[1:4] == c[1:4]
        Qg, Qc = np.array([float(v) for v in g[6:8]]), np.array([float(v) for v in c[6:8]])
        assert np.abs(Qg * Qg - Qc * Qc).max() < BN.TOL2
        assert np.abs(np.array([float(v) for v in g[4:6]]) - np.array([float(v) for v in c[4:6]])).max() < BN.TOL_MEAN
