"""GPU tests of the crystalline-particle detection: nbco_bond_vectors / nbco_bond_solid and their tree forms (Engine.bond_vectors,
bond_vectors_tree, bond_solid, bond_solid_tree) against the numpy model of tests/solid_numpy.py.  The model of the solid pass is always
fed the records THE DEVICE WROTE, copied back: xi then depends on no rounding of a square root or a division, and xi, n_solid,
solid_bonds and xi_max compare as integers between the exact form, the tree form and the model.  q-bar^2 compares with bond_numpy.TOL2
(1e-11): given equal records the forms differ by the order of at most 257 terms of magnitude at most 1.02, below 1e-13.  The records
themselves compare with the model's sums of engine.bond_harmonics to 1e-12 (sums of at most 256 terms |Y| <= 1.02 in another order:
256 * 2^-53 * 1.02 = 3e-14, and one division).  The sizes are those at which the kernels take another path: the exact form's tiles are
256 wide, the walk's waves 64, its workgroups 1024, a leaf of more than 64 particles takes several staging rounds."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import bond_numpy as BN
import shapes3d
import solid_numpy as SN

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "coulomb_oscillators_amd", "host")
ERR_ARG, ERR_UNSUPPORTED = 2, 4
POISON_NB, POISON_XI, POISON_Q, POISON_V = -7777, -8888, -123.456, -654.321
FORMS = ("exact", "tree")
EXACT_N, TREE_N = (1, 2, 255, 257, 513), (63, 64, 65, 1025)
DMIN, XI_MIN = 0.5, 2        # on the balls: both outcomes of d6 > dmin and of xi >= xi_min occur (asserted where n allows)


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


@functools.lru_cache(maxsize=None)
def ball(n):
    """the Gaussian ball of tests/test_gpu_bond_order.py (fp32, unit width), read-only"""
    x = np.random.default_rng(100 + n).normal(size=(n, 3)).astype(np.float32)
    x.setflags(write=False)
    return x


def ball_rmax(n):
    return 0.5 if n > 600 else 1.0


def vectors(e, form, d, n, rmax, want_nb=True, want_vec=True):
    """one call of the vector pass into poisoned buffers -> (nb, vec) as numpy arrays (None for what was not asked for)"""
    import torch
    nb = torch.full((n,), POISON_NB, dtype=torch.int32, device="cuda") if want_nb else False
    vec = torch.full((n, SN.VEC), POISON_V, dtype=torch.float64, device="cuda") if want_vec else False
    (e.bond_vectors if form == "exact" else e.bond_vectors_tree)(d, n, rmax, nb=nb, vec=vec)
    torch.cuda.synchronize()
    return (nb.cpu().numpy().astype(np.int64) if want_nb else None), (vec.cpu().numpy() if want_vec else None)


def solid(e, form, d, n, rmax, dmin, xi_min, vec=None, want=(True, True, True, True)):
    """one call of the solid pass into poisoned buffers -> (nb, xi, qbar, summary); vec: a device tensor of records or None"""
    import torch
    nb = torch.full((n,), POISON_NB, dtype=torch.int32, device="cuda") if want[0] else False
    xi = torch.full((n,), POISON_XI, dtype=torch.int32, device="cuda") if want[1] else False
    qbar = torch.full((n, 2), POISON_Q, dtype=torch.float64, device="cuda") if want[2] else False
    _, _, _, s = (e.bond_solid if form == "exact" else e.bond_solid_tree)(d, n, rmax, dmin, xi_min, vec=vec, nb=nb, xi=xi, qbar=qbar, summary=want[3])
    torch.cuda.synchronize()
    return (nb.cpu().numpy().astype(np.int64) if want[0] else None), (xi.cpu().numpy().astype(np.int64) if want[1] else None), \
        (qbar.cpu().numpy() if want[2] else None), s


def as_bytes(got):
    return tuple(None if g is None else g.tobytes() if isinstance(g, np.ndarray) else bytes(g) for g in got)


def check(got, m, dmin, xi_min, what=""):
    """a call's (nb, xi, qbar, summary) against the model of the same records: integers exactly, squares within TOL2"""
    nb, xi, qbar, s = got
    n = len(m["nb"])
    assert np.array_equal(nb, m["nb"]), (what, "nb", np.flatnonzero(nb != m["nb"])[:8])
    assert np.array_equal(xi, m["xi"]), (what, "xi", np.flatnonzero(xi != m["xi"])[:8])
    assert np.isfinite(qbar).all() and not qbar[m["nb"] == 0].any(), what
    err = np.abs(qbar * qbar - m["qbar2"]).max()
    print(what, "max |d qbar2|", err)
    assert err < BN.TOL2, (what, err)
    assert (s.n, s.bonds, s.isolated, s.solid_bonds, s.n_solid, s.xi_max) == (n, m["bonds"], m["isolated"], m["solid_bonds"], m["n_solid"], m["xi_max"]), what
    assert (s.dmin, s.xi_min) == (dmin, xi_min) and s.solid_bonds % 2 == 0, what
    assert np.abs(np.array(s.qbar_mean[:]) - m["qbar_mean"]).max() < BN.TOL_MEAN, what


def both_forms_against_the_model(e, pos, rmax, dmin, xi_min, what, e_tree=None):
    """the records from the exact form of the device; the model of the solid pass over them; the exact and the tree form given them.
    Returns the model."""
    n = len(pos)
    d = dev(pos)
    nb, vec = vectors(e, "exact", d, n, rmax)
    assert nb.max() <= 256     # the tolerance's premise
    m = SN.solid(pos, rmax, dmin, xi_min, vec)
    assert np.array_equal(nb, m["nb"])
    dv = dev(vec)
    for form in FORMS:
        check(solid(e_tree if form == "tree" and e_tree else e, form, d, n, rmax, dmin, xi_min, dv), m, dmin, xi_min, (what, form))
    assert np.array_equal(d.cpu().numpy(), pos, equal_nan=True) and dv.cpu().numpy().tobytes() == vec.tobytes()   # the inputs are not written
    return m


# ---- the vector pass ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,n", [("exact", n) for n in EXACT_N] + [("tree", n) for n in TREE_N])
def test_vectors_on_a_ball(eng, form, n):
    """nb is bond_order's; a_l q^_lm is the model's S_lm / nb; q^ has unit norm where a_l > 0; an isolated particle has a record of zeros"""
    import torch
    pos, rmax = ball(n), ball_rmax(n)
    d = dev(pos)
    nb, vec = vectors(eng, form, d, n, rmax)
    ref_nb, ref_q, _ = (eng.bond_order if form == "exact" else eng.bond_order_tree)(d, n, rmax, summary=False)
    torch.cuda.synchronize()
    assert np.array_equal(nb, ref_nb.cpu().numpy()) and nb.max() <= 256
    mnb, S = SN.sums(pos, rmax)
    assert np.array_equal(nb, mnb)
    assert np.isfinite(vec).all() and not vec[nb == 0].any()
    if n >= 255:
        assert (nb == 0).any() and nb.max() >= 20
    linked = nb > 0
    for lo, hi, a, Q, col in ((0, 9, 22, SN.Q4, 0), (9, 22, 23, SN.Q6, 1)):
        assert np.array_equal(vec[:, a] > 0, linked)     # (no sum of harmonics of these inputs vanishes)
        err = np.abs(vec[linked, lo:hi] * vec[linked, a:a + 1] - S[linked, lo:hi] / nb[linked, None]).max() if linked.any() else 0.0
        norm = np.abs(np.sqrt((vec[linked, lo:hi] ** 2).sum(axis=1)) - 1.0).max() if linked.any() else 0.0
        print(form, n, "l", 4 + 2 * col, "max |d a q^|", err, "max |norm - 1|", norm)
        assert err < 1e-12 and norm < 1e-14
        # q_l = sqrt(4 pi / (2l+1)) a_l is bond_order's q_l
        assert np.abs(Q * vec[:, a] ** 2 - ref_q.cpu().numpy()[:, col] ** 2).max() < BN.TOL2
    assert np.array_equal(d.cpu().numpy(), pos)


# ---- the solid pass against the model of the device's records ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sorted(EXACT_N + TREE_N))
def test_solid_pass_on_a_ball(eng, n):
    m = both_forms_against_the_model(eng, ball(n), ball_rmax(n), DMIN, XI_MIN, ("ball", n))
    if n >= 255:
        assert 0 < m["solid_bonds"] < m["bonds"] and 0 < m["n_solid"] < n and (m["nb"] == 0).any()


@pytest.mark.parametrize("name", ["sc", "ball"])
def test_solid_pass_with_leaves_of_several_staging_rounds(eng, engine_lib, name):
    """tree_L = 3 leaves about 275 particles per leaf of the sc lattice (five staging rounds of 64) and 128 of ball(1025) (two)"""
    from coulomb_oscillators_amd import Engine
    pos, rmax = (BN.sc()[0], math.sqrt(1.5)) if name == "sc" else (ball(1025), 0.5)
    e = Engine(tree_L=3)
    try:
        m = both_forms_against_the_model(eng, pos, rmax, 0.7 if name == "sc" else DMIN, 6 if name == "sc" else XI_MIN, (name, "tree_L=3"), e_tree=e)
        # the combined call on that tree: the records of its own walk, in tree order
        got = solid(e, "tree", dev(pos), len(pos), rmax, 0.7, 6)
    finally:
        e.close()
    if name == "sc":
        assert m["n_solid"] == 1331 and got[3].n_solid == 1331 and got[1].max() == 6     # the bulk of 11^3, every bond of it solid


@pytest.mark.parametrize("shape", shapes3d.SHAPES)
def test_solid_pass_on_every_shape(eng, oracle32, shape):
    """flat, collinear, tied, duplicated, stretched and late-run inputs at the sizes and radii of the bond-order shape test"""
    pos, rmax, ref, _, _ = shapes3d.bond_model(oracle32, shape)
    m = both_forms_against_the_model(eng, pos, rmax, DMIN, XI_MIN, shape)
    assert np.array_equal(m["nb"], ref["nb"])


def test_bcc_block_in_a_gas(eng):
    """1024 lattice points surrounded by 1024 gas points at dmin = 0.7, xi_min = 7: n_solid is the model's, and the solid particles
    are lattice points"""
    pos, lattice = SN.bcc_in_gas()
    rmax = math.sqrt(3.5)
    m = both_forms_against_the_model(eng, pos, rmax, 0.7, 7, "bcc in gas")
    assert 600 < m["n_solid"] <= 1024 and not (m["xi"][~lattice] >= 7).any()
    for form in FORMS:     # and with the records of the call's own
        nb, xi, _, s = solid(eng, form, dev(pos), len(pos), rmax, 0.7, 7)
        assert s.n_solid == m["n_solid"] == (xi >= 7).sum() and np.array_equal(xi, m["xi"]), form


def test_a_gas_has_no_solid_particle(eng):
    pos, rmax = SN.gas()
    m = both_forms_against_the_model(eng, pos, rmax, 0.7, 7, "gas")
    assert m["n_solid"] == 0 and m["xi_max"] == 3
    for form in FORMS:
        assert solid(eng, form, dev(pos), len(pos), rmax, 0.7, 7)[3].n_solid == 0


# ---- ideal lattices ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name,rmax2,coord,q4,q6", BN.IDEAL)
def test_ideal_lattice_values(eng, form, name, rmax2, coord, q4, q6):
    """the central particle and its neighbours have the same environment: every bond of the centre is solid and its q-bar_l is its q_l"""
    pos, centre = BN.LATTICES[name]()
    nb, xi, qbar, s = solid(eng, form, dev(pos), len(pos), math.sqrt(rmax2), 0.7, coord)
    assert nb[centre] == xi[centre] == coord and s.xi_max == coord and s.n_solid > 0
    assert abs(qbar[centre, 1] - q6) < 1e-7 and abs(qbar[centre, 0] - q4) < 1e-7


# ---- one call or two ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_combined_call_returns_the_bytes_of_the_two_stage_call(eng, form):
    """vec = None: the records of a pass 1 of the call's own (in the tree form on the same tree, in tree order) -- the bytes of
    bond_vectors followed by bond_solid in that form; and a second call returns the same bytes"""
    n, rmax = 1025, 0.5
    d = dev(ball(n))
    _, vec = vectors(eng, form, d, n, rmax)
    two = solid(eng, form, d, n, rmax, DMIN, XI_MIN, dev(vec))
    one = solid(eng, form, d, n, rmax, DMIN, XI_MIN)
    assert as_bytes(one) == as_bytes(two)
    assert as_bytes(solid(eng, form, d, n, rmax, DMIN, XI_MIN)) == as_bytes(one)
    assert as_bytes(solid(eng, form, d, n, rmax, DMIN, XI_MIN, dev(vec))) == as_bytes(two)
    assert vectors(eng, form, d, n, rmax)[1].tobytes() == vec.tobytes()
    assert one[3].solid_bonds > 0


# ---- edge cases -----------------------------------------------------------------------------------------------------------------------------
def test_two_coincident_particles_inside_a_lattice(eng):
    """a duplicate of a bulk point: the twins are not neighbours of each other, have the same record, and everybody near them counts both"""
    pos, centre = BN.fcc()
    pos = np.concatenate([pos, pos[centre:centre + 1]])
    m = both_forms_against_the_model(eng, pos, math.sqrt(3.0), 0.7, 12, "fcc twin")
    assert m["nb"][centre] == m["nb"][-1] == 12 and m["xi"][centre] == m["xi"][-1] and m["nb"].max() == 13


def test_a_nan_coordinate_is_isolated(eng):
    n, rmax = 513, 1.0
    pos = ball(n).copy()
    pos[300, 1] = np.nan
    d = dev(pos)
    nb, vec = vectors(eng, "exact", d, n, rmax)
    assert nb[300] == 0 and not vec[300].any() and np.isfinite(vec).all()
    m = SN.solid(pos, rmax, DMIN, XI_MIN, vec)
    got = solid(eng, "exact", d, n, rmax, DMIN, XI_MIN, dev(vec))
    check(got, m, DMIN, XI_MIN, "nan")
    assert got[0][300] == 0 and got[1][300] == 0 and not got[2][300].any()
    assert as_bytes(solid(eng, "exact", d, n, rmax, DMIN, XI_MIN)) == as_bytes(got)


@pytest.mark.parametrize("form", FORMS)
def test_rmax_below_the_smallest_spacing(eng, form):
    pos, _ = BN.sc(3)
    n = len(pos)
    d = dev(pos)
    nb, vec = vectors(eng, form, d, n, 0.999)
    assert not nb.any() and not vec.any()
    nb, xi, qbar, s = solid(eng, form, d, n, 0.999, -2.0, 0)
    assert not nb.any() and not xi.any() and not qbar.any()
    assert (s.n, s.bonds, s.isolated, s.solid_bonds, s.n_solid, s.xi_max) == (n, 0, n, 0, n, 0) and s.qbar_mean[:] == [0.0, 0.0]


@pytest.mark.parametrize("form", FORMS)
def test_thresholds_that_take_every_bond_and_none(eng, form):
    n, rmax = 1025, 0.5
    d = dev(ball(n))
    nb, xi, _, s = solid(eng, form, d, n, rmax, -2.0, 0)
    assert np.array_equal(xi, nb) and s.solid_bonds == s.bonds > 0 and s.n_solid == n and s.xi_max == nb.max()
    nb2, xi, _, s = solid(eng, form, d, n, rmax, 2.0, 1)
    assert np.array_equal(nb2, nb) and not xi.any() and (s.solid_bonds, s.n_solid, s.xi_max) == (0, 0, 0)


# ---- outputs and refusals --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_output_combinations(eng, form):
    """each NULL combination of the outputs returns what all together return; None allocates"""
    import itertools
    n, rmax = 1025, 0.5
    d = dev(ball(n))
    full = solid(eng, form, d, n, rmax, DMIN, XI_MIN)
    assert (full[0] != POISON_NB).all() and (full[1] != POISON_XI).all() and (full[2] != POISON_Q).all()     # fully overwritten
    for want in itertools.product((True, False), repeat=4):
        if not any(want) or all(want):
            continue
        got = solid(eng, form, d, n, rmax, DMIN, XI_MIN, want=want)
        for g, f, w in zip(as_bytes(got), as_bytes(full), want):
            assert (g is None) == (not w) and (g is None or g == f), want
    made = (eng.bond_solid if form == "exact" else eng.bond_solid_tree)(d, n, rmax, DMIN, XI_MIN)
    assert made[0].cpu().numpy().astype(np.int64).tobytes() == full[0].tobytes() and made[1].cpu().numpy().astype(np.int64).tobytes() == full[1].tobytes()
    assert made[2].cpu().numpy().tobytes() == full[2].tobytes() and bytes(made[3]) == bytes(full[3])
    nb, vec = vectors(eng, form, d, n, rmax)
    assert vectors(eng, form, d, n, rmax, want_vec=False)[0].tobytes() == nb.tobytes()
    assert vectors(eng, form, d, n, rmax, want_nb=False)[1].tobytes() == vec.tobytes()
    made_nb, made_vec = (eng.bond_vectors if form == "exact" else eng.bond_vectors_tree)(d, n, rmax)
    assert made_nb.cpu().numpy().astype(np.int64).tobytes() == nb.tobytes() and made_vec.cpu().numpy().tobytes() == vec.tobytes()


@pytest.mark.parametrize("form", FORMS)
def test_refusals_leave_the_outputs_alone(eng, form):
    import ctypes as C
    import torch
    from coulomb_oscillators_amd import SolidSummary
    from coulomb_oscillators_amd.engine import _ptr
    n, rmax = 255, 1.0
    d = dev(ball(n))
    nb = torch.full((n,), POISON_NB, dtype=torch.int32, device="cuda")
    xi = torch.full((n,), POISON_XI, dtype=torch.int32, device="cuda")
    qbar = torch.full((n, 2), POISON_Q, dtype=torch.float64, device="cuda")
    vec = torch.full((n, SN.VEC), POISON_V, dtype=torch.float64, device="cuda")
    s = SolidSummary()
    s.n, s.xi_max, s.dmin = -5, -6, -7.0
    fs = getattr(eng.lib, "nbco_bond_solid" + ("_tree" if form == "tree" else ""))
    fv = getattr(eng.lib, "nbco_bond_vectors" + ("_tree" if form == "tree" else ""))

    def call(ctx=eng.ctx, p=d, n=n, rmax=rmax, v=None, dmin=0.7, xi_min=7, a=nb, b=xi, q=qbar, c=s):
        return fs(ctx, _ptr(p), n, rmax, _ptr(v), dmin, xi_min, _ptr(a), _ptr(b), _ptr(q), C.byref(c) if c is not None else None)

    def call_v(ctx=eng.ctx, p=d, n=n, rmax=rmax, a=nb, v=vec):
        return fv(ctx, _ptr(p), n, rmax, _ptr(a), _ptr(v))
    bad = [dict(ctx=None), dict(p=None), dict(n=0), dict(n=-3), dict(rmax=0.0), dict(rmax=-1.0), dict(rmax=float("inf")), dict(rmax=float("nan"))]
    for kw in bad + [dict(a=None, b=None, q=None, c=None), dict(dmin=float("nan")), dict(dmin=float("inf")), dict(dmin=float("-inf")), dict(xi_min=-1)]:
        assert call(**kw) == ERR_ARG, kw
        assert call(v=vec, **kw) == ERR_ARG, kw
    for kw in bad + [dict(a=None, v=None)]:
        assert call_v(**kw) == ERR_ARG, kw
    assert call(n=1 << 31) == ERR_UNSUPPORTED and call_v(n=1 << 31) == ERR_UNSUPPORTED
    if form == "tree":
        assert call(n=(0x7fffffff // 4) + 1) == ERR_UNSUPPORTED and call_v(n=(0x7fffffff // 4) + 1) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (nb == POISON_NB).all() and (xi == POISON_XI).all() and (qbar == POISON_Q).all() and (vec == POISON_V).all()
    assert (s.n, s.xi_max, s.dmin) == (-5, -6, -7.0)
    assert call_v() == 0 and call(v=vec) == 0 and (s.n, s.dmin, s.xi_min) == (n, 0.7, 7)     # good calls afterwards


def test_tree_forms_refuse_leaves_the_build_cannot_hold(engine_lib):
    """tree_L = 2 at n = 20000 asks for 5000 particles per leaf: what nbco_bond_order_tree refuses, before any launch"""
    import torch
    from coulomb_oscillators_amd import Engine, EngineError
    n = 20000
    d = dev(np.random.default_rng(3).normal(size=(n, 3)).astype(np.float32))
    e = Engine(tree_L=2)
    try:
        xi = torch.full((n,), POISON_XI, dtype=torch.int32, device="cuda")
        vec = torch.full((n, SN.VEC), POISON_V, dtype=torch.float64, device="cuda")
        for fn in (lambda: e.bond_solid_tree(d, n, 0.05, 0.7, 7, nb=False, xi=xi, qbar=False), lambda: e.bond_vectors_tree(d, n, 0.05, nb=False, vec=vec)):
            with pytest.raises(EngineError) as err:
                fn()
            assert err.value.status == ERR_UNSUPPORTED and "per leaf" in str(err.value)
        torch.cuda.synchronize()
        assert (xi == POISON_XI).all() and (vec == POISON_V).all()
    finally:
        e.close()


# ---- state ---------------------------------------------------------------------------------------------------------------------------------------
def test_solid_calls_leave_a_kd_evaluation_and_the_run_as_they_were(oracle32):
    """an nbco_fmm_kdtree evaluation with tree_steps = 8, then a call of each of the four entry points: nbco_kd_get_info is unchanged, and
    the following nbco_kd_potential, nbco_kd_probe and nbco_integrate_steps return the bits they return on a context that never made them"""
    import torch
    from coulomb_oscillators_amd import Engine, EVAL_FMM_KDTREE, INTEG_LEAPFROG
    n, p, rmax = 3000, 4, 0.002
    buf, par = oracle32.init_reference(n), oracle32.params(n)
    probes = np.ascontiguousarray(buf[0][:16] * np.float32(1.01))

    def drive(with_calls):
        e = Engine(fmm_order=p, tree_steps=8, unsort=0)
        try:
            d, prm, t = torch.from_numpy(buf.copy()).cuda(), torch.from_numpy(par).cuda(), dev(probes)
            e.compute_force(EVAL_FMM_KDTREE, d, n, prm)
            if with_calls:
                info = bytes(e.kd_info())
                for form in FORMS:
                    nb, vec = vectors(e, form, d, n, rmax)
                    assert nb.sum() > 0 and bytes(e.kd_info()) == info, form
                    for v in (None, dev(vec)):
                        got = solid(e, form, d, n, rmax, 0.3, 2, v)
                        assert got[3].bonds == nb.sum() and got[3].solid_bonds > 0 and bytes(e.kd_info()) == info, form
            phi = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
            out = np.asarray(e.energy_kd(d, n, prm, phi)).tobytes() + phi.cpu().numpy().tobytes()
            a = torch.full((len(probes), 3), float("nan"), dtype=torch.float64, device="cuda")
            psi = torch.full((len(probes),), float("nan"), dtype=torch.float64, device="cuda")
            e.probe_kd(t, len(probes), prm, a=a, psi=psi)
            out += a.cpu().numpy().tobytes() + psi.cpu().numpy().tobytes()
            e.integrate_steps(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, 5e-4, 10)
            return out + d.cpu().numpy().tobytes() + bytes(e.kd_info())
        finally:
            e.close()
    assert drive(True) == drive(False)


# ---- CLI -------------------------------------------------------------------------------------------------------------------------------------------
def test_cli_gpu_files_agree_with_the_host_twin(engine_lib, tmp_path):
    """`nbco3 -n 2048 -p 4 -iters 2 -steps 2 -solid 0.0012 0.3 2`: snapshots byte-equal to a run without the flag; every solid file has the
    nb and xi of `nbco3 -cpu -solid` on that snapshot byte for byte and its q-bar^2 within the tolerance; solid.txt agrees.  The records of
    the two differ by rounding, so the model asserts first that no bond's d6 is within 1e-9 of dmin."""
    subprocess.check_call(["make", "-C", HOST, "-s"])
    exe = os.path.join(HOST, "nbco3")
    n, rmax, dmin, xi_min = 2048, 0.0012, 0.3, 2

    def nbco3(folder, *args):
        folder.mkdir()
        r = subprocess.run([exe, *[str(a) for a in args], "-o", str(folder)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        return folder
    common = ["-n", n, "-p", 4, "-iters", 2, "-steps", 2]
    plain, logged = nbco3(tmp_path / "plain", *common), nbco3(tmp_path / "logged", *common, "-solid", rmax, dmin, xi_min)
    snaps = sorted(f for f in os.listdir(logged) if f.startswith("out") and f.endswith(".bin"))
    assert snaps == ["out0_0.000500.bin", "out2_0.000500.bin"]
    assert not [f for f in os.listdir(plain) if f.startswith("solid")]
    lines = (logged / "solid.txt").read_text().splitlines()
    assert len(lines) == len(snaps)
    for k, name in enumerate(snaps):
        assert (plain / name).read_bytes() == (logged / name).read_bytes(), name
        pos = np.frombuffer((logged / name).read_bytes(), dtype=np.float32, count=3 * n).reshape(n, 3)
        m = SN.solid(pos, rmax, dmin, xi_min)
        assert np.abs(m["d6"] - dmin).min() > 1e-9 and 0 < m["n_solid"] < n
        # the host twin on this very snapshot: the program steps once before its first snapshot, and a step of 1e-30 moves no fp32 position
        twin = nbco3(tmp_path / ("twin%d" % k), "-cpu", "-cpu-threads", 4, "-iters", 0, "-ds", 1e-30, "-solid", rmax, dmin, xi_min, logged / name)
        assert (twin / "out0_0.000000.bin").read_bytes()[:12 * n] == (logged / name).read_bytes()[:12 * n]
        raw_g, raw_c = (logged / name.replace("out", "solid")).read_bytes(), (twin / "solid0_0.000000.bin").read_bytes()
        assert len(raw_g) == len(raw_c) == 24 * n
        assert raw_g[:8 * n] == raw_c[:8 * n], name
        nb, xi = np.frombuffer(raw_g, dtype=np.int32, count=n), np.frombuffer(raw_g, dtype=np.int32, count=n, offset=4 * n)
        assert np.array_equal(nb, m["nb"]) and np.array_equal(xi, m["xi"]) and 0 < (nb == 0).sum() < n
        qg, qc = np.frombuffer(raw_g, dtype=np.float64, offset=8 * n), np.frombuffer(raw_c, dtype=np.float64, offset=8 * n)
        assert np.abs(qg * qg - qc * qc).max() < BN.TOL2, name
        g, c = lines[k].split(), (twin / "solid.txt").read_text().split()
        assert len(g) == 6 and int(g[0]) == (0, 2)[k] and g[1:4] == c[1:4] == [str(m["n_solid"]), str(m["solid_bonds"]), str(m["xi_max"])]
        assert np.abs(np.array([float(v) for v in g[4:6]]) - np.array([float(v) for v in c[4:6]])).max() < BN.TOL_MEAN
