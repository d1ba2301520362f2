"""Every diagnostic on ONE long-lived context, as nbco3 and nbco drive them at a snapshot (host/nbco3.cpp: nbco_aperture_apply, so that
n shrinks, the tree is dropped and the order map compacted; nbco_energy_tree; nbco_beam_moments; nbco_slice_moments; nbco_probe_tree;
nbco_pair_hist_tree; nbco_bond_order_tree; nbco_bond_order; nbco_structure_factor; nbco_integrate_steps again), where the modules of
these features give each its own context at one particle count.  Four of the calls share one private child context, which is created
once and then sees another n at every snapshot; all scratch lives in buffers that only grow, so after a larger call the tail of every
table holds the larger call's data.  The calls that keep a caller's buffers across snapshots (trajectories, mode series and their
correlations) are in tests/test_gpu_snapshot_series.py, whose docstring says where each scratch buffer meets a smaller user.

Four bars, used throughout.  No tolerance is introduced here: each one is imported from, or cites, the module that derived it.

(M) the model.  The numpy references under tests/ applied to the state read back from the device right before the call.  Integer for
    integer and byte for byte where the feature's module compares that way: the aperture's state, loss record and rows
    (test_gpu_aperture), hist (test_gpu_beam_diag.check_hist), pair_hist* counts and nn2 (test_gpu_pair_hist.same).  Elsewhere the
    module's derived bound: test_gpu_beam_diag.check_moments, test_gpu_slice_moments.check_slices, test_gpu_energy3d.ENERGY_TOL with the
    1e-6 on the kinetic and elastic terms of test_energy_kd_against_fp64_direct_energy, the 1e-12 of
    test_probe_is_the_exact_sum_at_every_launch_shape, the 1e-10 of the restatements on the device tree
    (test_psi_against_the_restatement_on_the_device_tree, test_probe_kd_against_the_restatement_on_the_device_tree), and for 2-D
    test_energy_2d_against_exact_sum, test_energy_fmm_2d_matches_restatement, test_gpu_probe2d._check_exact / _check_fmm.  The bond
    order through test_gpu_bond_order.check (nb and the summary's integers exactly, the squares within bond_numpy.TOL2, whose premise
    nb <= 256 is asserted of every model), the structure factor as test_gpu_structure_factor.check (sk_numpy.bound, n_used = n and
    rho at k = 0 exactly n).
(F) fresh-context equality.  A context created for that call alone returns the same bytes for the same input and options; if it
    refuses, the long-lived one refuses with the same status.  energy_tree is also held to test_gpu_energy3d.fresh_energy_kd.
(R) the run does not notice.  A run with the diagnostic calls equals the run without them, bit for bit: the state, every field of
    kd_info before each snapshot (rebuilt included), kd_array("order"), n per snapshot and the loss records.
Preconditions: assertions computed on the CPU before the GPU is touched (tests/test_snapshots_host.py runs them without one).

Every output buffer is pre-filled with garbage before the call, as the features' modules do.

What is not held to (F), by design, as in test_gpu_context_reuse: energy_kd / energy_fmm / probe_kd behind a compute_force that REUSED
the tree (the middle of a tree_steps = 8 schedule: a fresh context has no such tree).  They are held to (M) there -- the restatements
on the device tree, and the exact energy -- and to (F) wherever that compute_force rebuilt.  That compute_force is an evaluation of
the run, so the run without the diagnostics makes it too."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import aperture_numpy as AP
import beam_numpy as BN
import bond_numpy as BO
import energy2d_numpy as E2
import energy3d_numpy as e3
import fmm2d_numpy as F2
import pairstat_numpy as PN
import probe2d_numpy as PR2
import probe3d_numpy as p3
import sk_numpy as SK
import slice_numpy as SN
import test_gpu_aperture as APT
import test_gpu_beam_diag as BD
import test_gpu_bond_order as BOT
import test_gpu_context_reuse as CR
import test_gpu_energy3d as EN3
import test_gpu_pair_hist as PH
import test_gpu_probe2d as PB2
import test_gpu_probe3d as PB3
import test_gpu_slice_moments as SL
import test_gpu_structure_factor as SFT

pytestmark = pytest.mark.gpu

X, Y, Z, VX, VY, VZ = range(6)
GARBAGE = BD.GARBAGE
_models = {}      # (name, digest of the state) -> what a numpy reference says of it: evaluated once, shared by the tests of this module


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def model(name, key, make):
    if (name, key) not in _models:
        _models[(name, key)] = make()
    return _models[(name, key)]


def digest(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


class Inputs:
    """one state on the device and on the host, with the probes and the windows of the calls"""


REFUSED = "refused"


def refusal(fn, *args):
    """fn(*args), or (REFUSED, status) when the library refuses the call"""
    from coulomb_oscillators_amd import EngineError
    try:
        return fn(*args)
    except EngineError as err:
        return dict(cmp=(REFUSED, err.status))


def assert_same_result(live, fresh, what):
    """bar (F) on the `cmp` entries: tuples of numpy arrays, byte strings and integers"""
    a, b = live["cmp"], fresh["cmp"]
    assert len(a) == len(b), what
    for k, (u, v) in enumerate(zip(a, b)):
        if isinstance(u, np.ndarray):
            assert isinstance(v, np.ndarray) and u.shape == v.shape and u.dtype == v.dtype and u.tobytes() == v.tobytes(), \
                "%s: output %d differs from the fresh context's" % (what, k)
        else:
            assert u == v, "%s: output %d: %r != %r (fresh context)" % (what, k, u, v)


def moments_call(e, fn, d, n):
    """one nbco_*beam_moments call into a structure pre-filled with 0x5a bytes"""
    from coulomb_oscillators_amd import Moments
    out = Moments()
    C.memset(C.byref(out), 0x5a, C.sizeof(out))
    e._chk(fn(e.ctx, C.c_void_p(d.data_ptr()), n, C.byref(out)))
    return dict(cmp=(bytes(out),), m=out)


def slices_call(e, fn, d, n, axis):
    """one nbco_*slice_moments call into records pre-filled with 0x5a bytes and a garbage n_outside"""
    from coulomb_oscillators_amd import HistAxis, Moments
    recs = (Moments * axis[1])()
    C.memset(recs, 0x5a, C.sizeof(recs))
    outside = C.c_longlong(GARBAGE)
    ax = HistAxis(int(axis[0]), int(axis[1]), float(axis[2]), float(axis[3]))
    e._chk(fn(e.ctx, C.c_void_p(d.data_ptr()), n, C.byref(ax), recs, C.byref(outside)))
    return dict(cmp=(bytes(recs), outside.value), recs=recs, outside=outside.value)


def energy_call(e, fn, d, n, prm):
    """one energy call with out3 pre-filled with NaN and phi with NaN"""
    import torch
    out = (C.c_double * 3)(float("nan"), float("nan"), float("nan"))
    phi = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    e._chk(fn(e.ctx, C.c_void_p(d.data_ptr()), n, C.c_void_p(prm.data_ptr()), out, C.c_void_p(phi.data_ptr())))
    out, psi = np.array(out[:]), phi.cpu().numpy()
    assert np.isfinite(out).all() and np.isfinite(psi).all()
    return dict(cmp=(out, psi), out=out, psi=psi)


def hist_call(fn, d, n, axes):
    import torch
    B = int(np.prod([a[1] for a in axes]))
    counts = torch.full((B + 1,), GARBAGE, dtype=torch.int64, device="cuda")
    fn(d, n, axes, counts)
    return dict(cmp=(counts.cpu().numpy(),))


def aperture_call(e, dim, d, n, half):
    """the aperture on a COPY of the state, with a record of n rows and APT.GUARD rows behind it"""
    from coulomb_oscillators_amd import AP_ELLIPSOID
    copy = d.clone()
    lost, rows = APT.lost_buffers(dim, n)
    kept = APT.fns(e, dim)[1](copy, n, AP_ELLIPSOID, half, lost=lost[:n * 2 * dim], lost_row=rows[:n])
    return dict(cmp=(kept, copy.cpu().numpy()[:3 * dim * kept], lost.cpu().numpy(), rows.cpu().numpy()))


def bond_call(e, form, d, n, rmax):
    """one bond-order call through test_gpu_bond_order.run, into poisoned nb and q"""
    nb, q, s = BOT.run(e, form, d, n, rmax)
    return dict(cmp=(nb, q, bytes(s)), raw=(nb, q, s))


def sk_call(fn, d, n, dim, h, kstep):
    """one structure-factor call into a rho pre-filled with test_gpu_structure_factor.POISON, all of which must be overwritten"""
    import torch
    rho = torch.full((SK.count(h[:dim]),), complex(SFT.POISON, SFT.POISON), dtype=torch.complex128, device="cuda")
    _, used = fn(d, n, h, kstep, rho=rho)
    got = rho.cpu().numpy()
    assert (got.real != SFT.POISON).all() and (got.imag != SFT.POISON).all()
    return dict(cmp=(got, used))


def check_bonds(pos, key, rmax, got, what):
    """bar (M) of the bond order: test_gpu_bond_order.check against bond_numpy.bond_order, whose TOL2 presumes nb <= 256"""
    m = model("bonds", key + repr(float(rmax)), lambda: BO.bond_order(pos, rmax))
    assert m["nb_max"] <= 256, (what, m["nb_max"])
    BOT.check(got["raw"], m, what)


def check_sk(pos, key, h, kstep, got, what, only=None):
    """bar (M) of the structure factor, as test_gpu_structure_factor.check: within sk_numpy.bound of the long double model (over the
    flat indices `only` where given, and over every 7th wave vector, the zero vector and the last one where the grid times n is above
    SK_MODEL_WORK), every particle counted, rho at k = 0 exactly n"""
    n, dim = pos.shape
    h, kstep = tuple(h[:dim]), tuple(kstep[:dim])
    rho, used = got["cmp"]
    K = SK.count(h)
    if only is None and K * n > SK_MODEL_WORK:     # (F) compares every byte; the model's cost is kept to a few seconds
        only = np.unique(np.concatenate([np.arange(0, K, 7), [SK.index(h, 0, 0, 0), K - 1]]))
    re, im, want_used = model("sk", key + repr((h, kstep, only is not None)), lambda: SK.structure_factor(pos, h, kstep, only=only))
    err, lim = SK.error(rho if only is None else rho[only], re, im), SK.bound(n, h)
    print("%s: h %s error %.3g, bound %.3g (fraction %.3g)" % (what, h, err, lim, err / lim))
    assert used == want_used == n, (what, used, want_used)
    assert err <= lim, (what, err, lim)
    assert rho[SK.index(h, 0, 0, 0)] == complex(n, 0.0), what


def check_aperture(dim, host, half, got, what):
    """bar (M) of the aperture: bytes (test_gpu_aperture.check_case)"""
    want_state, want_lost, want_rows = AP.apply(host, AP.ELLIPSOID, half)
    kept, state, lost, rows = got["cmp"]
    k = len(want_rows)
    assert kept == host.shape[1] - k, what
    assert APT.same(state.reshape(3, kept, dim), want_state), what + ": the compacted state"
    lost = lost.reshape(-1, 2 * dim)
    assert APT.same(lost[:k], want_lost) and APT.same(rows[:k], want_rows), what + ": the loss record"
    assert (lost[k:] == -7.25).all() and (rows[k:] == -77).all(), what + ": written behind the record"
    return kept


def check_hist(host, dim, axes, got, what):
    h = got["cmp"][0]
    want = BN.hist(host[:2], dim, axes)
    assert h.sum() == host.shape[1] and np.array_equal(h, want), (what, axes, np.flatnonzero(h != want)[:8])


# ---- 3-D: the calls ------------------------------------------------------------------------------------------------------------------
N0 = 8193                              # one over 8 x 1024 slice chunks and over 8 pair-walk workgroups; 33 aperture workgroup counts
OPTS_A = dict(fmm_order=4, unsort=0, tree_steps=8, m2l_first=1, track_order=1)     # what nbco3 runs
KS = (3.0, 3.0, 2.5, 2.0, 1.5)
RMS = (0.003, 0.001, 0.01)             # the rms radii of the reference ball (test_gpu_aperture.HALF is 2.5 of them)
STEPS, DT = 3, APT.DT
FORCE_AT = (1, 3)                      # snapshots 2 and 4: compute_force, then energy_kd, energy_fmm, probe_kd
PAIR_BINS, PAIR_RMAX = 64, PH.RMAX[1]
AX_Z = (Z, 64, -3 * RMS[2], 3 * RMS[2])
AX_SLICE = (Z, 16, -3 * RMS[2], 3 * RMS[2])      # +-3 rms of the INITIAL ball: late snapshots have empty outer slices
EPS2 = PB3.EPS2
# the bond radius of the 3-D states: test_snapshots_host.py asserts from the model that it keeps nb <= 256, the premise of
# bond_numpy.TOL2, and gives at least half of the particles a bond at every snapshot (43 at the most, 90 % at the least)
BOND_RMAX = 0.0008
SK_KSTEP = (900.0, 900.0, 900.0)       # of the state tests of test_gpu_structure_factor / test_gpu_modes on the reference ball
SK_MODEL_WORK = 1 << 22                # wave vectors x particles up to which the long double model is evaluated on the whole grid
SK_H = (4, 4, 4)                       # the grid of the snapshot sequence; the size walk takes its grids from GRIDS_B


def child_opts(opts):
    """the expansion and tree options the private child context takes from its parent (nbco_api.hip, private_child)"""
    return {k: v for k, v in opts.items() if k in ("fmm_order", "m2l_first", "tree_radius", "eps2", "far_fp64", "dens_inhom", "tree_L")}


def axes_xvx(o):
    """the 32 x 32 map over (x, vx): +-3 standard deviations of the initial ball"""
    buf = CR.state(o, N0)
    return [(X, 32, -3 * RMS[0], 3 * RMS[0]), (VX, 32, -3 * float(buf[1][:, 0].std()), 3 * float(buf[1][:, 0].std()))]


def inputs3d(o, d, n, prm, par, probes_host):
    x = Inputs()
    x.d, x.n, x.prm, x.par = d, n, prm, par
    x.host = d.cpu().numpy()[:9 * n].reshape(3, n, 3).copy()
    x.key = digest(x.host)
    x.t_host = probes_host
    x.t, x.m = dev(probes_host), len(probes_host)
    x.xvx = axes_xvx(o)
    x.sk_h = SK_H
    return x


def pair3(form):
    def call(e, x):
        return dict(cmp=PH.run(e, form, x.d, x.n, PAIR_BINS, PAIR_RMAX))
    return call


def probe3(name):
    def call(e, x):
        return dict(cmp=PB3.run(getattr(e, name), x.d, x.n, x.t, x.m, x.prm))
    return call


CALLS3D = {       # in the order of a snapshot of nbco3
    "energy_tree": lambda e, x: energy_call(e, e.lib.nbco_energy_tree, x.d, x.n, x.prm),
    "beam_moments": lambda e, x: moments_call(e, e.lib.nbco_beam_moments, x.d, x.n),
    "hist_z": lambda e, x: hist_call(e.hist, x.d, x.n, [AX_Z]),
    "hist_xvx": lambda e, x: hist_call(e.hist, x.d, x.n, x.xvx),
    "slice_moments": lambda e, x: slices_call(e, e.lib.nbco_slice_moments, x.d, x.n, AX_SLICE),
    "probe_tree": probe3("probe_tree"),
    "probe": probe3("probe"),
    "pair_hist_tree": pair3("tree"),
    "pair_hist": pair3("exact"),
    "bond_order_tree": lambda e, x: bond_call(e, "tree", x.d, x.n, BOND_RMAX),
    "bond_order": lambda e, x: bond_call(e, "exact", x.d, x.n, BOND_RMAX),
    "structure_factor": lambda e, x: sk_call(e.structure_factor, x.d, x.n, 3, x.sk_h, SK_KSTEP),
}
# the size walk: the 2-D form on a cloud of its own (x.cloud2, x.sk_h2) right before the 3-D form, so that the two alternate on one sk_part
WALK3D = {}
for _name, _fn in CALLS3D.items():
    if _name == "structure_factor":
        WALK3D["structure_factor_2d"] = lambda e, x: sk_call(e.structure_factor_2d, x.d2, len(x.cloud2), 2, x.sk_h2, SFT.K3)
    WALK3D[_name] = _fn
WALK3D["aperture_count"] = lambda e, x: dict(cmp=(e.aperture_count(x.d, x.n, AP.ELLIPSOID, APT.HALF),))
WALK3D["aperture"] = lambda e, x: aperture_call(e, 3, x.d, x.n, APT.HALF)
FRESH_ONLY = ("probe_tree",)           # (F) alone: no reference evaluates the field off a tree it cannot see


def check_energy3(x, got, tol, what):
    """kinetic and elastic to 1e-6, the Coulomb energy to the table of test_energy_kd_against_fp64_direct_energy, against fp64 numpy"""
    def exact():
        q = x.host.astype(np.float64)
        k = x.par.astype(np.float64)[3:6]
        return np.array([0.5 * (q[1] ** 2).sum(), 0.5 * (k * q[0] ** 2).sum(), 0.5 * float(x.par[0]) * e3.pair_potential(x.host[0], np.float32(EPS2)).sum()])
    want = model("energy3", x.key, exact)
    out = got["out"]
    err = abs(out[2] - want[2]) / want[2] if want[2] else abs(out[2])
    print("%s: Coulomb energy off by %.3e" % (what, err))
    assert abs(out[0] - want[0]) <= 1e-6 * want[0] and abs(out[1] - want[1]) <= 1e-6 * want[1], (what, out, want)
    assert abs(out[2] - want[2]) <= tol * want[2], (what, out, want)
    if got.get("psi") is not None:
        assert abs(0.5 * got["psi"].sum() - out[2]) <= 1e-13 * abs(out[2]), what   # (test_gpu_energy3d.call_twice)


def check_probe3(x, got, what):
    """the bound of test_probe_is_the_exact_sum_at_every_launch_shape"""
    ea, epsi, mag = model("probe3", x.key + digest(x.t_host), lambda: p3.exact(x.host[0], x.t_host, EPS2, with_abs=True))
    s = float(x.par[0])
    a, psi = got["cmp"]
    assert np.abs(a - ea * s).max() <= 1e-12 * mag.max() * s and np.abs(psi - epsi * s).max() <= 1e-12 * epsi.max() * s, what


def check_pairs(pos, key, got, what):
    PH.same(got["cmp"], model("pairs", key, lambda: PN.pair_hist(pos, PAIR_BINS, PAIR_RMAX)), what)


MODELS3D = {
    # order 4 is held to the order-3 entry of the table, as test_energy_tree_is_energy_kd_on_a_fresh_context_in_any_state holds it
    "energy_tree": lambda x, got, what: check_energy3(x, got, EN3.ENERGY_TOL[3], what),
    "beam_moments": lambda x, got, what: BD.check_moments(got["m"], model("moments3", x.key, lambda: BN.moments(x.host[:2], 3)), 3, what),
    "hist_z": lambda x, got, what: check_hist(x.host, 3, [AX_Z], got, what),
    "hist_xvx": lambda x, got, what: check_hist(x.host, 3, x.xvx, got, what),
    "slice_moments": lambda x, got, what: SL.check_slices(got["recs"], got["outside"], *model("slices3", x.key, lambda: SN.slice_moments(x.host[:2], 3, AX_SLICE)),
                                                          3, x.n, what),
    "probe": check_probe3,
    "pair_hist_tree": lambda x, got, what: check_pairs(x.host[0], x.key, got, what),
    "pair_hist": lambda x, got, what: check_pairs(x.host[0], x.key, got, what),
    "bond_order_tree": lambda x, got, what: check_bonds(x.host[0], x.key, BOND_RMAX, got, what),
    "bond_order": lambda x, got, what: check_bonds(x.host[0], x.key, BOND_RMAX, got, what),
    "structure_factor": lambda x, got, what: check_sk(x.host[0], x.key, x.sk_h, SK_KSTEP, got, what),
    "structure_factor_2d": lambda x, got, what: check_sk(x.cloud2, digest(x.cloud2), x.sk_h2, SFT.K3, got, what),
    "aperture_count": lambda x, got, what: None,      # (held to the model through "aperture": its n - n_kept)
    "aperture": lambda x, got, what: check_aperture(3, x.host, APT.HALF, got, what),
}


def run_calls(e, calls, x):
    return {name: refusal(fn, e, x) for name, fn in calls.items()}


def fresh_calls(opts, calls, x):
    """bar (F): every call on a context created for it alone"""
    from coulomb_oscillators_amd import Engine
    out = {}
    for name, fn in calls.items():
        f = Engine(**opts)
        try:
            out[name] = refusal(fn, f, x)
        finally:
            f.close()
    return out


def hold(calls, models, x, got, fresh, what, with_model=True):
    """bars (F) and (M) for the results `got` of one context's calls on the inputs x"""
    for name in calls:
        assert_same_result(got[name], fresh[name], "%s: %s" % (what, name))
        if with_model and name not in FRESH_ONLY:
            assert got[name]["cmp"][0] is not REFUSED, "%s: %s was refused with status %s" % (what, name, got[name]["cmp"][1])
            models[name](x, got[name], "%s: %s" % (what, name))
    if "aperture_count" in got and "aperture" in got:
        assert got["aperture_count"]["cmp"][0] == x.n - got["aperture"]["cmp"][0], what
    if "pair_hist_tree" in got:
        PH.same(got["pair_hist_tree"]["cmp"], got["pair_hist"]["cmp"], what + ": tree form against exact form")
    if "bond_order_tree" in got:
        a, b = got["bond_order_tree"]["cmp"][0], got["bond_order"]["cmp"][0]
        assert a is not REFUSED and b is not REFUSED and np.array_equal(a, b), what + ": nb of the tree form against the exact form"


# ---- (a) the 3-D snapshot sequence -----------------------------------------------------------------------------------------------------
def loss_model_3d(o):
    """(lost, kept) per aperture call, from the model on the UNMOVED initial state: fifteen steps of 5e-4 move a particle by about 1e-2
    of its radius"""
    pos = CR.state(o, N0)[0]
    keep = np.ones(N0, dtype=bool)
    out = []
    for k in KS:
        inside = AP.inside(pos, AP.ELLIPSOID, [k * r for r in RMS])
        out.append((int((keep & ~inside).sum()), int((keep & inside).sum())))
        keep &= inside
    return out


def preconditions_3d(o):
    """each of the four lossy calls loses at least 50 and keeps at least 1000; the state crosses 4097 / 4096 and ends below 4096"""
    assert np.allclose(np.array(RMS) * 2.5, APT.HALF, rtol=1e-12)
    table = loss_model_3d(o)
    for call in (0, 2, 3, 4):
        assert table[call][0] >= 50 and table[call][1] >= 1000, (call, table)
    assert table[1][0] == 0, table
    assert table[3][1] > 4096 > table[4][1], table
    return table


def bond_table(pos, insides, rmax):
    """(n, nb_max, particles with a bond) of the positions left behind each of the modelled apertures, from bond_numpy.bonds"""
    keep = np.ones(len(pos), dtype=bool)
    out = []
    for inside in insides:
        keep &= inside
        nb = np.bincount(BO.bonds(pos[keep], rmax)[0], minlength=int(keep.sum()))
        out.append((int(keep.sum()), int(nb.max()), int((nb > 0).sum())))
    return out


def assert_bond_table(table):
    """nb_max <= 256, the premise of bond_numpy.TOL2, and at least half of the particles with a bond, at every snapshot"""
    assert all(nb_max <= 256 and 2 * bonded >= n for n, nb_max, bonded in table), table
    return table


def bond_preconditions_3d(o):
    """BOND_RMAX on the unmoved state behind each modelled aperture (as loss_model_3d)"""
    pos = CR.state(o, N0)[0]
    return assert_bond_table(bond_table(pos, [AP.inside(pos, AP.ELLIPSOID, [k * r for r in RMS]) for k in KS], BOND_RMAX))


def after_force_3d(o, e, x, state_in, what):
    """behind a compute_force of the run: energy_kd, energy_fmm and probe_kd -- (M) through the restatements on the device tree and
    the exact energy, (F) when the evaluation rebuilt"""
    import torch
    from coulomb_oscillators_amd import EVAL_FMM_KDTREE, Engine

    def look(eng, d):
        ek = energy_call(eng, eng.lib.nbco_kd_potential, d, x.n, x.prm)
        ef = np.array(eng.energy_fmm(d, x.n, x.prm))
        a, psi = PB3.run(eng.probe_kd, x.t, x.m, x.prm)
        return dict(cmp=(ek["out"], ek["psi"], ef, a, psi), out=ek["out"], psi=ek["psi"])
    info = e.kd_info()
    got = look(e, x.d)
    p, par0 = OPTS_A["fmm_order"], float(x.par[0])
    pos = x.host[0]                                                 # unsort = 0: the state is in tree order
    want = e3.psi(EN3.device_tree(e), pos, p, np.float32(EPS2), x.par[0], coll=True)
    err = np.abs(got["psi"] - want).max() / np.abs(want).max()
    wa, wpsi, _, _ = p3.walk(PB3.device_tree(e), pos, x.t_host, p, 1.0, EPS2, x.n)
    ea = np.abs(got["cmp"][3] - wa * par0).max() / np.linalg.norm(wa * par0, axis=1).max()
    ep = np.abs(got["cmp"][4] - wpsi * par0).max() / np.abs(wpsi * par0).max()
    print("%s (rebuilt %d): psi against the restatement %.2e; probe_kd a %.2e psi %.2e" % (what, info.rebuilt, err, ea, ep))
    assert err <= 1e-10 and ea <= 1e-10 and ep <= 1e-10, (what, err, ea, ep)
    check_energy3(x, got, EN3.ENERGY_TOL[3], what + ": energy_kd")
    check_energy3(x, dict(out=got["cmp"][2]), EN3.ENERGY_TOL[3], what + ": energy_fmm")
    if info.rebuilt:
        f = Engine(**OPTS_A)
        try:
            s = state_in.clone()
            f.compute_force(EVAL_FMM_KDTREE, s, x.n, x.prm)
            assert torch.equal(s, x.d), what + ": the state behind compute_force differs from the fresh context's"
            assert_same_result(got, look(f, s), what + ": energy_kd, energy_fmm, probe_kd")
        finally:
            f.close()
    return info.rebuilt


def run_snapshots_3d(o, diagnostics=True, extra=None):
    """Driver (a).  compute_force, then five snapshots, three leapfrog steps apart (the rebuild schedule is mid-cycle at every snapshot,
    and a lossy call restarts it), and three steps behind the last.  A snapshot: the aperture (M), then on the n' rows left every call
    of CALLS3D to (F) and (M); at snapshots 2 and 4 compute_force and after_force_3d.  Returns what bar (R) compares.
    Loss counts (lost, kept) per call, from the model on the unmoved state (tests/test_snapshots_host.py prints them):
    (231, 7962), (0, 7962), (577, 7385), (1307, 6078), (2173, 3905).  On the device the second call loses the two particles that three
    steps have moved across the surface ("few"), so the compute_force of snapshot 2 rebuilds as that of snapshot 4 does.
    `extra` rides the same loop (tests/test_gpu_snapshot_series.py): extra.snapshot(e, snap, view, n, order, what) behind each snapshot's
    aperture and diagnostics, `order` being the order map compacted as the aperture compacts it; extra.finish(e) behind the last."""
    import torch
    from coulomb_oscillators_amd import AP_ELLIPSOID, EVAL_FMM_KDTREE, INTEG_LEAPFROG, Engine
    from coulomb_oscillators_amd.engine import KdInfo
    preconditions_3d(o)
    buf, par = CR.state(o, N0), o.params(N0)
    probes = np.ascontiguousarray(buf[0][:300] * np.float32(1.2))
    e = Engine(**OPTS_A)
    log = dict(n=[], info=[], order=[], lost=[], rows=[], rebuilt_at_force=[])
    try:
        d, prm = dev(buf.reshape(-1).copy()), dev(par)
        n = N0
        lost_ids = []

        def look():
            info = e.kd_info()
            log["info"].append(tuple(getattr(info, f[0]) for f in KdInfo._fields_))
            log["order"].append(e.kd_array("order"))

        e.compute_force(EVAL_FMM_KDTREE, d, n, prm)
        for snap, k in enumerate(KS):
            what = "snapshot %d (k = %g, n = %d before its aperture)" % (snap + 1, k, n)
            if snap:
                e.integrate_steps(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, DT, STEPS)
            look()
            half = [k * r for r in RMS]
            host = d.cpu().numpy()[:9 * n].reshape(3, n, 3).copy()
            lost, rows = APT.lost_buffers(3, n)
            kept = e.aperture(d, n, AP_ELLIPSOID, half, lost=lost[:6 * n], lost_row=rows[:n])
            got = dict(cmp=(kept, d.cpu().numpy()[:9 * kept], lost.cpu().numpy(), rows.cpu().numpy()))
            check_aperture(3, host, half, got, what + ": aperture")
            log["lost"].append(got["cmp"][2][:6 * (n - kept)].copy())
            log["rows"].append(got["cmp"][3][:n - kept].copy())
            lost_ids.append(log["order"][-1][log["rows"][-1]])          # through the order map as it was before the call
            n = kept
            log["n"].append(n)
            view = d[:9 * n]
            if diagnostics:
                x = inputs3d(o, view, n, prm, par, probes)
                before = view.clone()
                got = run_calls(e, CALLS3D, x)
                assert torch.equal(view, before), what + ": a diagnostic call wrote the state"
                hold(CALLS3D, MODELS3D, x, got, fresh_calls(OPTS_A, CALLS3D, x), what)
                want, wphi = EN3.fresh_energy_kd(view, n, prm, **child_opts(OPTS_A))
                assert np.array_equal(got["energy_tree"]["out"], want) and np.array_equal(got["energy_tree"]["psi"], wphi.cpu().numpy()), what + ": energy_tree"
            if extra is not None:
                extra.snapshot(e, snap, view, n, np.delete(log["order"][-1], log["rows"][-1]), what)
            if snap in FORCE_AT:
                state_in = view.clone()
                e.compute_force(EVAL_FMM_KDTREE, view, n, prm)
                if diagnostics:
                    x = inputs3d(o, view, n, prm, par, probes)
                    log["rebuilt_at_force"].append(after_force_3d(o, e, x, state_in, what + ": behind compute_force"))
        if extra is not None:
            extra.finish(e)
        e.integrate_steps(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, DT, STEPS)
        look()
        log["state"] = d.cpu().numpy()[:9 * n].copy()
        # the order map has followed the state: the initial particle numbers less those the loss records name
        gone = np.concatenate(lost_ids)
        assert len(np.unique(gone)) == len(gone) == N0 - n
        assert np.array_equal(np.sort(log["order"][-1]), np.setdiff1d(np.arange(N0), gone)), "kd_array(order) at the end of the run"
        q = log["state"].reshape(3, n, 3)
        assert np.isfinite(q).all()
    finally:
        e.close()
    return log


def assert_same_run(a, b, keys):
    """bar (R)"""
    for k in keys:
        if k == "state":
            assert a[k].tobytes() == b[k].tobytes(), "the final state differs from the run without the diagnostic calls"
        elif k in ("n", "info"):
            assert a[k] == b[k], (k, a[k], b[k])
        else:
            assert len(a[k]) == len(b[k]) and all(u.tobytes() == v.tobytes() for u, v in zip(a[k], b[k])), k


def drive_a(o):
    with_calls = run_snapshots_3d(o, True)
    plain = run_snapshots_3d(o, False)
    assert_same_run(with_calls, plain, ("n", "info", "order", "lost", "rows", "state"))
    assert with_calls["n"][-1] < 4096 < with_calls["n"][-2]
    return with_calls


# ---- (b) the size walk of the diagnostics ----------------------------------------------------------------------------------------------
SIZES_B = [8193, 300, 20000, 1, 65, 4097, 20000, 2]
GRIDS_B = [(8, 8, 8), (2, 2, 2), (2, 2, 2), (64, 0, 0), (0, 0, 64), (17, 1, 1), (1, 8, 8), (0, 0, 0)]      # structure_factor at step i
GRIDS_B2 = [(8, 8), (2, 2), (2, 64), (64, 0), (0, 64), (17, 55), (4, 4), (0, 0)]                           # structure_factor_2d at step i
CLOUD2_MAX = 4097                      # the 2-D form runs on sk_numpy.cloud(min(n, 4097), .., dim=2)
LARGEST_GRID = (1025, (64, 64, 64))    # the step appended for structure_factor alone: the largest grid, with several ranges
MODEL_MAX = 8193
OPTS_B = dict(fmm_order=4)


def sk_shape(dim, n, h, max_acc=17, extra=0, parts=1):
    """The launch shape of a wave-vector sum, FOLLOWING sk_shape and kgrid_run in csrc/k_reduce.hip (the defaults are SkTerm's: runs
    of at most 17 indices ix, no slot beside the tables, one complex number per record).  A precondition only: it says which paths
    the walk takes, and no result is compared with it."""
    hx, hy, hz = h[0], h[1], (h[2] if dim == 3 else 0)
    nch = (hx + max_acc) // max_acc
    L = (hx + nch) // nch
    ny, nz = 2 * hy + 1, 2 * hz + 1
    items, K = nch * ny * nz, (hx + 1) * ny * nz
    per = 1 + extra + (hy + 1) + (hz + 1 if dim == 3 else 0) + (nch if nch > 1 else 0)
    tile = min(256, 48 * 1024 // (16 * per))
    kt0 = (items + 255) // 256
    kt, best = kt0, 0.0
    for t in range(kt0, 4 * kt0 + 1):
        lanes = (items + t - 1) // t
        busy = float(items) * (256 // lanes) / (float(t) * 256)
        if busy > best:
            best, kt = busy, t
        if busy >= 0.85:
            break
    lanes = (items + kt - 1) // kt
    copies = 256 // lanes if lanes <= 128 else 1
    r0 = min((n + 511) // 512, max(1, 2048 // kt))
    r0 = max(1, min(r0, (256 << 20) // (16 * parts * K)))
    rng = ((n + r0 - 1) // r0 + 63) // 64 * 64
    return dict(dim=dim, n=n, h=tuple(h), nch=nch, L=L, items=items, K=K, lanes=lanes, copies=copies, tile=tile, ranges=(n + rng - 1) // rng)


def sk_walk_shapes():
    """the shapes of the calls that share the live context's sk_part in run_size_walk_3d, in the order of the calls"""
    out = []
    for n, h3, h2 in zip(SIZES_B, GRIDS_B, GRIDS_B2):
        out += [sk_shape(2, min(n, CLOUD2_MAX), h2), sk_shape(3, n, h3)]
    return out + [sk_shape(3, *LARGEST_GRID)]


def preconditions_walk():
    """what the walk is there for, asserted of the restated shapes: a call with one range directly behind one with at least 16; more
    ranges on a smaller K than an earlier call (another layout inside the bytes that call wrote); several chunks of ix; workgroups
    with several copies of their items and with one; a tile below 256"""
    assert len(GRIDS_B) == len(GRIDS_B2) == len(SIZES_B)
    t = sk_walk_shapes()
    assert any(a["ranges"] >= 16 and b["ranges"] == 1 for a, b in zip(t, t[1:])), t
    assert any(b["ranges"] > a["ranges"] > 1 and b["K"] < a["K"] for i, b in enumerate(t) for a in t[:i]), t
    assert any(s["nch"] > 1 for s in t) and any(s["nch"] > 1 and s["ranges"] > 1 for s in t), t
    assert any(s["copies"] > 1 for s in t) and any(s["copies"] == 1 for s in t), t
    assert any(s["tile"] < 256 for s in t), t
    big = t[-1]
    assert big["ranges"] > 1 and big["K"] == SK.count(LARGEST_GRID[1]) == 65 * 129 * 129, big
    return t


def run_size_walk_3d(o):
    """Driver (b), 3-D.  One context over SIZES_B, at every step every call of WALK3D (the aperture on a copy, at 2.5 rms): (F), and (M)
    where n <= 8193.  The private child context, the slice tables, the aperture's scan levels and the probes' sort scratch each see a
    smaller n behind a larger one.  The wave-vector grid changes with the step as n does (GRIDS_B for structure_factor, GRIDS_B2 for
    structure_factor_2d on a cloud of min(n, 4097) points right before it), so sk_part is cut anew at every call: preconditions_walk
    says into what.  A last step runs structure_factor alone on the largest grid at n = 1025, three ranges of 1.08 million wave
    vectors, held to (F) and, on every 37th wave vector, the zero vector and the last one, to (M)."""
    import torch
    from coulomb_oscillators_amd import Engine
    preconditions_walk()
    live = Engine(**OPTS_B)
    fresh = {}
    try:
        for step, n in enumerate(SIZES_B):
            buf, par = CR.state(o, n), o.params(n)
            d, prm = dev(buf.reshape(-1).copy()), dev(par)
            x = inputs3d(o, d, n, prm, par, np.ascontiguousarray(buf[0][:300] * np.float32(1.2)))
            x.sk_h, x.sk_h2 = GRIDS_B[step], GRIDS_B2[step]
            x.cloud2 = SK.cloud(min(n, CLOUD2_MAX), 5000 + step, dim=2)
            x.d2 = dev(x.cloud2)
            what = "size walk step %d: n %d" % (step, n)
            got = run_calls(live, WALK3D, x)
            assert np.array_equal(d.cpu().numpy(), buf.reshape(-1)), what + ": a call wrote the state"
            assert np.array_equal(x.d2.cpu().numpy(), x.cloud2), what + ": a call wrote the 2-D cloud"
            key = (n, x.sk_h, x.sk_h2)
            if key not in fresh:
                fresh[key] = fresh_calls(OPTS_B, WALK3D, x)
            hold(WALK3D, MODELS3D, x, got, fresh[key], what, with_model=n <= MODEL_MAX)
        n, h = LARGEST_GRID
        buf = CR.state(o, n)
        x = Inputs()
        x.d, x.n, x.sk_h = dev(buf.reshape(-1).copy()), n, h
        x.host = buf
        what = "size walk, the largest grid: n %d" % n
        call = {"structure_factor": CALLS3D["structure_factor"]}
        got = run_calls(live, call, x)
        assert_same_result(got["structure_factor"], fresh_calls(OPTS_B, call, x)["structure_factor"], what)
        K = SK.count(h)
        only = np.unique(np.concatenate([np.arange(0, K, 37), [SK.index(h, 0, 0, 0), K - 1]]))     # (test_parity_on_the_largest_grid)
        check_sk(buf[0], digest(buf[0]), h, SK_KSTEP, got["structure_factor"], what, only=only)
    finally:
        live.close()


# ---- 2-D: the calls ------------------------------------------------------------------------------------------------------------------
OPTS_2D = dict(fmm_order=5)
KS_2D = (1.9, 1.8, 1.7, 1.6)           # of the KV beam's rms radii A / 2: the beam is uniform inside A, so (k / 2)^2 of it is inside
WALK_K_2D = 1.7
SIZES_2D = [8193, 300, 4097, 1, 65, 8193]
EPS2_2D = PB2.EPS2_F32
# the bond radius in units of the larger KV semi-axis (as x.rmax of pair_hist_2d): test_snapshots_host.py asserts from the model that
# nb <= 256, the premise of bond_numpy.TOL2, and that at least half of the particles have a bond at every snapshot (23, all but two)
BOND_RMAX_2D = 0.03
SK_H_2D = (8, 8)
SK_TURNS_2D = 6.0                      # kstep_a = 6 / A_a: k . x runs over +-6 rad per index across the beam (the 3-D ball: 900 * 2.5 rms = 6.75, 2.25, 22.5)


def kv_rms():
    return tuple(a / 2 for a in F2.kv_params()[0])


def state2d(n):
    """[2, n, 2] of init2d(n, "kv", ..) and its parameter pack; a single particle is the head of the two-particle state (as in
    test_energy_2d_against_exact_sum)"""
    st, par = CR.state2d(max(n, 2))
    par = par.copy()
    par[0] *= max(n, 2) / n
    return np.ascontiguousarray(st[:, :n]), par


def vx_max():
    """the largest |vx| of the initial KV beam (a matched beam keeps it)"""
    return model("vx_max", N0, lambda: float(np.abs(state2d(N0)[0][1][:, 0]).max()))


def buffer2d(st):
    n = st.shape[1]
    return dev(np.concatenate([st.reshape(-1), np.zeros(2 * n)]))


def inputs2d(d, n, prm, par, probes_host):
    A = F2.kv_params()[0]
    x = Inputs()
    x.d, x.n, x.prm, x.par = d, n, prm, par
    x.host = d.cpu().numpy()[:6 * n].reshape(3, n, 2).copy()
    x.key = digest(x.host)
    x.t_host = probes_host
    x.t, x.m = dev(probes_host.reshape(-1)), len(probes_host)
    x.ax_x = (X, 64, -A[0], A[0])
    x.xvx = [(X, 32, -A[0], A[0]), (VX, 32, -vx_max(), vx_max())]
    x.ax_slice = (Y, 16, -A[1], A[1])
    x.rmax = 0.05 * max(A)
    x.bond_rmax = BOND_RMAX_2D * max(A)
    x.sk_h, x.sk_kstep = SK_H_2D, tuple(SK_TURNS_2D / a for a in A)
    x.half = [WALK_K_2D * r for r in kv_rms()]
    return x


def probe2(name):
    def call(e, x):
        import torch
        a = torch.full((x.m, 2), float("nan"), dtype=torch.float64, device="cuda")
        psi = torch.full((x.m,), float("nan"), dtype=torch.float64, device="cuda")
        getattr(e, name)(x.d, x.n, x.t, x.m, x.prm, a, psi)
        return dict(cmp=(a.cpu().numpy(), psi.cpu().numpy()))
    return call


CALLS2D = {
    "energy_fmm_2d": lambda e, x: energy_call(e, e.lib.nbco_2d_energy_fmm, x.d, x.n, x.prm),
    "energy_2d": lambda e, x: energy_call(e, e.lib.nbco_2d_energy, x.d, x.n, x.prm),
    "beam_moments_2d": lambda e, x: moments_call(e, e.lib.nbco_2d_beam_moments, x.d, x.n),
    "hist_x": lambda e, x: hist_call(e.hist_2d, x.d, x.n, [x.ax_x]),
    "hist_xvx": lambda e, x: hist_call(e.hist_2d, x.d, x.n, x.xvx),
    "slice_moments_2d": lambda e, x: slices_call(e, e.lib.nbco_2d_slice_moments, x.d, x.n, x.ax_slice),
    "probe_fmm_2d": probe2("probe_fmm_2d"),
    "probe_2d": probe2("probe_2d"),
    "pair_hist_2d": lambda e, x: dict(cmp=PH.run(e, "exact2d", x.d, x.n, PAIR_BINS, x.rmax)),
    "bond_order_2d": lambda e, x: bond_call(e, "exact2d", x.d, x.n, x.bond_rmax),
    "structure_factor_2d": lambda e, x: sk_call(e.structure_factor_2d, x.d, x.n, 2, x.sk_h, x.sk_kstep),
}
WALK2D = dict(CALLS2D)
WALK2D["aperture_2d"] = lambda e, x: aperture_call(e, 2, x.d, x.n, x.half)


def check_energy_fmm_2d(x, got, what):
    """the bounds of test_energy_fmm_2d_matches_restatement"""
    want, psi_w, S = model("energy_fmm_2d", x.key, lambda: E2.fmm_energy(x.host[:2], OPTS_2D["fmm_order"], EPS2_2D, x.par))
    out, psi = got["out"], got["psi"]
    assert abs(out[0] - want[0]) <= 1e-13 * want[0] and abs(out[1] - want[1]) <= 1e-13 * want[1], (what, out, want)
    assert abs(out[2] - want[2]) <= 1e-10 * S and np.abs(psi - psi_w).max() <= 1e-10 * np.abs(psi_w).max(), (what, out, want)


def check_energy_2d(x, got, what):
    """the bounds of test_energy_2d_against_exact_sum"""
    want, psi_w, ab = model("energy_2d", x.key, lambda: E2.exact(x.host[0], x.host[1], x.par, EPS2_2D))
    out, psi = got["out"], got["psi"]
    assert abs(out[0] - want[0]) <= 1e-13 * want[0] and abs(out[1] - want[1]) <= 1e-13 * want[1], (what, out, want)
    assert abs(out[2] - want[2]) <= 1e-11 * ab.sum() / 2 and np.abs(psi - psi_w).max() <= 1e-11 * ab.max(), (what, out, want)


MODELS2D = {
    "energy_fmm_2d": check_energy_fmm_2d,
    "energy_2d": check_energy_2d,
    "beam_moments_2d": lambda x, got, what: BD.check_moments(got["m"], model("moments2", x.key, lambda: BN.moments(x.host[:2], 2)), 2, what),
    "hist_x": lambda x, got, what: check_hist(x.host, 2, [x.ax_x], got, what),
    "hist_xvx": lambda x, got, what: check_hist(x.host, 2, x.xvx, got, what),
    "slice_moments_2d": lambda x, got, what: SL.check_slices(got["recs"], got["outside"], *model("slices2", x.key, lambda: SN.slice_moments(x.host[:2], 2, x.ax_slice)),
                                                             2, x.n, what),
    "probe_fmm_2d": lambda x, got, what: PB2._check_fmm(got["cmp"], model("probe_fmm_2d", x.key + digest(x.t_host), lambda: PR2.fmm(
        x.host[0], x.t_host, OPTS_2D["fmm_order"], EPS2_2D, x.par[0])), what),
    "probe_2d": lambda x, got, what: PB2._check_exact(got["cmp"], model("probe_2d", x.key + digest(x.t_host), lambda: PR2.exact(
        x.host[0], x.t_host, EPS2_2D, x.par[0])), what),
    "pair_hist_2d": lambda x, got, what: PH.same(got["cmp"], model("pairs2", x.key, lambda: PN.pair_hist(x.host[0], PAIR_BINS, x.rmax)), what),
    "bond_order_2d": lambda x, got, what: check_bonds(x.host[0], x.key, x.bond_rmax, got, what),
    "structure_factor_2d": lambda x, got, what: check_sk(x.host[0], x.key, x.sk_h, x.sk_kstep, got, what),
    "aperture_2d": lambda x, got, what: check_aperture(2, x.host, x.half, got, what),
}


def run_size_walk_2d():
    """Driver (b), the nbco_2d_ forms on a context of their own over SIZES_2D: (F) and (M) at every step"""
    from coulomb_oscillators_amd import Engine
    live = Engine(**OPTS_2D)
    fresh = {}
    try:
        for step, n in enumerate(SIZES_2D):
            st, par = state2d(n)
            d, prm = buffer2d(st), dev(par)
            x = inputs2d(d, n, prm, par, np.ascontiguousarray(st[0][:300] * 1.2))
            what = "2-D size walk step %d: n %d" % (step, n)
            before = d.clone()
            got = run_calls(live, WALK2D, x)
            assert np.array_equal(d.cpu().numpy(), before.cpu().numpy()), what + ": a call wrote the state"
            if n not in fresh:
                fresh[n] = fresh_calls(OPTS_2D, WALK2D, x)
            hold(WALK2D, MODELS2D, x, got, fresh[n], what)
    finally:
        live.close()


# ---- (c) the 2-D snapshot sequence -----------------------------------------------------------------------------------------------------
def loss_model_2d():
    st, _ = state2d(N0)
    keep = np.ones(N0, dtype=bool)
    out = []
    for k in KS_2D:
        inside = AP.inside(st[0], AP.ELLIPSOID, [k * r for r in kv_rms()])
        out.append((int((keep & ~inside).sum()), int((keep & inside).sum())))
        keep &= inside
    return out


def preconditions_2d():
    """every call loses at least 50 particles and keeps at least 1000, on the unmoved state (a matched KV beam keeps its size)"""
    table = loss_model_2d()
    assert all(lost >= 50 and kept >= 1000 for lost, kept in table), table
    return table


def bond_preconditions_2d():
    """BOND_RMAX_2D on the unmoved KV beam behind each modelled aperture (as loss_model_2d)"""
    pos = state2d(N0)[0][0]
    insides = [AP.inside(pos, AP.ELLIPSOID, [k * r for r in kv_rms()]) for k in KS_2D]
    return assert_bond_table(bond_table(pos, insides, BOND_RMAX_2D * max(F2.kv_params()[0])))


def run_snapshots_2d(diagnostics=True):
    """Driver (c): (a) for what nbco runs.  compute_force_2d(EVAL2D_FMM), four snapshots three leapfrog steps apart and three steps
    behind the last; a snapshot is aperture_2d (M) and then every call of CALLS2D to (F) and (M).  Returns what bar (R) compares."""
    import torch
    from coulomb_oscillators_amd import AP_ELLIPSOID, EVAL2D_FMM, INTEG_LEAPFROG, Engine
    preconditions_2d()
    st, par = state2d(N0)
    probes = np.ascontiguousarray(st[0][:300] * 1.2)
    e = Engine(**OPTS_2D)
    log = dict(n=[], lost=[], rows=[])
    try:
        d, prm = buffer2d(st), dev(par)
        n = N0
        e.compute_force_2d(EVAL2D_FMM, d, n, prm)
        for snap, k in enumerate(KS_2D):
            what = "2-D snapshot %d (k = %g, n = %d before its aperture)" % (snap + 1, k, n)
            if snap:
                e.integrate_steps_2d(INTEG_LEAPFROG, EVAL2D_FMM, d, n, prm, 5e-4, STEPS)
            half = [k * r for r in kv_rms()]
            host = d.cpu().numpy()[:6 * n].reshape(3, n, 2).copy()
            lost, rows = APT.lost_buffers(2, n)
            kept = e.aperture_2d(d, n, AP_ELLIPSOID, half, lost=lost[:4 * n], lost_row=rows[:n])
            got = dict(cmp=(kept, d.cpu().numpy()[:6 * kept], lost.cpu().numpy(), rows.cpu().numpy()))
            check_aperture(2, host, half, got, what + ": aperture_2d")
            assert n - kept >= 1 and kept >= 1000, what
            log["lost"].append(got["cmp"][2][:4 * (n - kept)].copy())
            log["rows"].append(got["cmp"][3][:n - kept].copy())
            n = kept
            log["n"].append(n)
            if diagnostics:
                view = d[:6 * n]
                x = inputs2d(view, n, prm, par, probes)
                before = view.clone()
                got = run_calls(e, CALLS2D, x)
                assert torch.equal(view, before), what + ": a diagnostic call wrote the state"
                hold(CALLS2D, MODELS2D, x, got, fresh_calls(OPTS_2D, CALLS2D, x), what)
        e.integrate_steps_2d(INTEG_LEAPFROG, EVAL2D_FMM, d, n, prm, 5e-4, STEPS)
        log["state"] = d.cpu().numpy()[:6 * n].copy()
        assert np.isfinite(log["state"]).all()
    finally:
        e.close()
    return log


def drive_c():
    with_calls = run_snapshots_2d(True)
    plain = run_snapshots_2d(False)
    assert_same_run(with_calls, plain, ("n", "lost", "rows", "state"))
    return with_calls


# ---- the tests: one driver each ----------------------------------------------------------------------------------------------------------
def test_snapshot_sequence_3d_on_one_context(oracle32):
    drive_a(oracle32)


def test_size_walk_of_the_diagnostics_3d(oracle32):
    run_size_walk_3d(oracle32)


def test_size_walk_of_the_diagnostics_2d(engine_lib):
    run_size_walk_2d()


def test_snapshot_sequence_2d_on_one_context(engine_lib):
    drive_c()
