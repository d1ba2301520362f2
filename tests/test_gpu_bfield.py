"""The uniform magnetic field on the GPU: nbco_drift_b, nbco_integrate_b, nbco_integrate_steps_b and the 2-D forms against the fp64 model
of tests/bfield_numpy.py, and the fused leapfrog passes against the step-by-step calls, bit for bit.

Tolerance of the 3-D comparisons to the fp64 model (the rule of integrators3d_numpy.gpu_tolerance): min(4 x floor, cap), per x and v, the
floor the distance of the model's float32 emulation -- multiply and add rounded separately, never the code under test -- from the
fp64 model on the same input; the factor 4 covers one fmaf against a multiply and an add."""
import numpy as np
import pytest

import bfield_numpy as bf
import integrators3d_numpy as ig
from direct_numpy import direct_rows_fp64, direct3_rows_fp32

pytestmark = pytest.mark.gpu

GRID_CAP, PER_THREAD, BLOCK = 2048, 4, 256          # k_axpy.hip: stream_grid's cap, particles per thread of the vector kernel, kBlock
N_TWICE = GRID_CAP * BLOCK * PER_THREAD + 5         # with x and v aligned: the vector kernel's grid-stride loop runs a second time, and a tail is left


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _held(tag, got, emu, want, cap=ig.GPU_TOL_CAP):
    floor = tuple(ig.rel_dist(emu[q], want[q]) for q in range(2))
    err = tuple(ig.rel_dist(got[q], want[q]) for q in range(2))
    tol = ig.gpu_tolerance(floor, cap=cap)
    print("%s: floor x %.2e v %.2e   error x %.2e v %.2e   tolerance x %.2e v %.2e" % (tag, *floor, *err, *tol))
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    assert err[0] <= tol[0] and err[1] <= tol[1], (tag, err, tol)
    return tol


# ---- the drift alone --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [0.7, -1.3])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 256, 257, 4099, N_TWICE])
def test_drift_b_against_model(engine, n, s):
    """x and v in one buffer [x n | v n]: v is 16-byte aligned only when n % 4 == 0, so a call is all vector groups (n % 4 == 0) or all
    one particle per lane (otherwise; at N_TWICE that kernel's grid-stride loop runs again); |v| is kept"""
    rng = np.random.default_rng(1000 + n)
    state = rng.normal(size=(2, n, 3)).astype(np.float32)
    want = bf.drift(state[0], state[1], bf.OMEGA, s)
    emu = bf.drift_f32(state[0], state[1], bf.OMEGA, s)
    d = dev(state)
    engine.drift_b(d[0], d[1], n, bf.OMEGA, s)
    got = d.cpu().numpy()
    tol = _held("n %d s %+.1f" % (n, s), got, emu, want)
    speed = lambda v: np.linalg.norm(np.asarray(v, dtype=np.float64), axis=1)
    kept = float(np.abs(speed(got[1]) - speed(state[1])).max() / np.abs(state[1]).max())
    print("   |v| moved by %.2e" % kept)
    assert kept <= tol[1]


@pytest.mark.parametrize("s", [0.7, -1.3])
@pytest.mark.parametrize("n", [5, 255, 257, 4099, N_TWICE])
def test_drift_b_vector_groups_then_tail(engine, n, s):
    """x and v as two tensors of their own, both 16-byte aligned, n % 4 != 0: n / 4 vector groups of four particles (helix_vec; at
    N_TWICE its grid-stride loop runs a second time), then the tail one particle per lane from particle 4 (n / 4) on.  Held to the
    model, and the bits are those of the packed call, which takes the other path for every particle."""
    import torch
    rng = np.random.default_rng(1000 + n)
    state = rng.normal(size=(2, n, 3)).astype(np.float32)
    want = bf.drift(state[0], state[1], bf.OMEGA, s)
    emu = bf.drift_f32(state[0], state[1], bf.OMEGA, s)
    x, v = dev(state[0]), dev(state[1])
    assert x.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 0 and n % 4 != 0
    engine.drift_b(x, v, n, bf.OMEGA, s)
    _held("separate n %d s %+.1f" % (n, s), (x.cpu().numpy(), v.cpu().numpy()), emu, want)
    d = dev(state)
    engine.drift_b(d[0], d[1], n, bf.OMEGA, s)
    assert torch.equal(d[0].view(torch.int32), x.view(torch.int32)) and torch.equal(d[1].view(torch.int32), v.view(torch.int32))


def test_drift_b_unaligned_x_and_zero_field(engine):
    """x itself off the 16-byte grid (the scalar path for every particle) gives the bits of the aligned call; Omega = 0 is x += v s"""
    import torch
    n = 1029
    rng = np.random.default_rng(7)
    state = rng.normal(size=(2, n, 3)).astype(np.float32)
    a = dev(state)
    engine.drift_b(a[0], a[1], n, bf.OMEGA, 0.9)
    raw = torch.zeros(6 * n + 1, dtype=torch.float32, device="cuda")
    raw[1:] = dev(state).reshape(-1)
    engine.drift_b(raw[1:3 * n + 1], raw[3 * n + 1:], n, bf.OMEGA, 0.9)
    assert torch.equal(raw[1:].view(torch.int32), a.reshape(-1).view(torch.int32))
    z = dev(state)
    engine.drift_b(z[0], z[1], n, (0.0, 0.0, 0.0), 0.5)
    f = np.float32
    assert np.array_equal(z[1].cpu().numpy(), state[1])
    assert np.abs(z[0].cpu().numpy() - (state[0] + f(0.5) * state[1])).max() <= 2e-7 * np.abs(state).max()


# ---- the five schemes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", ig.SCALES)
@pytest.mark.parametrize("scheme", ig.SCHEMES, ids=[ig.NAMES[s] for s in ig.SCHEMES])
def test_schemes_elastic_only_against_model(engine, oracle32, scheme, scale):
    from coulomb_oscillators_amd import EVAL_DIRECT_KAHAN
    buf, par = ig.elastic_only_input(oracle32)
    k = par[3:6]
    want = bf.run(scheme, ig.elastic_force(k.astype(np.float64)), buf[0], buf[1], ig.DT, ig.STEPS, bf.OMEGA, scale)[-1]
    emu = bf.run(scheme, bf.elastic_force_f32(k), buf[0], buf[1], ig.DT, ig.STEPS, bf.OMEGA, scale, f32=True)[-1]
    d, prm = dev(buf.copy()), dev(par)
    engine.compute_force(EVAL_DIRECT_KAHAN, d, ig.N, prm, elastic=True)
    for _ in range(ig.STEPS):
        engine.integrate_b(scheme, EVAL_DIRECT_KAHAN, d, ig.N, prm, ig.DT, bf.OMEGA, scale, elastic=True)
    _held("%s scale %.1f" % (ig.NAMES[scheme], scale), d.cpu().numpy(), emu, want)


@pytest.mark.parametrize("scheme", ig.SCHEMES, ids=[ig.NAMES[s] for s in ig.SCHEMES])
def test_schemes_elastic_only_odd_n_against_model(engine, oracle32, scheme):
    """the same comparison at n = 257: v = buf + 3 n and a = buf + 6 n are off the 16-byte grid, so leapfrog's fused kick and drift is
    helix_scalar<true> (one particle per lane) and every drift the one-particle kernel; integrate_steps_b gives the same bits"""
    import torch
    from coulomb_oscillators_amd import EVAL_DIRECT_KAHAN
    n = 257
    buf, par = oracle32.init_reference(n), oracle32.params(n)
    par[0] = 0
    k = par[3:6]
    want = bf.run(scheme, ig.elastic_force(k.astype(np.float64)), buf[0], buf[1], ig.DT, ig.STEPS, bf.OMEGA)[-1]
    emu = bf.run(scheme, bf.elastic_force_f32(k), buf[0], buf[1], ig.DT, ig.STEPS, bf.OMEGA, f32=True)[-1]
    d, prm = dev(buf.copy()), dev(par)
    assert d[1].data_ptr() % 16 != 0
    engine.compute_force(EVAL_DIRECT_KAHAN, d, n, prm, elastic=True)
    start = d.clone()
    for _ in range(ig.STEPS):
        engine.integrate_b(scheme, EVAL_DIRECT_KAHAN, d, n, prm, ig.DT, bf.OMEGA, elastic=True)
    _held("%s n %d" % (ig.NAMES[scheme], n), d.cpu().numpy(), emu, want)
    engine.integrate_steps_b(scheme, EVAL_DIRECT_KAHAN, start, n, prm, ig.DT, ig.STEPS, bf.OMEGA)
    assert torch.equal(start.view(torch.int32), d.view(torch.int32))


@pytest.mark.parametrize("scheme", [ig.LEAPFROG, ig.PEFRL], ids=["leapfrog", "pefrl"])
def test_schemes_with_coulomb_against_model_per_step(engine, oracle32, scheme):
    """n = 256, dt = 0.02, three steps with the direct evaluator, the model's force from direct_numpy (fp64 sum; float32 Kahan sum for
    the emulation); cap 1e-2 and factor 4 as test_integrators_coulomb_against_fp64_oracle_per_step"""
    import torch
    from coulomb_oscillators_amd import EVAL_DIRECT_KAHAN
    n, dt, steps = 256, 0.02, 3
    buf, par = oracle32.init_reference(n), oracle32.params(n)
    eps2, rows = float(np.float32(1e-18)), np.arange(n)
    k64 = par[3:6].astype(np.float64)
    f64 = lambda x: direct_rows_fp64(x, rows, float(par[0]), eps2) - k64 * x
    f32 = lambda x: direct3_rows_fp32(x.astype(np.float32), rows, par[0], np.float32(eps2)) - par[3:6] * x
    want = bf.run(scheme, f64, buf[0], buf[1], dt, steps, bf.OMEGA)
    emu = bf.run(scheme, f32, buf[0], buf[1], dt, steps, bf.OMEGA, f32=True)
    d, prm = dev(buf.copy()), dev(par)
    engine.compute_force(EVAL_DIRECT_KAHAN, d, n, prm, elastic=True)
    start = d.clone()
    for s in range(steps):
        engine.integrate_b(scheme, EVAL_DIRECT_KAHAN, d, n, prm, dt, bf.OMEGA)
        _held("%s step %d" % (ig.NAMES[scheme], s + 1), d.cpu().numpy(), emu[s], want[s], cap=1e-2)
    engine.integrate_steps_b(scheme, EVAL_DIRECT_KAHAN, start, n, prm, dt, steps, bf.OMEGA)
    assert torch.equal(start.view(torch.int32), d.view(torch.int32))


# ---- fused equals step by step ----------------------------------------------------------------------------------------------------
def _state(oracle32, n):
    return dev(oracle32.init_reference(n).copy()), dev(oracle32.params(n))


@pytest.mark.parametrize("n,p,tree_steps,steps", [(20000, 4, 1, 5), (65536, 6, 3, 8), (5000, 6, 1, 4), (20003, 4, 1, 5), (5001, 6, 2, 4)])
def test_fused_leapfrog_equals_step_by_step(oracle32, n, p, tree_steps, steps):
    """kd_turnaround_kernel<., Helix3> against the separate passes; afterwards one integrate_b and two more fused steps carry on identically
    (the pattern of test_gpu_integrate_steps.py).  The opening kick and drift of every call is helix_vec<kick> where n % 4 == 0 and
    helix_scalar<true> at n = 20003 and 5001, where v and a are off the 16-byte grid."""
    import torch
    from coulomb_oscillators_amd import Engine, EVAL_FMM_KDTREE, INTEG_LEAPFROG
    dt, om = 5e-4, (300.0, -200.0, 700.0)      # |Omega| dt = 0.39: the field turns the velocities visibly within a step
    out = []
    for fused in (False, True):
        e = Engine(fmm_order=p, unsort=0, tree_steps=tree_steps)
        d, prm = _state(oracle32, n)
        e.compute_force(EVAL_FMM_KDTREE, d, n, prm)
        if fused:
            e.integrate_steps_b(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, dt, steps, om)
            e.integrate_b(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, dt, om)
            e.integrate_steps_b(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, dt, 2, om)
        else:
            for _ in range(steps + 3):
                e.integrate_b(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, dt, om)
        torch.cuda.synchronize()
        assert torch.isfinite(d).all()
        out.append(d.clone())
        e.close()
    for part, name in enumerate(("positions", "velocities", "accelerations")):
        assert torch.equal(out[0][part].view(torch.int32), out[1][part].view(torch.int32)), name + " differ"
    # and the field was there: the plain run ends elsewhere
    e = Engine(fmm_order=p, unsort=0, tree_steps=tree_steps)
    d, prm = _state(oracle32, n)
    e.compute_force(EVAL_FMM_KDTREE, d, n, prm)
    e.integrate_steps(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, dt, steps + 3)
    torch.cuda.synchronize()
    e.close()
    assert not torch.equal(d[1], out[1][1])


@pytest.mark.parametrize("scheme_name,kind_name,opts", [("INTEG_LEAPFROG", "EVAL_FMM_KDTREE", dict(unsort=0, tree_steps=2)), ("INTEG_PEFRL", "EVAL_FMM_KDTREE", dict(unsort=0)),
                                                        ("INTEG_FORESTRUTH", "EVAL_DIRECT", dict())])
def test_zero_field_is_the_plain_call(oracle32, scheme_name, kind_name, opts):
    import torch
    import coulomb_oscillators_amd as co
    scheme, kind = getattr(co, scheme_name), getattr(co, kind_name)
    n, steps, dt, zero = 8192, 3, 5e-4, (0.0, 0.0, 0.0)
    out = []
    for field in (False, True):
        e = co.Engine(fmm_order=4, **opts)
        d, prm = _state(oracle32, n)
        e.compute_force(kind, d, n, prm)
        if field:
            e.integrate_b(scheme, kind, d, n, prm, dt, zero)
            e.integrate_steps_b(scheme, kind, d, n, prm, dt, steps, zero)
        else:
            e.integrate(scheme, kind, d, n, prm, dt)
            e.integrate_steps(scheme, kind, d, n, prm, dt, steps)
        torch.cuda.synchronize()
        out.append(d.clone())
        e.close()
    assert torch.equal(out[0].view(torch.int32), out[1].view(torch.int32))


@pytest.mark.parametrize("scheme_name,kind_name,opts", [("INTEG_PEFRL", "EVAL_FMM_KDTREE", dict(unsort=0)), ("INTEG_LEAPFROG", "EVAL_FMM_KDTREE", dict(unsort=1)),
                                                        ("INTEG_LEAPFROG", "EVAL_DIRECT", dict()), ("INTEG_FORESTRUTH", "EVAL_FMM_TRACELESS", dict())])
def test_other_compositions_loop(oracle32, scheme_name, kind_name, opts):
    import torch
    import coulomb_oscillators_amd as co
    scheme, kind = getattr(co, scheme_name), getattr(co, kind_name)
    n, steps, dt, om = 8192, 3, 5e-4, (300.0, -200.0, 700.0)
    out = []
    for fused in (False, True):
        e = co.Engine(fmm_order=4, **opts)
        d, prm = _state(oracle32, n)
        e.compute_force(kind, d, n, prm)
        if fused:
            e.integrate_steps_b(scheme, kind, d, n, prm, dt, steps, om)
        else:
            for _ in range(steps):
                e.integrate_b(scheme, kind, d, n, prm, dt, om)
        torch.cuda.synchronize()
        out.append(d.clone())
        e.close()
    assert torch.isfinite(out[0]).all()
    assert torch.equal(out[0].view(torch.int32), out[1].view(torch.int32))


# ---- refusals and context state ---------------------------------------------------------------------------------------------------
def test_refusals_leave_state_and_context_alone(oracle32):
    import torch
    from coulomb_oscillators_amd import Engine, EngineError, EVAL_FMM_KDTREE, INTEG_LEAPFROG
    n, dt, om = 8192, 5e-4, (300.0, -200.0, 700.0)
    live, fresh = Engine(fmm_order=4, unsort=0), Engine(fmm_order=4, unsort=0)
    d, prm = _state(oracle32, n)
    live.compute_force(EVAL_FMM_KDTREE, d, n, prm)
    live.integrate_steps_b(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, dt, 2, om)
    torch.cuda.synchronize()
    before = d.clone()
    bad = [dict(omega=(np.nan, 0.0, 0.0)), dict(omega=(0.0, np.inf, 1.0)), dict(scheme=7), dict(scheme=-1), dict(kind=9), dict(kind=-1)]
    for case in bad:
        a = dict(scheme=INTEG_LEAPFROG, kind=EVAL_FMM_KDTREE, omega=om)
        a.update(case)
        for steps in (None, 3):
            with pytest.raises(EngineError) as ei:
                if steps is None:
                    live.integrate_b(a["scheme"], a["kind"], d, n, prm, dt, a["omega"])
                else:
                    live.integrate_steps_b(a["scheme"], a["kind"], d, n, prm, dt, steps, a["omega"])
            assert ei.value.status == 2, case                                      # NBCO_ERR_ARG
            torch.cuda.synchronize()
            assert torch.equal(d.view(torch.int32), before.view(torch.int32)), case
    with pytest.raises(EngineError):
        live.drift_b(d[0], d[1], n, (0.0, np.nan, 0.0), 1.0)
    assert live.lib.nbco_integrate_b(live.ctx, INTEG_LEAPFROG, EVAL_FMM_KDTREE, d.data_ptr(), n, prm.data_ptr(), dt, 1.0, 1, None) == 2      # NULL omega3_host
    assert live.lib.nbco_integrate_steps_b(live.ctx, INTEG_LEAPFROG, EVAL_FMM_KDTREE, d.data_ptr(), n, prm.data_ptr(), dt, 1.0, 1, 3, None) == 2
    torch.cuda.synchronize()
    assert torch.equal(d.view(torch.int32), before.view(torch.int32))
    # the refused context evaluates like a fresh one
    x1, x2 = before.clone(), before.clone()
    live.set(unsort=1)
    fresh.set(unsort=1)
    live.compute_force(EVAL_FMM_KDTREE, x1, n, prm)
    fresh.compute_force(EVAL_FMM_KDTREE, x2, n, prm)
    torch.cuda.synchronize()
    assert torch.equal(x1.view(torch.int32), x2.view(torch.int32))
    live.close()
    fresh.close()


def test_context_state_after_a_magnetic_step(oracle32):
    """a scheme that ends on a drift leaves the particles moved: nbco_kd_probe refuses, as after nbco_integrate; a leapfrog step ends on
    an evaluation, and nbco_kd_potential gives what it gives after the same step driven call by call"""
    import torch
    from coulomb_oscillators_amd import Engine, EngineError, EVAL_FMM_KDTREE, INTEG_LEAPFROG, INTEG_FORESTRUTH
    n, dt, om = 8192, 5e-4, (300.0, -200.0, 700.0)
    e = Engine(fmm_order=4, unsort=1)
    d, prm = _state(oracle32, n)
    probes = d[0][:16].clone()
    a_out = torch.zeros(16, 3, dtype=torch.float64, device="cuda")
    e.compute_force(EVAL_FMM_KDTREE, d, n, prm)
    e.probe_kd(probes, 16, prm, a=a_out)                                       # fine after an evaluation
    e.integrate_b(INTEG_FORESTRUTH, EVAL_FMM_KDTREE, d, n, prm, dt, om)
    with pytest.raises(EngineError, match="moved the particles"):
        e.probe_kd(probes, 16, prm, a=a_out)
    e.compute_force(EVAL_FMM_KDTREE, d, n, prm)
    e.drift_b(d[0], d[1], n, om, dt)
    with pytest.raises(EngineError, match="moved the particles"):
        e.probe_kd(probes, 16, prm, a=a_out)
    e.close()
    res = []
    for whole in (True, False):
        e = Engine(fmm_order=4, unsort=1)
        d, prm = _state(oracle32, n)
        e.compute_force(EVAL_FMM_KDTREE, d, n, prm)
        if whole:
            e.integrate_b(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, dt, om)
        else:
            ds = float(np.float32(np.longdouble(dt) * 0.5))
            e.step(d[1], d[2], ds, n)
            e.drift_b(d[0], d[1], n, om, dt)
            e.compute_force(EVAL_FMM_KDTREE, d, n, prm)
            e.step(d[1], d[2], ds, n)
        phi = torch.zeros(n, dtype=torch.float64, device="cuda")
        en = e.energy_kd(d, n, prm, phi)
        torch.cuda.synchronize()
        res.append((d.clone(), phi, en))
        e.close()
    assert torch.equal(res[0][0].view(torch.int32), res[1][0].view(torch.int32))
    assert torch.equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])


# ---- 2-D --------------------------------------------------------------------------------------------------------------------------
OMEGA_2D = 700.0       # omega dt = 0.35 at the 2-D tests' dt


@pytest.mark.parametrize("kind", [0, 2], ids=["direct", "fmm"])
@pytest.mark.parametrize("scheme", [0, 1, 2, 3, 4])
def test_2d_schemes_against_model(engine, scheme, kind):
    """n = 2048, p = 5, two steps against fmm2d_numpy's forces under the model's sequences with the rotated drift, within 1e-10 (the
    bound test_gpu_fmm2d.py holds the integrators to); integrate_steps_b_2d equals the calls, and a second run is bit-identical"""
    import torch
    import fmm2d_numpy as F
    from coulomb_oscillators_amd import init2d
    n, p, dt, steps = 2048, 5, 5e-4, 2
    eps2 = float(np.float32(1e-18))
    engine.set(fmm_order=p, eps2=1e-18, tree_radius=1.0, coll=1, dens_inhom=1.0, tree_L=0)
    A, om, xi, om0 = F.kv_params()
    st = init2d(n, "kv", A, om)
    ph = np.array([xi / n, 0.0, om0[0] ** 2, om0[1] ** 2])
    prm = dev(ph)
    buf0 = np.concatenate([st.reshape(-1), np.zeros(2 * n)])
    k = np.array(ph[2:])

    def f(b):
        if kind < 2:
            b[2] = F.direct(b[0], eps2, ph[0])
        else:
            out, a = F.fmm(b[:2].copy(), p, eps2, ph)
            b[:2] = out
            b[2] = a
        b[2] -= k * b[0]
    ref = bf.integrate_2d(scheme, buf0.copy().reshape(3, n, 2), f, dt, OMEGA_2D, steps=steps)
    d = dev(buf0.copy())
    for _ in range(steps):
        engine.integrate_b_2d(scheme, kind, d, n, prm, dt, OMEGA_2D)
    got = d.cpu().numpy().reshape(3, n, 2)
    for q in range(3):
        mag = np.linalg.norm(ref[q], axis=1)
        err = float((np.linalg.norm(got[q] - ref[q], axis=1) / (mag + mag.mean())).max())
        print("scheme %d kind %d part %d: %.2e" % (scheme, kind, q, err))
        assert err <= 1e-10, q
    plain = F.integrate(scheme, buf0.copy().reshape(3, n, 2), f, dt, steps=steps)
    assert np.abs(plain[1] - ref[1]).max() > 1e-3 * np.abs(ref[1]).max()        # the field was there
    for _ in range(2):
        d2 = dev(buf0.copy())
        engine.integrate_steps_b_2d(scheme, kind, d2, n, prm, dt, steps, OMEGA_2D)
        assert torch.equal(d.view(torch.int64), d2.view(torch.int64))
    d3 = dev(buf0.copy())
    d4 = dev(buf0.copy())
    engine.integrate_steps_b_2d(scheme, kind, d3, n, prm, dt, steps, 0.0)
    engine.integrate_steps_2d(scheme, kind, d4, n, prm, dt, steps)
    assert torch.equal(d3.view(torch.int64), d4.view(torch.int64))               # omega = 0 is the plain call


@pytest.mark.parametrize("n", [1, 2, 3, 257])
def test_2d_drift_b(engine, n):
    """fp64: three roundings per component against the model's one, relative to the largest component"""
    rng = np.random.default_rng(n)
    state = rng.normal(size=(2, n, 2))
    for s in (0.7, -1.3):
        want = bf.drift(state[0], state[1], 0.9, s)
        d = dev(state)
        engine.drift_b_2d(d[0], d[1], n, 0.9, s)
        got = d.cpu().numpy()
        for q in range(2):
            assert ig.rel_dist(got[q], want[q]) <= 8 * np.finfo(np.float64).eps, (n, s, q)
    with pytest.raises(Exception):
        engine.drift_b_2d(d[0], d[1], n, np.nan, 1.0)
