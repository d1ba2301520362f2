"""The Langevin bath on the GPU: nbco_bath_apply against the numpy model of tests/bath_numpy.py bit for bit, nbco_integrate_t against the
sequence of calls it stands for, the fused leapfrog passes of nbco_integrate_steps_t against the step-by-step calls, bit for bit, the
refusals, the statistics of a device run, and the 2-D forms."""
import functools

import numpy as np
import pytest

import bath_numpy as bn
import integrators3d_numpy as ig

pytestmark = pytest.mark.gpu

GRID_CAP, PER_THREAD, BLOCK = 2048, 4, 256          # k_axpy.hip: stream_grid's cap, particles per thread of the vector kernel, kBlock
N_TWICE = GRID_CAP * BLOCK * PER_THREAD + 5         # more than one grid pass of the vector kernel (aligned v) and a tail; the size test_gpu_bfield.py uses
SEED = 0x0123456789ABCDEF                           # both words non-zero
GAMMA, KT = (1.0, 0.0, 2.5), (0.5, 1.0, 0.0)        # anisotropic: the y axis is left alone (gamma = 0), the z axis is cooled only (kT = 0)
S_HALF = 0.35


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _coeffs():
    from coulomb_oscillators_amd import bath_coeffs
    return bath_coeffs


@functools.lru_cache(maxsize=2)
def _input(n):
    return np.random.default_rng(4000 + n).normal(size=(2, n, 3)).astype(np.float32)


@functools.lru_cache(maxsize=2)
def _model(n, half, tick):
    """the float32 model on _input(n)'s velocities, computed once per case and shared by the aligned and the packed call"""
    c1, c2 = _coeffs()(GAMMA, KT, S_HALF)
    want = bn.kick(_input(n)[1], c1, c2, SEED, tick, half)
    want.setflags(write=False)
    return want


# ---- O alone --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tick", [0, 7, 2 ** 32 + 5])
@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 256, 257, 4099, N_TWICE])
def test_bath_apply_is_the_model_bit_for_bit(engine, n, half, tick):
    """v as a tensor of its own (16-byte aligned: n / 4 vector groups of four particles, then the tail one particle per lane) and as
    buf + 3 n of a packed state (off the 16-byte grid when n % 4 != 0: one particle per lane throughout): both are the model's bytes, the
    y axis keeps the bytes it had, and x is not touched.  This test fails without the feature."""
    state = _input(n)
    want = _model(n, half, tick)
    v = dev(state[1])
    assert v.data_ptr() % 16 == 0
    engine.bath_apply(v, n, GAMMA, KT, S_HALF, half, tick, seed=SEED)
    got = v.cpu().numpy()
    assert got.tobytes() == want.tobytes(), ("aligned", n, half, tick, int((got != want).sum()))
    d = dev(state)
    assert (d[1].data_ptr() % 16 != 0) == (n % 4 != 0)
    engine.bath_apply(d[1], n, GAMMA, KT, S_HALF, half, tick, seed=SEED)
    got = d.cpu().numpy()
    assert got[1].tobytes() == want.tobytes(), ("packed", n, half, tick, int((got[1] != want).sum()))
    assert got[0].tobytes() == state[0].tobytes()
    assert got[1][:, 1].tobytes() == state[1][:, 1].tobytes()
    if n >= 255:
        assert not np.array_equal(got[1][:, 0], state[1][:, 0]) and not np.array_equal(got[1][:, 2], state[1][:, 2])
        c1 = np.float32(_coeffs()(GAMMA, KT, S_HALF)[0][2])
        assert np.array_equal(got[1][:, 2], c1 * state[1][:, 2])          # kT = 0: friction alone


def test_bath_apply_prefix_second_call_and_streams(engine):
    """a row's new v depends on (seed, tick, half, row, its old v) and nothing else: the first m rows of a call over n are a call over m;
    a second call returns the same bytes; another seed word, tick word or half gives another stream"""
    import torch
    n = 4099
    state = _input(n)
    full = dev(state[1])
    engine.bath_apply(full, n, GAMMA, KT, S_HALF, 1, 7, seed=SEED)
    for m in (1, 5, 256, 1030, 4098):
        part = dev(state[1][:m].copy())
        engine.bath_apply(part, m, GAMMA, KT, S_HALF, 1, 7, seed=SEED)
        assert torch.equal(part.view(torch.int32), full[:m].view(torch.int32)), m
    again = dev(state[1])
    engine.bath_apply(again, n, GAMMA, KT, S_HALF, 1, 7, seed=SEED)
    assert torch.equal(again.view(torch.int32), full.view(torch.int32))
    for kw in (dict(seed=SEED + 1), dict(seed=SEED + (1 << 32)), dict(tick=8), dict(tick=7 + (1 << 32)), dict(half=0)):
        a = dict(seed=SEED, tick=7, half=1)
        a.update(kw)
        other = dev(state[1])
        engine.bath_apply(other, n, GAMMA, KT, S_HALF, a["half"], a["tick"], seed=a["seed"])
        assert not torch.equal(other[:, 0], full[:, 0]), kw
    # n = 0 is accepted and does nothing
    engine.bath_apply(full, 0, GAMMA, KT, S_HALF, 1, 7, seed=SEED)
    assert torch.equal(again.view(torch.int32), full.view(torch.int32))


# ---- one step: O S O ------------------------------------------------------------------------------------------------------------
def _state(oracle32, n):
    return dev(oracle32.init_reference(n).copy()), dev(oracle32.params(n))


OMEGA = (300.0, -200.0, 700.0)        # |Omega| dt = 0.39 at dt = 5e-4
BATH = dict(gamma=(400.0, 0.0, 1500.0), kT=(2e-6, 1.0, 0.0))      # gamma dt = 0.2 and 0.75 at dt = 5e-4; kT of the order of the initial v^2


@pytest.mark.parametrize("field", [False, True], ids=["plain", "omega"])
@pytest.mark.parametrize("kind_name,n", [("EVAL_DIRECT", 257), ("EVAL_FMM_KDTREE", 5000)])
@pytest.mark.parametrize("scheme", ig.SCHEMES, ids=[ig.NAMES[s] for s in ig.SCHEMES])
def test_integrate_t_is_the_sequence_of_calls(oracle32, scheme, kind_name, n, field):
    """nbco_integrate_t against [bath_apply half 0, nbco_integrate or _b, bath_apply half 1] on a second context, three steps"""
    import torch
    import coulomb_oscillators_amd as co
    kind, dt, om = getattr(co, kind_name), 5e-4, OMEGA if field else None
    out = []
    for whole in (True, False):
        e = co.Engine(fmm_order=4, unsort=0)
        d, prm = _state(oracle32, n)
        e.compute_force(kind, d, n, prm)
        for tick in (5, 6, 7):
            if whole:
                e.integrate_t(scheme, kind, d, n, prm, dt, BATH["gamma"], BATH["kT"], tick, seed=SEED, omega=om)
            else:
                e.bath_apply(d[1], n, BATH["gamma"], BATH["kT"], 0.5 * dt, 0, tick, seed=SEED)
                if field:
                    e.integrate_b(scheme, kind, d, n, prm, dt, om)
                else:
                    e.integrate(scheme, kind, d, n, prm, dt)
                e.bath_apply(d[1], n, BATH["gamma"], BATH["kT"], 0.5 * dt, 1, tick, seed=SEED)
        torch.cuda.synchronize()
        assert torch.isfinite(d).all()
        out.append(d.clone())
        e.close()
    assert torch.equal(out[0].view(torch.int32), out[1].view(torch.int32))
    # the bath was there
    e = co.Engine(fmm_order=4, unsort=0)
    d, prm = _state(oracle32, n)
    e.compute_force(kind, d, n, prm)
    for _ in range(3):
        if field:
            e.integrate_b(scheme, kind, d, n, prm, dt, om)
        else:
            e.integrate(scheme, kind, d, n, prm, dt)
    torch.cuda.synchronize()
    e.close()
    assert not torch.equal(d[1], out[0][1])


# ---- fused equals step by step --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", [False, True], ids=["plain", "omega"])
@pytest.mark.parametrize("n,p,tree_steps,steps", [(20000, 4, 1, 5), (65536, 6, 3, 8), (5000, 6, 1, 4), (20003, 4, 1, 5), (5001, 6, 2, 4)])
def test_fused_leapfrog_equals_step_by_step(oracle32, n, p, tree_steps, steps, field):
    """kd_turnaround_kernel<., ., Bath3> against `steps` calls of integrate_t; afterwards one integrate_t and two more fused steps carry on
    identically (the pattern of test_gpu_bfield.py), the ticks running on.  Omega = 0 and |Omega| dt = 0.39."""
    import torch
    from coulomb_oscillators_amd import Engine, EVAL_FMM_KDTREE, INTEG_LEAPFROG
    dt, om, t0 = 5e-4, OMEGA if field else None, 2 ** 32 - 3      # the tick's low word wraps inside the fused run
    g, kT = BATH["gamma"], BATH["kT"]
    out = []
    for fused in (False, True):
        e = Engine(fmm_order=p, unsort=0, tree_steps=tree_steps)
        d, prm = _state(oracle32, n)
        e.compute_force(EVAL_FMM_KDTREE, d, n, prm)
        if fused:
            e.integrate_steps_t(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, dt, steps, g, kT, t0, seed=SEED, omega=om)
            e.integrate_t(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, dt, g, kT, t0 + steps, seed=SEED, omega=om)
            e.integrate_steps_t(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, dt, 2, g, kT, t0 + steps + 1, seed=SEED, omega=om)
        else:
            for k in range(steps + 3):
                e.integrate_t(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, dt, g, kT, t0 + k, seed=SEED, omega=om)
        torch.cuda.synchronize()
        assert torch.isfinite(d).all()
        out.append(d.clone())
        e.close()
    for part, name in enumerate(("positions", "velocities", "accelerations")):
        assert torch.equal(out[0][part].view(torch.int32), out[1][part].view(torch.int32)), name + " differ"
    # and the bath was there: the run without it ends elsewhere
    e = Engine(fmm_order=p, unsort=0, tree_steps=tree_steps)
    d, prm = _state(oracle32, n)
    e.compute_force(EVAL_FMM_KDTREE, d, n, prm)
    if field:
        e.integrate_steps_b(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, dt, steps + 3, om)
    else:
        e.integrate_steps(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, dt, steps + 3)
    torch.cuda.synchronize()
    e.close()
    assert not torch.equal(d[1], out[1][1])


@pytest.mark.parametrize("scheme_name,kind_name,opts", [("INTEG_PEFRL", "EVAL_FMM_KDTREE", dict(unsort=0)), ("INTEG_LEAPFROG", "EVAL_FMM_KDTREE", dict(unsort=1)),
                                                        ("INTEG_LEAPFROG", "EVAL_DIRECT", dict()), ("INTEG_FORESTRUTH", "EVAL_FMM_TRACELESS", dict())])
def test_other_compositions_loop(oracle32, scheme_name, kind_name, opts):
    import torch
    import coulomb_oscillators_amd as co
    scheme, kind = getattr(co, scheme_name), getattr(co, kind_name)
    n, steps, dt = 8192, 3, 5e-4
    out = []
    for fused in (False, True):
        e = co.Engine(fmm_order=4, **opts)
        d, prm = _state(oracle32, n)
        e.compute_force(kind, d, n, prm)
        if fused:
            e.integrate_steps_t(scheme, kind, d, n, prm, dt, steps, BATH["gamma"], BATH["kT"], 40, seed=SEED, omega=OMEGA)
        else:
            for k in range(steps):
                e.integrate_t(scheme, kind, d, n, prm, dt, BATH["gamma"], BATH["kT"], 40 + k, seed=SEED, omega=OMEGA)
        torch.cuda.synchronize()
        out.append(d.clone())
        e.close()
    assert torch.isfinite(out[0]).all()
    assert torch.equal(out[0].view(torch.int32), out[1].view(torch.int32))


# ---- gamma = 0 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", [False, True], ids=["plain", "omega"])
@pytest.mark.parametrize("scheme_name,kind_name,opts", [("INTEG_LEAPFROG", "EVAL_FMM_KDTREE", dict(unsort=0, tree_steps=2)), ("INTEG_PEFRL", "EVAL_FMM_KDTREE", dict(unsort=0)),
                                                        ("INTEG_FORESTRUTH", "EVAL_DIRECT", dict())])
def test_zero_rates_are_the_counterpart(oracle32, scheme_name, kind_name, opts, field):
    """every gamma exactly 0, whatever kT: the bytes and nbco_kd_get_info of nbco_integrate(_steps) (no field) and of the _b calls"""
    import torch
    import coulomb_oscillators_amd as co
    scheme, kind = getattr(co, scheme_name), getattr(co, kind_name)
    n, steps, dt, zero, kT = 8192, 3, 5e-4, (0.0, 0.0, 0.0), (1.0, 2.0, 3.0)
    out = []
    for bath in (False, True):
        e = co.Engine(fmm_order=4, **opts)
        d, prm = _state(oracle32, n)
        e.compute_force(kind, d, n, prm)
        if bath:
            e.integrate_t(scheme, kind, d, n, prm, dt, zero, kT, 3, seed=SEED, omega=OMEGA if field else None)
            e.integrate_steps_t(scheme, kind, d, n, prm, dt, steps, zero, kT, 4, seed=SEED, omega=OMEGA if field else None)
        elif field:
            e.integrate_b(scheme, kind, d, n, prm, dt, OMEGA)
            e.integrate_steps_b(scheme, kind, d, n, prm, dt, steps, OMEGA)
        else:
            e.integrate(scheme, kind, d, n, prm, dt)
            e.integrate_steps(scheme, kind, d, n, prm, dt, steps)
        torch.cuda.synchronize()
        info = bytes(e.kd_info()) if kind == co.EVAL_FMM_KDTREE else b""
        out.append((d.clone(), info))
        e.close()
    assert torch.equal(out[0][0].view(torch.int32), out[1][0].view(torch.int32))
    assert out[0][1] == out[1][1]


# ---- refusals and context state -------------------------------------------------------------------------------------------------
def test_refusals_leave_state_and_context_alone(oracle32):
    import ctypes as C
    import torch
    from coulomb_oscillators_amd import Engine, EngineError, EVAL_FMM_KDTREE, INTEG_LEAPFROG
    from coulomb_oscillators_amd.engine import Bath
    n, dt = 8192, 5e-4
    live, fresh = Engine(fmm_order=4, unsort=0), Engine(fmm_order=4, unsort=0)
    d, prm = _state(oracle32, n)
    d2 = d.clone()
    for e, s in ((live, d), (fresh, d2)):
        e.compute_force(EVAL_FMM_KDTREE, s, n, prm)
        e.integrate_steps_t(INTEG_LEAPFROG, EVAL_FMM_KDTREE, s, n, prm, dt, 2, BATH["gamma"], BATH["kT"], 0, seed=SEED, omega=OMEGA)
    torch.cuda.synchronize()
    assert torch.equal(d.view(torch.int32), d2.view(torch.int32))
    before = d.clone()
    good = dict(scheme=INTEG_LEAPFROG, kind=EVAL_FMM_KDTREE, gamma=BATH["gamma"], kT=BATH["kT"], omega=OMEGA, dt=dt)
    bad = [dict(gamma=(np.nan, 0.0, 0.0)), dict(gamma=(1.0, -1.0, 0.0)), dict(gamma=(0.0, np.inf, 0.0)), dict(kT=(0.0, -1e-30, 0.0)), dict(kT=(np.nan, 1.0, 1.0)),
           dict(kT=(np.inf, 1.0, 1.0)), dict(gamma=(0.0, 0.0, 0.0), kT=(-1.0, 0.0, 0.0)), dict(scheme=7), dict(scheme=-1), dict(kind=9), dict(kind=-1),
           dict(omega=(np.nan, 0.0, 0.0)), dict(dt=-dt), dict(dt=np.nan)]
    for case in bad:
        a = dict(good)
        a.update(case)
        for steps in (None, 3):
            with pytest.raises(EngineError) as ei:
                if steps is None:
                    live.integrate_t(a["scheme"], a["kind"], d, n, prm, a["dt"], a["gamma"], a["kT"], 2, seed=SEED, omega=a["omega"])
                else:
                    live.integrate_steps_t(a["scheme"], a["kind"], d, n, prm, a["dt"], steps, a["gamma"], a["kT"], 2, seed=SEED, omega=a["omega"])
            assert ei.value.status == 2, case                                      # NBCO_ERR_ARG
            torch.cuda.synchronize()
            assert torch.equal(d.view(torch.int32), before.view(torch.int32)), case
    for kw in (dict(half=2), dict(half=-1), dict(s=-0.1), dict(s=np.nan), dict(gamma=(0.0, -2.0, 0.0)), dict(kT=(0.0, np.nan, 0.0))):
        a = dict(half=0, s=0.5 * dt, gamma=BATH["gamma"], kT=BATH["kT"])
        a.update(kw)
        with pytest.raises(EngineError) as ei:
            live.bath_apply(d[1], n, a["gamma"], a["kT"], a["s"], a["half"], 2, seed=SEED)
        assert ei.value.status == 2, kw
    b = Bath((C.c_double * 3)(*BATH["gamma"]), (C.c_double * 3)(*BATH["kT"]), SEED)
    L, ptr = live.lib, C.c_void_p(d.data_ptr())
    vptr = C.c_void_p(d[1].data_ptr())
    assert L.nbco_integrate_t(live.ctx, INTEG_LEAPFROG, EVAL_FMM_KDTREE, ptr, n, C.c_void_p(prm.data_ptr()), dt, 1.0, 1, None, None, 0) == 2       # NULL bath
    assert L.nbco_integrate_steps_t(live.ctx, INTEG_LEAPFROG, EVAL_FMM_KDTREE, ptr, n, C.c_void_p(prm.data_ptr()), dt, 1.0, 1, 3, None, None, 0) == 2
    assert L.nbco_bath_apply(live.ctx, vptr, n, None, 0.5 * dt, 0, 0) == 2
    assert L.nbco_bath_apply(live.ctx, vptr, 2 ** 31, C.byref(b), 0.5 * dt, 0, 0) == 4                                                               # NBCO_ERR_UNSUPPORTED
    assert L.nbco_integrate_t(live.ctx, INTEG_LEAPFROG, 0, ptr, 2 ** 31, C.c_void_p(prm.data_ptr()), dt, 1.0, 1, None, C.byref(b), 0) == 4
    assert L.nbco_2d_bath_apply(live.ctx, vptr, 2 ** 31, C.byref(b), 0.5 * dt, 0, 0) == 4
    torch.cuda.synchronize()
    assert torch.equal(d.view(torch.int32), before.view(torch.int32))
    # the refused context goes on like the one that was never refused: the diagnostics of the last evaluation, then a step
    probes = before[0][:16].clone()
    res = []
    for e, s in ((live, d), (fresh, d2)):
        a_out = torch.zeros(16, 3, dtype=torch.float64, device="cuda")
        en = e.energy_fmm(s, n, prm)
        e.probe_kd(probes, 16, prm, a=a_out)
        e.integrate_steps_t(INTEG_LEAPFROG, EVAL_FMM_KDTREE, s, n, prm, dt, 2, BATH["gamma"], BATH["kT"], 2, seed=SEED, omega=OMEGA)
        torch.cuda.synchronize()
        res.append((en, a_out, s.clone()))
    assert res[0][0] == res[1][0] and torch.equal(res[0][1], res[1][1])
    assert torch.equal(res[0][2].view(torch.int32), res[1][2].view(torch.int32))
    live.close()
    fresh.close()


def test_bath_apply_leaves_the_context_state_alone(oracle32):
    """positions do not move: after bath_apply alone nbco_kd_probe is still accepted and gives what it gave"""
    import torch
    from coulomb_oscillators_amd import Engine, EVAL_FMM_KDTREE
    n = 8192
    e = Engine(fmm_order=4, unsort=1)
    d, prm = _state(oracle32, n)
    probes = d[0][:16].clone()
    a1 = torch.zeros(16, 3, dtype=torch.float64, device="cuda")
    a2 = torch.zeros(16, 3, dtype=torch.float64, device="cuda")
    e.compute_force(EVAL_FMM_KDTREE, d, n, prm)
    e.probe_kd(probes, 16, prm, a=a1)
    x_before = d[0].clone()
    e.bath_apply(d[1], n, BATH["gamma"], BATH["kT"], 2.5e-4, 0, 0, seed=SEED)
    e.probe_kd(probes, 16, prm, a=a2)
    torch.cuda.synchronize()
    assert torch.equal(a1, a2) and torch.equal(d[0], x_before)
    e.close()


# ---- statistics on the device ---------------------------------------------------------------------------------------------------
def test_free_particles_reach_the_bath_temperature(engine):
    """n = 65536 free particles (param[0] = 0, elastic = 0), cold start, gamma = 1, dt = 0.5, kT = (0.5, 1, 2), seed 12345, 40 leapfrog steps
    over the direct evaluator (which keeps the rows): per axis |<v^2> / kT - 1| <= 5 sqrt(2 / n) = 0.0276, five standard errors of a
    variance estimate at a kurtosis of at most 3.  The velocities equal the float32 model's: a = 0, so the kicks add a zero and a step is
    its two half bath steps (compared as values: a kick may turn a -0 into +0)."""
    from coulomb_oscillators_amd import EVAL_DIRECT, INTEG_LEAPFROG, bath_coeffs
    n, dt, steps, gamma, kT, seed = 65536, 0.5, 40, (1.0, 1.0, 1.0), (0.5, 1.0, 2.0), 12345
    rng = np.random.default_rng(1)
    state = np.zeros((3, n, 3), dtype=np.float32)
    state[0] = rng.normal(size=(n, 3))
    d = dev(state)
    prm = dev(np.zeros(6, dtype=np.float32))
    engine.compute_force(EVAL_DIRECT, d, n, prm, elastic=False)
    engine.integrate_steps_t(INTEG_LEAPFROG, EVAL_DIRECT, d, n, prm, dt, steps, gamma, kT, 0, seed=seed, elastic=False)
    got = d.cpu().numpy()
    assert np.isfinite(got).all()
    bound = 5 * np.sqrt(2.0 / n)
    for a in range(3):
        dev_a = float((got[1][:, a].astype(np.float64) ** 2).mean() / kT[a] - 1)
        print("axis %d: <v^2> / kT - 1 = %+.2e (bound %.4f)" % (a, dev_a, bound))
        assert abs(dev_a) <= bound
    want = bn.free_bath_run(state[1], dt, steps, bn.Bath(gamma, kT, seed, coeffs=bath_coeffs))
    assert np.array_equal(got[1], want)


# ---- 2-D ------------------------------------------------------------------------------------------------------------------------
BATH_2D = dict(gamma=(400.0, 1500.0), kT=(3e-4, 0.0))


@pytest.mark.parametrize("n", [1, 2, 3, 257])
def test_2d_bath_apply_is_the_model_bit_for_bit(engine, n):
    from coulomb_oscillators_amd import bath_coeffs
    v0 = np.random.default_rng(n).normal(size=(n, 2))
    for half, tick in ((0, 0), (1, 7), (0, 2 ** 32 + 5)):
        c1, c2 = bath_coeffs(GAMMA[:2], KT[:2], S_HALF)
        want = bn.kick(v0, c1, c2, SEED, tick, half)
        v = dev(v0)
        engine.bath_apply_2d(v, n, GAMMA[:2], KT[:2], S_HALF, half, tick, seed=SEED)
        got = v.cpu().numpy()
        assert got.tobytes() == want.tobytes(), (n, half, tick)
        assert got[:, 1].tobytes() == v0[:, 1].tobytes()                   # gamma = 0
    with pytest.raises(Exception):
        engine.bath_apply_2d(v, n, (np.nan, 0.0), KT[:2], S_HALF, 0, 0)


@pytest.mark.parametrize("n", [1, 2, 3, 257])
@pytest.mark.parametrize("kind", [0, 2], ids=["direct", "fmm"])
@pytest.mark.parametrize("scheme", [0, 1, 2, 3, 4])
def test_2d_schemes_against_model(engine, scheme, kind, n):
    """the first n particles of a KV beam of 257, p = 5, two steps against fmm2d_numpy's forces under the model's sequences wrapped in the bath's half steps, within 1e-10 (the bound
    test_gpu_fmm2d.py holds the integrators to: the forces of the two sides differ in their last bits; the bath step itself is exact);
    integrate_steps_t_2d equals the calls bit for bit, a second run is identical, and gamma = 0 is the plain call"""
    import torch
    import fmm2d_numpy as F
    from coulomb_oscillators_amd import init2d, bath_coeffs
    p, dt, steps, t0 = 5, 5e-4, 2, 2 ** 32 - 1
    eps2 = float(np.float32(1e-18))
    engine.set(fmm_order=p, eps2=1e-18, tree_radius=1.0, coll=1, dens_inhom=1.0, tree_L=0)
    A, om, xi, om0 = F.kv_params()
    st = init2d(257, "kv", A, om)[:, :n].copy()      # (the first n of a beam of 257: init2d centres and scales by the beam's own rms, which one particle does not have)
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
    g, kT = BATH_2D["gamma"], BATH_2D["kT"]
    model = bn.Bath(g, kT, SEED, coeffs=lambda gg, tt, s: tuple(c[:2] for c in bath_coeffs(gg, tt, s)))
    ref = bn.integrate_2d(scheme, buf0.copy().reshape(3, n, 2), f, dt, model, tick0=t0, steps=steps)
    d = dev(buf0.copy())
    for s in range(steps):
        engine.integrate_t_2d(scheme, kind, d, n, prm, dt, g, kT, t0 + s, seed=SEED)
    got = d.cpu().numpy().reshape(3, n, 2)
    for q in range(3):
        mag = np.linalg.norm(ref[q], axis=1)
        err = float((np.linalg.norm(got[q] - ref[q], axis=1) / (mag + mag.mean())).max())
        print("scheme %d kind %d n %d part %d: %.2e" % (scheme, kind, n, q, err))
        assert err <= 1e-10, q
    plain = F.integrate(scheme, buf0.copy().reshape(3, n, 2), f, dt, steps=steps)
    assert np.abs(plain[1] - ref[1]).max() > 1e-3 * np.abs(ref[1]).max()        # the bath was there
    for _ in range(2):
        d2 = dev(buf0.copy())
        engine.integrate_steps_t_2d(scheme, kind, d2, n, prm, dt, steps, g, kT, t0, seed=SEED)
        assert torch.equal(d.view(torch.int64), d2.view(torch.int64))
    d3 = dev(buf0.copy())
    d4 = dev(buf0.copy())
    engine.integrate_steps_t_2d(scheme, kind, d3, n, prm, dt, steps, (0.0, 0.0), (1.0, 2.0), t0, seed=SEED)
    engine.integrate_steps_2d(scheme, kind, d4, n, prm, dt, steps)
    assert torch.equal(d3.view(torch.int64), d4.view(torch.int64))               # gamma = 0 is the plain call
