"""nbco_integrate_steps: `steps` steps in one call.  Bar: the final state equals `steps` calls of nbco_integrate BIT FOR BIT -- the
fused pass between two force evaluations (kd_turnaround_kernel: tree order, elastic term, two half kicks, drift, next build's
prologue) performs the same operations with the same roundings as the four kernels it replaces."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _state(oracle32, n):
    import torch
    buf = oracle32.init_reference(n)
    return torch.from_numpy(buf.copy()).cuda(), torch.from_numpy(oracle32.params(n)).cuda()


@pytest.mark.parametrize("n,p,tree_steps,elastic,steps", [(20000, 4, 1, True, 5), (20000, 4, 1, False, 3), (65536, 6, 3, True, 8), (65536, 5, 8, True, 11),
                                                          (100000, 3, 2, True, 4), (5000, 6, 1, True, 4)])
def test_fused_leapfrog_equals_step_by_step(oracle32, n, p, tree_steps, elastic, steps):
    import torch
    from coulomb_oscillators_amd import Engine, EVAL_FMM_KDTREE, INTEG_LEAPFROG
    dt = 5e-4
    out = []
    for fused in (False, True):
        e = Engine(fmm_order=p, unsort=0, tree_steps=tree_steps)
        d, prm = _state(oracle32, n)
        e.compute_force(EVAL_FMM_KDTREE, d, n, prm, elastic=elastic)
        if fused:
            e.integrate_steps(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, dt, steps, elastic=elastic)
            # and the engine is in a state from which step-by-step calls carry on identically
            e.integrate(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, dt, elastic=elastic)
            e.integrate_steps(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, dt, 2, elastic=elastic)
        else:
            for _ in range(steps + 3):
                e.integrate(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, dt, elastic=elastic)
        torch.cuda.synchronize()
        assert torch.isfinite(d).all()
        out.append(d.clone())
        e.close()
    assert torch.equal(out[0][0], out[1][0]), "positions differ"
    assert torch.equal(out[0][1], out[1][1]), "velocities differ"
    assert torch.equal(out[0][2], out[1][2]), "accelerations differ"


@pytest.mark.parametrize("scheme_name,kind_name,opts", [("INTEG_PEFRL", "EVAL_FMM_KDTREE", dict(unsort=0)), ("INTEG_LEAPFROG", "EVAL_FMM_KDTREE", dict(unsort=1)),
                                                        ("INTEG_LEAPFROG", "EVAL_DIRECT", dict()), ("INTEG_LEAPFROG", "EVAL_FMM_KDTREE", dict(unsort=0, track_order=1)),
                                                        ("INTEG_FORESTRUTH", "EVAL_FMM_TRACELESS", dict())])
def test_everything_else_loops(oracle32, scheme_name, kind_name, opts):
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
            e.integrate_steps(scheme, kind, d, n, prm, dt, steps)
        else:
            for _ in range(steps):
                e.integrate(scheme, kind, d, n, prm, dt)
        torch.cuda.synchronize()
        out.append(d.clone())
        e.close()
    assert torch.equal(out[0], out[1])


def test_one_step_and_zero_steps(oracle32):
    import torch
    from coulomb_oscillators_amd import Engine, EVAL_FMM_KDTREE, INTEG_LEAPFROG
    n = 8192
    e = Engine(fmm_order=4, unsort=0)
    d, prm = _state(oracle32, n)
    e.compute_force(EVAL_FMM_KDTREE, d, n, prm)
    before = d.clone()
    e.integrate_steps(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, 5e-4, 0)
    torch.cuda.synchronize()
    assert torch.equal(d, before)
    e.integrate_steps(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d, n, prm, 5e-4, 1)
    e2 = Engine(fmm_order=4, unsort=0)
    d2 = before.clone()
    e2.compute_force(EVAL_FMM_KDTREE, d2, n, prm)   # (same tree state as e had)
    d2.copy_(before)
    e2.integrate(INTEG_LEAPFROG, EVAL_FMM_KDTREE, d2, n, prm, 5e-4)
    torch.cuda.synchronize()
    assert torch.equal(d, d2)


@pytest.mark.parametrize("tree_steps", [1, 3])
def test_refused_evaluation_inside_a_fused_run_leaves_the_context_sound(oracle32, tree_steps):
    """an evaluation refused in the middle of nbco_integrate_steps (list overflow with list_factor = 1, list_grow = 0; a rebuild with
    tree_steps = 1, a tree-reuse evaluation with 3) leaves nothing behind in the context: with the state put back and the lists
    at their default size, the engine carries on bit for bit like a twin that was never refused anything"""
    import torch
    from coulomb_oscillators_amd import Engine, EngineError, EVAL_FMM_KDTREE, INTEG_LEAPFROG
    n, p, dt = 65536, 6, 5e-4
    live, twin = (Engine(fmm_order=p, unsort=0, tree_steps=tree_steps) for _ in range(2))
    d, prm = _state(oracle32, n)
    states = {live: d, twin: d.clone()}
    for e, s in states.items():
        e.compute_force(EVAL_FMM_KDTREE, s, n, prm)
        e.integrate_steps(INTEG_LEAPFROG, EVAL_FMM_KDTREE, s, n, prm, dt, 3)
    torch.cuda.synchronize()
    saved = states[live].clone()
    live.set(list_factor=1, list_grow=0)
    with pytest.raises(EngineError, match="list capacity"):
        live.integrate_steps(INTEG_LEAPFROG, EVAL_FMM_KDTREE, states[live], n, prm, dt, 4)
    live.set(list_factor=48, list_grow=1)
    torch.cuda.synchronize()
    states[live].copy_(saved)
    for e, s in states.items():
        e.integrate_steps(INTEG_LEAPFROG, EVAL_FMM_KDTREE, s, n, prm, dt, 5)
        for _ in range(2):
            e.integrate(INTEG_LEAPFROG, EVAL_FMM_KDTREE, s, n, prm, dt)
    torch.cuda.synchronize()
    assert torch.isfinite(states[live]).all()
    for part, name in enumerate(("positions", "velocities", "accelerations")):
        assert torch.equal(states[live][part], states[twin][part]), name + " differ"
    live.close()
    twin.close()


def test_plain_calls_refuse_before_any_launch(oracle32):
    """nbco_integrate and nbco_integrate_steps refuse an unknown scheme or kind (also with steps = 0) and a kd-tree call over the 32-bit
    index limit before their first launch, as their _b and _t forms do: the state keeps its bytes, and the refused context goes on bit for
    bit like a twin that was never refused anything"""
    import ctypes as C
    import torch
    from coulomb_oscillators_amd import Engine, EngineError, EVAL_FMM_KDTREE, INTEG_LEAPFROG
    n, dt = 5000, 5e-4
    live, twin = Engine(fmm_order=4, unsort=0), Engine(fmm_order=4, unsort=0)
    d, prm = _state(oracle32, n)
    d2 = d.clone()
    for e, s in ((live, d), (twin, d2)):
        e.compute_force(EVAL_FMM_KDTREE, s, n, prm)
        e.integrate_steps(INTEG_LEAPFROG, EVAL_FMM_KDTREE, s, n, prm, dt, 2)
    torch.cuda.synchronize()
    assert torch.equal(d.view(torch.int32), d2.view(torch.int32))
    before = d.clone()
    for case in (dict(scheme=7), dict(scheme=-1), dict(kind=9), dict(kind=-1)):
        a = dict(scheme=INTEG_LEAPFROG, kind=EVAL_FMM_KDTREE)
        a.update(case)
        for steps in (None, 3, 0):
            with pytest.raises(EngineError) as ei:
                if steps is None:
                    live.integrate(a["scheme"], a["kind"], d, n, prm, dt)
                else:
                    live.integrate_steps(a["scheme"], a["kind"], d, n, prm, dt, steps)
            assert ei.value.status == 2, (case, steps)                             # NBCO_ERR_ARG
            torch.cuda.synchronize()
            assert torch.equal(d.view(torch.int32), before.view(torch.int32)), (case, steps)
    L, ptr, pp = live.lib, C.c_void_p(d.data_ptr()), C.c_void_p(prm.data_ptr())
    big = 0x7fffffff // 4 + 1                                                      # refused before the buffer is read
    assert L.nbco_integrate(live.ctx, INTEG_LEAPFROG, EVAL_FMM_KDTREE, ptr, big, pp, dt, 1.0, 1) == 4                 # NBCO_ERR_UNSUPPORTED
    assert L.nbco_integrate_steps(live.ctx, INTEG_LEAPFROG, EVAL_FMM_KDTREE, ptr, big, pp, dt, 1.0, 1, 3) == 4
    torch.cuda.synchronize()
    assert torch.equal(d.view(torch.int32), before.view(torch.int32))
    probes = before[0][:16].clone()
    res = []
    for e, s in ((live, d), (twin, d2)):
        a_out = torch.zeros(16, 3, dtype=torch.float64, device="cuda")
        en = e.energy_fmm(s, n, prm)
        e.probe_kd(probes, 16, prm, a=a_out)
        e.integrate_steps(INTEG_LEAPFROG, EVAL_FMM_KDTREE, s, n, prm, dt, 2)
        torch.cuda.synchronize()
        res.append((en, a_out, s.clone()))
    assert res[0][0] == res[1][0] and torch.equal(res[0][1], res[1][1])
    assert torch.equal(res[0][2].view(torch.int32), res[1][2].view(torch.int32))
    live.close()
    twin.close()
