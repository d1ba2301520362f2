#!/usr/bin/env python3
"""Randomised differential run of the kd-tree evaluator against the oracle (GPU box): python tools/fuzz_kd.py [--one-context] [seed] [cases]
Tree arrays and interaction lists must be identical; forces are compared with the fp32 oracle (1e-5) and, when they differ
more, with the fp64 oracle.  Both traversal orders are drawn (m2l_first), and a share of the cases runs
a short leapfrog sequence with tree reuse (unsort = 0, tree_steps = T) instead of one evaluation: at every evaluation the oracle is
given the positions the engine is about to evaluate and rebuilds / reuses its tree as the engine must
(tests/test_gpu_fmm_kd_driver.py has the scheme).  --one-context keeps ONE context for the whole run and takes it from case to case
with nbco_set_opts, as nbco3 does, instead of creating one per case: the walk through random (n, p, r) then also meets the launch
estimates, grown scratch and sticky build modes that the case before left behind (tests/test_gpu_context_reuse.py)."""
import sys, time, numpy as np, torch
import os; ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
from coulomb_oscillators_amd import Engine
from oracle.pyoracle import Oracle
from nbutil import force_err, canon_pairs
ONE_CONTEXT = "--one-context" in sys.argv
sys.argv = [a for a in sys.argv if a != "--one-context"]
_shared = None
def context(**opts):
    """the context of a case: a new one, or (--one-context) the run's only one, set to the case's options"""
    global _shared
    if not ONE_CONTEXT: return Engine(**opts)
    full = dict(unsort=1, tree_steps=1, tree_radius=1.0, dens_inhom=1.0, m2l_first=0); full.update(opts)
    if _shared is None: _shared = Engine(**full)
    else: _shared.set(**full)
    return _shared
def release(e):
    if not ONE_CONTEXT: e.close()
o = Oracle(np.float32)
rng = np.random.default_rng(int(sys.argv[1]) if len(sys.argv) > 1 else 1)
bad = 0
def arbitrate(got, want, pv, par, okw):
    # both fp32 evaluations may simply be at the end of fp32 (tiny leaves at low order): then they are equally far from
    # the fp64 oracle and the case is not a defect of either.  (a reuse evaluation cannot be replayed in fp64 from its inputs alone)
    o64 = Oracle(np.float64)
    _, w64 = o64.fmm_kd(pv.astype(np.float64), par.astype(np.float64), threads=8, **okw)
    eg, ec = force_err(got, w64), force_err(want, w64)
    return eg <= 2 * ec + 1e-6, f" [vs fp64: gpu {eg:.2e}, fp32 oracle {ec:.2e}]"
def reuse_case(n, p, buf, par, radius, dens, m2l_first, T, evals, dt):
    """0 = every evaluation of the sequence agrees with the oracle, 1 otherwise"""
    e = context(fmm_order=p, unsort=0, tree_steps=T, tree_radius=radius, dens_inhom=dens, m2l_first=m2l_first)
    d = torch.from_numpy(buf.copy()).cuda(); prm = torch.from_numpy(par).cuda()
    ok, worst, changed, built = True, 0.0, 0, None
    for k in range(evals):
        if k: e.step(d[1], d[2], dt / 2, n); e.step(d[0], d[1], dt, n)
        x_in = d[:2].cpu().numpy()
        e.fmm_cart3_kdtree(d, d[2], n, prm); torch.cuda.synchronize()
        reuse = int(k % T != 0)
        pv, want = o.fmm_kd(x_in, par, p=p, threads=8, unsort=False, radius=radius, dens_inhom=dens, m2l_first=m2l_first, reuse=reuse)
        tree = o.kd_tree(); got = d.cpu().numpy()
        if not reuse: built = tree
        changed = max(changed, sum(len(np.setxor1d(canon_pairs(built[q]), canon_pairs(tree[q]))) for q in ("p2p", "m2l")))
        same = (e.kd_info().rebuilt == 1 - reuse and np.array_equal(got[:2], pv) and np.array_equal(e.kd_array("unsort"), o.kd_unsort(n))
                and all(np.array_equal(canon_pairs(e.kd_array(q)), canon_pairs(tree[q])) for q in ("p2p", "m2l"))
                and all(np.array_equal(e.kd_array(q), tree[q]) for q in ("index", "mult", "splitdim", "lbound", "rbound", "center")))
        err = force_err(got[2], want) if np.isfinite(want).all() else 0.0
        worst = max(worst, err)
        if not same or not err < 1e-5:
            ok = False; print(f"   evaluation {k} ({'reuse' if reuse else 'rebuild'}): state/tree/lists identical {same}, err {err:.2e}", flush=True)
        e.add_elastic(d[0], d[2], n, prm[3:])
        if k: e.step(d[1], d[2], dt / 2, n)
    print("OK " if ok else "BAD", f"n={n} p={p} r={radius} i={dens} m2l_first={m2l_first} reuse T={T} evals={evals} dt={dt:g} L={e.kd_info().L} worst err={worst:.2e} list entries changed {changed}", flush=True)
    release(e)
    return 0 if ok else 1
for it in range(int(sys.argv[2]) if len(sys.argv) > 2 else 40):
    n = int(rng.choice([rng.integers(2, 300), rng.integers(300, 9000), rng.integers(9000, 70000), rng.integers(70000, 300000)]))
    p = int(rng.integers(1, 9))
    kind = rng.choice(["gauss", "cube", "clumps", "quant", "dup"])
    radius = float(rng.choice([1.0, 1.0, 1.5, 2.0]))
    dens = float(rng.choice([1.0, 1.0, 0.5, 4.0]))
    m2l_first = int(rng.integers(0, 2))
    if kind == "gauss": buf = o.init_reference(n)
    elif kind == "cube": buf = o.init_reference(n, test_mode=True)
    else:
        buf = np.zeros((3, n, 3), dtype=np.float32)
        c = rng.standard_normal((8, 3)).astype(np.float32)
        buf[0] = c[rng.integers(0, 8, n)] + 0.05 * rng.standard_normal((n, 3)).astype(np.float32)
        if kind == "quant": buf[0] = (np.round(buf[0] / 2e-3) * 2e-3).astype(np.float32)
        if kind == "dup" and n > 10: buf[0, : n // 3] = buf[0, n // 3: 2 * (n // 3)][: n // 3]
    par = o.params(n)
    if kind in ("gauss", "cube") and n >= 300 and rng.integers(0, 3) == 0:
        # a moving state needs velocities: the reference's initial states have them
        T = int(rng.integers(2, 9))
        try: bad += reuse_case(n, p, buf, par, radius, dens, m2l_first, T, int(rng.integers(T, 2 * T + 2)), float(np.float32(rng.choice([5e-4, 5e-3, 2e-2]))))
        except Exception as ex: bad += 1; print("EXC", n, p, kind, radius, dens, "reuse", ex, flush=True)
        continue
    okw = dict(p=p, unsort=True, radius=radius, dens_inhom=dens, m2l_first=m2l_first)
    try:
        _, want = o.fmm_kd(buf[:2], par, threads=8, **okw)
    except Exception as ex:
        print("oracle failed", n, p, kind, ex); continue
    tree = o.kd_tree()
    e = context(fmm_order=p, unsort=1, tree_radius=radius, dens_inhom=dens, m2l_first=m2l_first)
    d = torch.from_numpy(buf[:2].copy()).cuda(); a = torch.zeros((n, 3), device="cuda"); prm = torch.from_numpy(par).cuda()
    try:
        e.fmm_cart3_kdtree(d, a, n, prm); torch.cuda.synchronize()
        got = a.cpu().numpy()
        fin = np.isfinite(want).all()
        err = force_err(got, want) if fin else float("nan")
        info = e.kd_info()
        same_lists = all(np.array_equal(canon_pairs(e.kd_array(k)), canon_pairs(tree[k])) for k in ("p2p", "m2l"))
        same_tree = all(np.array_equal(e.kd_array(k), tree[k]) for k in ("index", "mult", "splitdim", "lbound", "rbound"))
        ok = same_lists and same_tree and (not fin or err < 1e-5)
        note = ""
        if not ok and same_lists and same_tree and fin:
            ok, note = arbitrate(got, want, buf[:2], par, okw)
        if not ok: bad += 1
        if not same_lists:
            for k in ("p2p", "m2l"):
                ga, wa = canon_pairs(e.kd_array(k)), canon_pairs(tree[k])
                og, ow = np.setdiff1d(ga, wa), np.setdiff1d(wa, ga)
                fmt = lambda v: [(int(x) >> 32, int(x) & 0xFFFFFFFF) for x in v[:4]]
                print(f"   {k}: gpu {len(ga)} pairs, oracle {len(wa)}; only gpu {len(og)} {fmt(og)}, only oracle {len(ow)} {fmt(ow)}", flush=True)
        print("OK " if ok else "BAD", f"n={n} p={p} {kind} r={radius} i={dens} m2l_first={m2l_first} L={info.L} mode={info.build_mode} err={err:.2e} lists={same_lists} tree={same_tree}{note}", flush=True)
    except Exception as ex:
        bad += 1; print("EXC", n, p, kind, radius, dens, ex, flush=True)
    release(e)
print("bad:", bad)
