"""The five 3-D schemes of integrator.cuh:32-167 restated over fp64 numpy arrays: the sub-step sequence and every constant spelled
out, the force a callback.  Test infrastructure: the yardstick of tests/test_integrators3d_host.py and of the integrator tests in
tests/test_gpu_yardsticks.py.  Nothing here is shared with the oracle or the engine; the constants are typed from the reference's
text (integrator.cuh:98 and :130-132).

    K(s): v += a s        D(s): x += v s        F: a = force(x)

A scheme takes the acceleration of the incoming positions in `a` (the caller evaluates the force once before the first step) and
leaves the acceleration of the last force evaluation there.  `scale` multiplies every kick and no drift."""
import numpy as np

EULER, PRE_EULER, LEAPFROG, FORESTRUTH, PEFRL = 0, 1, 2, 3, 4
NAMES = {EULER: "euler", PRE_EULER: "pre_euler", LEAPFROG: "leapfrog", FORESTRUTH: "forestruth", PEFRL: "pefrl"}

CONSTANTS = {
    "fr_par": 1.3512071919596576340476878089715,       # 1 / (2 - 2^(1/3)), integrator.cuh:98
    "pefrl_parx": +0.1786178958448091E+00,             # integrator.cuh:130
    "pefrl_parl": -0.2123418310626054E+00,             # :131
    "pefrl_parc": -0.6626458266981849E-01,             # :132
    "leapfrog_half": 0.5,                              # the two half kicks of leapfrog, :68-96
}
# which schemes a constant enters
USED_BY = {"fr_par": (FORESTRUTH,), "pefrl_parx": (PEFRL,), "pefrl_parl": (PEFRL,), "pefrl_parc": (PEFRL,), "leapfrog_half": (LEAPFROG,)}


def integrate(scheme, force, x, v, a, dt, scale=1.0, consts=CONSTANTS):
    """one step; returns the new (x, v, a) and leaves its arguments alone"""
    x, v, a = (np.array(t, dtype=np.float64) for t in (x, v, a))
    st = {"x": x, "v": v, "a": a}

    def K(s):
        st["v"] = st["v"] + st["a"] * s

    def D(s):
        st["x"] = st["x"] + st["v"] * s

    def F():
        st["a"] = np.asarray(force(st["x"]), dtype=np.float64)

    ds = dt * scale
    if scheme == EULER:                                                  # symplectic_euler, :32-48
        K(ds); D(dt); F()
    elif scheme == PRE_EULER:                                            # pre_symplectic_euler, :50-66
        F(); K(ds); D(dt)
    elif scheme == LEAPFROG:                                             # leapfrog, :68-96
        h = consts["leapfrog_half"]
        K(ds * h); D(dt); F(); K(ds * h)
    elif scheme == FORESTRUTH:                                           # forestruth, :98-128
        th = consts["fr_par"]
        D(dt * th / 2); F()
        K(ds * th); D(dt * (1 - th) / 2); F()
        K(ds * (1 - 2 * th)); D(dt * (1 - th) / 2); F()
        K(ds * th); D(dt * th / 2)
    elif scheme == PEFRL:                                                # pefrl, :130-167
        xi, la, ch = consts["pefrl_parx"], consts["pefrl_parl"], consts["pefrl_parc"]
        D(dt * xi); F()
        K(ds * (1 - 2 * la) / 2); D(dt * ch); F()
        K(ds * la); D(dt * (1 - 2 * (ch + xi))); F()
        K(ds * la); D(dt * ch); F()
        K(ds * (1 - 2 * la) / 2); D(dt * xi)
    else:
        raise ValueError("unknown scheme %r" % (scheme,))
    return st["x"], st["v"], st["a"]


def run(scheme, force, x, v, dt, steps, scale=1.0, consts=CONSTANTS):
    """force once, then `steps` steps (main3.cu:832-846); returns the (x, v, a) after every step"""
    x = np.array(x, dtype=np.float64)
    v = np.array(v, dtype=np.float64)
    a = np.asarray(force(x), dtype=np.float64)
    out = []
    for _ in range(steps):
        x, v, a = integrate(scheme, force, x, v, a, dt, scale, consts)
        out.append((x, v, a))
    return out


def elastic_force(k):
    """a = -k o x"""
    k = np.asarray(k, dtype=np.float64)
    return lambda x: -k * x


def rel_dist(got, want):
    """largest deviation relative to the largest component of `want`"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max())


# ---- the elastic-only comparison shared by tests/test_integrators3d_host.py and tests/test_gpu_yardsticks.py ----------------------
# a = -k o x alone (param[0] = 0 switches the Coulomb sum off), the reference's initial state, a step at which the constants show
N, DT, STEPS = 256, 1.0, 6
SCALES = (1.0, 0.5)
SCHEMES = (EULER, PRE_EULER, LEAPFROG, FORESTRUTH, PEFRL)
GPU_TOL_FACTOR, GPU_TOL_CAP = 4.0, 1e-5      # fma against mul + add; the cap keeps a broken oracle from loosening the bound


def elastic_only_input(oracle32):
    """(buf fp32 [pos|vel|acc], par fp32 with param[0] = 0)"""
    buf = oracle32.init_reference(N)
    par = oracle32.params(N)
    par[0] = 0
    return buf, par


def restated(buf, par, scheme, scale, consts=CONSTANTS, steps=STEPS):
    """final (x, v) of the fp64 restatement on the fp32 input"""
    k = par[3:6].astype(np.float64)
    x, v, _ = run(scheme, elastic_force(k), buf[0], buf[1], DT, steps, scale, consts)[-1]
    return x, v


def oracle_run(o, buf, par, scheme, scale, steps=STEPS):
    """final (x, v) of the oracle `o` (fp32 or fp64) on the same input: force once, then `steps` steps"""
    from oracle import pyoracle as po
    b = np.array(buf, dtype=o.dtype, order="C")          # a copy: the oracle integrates in place
    p = np.array(par, dtype=o.dtype)
    o.compute_force(po.KIND_DIRECT3, b, p, elastic=True)
    for _ in range(steps):
        o.integrate(scheme, po.KIND_DIRECT3, b, p, DT, scale, elastic=True)
    return b[0], b[1]


def oracle32_floor(oracle32, buf, par, scheme, scale):
    """distance of the fp32 oracle from the restatement, (x, v)"""
    want = restated(buf, par, scheme, scale)
    got = oracle_run(oracle32, buf, par, scheme, scale)
    return tuple(rel_dist(g, w) for g, w in zip(got, want))


def gpu_tolerance(floor, factor=GPU_TOL_FACTOR, cap=GPU_TOL_CAP):
    return tuple(min(factor * f, cap) for f in floor)
