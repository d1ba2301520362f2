"""The uniform magnetic field restated over numpy: the helix matrices from the formulas of include/nbco.h in numpy.longdouble, the helix
drift, the five schemes with the drift D(s): x += v s replaced by it, and a float32 emulation (every multiply and every add rounded)
that gives the tolerance floors of tests/test_gpu_bfield.py.  Test infrastructure; nothing here is shared with the engine.

    w = |Omega|, n = Omega / w, N v = n x v, theta = w s
    R(s) = I - sin(theta) N + (1 - cos(theta)) N^2                          v <- R v
    A(s) = s I - ((1 - cos(theta)) / w) N + ((theta - sin(theta)) / w) N^2   x <- x + A v   (with the OLD v)

The sub-step sequences and their constants are those of tests/integrators3d_numpy.py: sequence() runs its integrate() once over
recording stand-ins for dt and scale and notes which kick, drift and force evaluation follow each other with which coefficient."""
import numpy as np

import integrators3d_numpy as ig

LD = np.longdouble


def _small(theta):
    """(1 - cos) and (theta - sin) in long double, without the cancellation at small theta"""
    vc = 2 * np.sin(theta / 2) ** 2
    if abs(theta) < 1:
        t2, term, tms, k = theta * theta, theta ** 3 / 6, LD(0), 1
        while term != 0 and k < 40:
            tms += term
            term = -term * t2 / ((2 * k + 2) * (2 * k + 3))
            k += 1
    else:
        tms = theta - np.sin(theta)
    return vc, tms


def matrices(omega, s):
    """(R, A), 3 x 3 numpy.longdouble"""
    o = np.array([LD(float(w)) for w in omega])
    s = LD(float(s))
    eye = np.eye(3, dtype=LD)
    w = np.sqrt((o * o).sum())
    if w == 0:
        return eye.copy(), s * eye
    n = o / w
    N = np.array([[0, -n[2], n[1]], [n[2], 0, -n[0]], [-n[1], n[0], 0]], dtype=LD)
    N2 = np.outer(n, n) - eye
    theta = w * s
    vc, tms = _small(theta)
    return eye - np.sin(theta) * N + vc * N2, s * eye - (vc / w) * N + (tms / w) * N2


def matrices_2d(omega, s):
    """(R, A), 2 x 2 numpy.longdouble; omega a scalar, N = [[0, -1], [1, 0]]"""
    w, s = LD(float(omega)), LD(float(s))
    eye = np.eye(2, dtype=LD)
    if w == 0:
        return eye.copy(), s * eye
    N = np.array([[0, -1], [1, 0]], dtype=LD)
    theta = w * s
    vc, tms = _small(theta)
    return eye - np.sin(theta) * N - vc * eye, s * eye - (vc / w) * N - (tms / w) * eye


def drift(x, v, omega, s):
    """the helix drift in fp64: (x + A v, R v); works for [n, 3] with a 3-vector omega and for [n, 2] with a scalar"""
    x, v = np.asarray(x, dtype=np.float64), np.asarray(v, dtype=np.float64)
    R, A = (matrices if x.shape[-1] == 3 else matrices_2d)(omega, s)
    R, A = R.astype(np.float64), A.astype(np.float64)
    return x + v @ A.T, v @ R.T


def drift_f32(x, v, omega, s):
    """the float32 emulation: the model's matrices narrowed to float32, then per component the sums of the engine's order with the
    multiply and the add rounded separately (the engine fuses each pair into one fmaf)"""
    f = np.float32
    x, v = np.asarray(x, dtype=f), np.asarray(v, dtype=f)
    R, A = matrices(omega, s)
    R, A = R.astype(f), A.astype(f)
    xn, vn = np.empty_like(x), np.empty_like(v)
    for c in range(3):
        xn[:, c] = ((x[:, c] + A[c, 0] * v[:, 0]) + A[c, 1] * v[:, 1]) + A[c, 2] * v[:, 2]
        vn[:, c] = (R[c, 0] * v[:, 0] + R[c, 1] * v[:, 1]) + R[c, 2] * v[:, 2]
    return xn, vn


# ---- the sub-step sequence of a scheme, read off integrators3d_numpy.integrate ------------------------------------------------------
class _Coef:
    """stands in for dt or scale: follows the scalar arithmetic of a coefficient and remembers whether `scale` entered (a kick)"""
    __array_ufunc__ = None      # ndarray * _Coef is ours (__rmul__), not numpy's

    def __init__(self, value, kick=False):
        self.value, self.kick = float(value), kick

    def __mul__(self, other):
        if isinstance(other, _Coef):
            return _Coef(self.value * other.value, self.kick or other.kick)
        if isinstance(other, np.ndarray):
            return _Term(self)
        return _Coef(self.value * other, self.kick)

    __rmul__ = __mul__

    def __truediv__(self, other):
        return _Coef(self.value / other, self.kick)


class _Term:
    """`array * coefficient`: adding it to the state is one sub-step, which is noted instead of carried out"""
    __array_ufunc__ = None
    log = None

    def __init__(self, coef):
        self.coef = coef

    def __radd__(self, state):
        _Term.log.append(("K" if self.coef.kick else "D", self.coef.value))
        return state


def sequence(scheme, dt, scale=1.0):
    """[("K", s) | ("D", s) | ("F",)] of one step, the coefficients as integrators3d_numpy.integrate forms them in fp64"""
    log = []
    _Term.log = log
    z = np.zeros(1)
    ig.integrate(scheme, lambda x: (log.append(("F",)), z)[1], z, z, z, _Coef(dt), _Coef(scale, kick=True))
    _Term.log = None
    return log


def integrate(scheme, force, x, v, a, dt, omega, scale=1.0, f32=False):
    """one step with the helix drift; f32: the float32 emulation (kicks and drifts in float32, multiply and add rounded separately;
    `force` must then return float32)"""
    t = np.float32 if f32 else np.float64
    x, v, a = (np.array(q, dtype=t) for q in (x, v, a))
    for op in sequence(scheme, dt, scale):
        if op[0] == "K":
            v = v + a * t(op[1])
        elif op[0] == "D":
            x, v = (drift_f32 if f32 else drift)(x, v, omega, op[1])
        else:
            a = np.asarray(force(x), dtype=t)
    return x, v, a


def run(scheme, force, x, v, dt, steps, omega, scale=1.0, f32=False):
    """force once, then `steps` steps; returns the (x, v, a) after every step"""
    t = np.float32 if f32 else np.float64
    x, v = np.array(x, dtype=t), np.array(v, dtype=t)
    a = np.asarray(force(x), dtype=t)
    out = []
    for _ in range(steps):
        x, v, a = integrate(scheme, force, x, v, a, dt, omega, scale, f32)
        out.append((x, v, a))
    return out


def integrate_2d(scheme, buf, f, dt, omega, scale=1.0, steps=1):
    """the 2-D form in the conventions of fmm2d_numpy.integrate: buf = [x, v, a] (each [n, 2]), f(buf) evaluates a in place (and may
    re-order the state); the same five sequences, the drift a rotation about the field out of the plane"""
    for _ in range(steps):
        for op in sequence(scheme, dt, scale):
            if op[0] == "K":
                buf[1] += buf[2] * op[1]
            elif op[0] == "D":
                buf[0], buf[1] = drift(buf[0], buf[1], omega, op[1])
            else:
                f(buf)
    return buf


def elastic_force_f32(k):
    k = np.asarray(k, dtype=np.float32)
    return lambda x: -k * x


# ---- closed forms -----------------------------------------------------------------------------------------------------------------
def free_helix(x0, v0, omega, t):
    """a free particle in the field after the time t: the flow itself"""
    return drift(x0, v0, omega, t)


def penning_orbit(x0, v0, kz, wc, t):
    """one particle in an ideal Penning trap, a = v x (0, 0, wc) - k o x with k = (-kz/2, -kz/2, kz), wc^2 > 2 kz: axial oscillation at
    sqrt(kz); in the plane u = x + i y obeys u'' = -i wc u' + (kz / 2) u, so u = c+ exp(-i w+ t) + c- exp(-i w- t) with the modified
    cyclotron and the magnetron frequency w+- = (wc +- sqrt(wc^2 - 2 kz)) / 2.  Returns (x, v) at t."""
    x0, v0 = np.asarray(x0, dtype=np.float64), np.asarray(v0, dtype=np.float64)
    wz = np.sqrt(kz)
    root = np.sqrt(wc * wc - 2 * kz)
    wp, wm = (wc + root) / 2, (wc - root) / 2
    u0, du0 = complex(x0[0], x0[1]), complex(v0[0], v0[1])
    # u0 = c+ + c-, du0 = -i (w+ c+ + w- c-)
    cp = (1j * du0 - wm * u0) / (wp - wm)
    cm = u0 - cp
    u = cp * np.exp(-1j * wp * t) + cm * np.exp(-1j * wm * t)
    du = -1j * (wp * cp * np.exp(-1j * wp * t) + wm * cm * np.exp(-1j * wm * t))
    z = x0[2] * np.cos(wz * t) + v0[2] / wz * np.sin(wz * t)
    dz = -x0[2] * wz * np.sin(wz * t) + v0[2] * np.cos(wz * t)
    return np.array([u.real, u.imag, z]), np.array([du.real, du.imag, dz])


ORDERS = {ig.EULER: 1, ig.PRE_EULER: 1, ig.LEAPFROG: 2, ig.FORESTRUTH: 4, ig.PEFRL: 4}
REVERSIBLE = (ig.LEAPFROG, ig.FORESTRUTH, ig.PEFRL)
OMEGA = (0.3, -0.2, 0.7)      # the oblique field of the elastic-only comparison
