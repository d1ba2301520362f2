"""The Langevin bath restated over numpy (include/nbco.h, nbco_bath_apply): Philox4x32-10 in uint64 arithmetic, the noise xi, the
coefficients in numpy.longdouble, the step v' = (c1 v) + (c2 xi) in the state's own precision -- which is the engine's rule to the bit --
and the five schemes wrapped in the two half steps, O(dt/2, half 0) S(dt) O(dt/2, half 1).  Test infrastructure; nothing here is shared
with the engine.

The sub-step sequence of a scheme comes from bfield_numpy.sequence, which reads it off integrators3d_numpy.integrate."""
import numpy as np

import bfield_numpy as bf
import integrators3d_numpy as ig

LD = np.longdouble
U64 = np.uint64
M32 = U64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = U64(0xD2511F53), U64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = U64(0x9E3779B9), U64(0xBB67AE85)
XI_SCALE = float.fromhex("0x1.bb67ae8584caap-32")      # sqrt(3) 2^-32
XI_CENTRE = 0x1FFFFFFFE                                # 4 (2^32 - 1) / 2


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (or scalars) of one shape, key: two uint32 scalars; returns the four output words as uint64 arrays below
    2^32.  Ten rounds, the key bumped between them; every product is a 32 x 32 -> 64 bit one and fits uint64."""
    c = [np.asarray(w, dtype=U64) & M32 for w in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = U64(int(key[0]) & 0xFFFFFFFF), U64(int(key[1]) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c[0], PHILOX_M1 * c[2]
        c = [(p1 >> U64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> U64(32)) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c


def xi(seed, tick, half, rows, axis):
    """float64 noise of the rows `rows` on `axis`: key = the seed's two words, counter = (row, axis + 4 half, the tick's two words); the
    four words summed as an integer, centred, times sqrt(3) 2^-32 (one rounding: the integer is below 2^34 in size, so exact in fp64)"""
    seed, tick = int(seed), int(tick)
    rows = np.asarray(rows, dtype=U64)
    w = philox4x32_10((rows, U64(axis + 4 * half), U64(tick & 0xFFFFFFFF), U64(tick >> 32)), (seed & 0xFFFFFFFF, seed >> 32))
    s = (w[0] + w[1] + w[2] + w[3]).astype(np.int64) - np.int64(XI_CENTRE)
    return s.astype(np.float64) * XI_SCALE


def coeffs_ld(gamma, kT, s):
    """(c1, c2) in numpy.longdouble from the formulas: c1 = exp(-gamma s), c2 = sqrt(kT (1 - exp(-2 gamma s))), the latter through expm1"""
    g, t, s = np.array([LD(float(q)) for q in gamma]), np.array([LD(float(q)) for q in kT]), LD(float(s))
    return np.exp(-g * s), np.sqrt(t * -np.expm1(-2 * g * s))


def kick(v, c1, c2, seed, tick, half, rows=None):
    """O on the velocities v[n, dim] in v's own dtype (float32 or float64): the coefficients (float64, from nbco_bath_coeffs) narrowed to
    that dtype once, xi narrowed to it, each product and the sum rounded once.  An axis with c1 = 1 and c2 = 0 after narrowing is left
    alone.  rows: the particles' rows in the state (default 0 .. n - 1).  Returns a new array."""
    v = np.array(v)
    t = v.dtype.type
    rows = np.arange(v.shape[0]) if rows is None else rows
    for a in range(v.shape[1]):
        a1, a2 = t(c1[a]), t(c2[a])
        if a1 == 1 and a2 == 0:
            continue
        v[:, a] = (a1 * v[:, a]) + (a2 * xi(seed, tick, half, rows, a).astype(t))
    return v


class Bath:
    """gamma, kT per axis and the seed; coeffs: the function that forms (c1, c2) for a step s -- the engine's bath_coeffs where the bytes
    are compared, coeffs_ld (the default) where the model stands alone"""

    def __init__(self, gamma, kT, seed, coeffs=None):
        self.gamma, self.kT, self.seed = tuple(gamma), tuple(kT), int(seed)
        self.coeffs = coeffs or (lambda g, t, s: tuple(np.asarray(c, dtype=np.float64) for c in coeffs_ld(g, t, s)))

    def half_step(self, v, dt, tick, half):
        c1, c2 = self.coeffs(self.gamma, self.kT, 0.5 * dt)
        return kick(v, c1, c2, self.seed, tick, half)


def integrate(scheme, force, x, v, a, dt, bath, tick, omega=None, scale=1.0, dtype=np.float64):
    """one step O S O in `dtype`; omega: None, or the uniform field whose helix drift replaces D (bfield_numpy)"""
    t = dtype
    x, v, a = (np.array(q, dtype=t) for q in (x, v, a))
    v = bath.half_step(v, dt, tick, 0)
    for op in bf.sequence(scheme, dt, scale):
        if op[0] == "K":
            v = v + a * t(op[1])
        elif op[0] == "D":
            if omega is None:
                x = x + v * t(op[1])
            else:
                x, v = (bf.drift_f32 if t is np.float32 else bf.drift)(x, v, omega, op[1])
        else:
            a = np.asarray(force(x), dtype=t)
    v = bath.half_step(v, dt, tick, 1)
    return x, v, a


def run(scheme, force, x, v, dt, steps, bath, tick0=0, omega=None, scale=1.0, dtype=np.float64):
    """force once, then `steps` steps at the ticks tick0 ..; returns the (x, v, a) after every step"""
    x, v = np.array(x, dtype=dtype), np.array(v, dtype=dtype)
    a = np.asarray(force(x), dtype=dtype)
    out = []
    for k in range(steps):
        x, v, a = integrate(scheme, force, x, v, a, dt, bath, tick0 + k, omega, scale, dtype)
        out.append((x, v, a))
    return out


def integrate_2d(scheme, buf, f, dt, bath, tick0=0, omega=0.0, scale=1.0, steps=1):
    """the 2-D form in the conventions of fmm2d_numpy.integrate and bfield_numpy.integrate_2d: buf = [x, v, a] (each [n, 2], float64),
    f(buf) evaluates a in place and may re-order the state -- the noise is keyed by the row at the moment O is applied"""
    for k in range(steps):
        buf[1] = bath.half_step(buf[1], dt, tick0 + k, 0)
        for op in bf.sequence(scheme, dt, scale):
            if op[0] == "K":
                buf[1] += buf[2] * op[1]
            elif op[0] == "D":
                if omega == 0.0:
                    buf[0] += buf[1] * op[1]
                else:
                    buf[0], buf[1] = bf.drift(buf[0], buf[1], omega, op[1])
            else:
                f(buf)
        buf[1] = bath.half_step(buf[1], dt, tick0 + k, 1)
    return buf


def free_bath_run(v, dt, steps, bath, tick0=0):
    """velocities of free particles (a = 0: the kicks add nothing) after `steps` steps: the two half bath steps per step, nothing else"""
    v = np.array(v)
    for k in range(steps):
        v = bath.half_step(v, dt, tick0 + k, 0)
        v = bath.half_step(v, dt, tick0 + k, 1)
    return v


KNOWN_ANSWERS = [        # (counter, key, output): the first and the third are the published Random123 vectors
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]
