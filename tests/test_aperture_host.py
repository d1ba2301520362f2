"""The fp64 reference of the aperture (tests/aperture_numpy.py) on hand-made points whose answer can be read off the rule of
include/nbco.h -- the half axes are powers of two, so w = 1 / half, u = d w and u u are exact -- and the source rule its kernels
depend on.  No GPU.  (`nbco3 -cpu -aperture` is held to the same model in test_cli_aperture.py.)"""
import os
import re

import numpy as np
import pytest

import aperture_numpy as AP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "coulomb_oscillators_amd", "csrc")
INF, NAN = np.inf, np.nan


def up(v, dtype):
    """the next value of dtype away from zero"""
    v = dtype(v)
    return np.nextafter(v, dtype(np.copysign(np.inf, v)))


@pytest.mark.parametrize("dtype,dim", [(np.float32, 3), (np.float64, 2)])
def test_surface_points_are_inside_and_one_ulp_beyond_is_outside(dtype, dim):
    half = np.array([2.0, 0.5, 4.0][:dim])
    centre = np.array([8.0, -2.0, 16.0][:dim])          # exact in both types, as are centre +- half; |centre +- half| >= 2 half, so that
                                                        # one ulp of the coordinate is a whole number of ulps of d = x - centre
    for shape in (AP.ELLIPSOID, AP.BOX):
        for a in range(dim):
            for sign in (-1.0, 1.0):
                on = centre.copy()
                on[a] += sign * half[a]
                pts = np.array([on, on], dtype=dtype)
                pts[1, a] = np.nextafter(pts[1, a], dtype(sign * np.inf))      # one ulp further out along the axis
                got = AP.inside(pts, shape, half, centre)
                assert got.tolist() == [True, False], (shape, a, sign, pts)
    # s == 1 from two axes: u = (0.6, 0.8) is not exact, but u = (1, 0) and a diagonal of the box are
    corner = np.array([centre + half, centre - half], dtype=dtype)
    assert AP.inside(corner, AP.BOX, half, centre).all()
    assert not AP.inside(corner, AP.ELLIPSOID, half, centre).any()      # s = dim > 1
    assert AP.inside(np.array([centre], dtype=dtype), AP.ELLIPSOID, half, centre).all()


@pytest.mark.parametrize("dtype,dim", [(np.float32, 3), (np.float64, 2)])
def test_an_open_axis_decides_nothing_and_non_finite_coordinates_are_outside(dtype, dim):
    big = dtype(1e30)
    half = np.array([2.0, INF, 4.0][:dim])
    z = [0.0] * (dim - 2)
    pts = np.array([[0.0, big] + z, [0.0, -big] + z, [2.0, big] + z, [up(2.0, dtype), 0.0] + z,      # a pipe along y
                    [0.0, INF] + z, [0.0, -INF] + z, [0.0, NAN] + z, [NAN, 0.0] + z, [INF, 0.0] + z], dtype=dtype)
    want = [True, True, True, False, False, False, False, False, False]
    for shape in (AP.ELLIPSOID, AP.BOX):
        assert AP.inside(pts, shape, half).tolist() == want, shape
    # every axis open: only the non-finite rows are lost
    assert AP.inside(pts, AP.BOX, [INF] * dim).tolist() == [True] * 4 + [False] * 5
    assert AP.inside(pts, AP.ELLIPSOID, [INF] * dim).tolist() == [True] * 4 + [False] * 5


def test_the_two_summation_orders():
    """(u_x u_x + u_y u_y) + u_z u_z, not u_x u_x + (u_y u_y + u_z u_z): with e = 1.2 * 2^-27, e e = 0.72 * 2^-53 is below half an
    ulp of 1 and 2 e e above it, so the two orders round to different sides of 1"""
    e = np.float32(1.2 * 2.0 ** -27)
    p = np.array([[e, e, 1.0], [1.0, e, e]], dtype=np.float32)
    u = p.astype(np.float64)
    left = (u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2]
    right = u[:, 0] * u[:, 0] + (u[:, 1] * u[:, 1] + u[:, 2] * u[:, 2])
    assert (left <= 1.0).tolist() == [False, True] and (right <= 1.0).tolist() == [True, False]
    assert AP.inside(p, AP.ELLIPSOID, np.ones(3)).tolist() == [False, True]
    # 2-D: one sum, nothing to order
    q = np.array([[0.6, 0.8], [1.0, 0.0], [np.nextafter(1.0, 2.0), 0.0]])
    s = q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]
    assert np.array_equal(AP.inside(q, AP.ELLIPSOID, [1.0, 1.0]), s <= 1.0) and AP.inside(q, AP.ELLIPSOID, [1.0, 1.0])[1]


def test_w_is_one_over_half_not_a_division_per_particle():
    """u = d * (1 / half) and d / half differ in the last bit for most half axes: the model multiplies"""
    half = np.array([0.0075, 0.0025, 0.025])
    rng = np.random.default_rng(3)
    v = rng.standard_normal((200000, 3))
    v /= np.sqrt((v * v).sum(axis=1))[:, None]
    p = (v * half).astype(np.float32)
    x = p.astype(np.float64)
    u, q = x * (1.0 / half), x / half
    s_mul = (u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2]
    s_div = (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]
    got = AP.inside(p, AP.ELLIPSOID, half)
    assert np.array_equal(got, s_mul <= 1.0)
    assert 0 < got.sum() < len(p) and (s_mul != s_div).any()


def test_apply_is_a_stable_compaction_with_its_record():
    rng = np.random.default_rng(11)
    n = 1000
    st = rng.standard_normal((3, n, 3)).astype(np.float32)
    st[0, 5] = NAN
    kept, lost, rows = AP.apply(st, AP.BOX, [1.0, INF, 1.5], [0.1, 0.0, 0.0])
    keep = AP.inside(st[0], AP.BOX, [1.0, INF, 1.5], [0.1, 0.0, 0.0])
    assert 0 < keep.sum() < n and not keep[5]
    assert kept.shape == (3, keep.sum(), 3) and lost.shape == (n - keep.sum(), 6) and rows.dtype == np.int32
    assert np.array_equal(rows, np.nonzero(~keep)[0]) and np.all(np.diff(rows) > 0)
    assert kept.tobytes() == st[:, keep].tobytes()
    assert lost.tobytes() == np.concatenate([st[0, ~keep], st[1, ~keep]], axis=1).tobytes()
    again, lost2, rows2 = AP.apply(kept, AP.BOX, [1.0, INF, 1.5], [0.1, 0.0, 0.0])
    assert again.tobytes() == kept.tobytes() and len(rows2) == 0 and lost2.shape == (0, 6)


def test_the_rule_is_compiled_without_contraction():
    """as tests/test_source_rules.py: the pragma in force where aperture_inside is defined"""
    state = "default"
    for line in open(os.path.join(CSRC, "aperture_kernels.hpp")):
        m = re.search(r"#pragma clang fp contract\((\w+)\)", line)
        if m:
            state = m.group(1)
        if re.search(r"\baperture_inside\s*\(", line) and "__device__" in line:
            assert state == "off"
            break
    else:
        raise AssertionError("definition of aperture_inside not found")
    mk = open(os.path.join(ROOT, "coulomb_oscillators_amd", "host", "Makefile")).read()
    assert re.search(r"-ffp-contract=off[^\n]*nbco3\.cpp", mk)      # nbco_cpu::aperture_inside
