"""CPU tests of the 3-D integrators' yardstick: the fp64 restatement of the five schemes (tests/integrators3d_numpy.py) against
oracle64.integrate, and the proof that the step chosen for the GPU comparison (tests/test_gpu_yardsticks.py) shows every constant.

The flow is the elastic force a = -k o x alone (the Coulomb constant param[0] is 0), n = 256 particles of the reference's initial
state, dt = 1.0, six steps: a linear map per step whose entries are polynomials in dt, scale and the scheme's constants, so that a
constant wrong by 1e-3 of its value moves the state by about 1e-3 of it -- at the suite's usual dt = 5e-4 the same mistake
moves it by less than fp32 rounding.

Measured (gcc oracle, x86-64): oracle32 against the fp64 restatement after six steps, the larger of x and v, relative to the
largest component:    scale 1.0    scale 0.5
    euler             6.3e-08      1.0e-07
    pre_euler         6.3e-08      1.0e-07      (the same states as euler: F K D after an initial F is K D F)
    leapfrog          8.4e-08      1.3e-07
    forestruth        1.3e-06      7.4e-07
    pefrl             2.6e-07      2.1e-07
The GPU tolerance is 4 x that figure (fma against mul + add), at most 1e-5, for x and v apart.  Shift of the final state for a 1e-3
change of one constant (the smaller of the two scales, the larger of x and v): fr_par 2.9e-03, pefrl_parx 4.9e-05, pefrl_parl
4.9e-05, pefrl_parc 4.1e-05, leapfrog half 3.6e-03, scale 2.2e-03 or more: 40 x the tolerance in the tightest case (PEFRL)."""
import numpy as np
import pytest

import integrators3d_numpy as ig
from integrators3d_numpy import SCALES, SCHEMES, elastic_only_input, gpu_tolerance, oracle32_floor, oracle_run, restated


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_restatement_agrees_with_the_fp64_oracle(oracle32, oracle64, scheme, scale):
    buf, par = elastic_only_input(oracle32)
    want = oracle_run(oracle64, buf, par, scheme, scale)
    got = restated(buf, par, scheme, scale)
    for g, w, name in zip(got, want, "xv"):
        assert np.isfinite(w).all() and np.abs(w).max() > 0
        assert ig.rel_dist(g, w) <= 1e-12, (ig.NAMES[scheme], name, ig.rel_dist(g, w))


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_the_state_stays_of_order_one(oracle32, scheme, scale):
    """the step is large but none of the schemes blows up over the six steps: the comparison is between numbers of the size of
    the initial state, not between overflowing ones"""
    buf, par = elastic_only_input(oracle32)
    x, v = restated(buf, par, scheme, scale)
    assert np.abs(x).max() < 100 * np.abs(buf[0]).max() and np.abs(v).max() < 100 * np.abs(buf[1]).max()


def test_the_oracle_run_leaves_its_input_alone(oracle32):
    """the oracle integrates in place; the shared input must still be the initial state for whoever starts from it next"""
    buf, par = elastic_only_input(oracle32)
    before = buf.copy()
    oracle_run(oracle32, buf, par, ig.LEAPFROG, 1.0)
    oracle32_floor(oracle32, buf, par, ig.EULER, 0.5)
    assert np.array_equal(buf, before) and par[0] == 0


def _perturbed_cases():
    for name, schemes in ig.USED_BY.items():
        for s in schemes:
            yield name, s
    for s in SCHEMES:
        yield "scale", s


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("name,scheme", list(_perturbed_cases()))
def test_a_constant_wrong_by_1e_3_would_fail_the_gpu_test(oracle32, name, scheme, scale):
    """one constant times (1 + 1e-3): x or v of the scheme that uses it moves by at least 10 x the tolerance of the GPU test"""
    buf, par = elastic_only_input(oracle32)
    floor = oracle32_floor(oracle32, buf, par, scheme, scale)
    tol = gpu_tolerance(floor)
    want = restated(buf, par, scheme, scale)
    if name == "scale":
        off = restated(buf, par, scheme, scale * (1 + 1e-3))
    else:
        consts = dict(ig.CONSTANTS)
        consts[name] *= 1 + 1e-3
        off = restated(buf, par, scheme, scale, consts)
    shift = tuple(ig.rel_dist(o, w) for o, w in zip(off, want))
    print("%-10s scale %.1f  %-13s x 1.001: shift x %.2e v %.2e   oracle32 floor x %.2e v %.2e   gpu tolerance x %.2e v %.2e"
          % (ig.NAMES[scheme], scale, name, shift[0], shift[1], floor[0], floor[1], tol[0], tol[1]))
    assert shift[0] >= 10 * tol[0] or shift[1] >= 10 * tol[1], (shift, tol)


def test_a_constant_of_another_scheme_changes_nothing(oracle32):
    """the table of which scheme uses which constant is the restatement's own: a constant outside it leaves the bits alone"""
    buf, par = elastic_only_input(oracle32)
    for name, schemes in ig.USED_BY.items():
        consts = dict(ig.CONSTANTS)
        consts[name] *= 1 + 1e-3
        for s in SCHEMES:
            if s in schemes:
                continue
            a, b = restated(buf, par, s, 1.0, consts, steps=2), restated(buf, par, s, 1.0, steps=2)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
