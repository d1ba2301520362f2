"""fp64 reference of the aperture (nbco_aperture_count / nbco_aperture_apply and their nbco_2d_ forms, `nbco3 -aperture`), the rule of
include/nbco.h verbatim: w_a = 1.0 / half_a (half_a = +inf opens the axis: w_a = 0); d_a = (double) x_a - centre_a; a particle with a
non-finite coordinate is outside; ellipsoid: u_a = d_a * w_a, s = (u_x u_x + u_y u_y) + u_z u_z (2-D: u_x u_x + u_y u_y), inside iff
s <= 1.0; box: inside iff fabs(d_a) <= half_a on every axis.  Every product and sum is a numpy fp64 operation of its own, so rounded
once.  `apply` is the stable compaction of a state [pos | vel | acc] and its loss record."""
import numpy as np

ELLIPSOID, BOX = 0, 1


def inside(pos, shape, half, centre=None):
    """bool per row of pos, (n, 3) or (n, 2) of any float type (widened first); half and centre have one value per column"""
    x = np.asarray(pos).astype(np.float64)
    dim = x.shape[1]
    half = np.asarray(half, dtype=np.float64)
    centre = np.zeros(dim) if centre is None else np.asarray(centre, dtype=np.float64)
    assert half.shape == (dim,) and centre.shape == (dim,)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        w = 1.0 / half
        d = x - centre[None, :]
        finite = np.isfinite(x).all(axis=1)
        if shape == BOX:
            return finite & (np.abs(d) <= half[None, :]).all(axis=1)
        assert shape == ELLIPSOID
        u = d * w[None, :]
        s = u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]
        if dim == 3:
            s = s + u[:, 2] * u[:, 2]
        return finite & (s <= 1.0)


def apply(state, shape, half, centre=None):
    """state: (3, n, D) = [pos, vel, acc].  Returns (kept state (3, n', D), lost records (k, 2 D) = pos | vel, lost rows (k,) int32), the
    kept and the lost particles each in state order"""
    state = np.asarray(state)
    keep = inside(state[0], shape, half, centre)
    rows = np.nonzero(~keep)[0].astype(np.int32)
    lost = np.concatenate([state[0][rows], state[1][rows]], axis=1)
    return np.ascontiguousarray(state[:, keep]), np.ascontiguousarray(lost), rows
