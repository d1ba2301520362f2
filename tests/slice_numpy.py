"""fp64 numpy reference of the slice diagnostics (include/nbco.h: nbco_slice_moments and its 2-D form): the bin rule of
beam_numpy.bin_of on the slicing coordinate, then beam_numpy.moments over each slice's particles in state order."""
import numpy as np

import beam_numpy as BN


def empty(dim):
    """the record of an empty slice: n = 0, the right dim, zeros (also as the yardsticks of the sums)"""
    z = dict(mean=np.zeros(6), cov=np.zeros((6, 6)), m4=np.zeros((3, 5)))
    return dict(n=0, dim=dim, mean=np.zeros(6), min=np.zeros(6), max=np.zeros(6), cov=np.zeros((6, 6)), m4=np.zeros((3, 5)),
                emit=np.zeros(3), halo_q=np.zeros(3), halo=np.zeros(3), scale=z)


def members(state, dim, axis):
    """(rows of every slice in state order, number of particles outside) for axis = (coord, bins, lo, hi)"""
    coord, bins, lo, hi = axis
    q = BN.phase_space(state, dim)[:, BN.coord_index(coord, dim)]
    inside, b = BN.bin_of(q, bins, lo, hi)
    rows = np.flatnonzero(inside)
    order = rows[np.argsort(b[rows], kind="stable")]
    cuts = np.searchsorted(b[order], np.arange(bins + 1))
    return [order[cuts[s]:cuts[s + 1]] for s in range(bins)], int(len(q) - inside.sum())


def slice_moments(state, dim, axis):
    """(list of `bins` dicts as beam_numpy.moments returns them, n_outside)"""
    st = np.asarray(state).reshape(2, -1, dim)
    rows, outside = members(st, dim, axis)
    return [BN.moments(st[:, r], dim) if len(r) else empty(dim) for r in rows], outside
