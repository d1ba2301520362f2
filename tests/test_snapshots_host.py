"""The preconditions of tests/test_gpu_snapshots.py, computed from the aperture model (tests/aperture_numpy.py) on the unmoved initial
states: no GPU is needed.  The snapshot sequences shrink n by an aperture at every snapshot; what they are there for -- tables and
private contexts that see a smaller n than before, the "loses nobody" path inside a run, a state that crosses 4097 / 4096 -- needs
every lossy call to lose a fair number and to keep a beam worth evaluating."""
import test_gpu_snapshots as T


def test_losses_of_the_3d_snapshot_sequence(oracle32):
    """each of the four lossy calls loses at least 50 particles and keeps at least 1000, the second call loses nobody, and the last
    snapshot is below 4096.  For a Gaussian the fraction outside k rms is 2.9 %, 10.0 %, 26.1 % and 52.2 % at k = 3, 2.5, 2, 1.5, and
    the reference normalises its ball to the sample's own moments: 8193 -> about 7950 -> 7950 -> 7370 -> 6050 -> 3910."""
    table = T.preconditions_3d(oracle32)
    print("3-D (lost, kept) per aperture call:", table)
    assert len(table) == len(T.KS) == 5
    expected = [T.N0 * f for f in (0.971, 0.971, 0.900, 0.739, 0.478)]
    assert all(abs(kept - want) < 0.02 * T.N0 for (_, kept), want in zip(table, expected)), (table, expected)


def test_losses_of_the_2d_snapshot_sequence(engine_lib):
    """every aperture_2d call loses at least 50 particles and keeps at least 1000: a KV beam is uniform inside its semi-axes A = 2 rms,
    so (k / 2)^2 of it lies inside k rms"""
    table = T.preconditions_2d()
    print("2-D (lost, kept) per aperture call:", table)
    assert len(table) == len(T.KS_2D) == 4
    assert all(abs(kept - T.N0 * (k / 2) ** 2) < 0.02 * T.N0 for (_, kept), k in zip(table, T.KS_2D)), table


def test_bond_radius_of_the_3d_snapshot_sequence(oracle32):
    """BOND_RMAX keeps nb <= 256 at every snapshot (the premise of bond_numpy.TOL2, which the snapshot tests hold q to) and gives at
    least half of the particles a bond; the table covers every modelled aperture and its n are those of the loss model"""
    table = T.bond_preconditions_3d(oracle32)
    print("3-D (n, nb_max, particles with a bond) per snapshot at rmax = %g:" % T.BOND_RMAX, table)
    assert [n for n, _, _ in table] == [kept for _, kept in T.loss_model_3d(oracle32)]
    assert all(nb_max >= 12 for _, nb_max, _ in table), table      # enough neighbours for a q6 worth the name


def test_bond_radius_of_the_2d_snapshot_sequence(engine_lib):
    table = T.bond_preconditions_2d()
    print("2-D (n, nb_max, particles with a bond) per snapshot at rmax = %g max(A):" % T.BOND_RMAX_2D, table)
    assert [n for n, _, _ in table] == [kept for _, kept in T.loss_model_2d()]
    assert all(nb_max >= 6 for _, nb_max, _ in table), table


def test_shapes_of_the_structure_factor_walk():
    """the size walk's table of launch shapes (a restatement of sk_shape in csrc/k_reduce.hip) contains what it is there for: one range
    directly behind at least 16, more ranges on a smaller K than before, several chunks of ix, workgroups with several copies of their
    items and with one, a tile below 256, and the largest grid in several ranges"""
    table = T.preconditions_walk()
    for s in table:
        print(s)
    assert len(table) == 2 * len(T.SIZES_B) + 1
    # hand-checked against the launcher's rules: 289 items in 5 workgroups of 58 lanes and 4 copies, 19 slots per particle
    first = table[1]
    assert (first["items"], first["lanes"], first["copies"], first["tile"], first["ranges"], first["K"]) == (289, 58, 4, 161, 17, 2601), first
