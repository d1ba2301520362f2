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
