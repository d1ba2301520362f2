"""CPU checks of the helpers in tests/direct_numpy.py."""
import numpy as np

from direct_numpy import direct3_rows_fp32, direct_launch_shape, direct_rows_fp64, same_bits


def test_launch_shape_helper_on_256_cus():
    """the restatement gives the shapes the cases below are named after (pure arithmetic)"""
    assert direct_launch_shape(20003, 256) == (40, 2, 1, 35)
    assert direct_launch_shape(20259, 256) == (40, 2, 2, 35)
    assert direct_launch_shape(65573, 256) == (16, 17, 2, 37)
    assert direct_launch_shape(5000, 256)[1] == 1 and direct_launch_shape(262144, 256) == (4, 256, 256, 256)


def test_row_restatement_is_oracle32_direct3(oracle32):
    """bit for bit, so that its error at n = 65573 is the reference's own """
    n = 777
    pos, par = oracle32.init_reference(n)[0], oracle32.params(n)
    rows = np.array([0, 1, 255, 256, 776])
    assert same_bits(direct3_rows_fp32(pos, rows, par[0], 1e-18), oracle32.direct3(pos, par)[rows])




def test_fp64_rows_are_oracle64_direct3(oracle32, oracle64):
    n = 777
    pos, par = oracle32.init_reference(n)[0], oracle32.params(n)
    rows = np.array([0, 1, 255, 256, 776])
    want = oracle64.direct3(pos.astype(np.float64), par.astype(np.float64))[rows]
    np.testing.assert_allclose(direct_rows_fp64(pos, rows, float(par[0]), 1e-18), want, rtol=0, atol=1e-12 * np.abs(want).max())
