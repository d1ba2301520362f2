"""Helpers of tests/test_gpu_yardsticks.py that need no GPU: launch_direct's split arithmetic restated, and direct sums over a
sample of the rows in fp64 and in the reference's float32 Kahan order.  tests/test_direct_numpy_host.py checks them on the CPU."""
import numpy as np

K_BLOCK, K_IB, K_TILE = 256, 4, 256          # k_direct.hip:16-18


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


def direct_launch_shape(n, cus):
    """launch_direct's split arithmetic (k_direct.hip:194-202) restated:
    (splits, tiles_per_split, tiles in the last split, sources in the last tile)"""
    iblocks = (n + K_BLOCK * K_IB - 1) // (K_BLOCK * K_IB)
    ntiles = (n + K_TILE - 1) // K_TILE
    splits = (4 * cus + iblocks - 1) // iblocks                 # aim for >= 4 workgroups per CU
    splits = max(1, min(splits, ntiles, 64))
    tiles_per_split = (ntiles + splits - 1) // splits
    splits = (ntiles + tiles_per_split - 1) // tiles_per_split
    return splits, tiles_per_split, ntiles - (splits - 1) * tiles_per_split, n - (ntiles - 1) * K_TILE


def find_n(cus, want, lo, hi):
    """smallest n in [lo, hi) whose launch shape satisfies `want` (on 256 CUs the n of the issue; elsewhere whatever reaches the path)"""
    for n in range(lo, hi):
        if want(*direct_launch_shape(n, cus)):
            return n
    raise AssertionError("no n in [%d, %d) reaches the launch shape on %d CUs: the shapes of this test are stale" % (lo, hi, cus))


def direct_rows_fp64(pos, rows, k, eps2):
    """fp64 direct sum of the rows `rows` over all sources, numpy"""
    p = pos.astype(np.float64)
    t = p[rows]
    out = np.zeros((len(rows), 3))
    for s in range(0, len(p), 8192):
        d = t[:, None, :] - p[None, s:s + 8192, :]
        r2 = (d * d).sum(-1) + eps2
        out += (d / (r2 * np.sqrt(r2))[..., None]).sum(1)
    return out * k


def direct3_rows_fp32(pos, rows, k, eps2):
    """the reference's per-term Kahan sum (direct.cuh:207-221, as oracle32.direct3 runs it) for the rows `rows` only, operation by
    operation in float32 -- what stands in for oracle32.direct3 where a whole evaluation is too slow for a test"""
    f = np.float32
    t = pos[rows].astype(f)
    acc, c = np.zeros_like(t), np.zeros_like(t)
    one, e = f(1), f(eps2)
    for j in range(len(pos)):
        d = t - pos[j]
        inv2 = one / ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]) + e)
        y = d * inv2[:, None] * np.sqrt(inv2)[:, None] - c
        s = acc + y
        c = (s - acc) - y
        acc = s
    return f(k) * acc
