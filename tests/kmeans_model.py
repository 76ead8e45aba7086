"""The integer side of aqlm_hip_kmeans_assign / aqlm_hip_kmeans_update restated in numpy (include/aqlm_hip.h): the
fixed-point unit, the quantisation of a point, the sums and counts of the clusters, and the update of the centroids.  The scores of
the assignment are NOT modelled: they are held by the epsilon contract (tests/test_kmeans_gpu.py).

    s        = min(40, 62 - ceil_log2(n)) - E,   data_absmax = m * 2^E with 1 <= m < 2 (zero and subnormals: E = -126)
    q_t      = rint(x_t * 2^s)                   exact product, ties to even
    sums     = per cluster the int64 sum of q over its points, counts = their number; a point with a non-finite element or one
               above data_absmax joins neither
    centroid = (float)((double)sums * 2^-s / (double)counts) where counts > 0, else the old centroid bit for bit
"""
import numpy as np


def exponent(data_absmax) -> int:
    bits = int(np.float32(data_absmax).view(np.uint32))
    field = (bits >> 23) & 0xFF
    return max(field, 1) - 127


def shift(n: int, data_absmax) -> int:
    ceil_log2 = 0
    while (1 << ceil_log2) < n:
        ceil_log2 += 1
    return min(40, 62 - ceil_log2) - exponent(data_absmax)


def accepted(data: np.ndarray, data_absmax) -> np.ndarray:
    """[n] bool: the points that join the sums."""
    with np.errstate(invalid="ignore"):
        return np.all(np.abs(data) <= np.float32(data_absmax), axis=1)  # (False for NaN; Inf is above every finite maximum)


def quantise(data: np.ndarray, n: int, data_absmax) -> np.ndarray:
    """[.., d] int64: a power of two times an fp32 value is exact in float64, rint rounds ties to even."""
    assert data.dtype == np.float32
    return np.rint(data.astype(np.float64) * 2.0 ** shift(n, data_absmax)).astype(np.int64)


def sums_and_counts(data: np.ndarray, indices: np.ndarray, k: int, data_absmax, n=None):
    """(sums int64 [k, d], counts int32 [k]) of the assignment ``indices`` of the rows of ``data``; ``n``: the number of points of the
    call that sets the unit (default: the rows given)."""
    d = data.shape[1]
    n = data.shape[0] if n is None else n
    keep = accepted(data, data_absmax)
    sums = np.zeros((k, d), dtype=np.int64)
    counts = np.zeros((k,), dtype=np.int32)
    idx = np.asarray(indices, dtype=np.int64)[keep]
    np.add.at(sums, idx, quantise(data[keep], n, data_absmax))
    np.add.at(counts, idx, 1)
    return sums, counts


def update(centroids: np.ndarray, sums: np.ndarray, counts: np.ndarray, n: int, data_absmax) -> np.ndarray:
    """The centroids after the update: float32 [k, d]; the rows of empty clusters are the old bits."""
    assert centroids.dtype == np.float32 and sums.dtype == np.int64
    out = centroids.copy()
    full = counts > 0
    mean = sums[full].astype(np.float64) * 2.0 ** -shift(n, data_absmax) / counts[full].astype(np.float64)[:, None]
    out[full] = mean.astype(np.float32)
    return out
