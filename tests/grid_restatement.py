"""Plain NumPy restatement of the 0.01-grid median (partition_stat_tp, wufunctions.cpp:364-424) and of the MAD the scan
thresholds take from it (RDtmp[i] = abs(RDtrans[i] - tmedian), rsi.cpp:1276), in float64 throughout:

  ymin / ymax of the selected values; below 0.01 of range the result is their mean, summed in index order;
  np = (size_t)((ymax - ymin) / 0.01 + 2) buckets, value x in bucket (size_t)((x - ymin) / 0.01 + 0.5);
  the first bucket b at which the running count reaches n // 2; the result ymin + b * 0.01.

tests/test_grid_restatement.py pins it to the oracle's partition_stat_tp on every array tests/test_grid_quantiles.py gives
the device; the device is then held to it with ==."""
import numpy as np

DY = 0.01
CAP = 1 << 20   # buckets of the device chain's resident histogram (pipeline.hip: kGridCap); wider ranges take the host-driven form


def span(v):
    """(ymin, ymax, np) of float32 values v, np = None when the range is under the grid step."""
    d = np.asarray(v, dtype=np.float32).astype(np.float64)
    ymin, ymax = float(d.min()), float(d.max())
    if ymax - ymin < DY:
        return ymin, ymax, None
    return ymin, ymax, int((ymax - ymin) / DY + 2)


def buckets(v, ymin):
    """(size_t)((x - ymin) / 0.01 + 0.5) of float32 values, each operation a double one."""
    d = np.asarray(v, dtype=np.float32).astype(np.float64)
    return ((d - ymin) / DY + 0.5).astype(np.uint64)


def index_order_mean(v):
    d = np.asarray(v, dtype=np.float32).astype(np.float64)
    return float(np.cumsum(d)[-1]) / d.size    # cumsum adds in index order (np.sum adds pairwise)


def median(v):
    """partition_stat_tp's "median" of float32 values v (all selected): (value, count).  Nothing selected: (0.0, 0)."""
    v = np.asarray(v, dtype=np.float32)
    if v.size == 0:
        return 0.0, 0
    if not np.all(np.isfinite(v)):
        raise ValueError("non-finite value")
    ymin, _, npb = span(v)
    if npb is None:
        return index_order_mean(v), v.size
    cum = np.cumsum(np.bincount(buckets(v, ymin).astype(np.int64), minlength=npb))
    b = int(np.argmax(cum >= v.size // 2))
    return ymin + b * DY, v.size


def median_bucket(v):
    """The bucket median() takes its result from (None below the grid step)."""
    v = np.asarray(v, dtype=np.float32)
    ymin, _, npb = span(v)
    if npb is None:
        return None
    cum = np.cumsum(np.bincount(buckets(v, ymin).astype(np.int64), minlength=npb))
    return int(np.argmax(cum >= v.size // 2))


def abs_dev(v, center):
    """(float)fabs((double)x - center), as the device's sel_value and the reference's RDtmp."""
    return np.abs(np.asarray(v, dtype=np.float32).astype(np.float64) - float(center)).astype(np.float32)


def selected(x, mask=None):
    x = np.asarray(x, dtype=np.float32)
    return x if mask is None else x[np.asarray(mask) == 0]


def pair(x, mask=None):
    """(median, count, MAD, count) of the selection, the MAD centred on that median."""
    s = selected(x, mask)
    med, n = median(s)
    mad, n2 = median(abs_dev(s, med))
    return med, n, mad, n2


def mad(x, center, mask=None):
    s = selected(x, mask)
    m, n = median(abs_dev(s, center))
    return float(center), 0, m, n


def med_mad_i32(xi, center):
    """-MED: the int32 bin medians become floats, the MAD is taken around `center`."""
    return mad(np.asarray(xi, dtype=np.int32).astype(np.float32), center)
