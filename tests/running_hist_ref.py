"""Shared by test_running_hist.py (GPU) and test_running_hist_host.py (CPU): a NumPy restatement of the bin rule and
of the first-chunk range of include/pbbi.h ("running histogram"), and the edge-case data."""
import numpy as np


def auto_range(first_chunk, margin):
    """(lo, hi) per dimension from the (c, D, N) first chunk: a, b = its finite extremes (0, 0 without one), span =
    b - a, lo = a - margin * span, hi = b + margin * span, in this order; !(hi > lo): a -/+ 0.5."""
    x = np.asarray(first_chunk, dtype=np.float64)
    D = x.shape[1]
    lo, hi = np.empty(D), np.empty(D)
    for d in range(D):
        v = x[:, d, :].ravel()
        v = v[np.isfinite(v)]
        a, b = (np.float64(v.min()), np.float64(v.max())) if v.size else (np.float64(0.0), np.float64(0.0))
        span = b - a
        l, h = a - np.float64(margin) * span, b + np.float64(margin) * span
        if not h > l:
            l, h = a - 0.5, a + 0.5
        lo[d], hi[d] = l, h
    return lo, hi


def numpy_state(x, lo, hi, bins):
    """What the device state must hold after the (S, D, N) draws x (converted to float64 first): counts (D, bins + 2)
    uint64, nan (D,) uint64, min / max (D,) over the non-NaN values (+inf / -inf without one).  The bin of x:
    t = (x - lo) * inv, inv = bins / (hi - lo);  x < lo: 0;  x >= hi: bins + 1;  else 1 + min(floor(t), bins - 1)."""
    x = np.asarray(x, dtype=np.float64)
    D = x.shape[1]
    lo, hi = np.broadcast_to(np.asarray(lo, dtype=np.float64), (D,)), np.broadcast_to(np.asarray(hi, dtype=np.float64), (D,))
    counts = np.zeros((D, bins + 2), dtype=np.uint64)
    nan = np.zeros(D, dtype=np.uint64)
    mn, mx = np.full(D, np.inf), np.full(D, -np.inf)
    for d in range(D):
        v = x[:, d, :].ravel()
        isnan = np.isnan(v)
        nan[d] = isnan.sum()
        v = v[~isnan]
        if v.size == 0:
            continue
        mn[d], mx[d] = v.min(), v.max()
        inv = np.float64(bins) / (hi[d] - lo[d])
        inside = (v >= lo[d]) & (v < hi[d])
        t = (v[inside] - lo[d]) * inv
        k = np.where(v < lo[d], 0, bins + 1).astype(np.int64)
        k[inside] = 1 + np.minimum(np.floor(t).astype(np.int64), bins - 1)
        counts[d] = np.bincount(k, minlength=bins + 2).astype(np.uint64)
    return dict(counts=counts, nan=nan, min=mn, max=mx, lo=np.array(lo), hi=np.array(hi))


def edge_values(lo, width, bins, dtype=np.float64):
    """Values exactly at lo, at hi = lo + bins * width and at interior edges (lo and width dyadic: the edges are exact
    in `dtype`), one ulp of `dtype` either side of each, and +inf, -inf, NaN."""
    edges = np.array([lo + k * width for k in (0, 1, 2, bins // 2, bins - 1, bins)], dtype=dtype)
    assert np.array_equal(edges.astype(np.float64), [lo + k * width for k in (0, 1, 2, bins // 2, bins - 1, bins)])
    below, above = np.nextafter(edges, dtype(-np.inf)), np.nextafter(edges, dtype(np.inf))
    return np.concatenate([edges, below, above, np.array([np.inf, -np.inf, np.nan, np.nan], dtype=dtype)])


def same_state(got, want):
    """Every field of two read() results equal (counts, nan as integers; lo, hi, min, max as values)."""
    for k in ("counts", "nan"):
        assert got[k].dtype == np.uint64 and np.array_equal(got[k], want[k]), k
    for k in ("lo", "hi", "min", "max"):
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
