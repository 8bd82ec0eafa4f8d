"""TEST INFRASTRUCTURE: the oracle of the histogram's bin rule, np.searchsorted(edges, x, side="right") - 1, for the tests of tests/README.histogram.md."""
import numpy as np


def counts_of(x, edges):
    """-> uint64 [bins + 3]: the bins, then under (x < edges[0]), over (x >= edges[bins]), nan"""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    edges = np.asarray(edges, dtype=np.float64)
    bins = len(edges) - 1
    nan = np.isnan(x)
    k = np.searchsorted(edges, x[~nan], side="right") - 1
    c = np.zeros(bins + 3, dtype=np.uint64)
    c[:bins] = np.bincount(k[(k >= 0) & (k < bins)], minlength=bins)
    c[bins], c[bins + 1], c[bins + 2] = np.sum(k < 0), np.sum(k >= bins), np.sum(nan)
    return c


def counts_of_array(draws, D, edges):
    """draws [rows][PR][C], D datasets of C / D columns each, edges [bins + 1] or [PR][bins + 1] -> uint64 [D][PR][bins + 3]"""
    rows, PR, C = draws.shape
    e = np.asarray(edges, dtype=np.float64)
    if e.ndim == 1:
        e = np.broadcast_to(e, (PR, e.size))
    cpd = C // D
    return np.array([[counts_of(draws[:, p, d * cpd:(d + 1) * cpd], e[p]) for p in range(PR)] for d in range(D)], dtype=np.uint64)
