"""numpy reference of contract (C), matches pruned by pairwise length consistency (include/simpleicp_hip_consistency.h, DESIGN.md
section 21), written from the contract text.  TEST INFRASTRUCTURE ONLY.

float64 numpy, one expression per contract line; contract (D) goes through the correctly rounded ``global_ref.fma``, the square
root is numpy's (correctly rounded).  The pairs are taken in blocks of rows, so that no (m, m, 3) array exists.  The core numbers
come from a plain sequential peel: take a row of the smallest remaining degree, its core number is the largest such degree seen so
far, remove it.
"""
import numpy as np

import global_ref

MAX_ROWS = 32768                                                      # SICP_CONSISTENCY_MAX_ROWS of the header
BLOCK = 256


def lengths(X, rows, cols):
    """sqrt(d2) between the rows `rows` and the rows `cols` of X (slices), contract (D): (len(rows), len(cols))."""
    with np.errstate(all="ignore"):
        dx = X[rows, None, 0] - X[None, cols, 0]
        dy = X[rows, None, 1] - X[None, cols, 1]
        dz = X[rows, None, 2] - X[None, cols, 2]
        return np.sqrt(global_ref.fma(dz, dz, global_ref.fma(dy, dy, dx * dx)))


def valid_rows(src, dst):
    return np.isfinite(src).all(axis=1) & np.isfinite(dst).all(axis=1)


def adjacency(src, dst, tolerance, min_length, full=False):
    """The (m, m) bool compatibility matrix.  full=False evaluates the pairs i <= j of every block and mirrors them (the contract
    says why that is the same bits); full=True evaluates every ordered pair."""
    src, dst = np.ascontiguousarray(src, dtype=np.float64), np.ascontiguousarray(dst, dtype=np.float64)
    tolerance, min_length = np.float64(tolerance), np.float64(min_length)
    m = len(src)
    valid = valid_rows(src, dst)
    # (an invalid row takes no part: its coordinates are replaced so that no warning and no NaN arises on the way)
    S, D = np.where(valid[:, None], src, 0.0), np.where(valid[:, None], dst, 0.0)
    A = np.zeros((m, m), bool)
    for r0 in range(0, m, BLOCK):
        rows = slice(r0, min(r0 + BLOCK, m))
        cols = slice(0, m) if full else slice(r0, m)
        a, b = lengths(S, rows, cols), lengths(D, rows, cols)
        with np.errstate(all="ignore"):
            ok = np.isfinite(a) & np.isfinite(b) & (np.abs(a - b) <= tolerance) & (a >= min_length) & (b >= min_length)
        ok &= valid[rows, None] & valid[None, cols]
        A[rows, cols] = ok
        if not full:
            A[cols, rows] |= ok.T
    A[np.arange(m), np.arange(m)] = False
    return A


def core_numbers(A):
    """The core number of every row of the graph A, by the sequential peel."""
    A = np.asarray(A, bool)
    m = len(A)
    deg = A.sum(axis=1).astype(np.int64)
    core = np.zeros(m, np.int32)
    gone = np.zeros(m, bool)
    big = np.int64(m + 1)
    k = 0
    for _ in range(m):
        v = int(np.argmin(np.where(gone, big, deg)))
        k = max(k, int(deg[v]))
        core[v] = k
        gone[v] = True
        deg -= A[v]                                                  # (the rows that are gone are never looked at again)
    return core


def subrounds(A):
    """The passes of the peel whose level jumps to the smallest remaining degree: every pass removes {alive, degree <= level}."""
    A = np.asarray(A, bool)
    deg = A.sum(axis=1).astype(np.int64)
    alive = np.ones(len(A), bool)
    k = n = 0
    while alive.any():
        k = max(k, int(deg[alive].min()))
        front = alive & (deg <= k)
        alive &= ~front
        deg -= A[:, front].sum(axis=1)
        n += 1
    return n


def consistency(src, dst, tolerance, min_length, A=None):
    """(degree_out (m,) int32, core_out (m,) int32, record without n_subrounds) of contract (C)."""
    src, dst = np.ascontiguousarray(src, dtype=np.float64), np.ascontiguousarray(dst, dtype=np.float64)
    if A is None:
        A = adjacency(src, dst, tolerance, min_length)
    degree = A.sum(axis=1).astype(np.int32)
    core = core_numbers(A)
    top = int(core.max())
    rec = dict(n_rows=len(src), n_valid=int(valid_rows(src, dst).sum()), n_edges=int(degree.astype(np.int64).sum()) // 2,
               max_degree=int(degree.max()), max_core=top, n_max_core=int((core == top).sum()) if top >= 1 else 0)
    return degree, core, rec


def keep_mask(core, rec):
    """The rows of the maximal core: core == max_core where max_core >= 1, else none."""
    return core == rec["max_core"] if rec["max_core"] >= 1 else np.zeros(len(core), bool)
