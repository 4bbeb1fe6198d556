"""numpy references of contracts (M) and (R) (include/simpleicp_hip_global.h), written from the contract
text.  TEST INFRASTRUCTURE ONLY.

(M) is float32 numpy, a loop over the columns.  (R) is float64 numpy, one expression per contract line, vectorised over the
hypotheses.  The score needs fused multiply-adds ((T) and (D)); this Python has no math.fma, so ``fma`` below forms the correctly
rounded a*b + c from error-free transformations and an addition rounded to odd (Boldo and Melquiond, "Emulation of a FMA and
correctly rounded sums: proved algorithms using rounding to odd", IEEE TC 2008) -- tests/test_global_host.py checks it against
the C library's fma.
"""
import numpy as np


# ---- contract (M) ----
def match(query, target):
    """(idx (nq,) int32, d2 (nq,) float32, record) of contract (M)."""
    q = np.ascontiguousarray(query, dtype=np.float32)
    g = np.ascontiguousarray(target, dtype=np.float32)
    assert q.ndim == 2 and g.ndim == 2 and q.shape[1] == g.shape[1] >= 1
    with np.errstate(all="ignore"):
        d2 = None
        for b in range(q.shape[1]):
            t = q[:, None, b] - g[None, :, b]
            p = t * t
            d2 = p if d2 is None else d2 + p
    assert d2.dtype == np.float32
    ok = d2 < np.float32(np.inf)                                      # (a NaN compares false)
    masked = np.where(ok, d2, np.float32(np.inf))
    idx = np.argmin(masked, axis=1).astype(np.int32)                  # (the first minimum: the lowest index)
    best = masked[np.arange(len(q)), idx]
    none = ~ok.any(axis=1)
    idx[none] = -1
    return idx, best, dict(n_query=len(q), n_target=len(g), n_unmatched=int(none.sum()))


def mutual(idx, back):
    """idx[i] unless back[idx[i]] != i: -1 then."""
    idx, back = np.asarray(idx, dtype=np.int64), np.asarray(back, dtype=np.int64)
    agree = (idx >= 0) & (back[np.maximum(idx, 0)] == np.arange(len(idx)))
    return np.where(agree, idx, -1)


# ---- a correctly rounded fused multiply-add in float64 numpy ----
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = 134217729.0 * a
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _add_odd(a, b):
    """a + b rounded to odd: the exact sum if it is a double, else the neighbour with the odd significand."""
    s, e = _two_sum(a, b)
    bits = s.view(np.uint64)
    move = (e != 0) & ((bits & np.uint64(1)) == 0)
    away = (e > 0) == (s > 0)                                         # the exact sum lies on the far side of s from zero
    bits = np.where(move, np.where(away, bits + np.uint64(1), bits - np.uint64(1)), bits)
    return bits.view(np.float64)


def fma(a, b, c):
    """round(a*b + c), one rounding, elementwise in float64 (operands whose products neither overflow nor underflow; anything
    non-finite falls back to a*b + c, which is NaN or infinite where the fused result is)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    a, b, c = np.ascontiguousarray(a), np.ascontiguousarray(b), np.ascontiguousarray(c)
    with np.errstate(all="ignore"):
        ph, pl = _two_prod(a, b)
        uh, ul = _two_sum(c, pl)
        th, tl = _two_sum(ph, uh)
        r = th + _add_odd(np.ascontiguousarray(tl), np.ascontiguousarray(ul))
        plain = a * b + c
    return np.where(np.isfinite(r) & np.isfinite(plain), r, plain)


# ---- contract (R) ----
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _len2(a, b):
    d = a - b
    return _dot(d, d)


def frame(a0, a1, a2):
    """(e1, e2, e3, c) of the triangles (a0, a1, a2), each (h, 3): contract (R), step 3."""
    u = a1 - a0
    e1 = u / np.sqrt(_dot(u, u))[..., None]
    v = a2 - a0
    s = _dot(e1, v)
    w = v - s[..., None] * e1
    e2 = w / np.sqrt(_dot(w, w))[..., None]
    e3 = _cross(e1, e2)
    c = ((a0 + a1) + a2) / 3.0
    return e1, e2, e3, c


def poses(src, dst, triples, edge_ratio):
    """(verdict (h,): 0 valid, -1 void, -2 pruned; R (h, 3, 3); t (h, 3)) -- steps 1 to 4; R and t are +0.0 unless valid."""
    src, dst = np.ascontiguousarray(src, dtype=np.float64), np.ascontiguousarray(dst, dtype=np.float64)
    tri = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    m = len(src)
    in_range = ((tri >= 0) & (tri < m)).all(axis=1)
    distinct = (tri[:, 0] != tri[:, 1]) & (tri[:, 0] != tri[:, 2]) & (tri[:, 1] != tri[:, 2])
    there = in_range & distinct
    j = np.where(there[:, None], tri, 0)                              # (nothing is dereferenced through a bad index)
    p, q = src[j], dst[j]                                             # (h, 3 points, 3 coordinates)
    r2 = float(edge_ratio) * float(edge_ratio)
    with np.errstate(all="ignore"):
        pruned = np.zeros(len(tri), bool)
        for a, b in ((0, 1), (0, 2), (1, 2)):
            ls2, lt2 = _len2(p[:, a], p[:, b]), _len2(q[:, a], q[:, b])
            pruned |= (ls2 < r2 * lt2) | (lt2 < r2 * ls2)                # (a NaN compares false: it prunes nothing)
        p1, p2, p3, cp = frame(p[:, 0], p[:, 1], p[:, 2])
        q1, q2, q3, cq = frame(q[:, 0], q[:, 1], q[:, 2])
        R = (q1[:, :, None] * p1[:, None, :] + q2[:, :, None] * p2[:, None, :]) + q3[:, :, None] * p3[:, None, :]
        t = cq - ((R[:, :, 0] * cp[:, None, 0] + R[:, :, 1] * cp[:, None, 1]) + R[:, :, 2] * cp[:, None, 2])
    finite = np.isfinite(R).all(axis=(1, 2)) & np.isfinite(t).all(axis=1)
    verdict = np.where(~there, -1, np.where(pruned, -2, np.where(finite, 0, -1)))
    R = np.where((verdict == 0)[:, None, None], R, 0.0)
    t = np.where((verdict == 0)[:, None], t, 0.0)
    return verdict, R, t


def count_inliers(R, t, src, dst, max_distance):
    """Step 5 for the poses R (h, 3, 3), t (h, 3): rows c with d2(R src[c] + t, dst[c]) < max_distance * max_distance."""
    src, dst = np.ascontiguousarray(src, dtype=np.float64), np.ascontiguousarray(dst, dtype=np.float64)
    md2 = float(max_distance) * float(max_distance)
    out = np.empty(len(R), np.int64)
    x, y, z = src[None, :, 0], src[None, :, 1], src[None, :, 2]
    with np.errstate(all="ignore"):
        for lo in range(0, len(R), 256):
            Rk, tk = R[lo:lo + 256], t[lo:lo + 256]
            d = []
            for r in range(3):                                        # contract (T), then the difference to dst
                acc = fma(Rk[:, r, 2, None], z, fma(Rk[:, r, 1, None], y, Rk[:, r, 0, None] * x))
                d.append((acc + tk[:, r, None]) - dst[None, :, r])
            d2 = fma(d[2], d[2], fma(d[1], d[1], d[0] * d[0]))        # contract (D)
            out[lo:lo + 256] = (d2 < md2).sum(axis=1)                 # (a NaN fails)
    return out


def ransac(src, dst, triples, max_distance, edge_ratio):
    """(poses (h, 12) float64, inliers (h,) int32, record) of contract (R)."""
    verdict, R, t = poses(src, dst, triples, edge_ratio)
    inliers = verdict.astype(np.int32)
    valid = np.flatnonzero(verdict == 0)
    if len(valid):
        inliers[valid] = count_inliers(R[valid], t[valid], src, dst, max_distance)
    best_inliers = int(inliers.max()) if len(valid) else -1
    best = int(np.flatnonzero(inliers == best_inliers)[0]) if len(valid) else -1
    rec = dict(n_hypotheses=len(inliers), n_void=int((verdict == -1).sum()), n_pruned=int((verdict == -2).sum()), best=best,
               best_inliers=best_inliers)
    return np.concatenate([R.reshape(-1, 9), t], axis=1), inliers, rec


# ---- a threshold that tells the fused sum of contract (D) from the unfused one ----
def d2_fused_and_plain(R, t, src, dst):
    """d2 of every row under one pose (R (3, 3), t (3,)) as contract (D) forms it, and the same three squares with every product and
    every sum rounded on its own (contract (T) fused in both): what a scoring without fused multiply-adds would compare."""
    src, dst = np.ascontiguousarray(src, dtype=np.float64), np.ascontiguousarray(dst, dtype=np.float64)
    x, y, z = src[:, 0], src[:, 1], src[:, 2]
    d = [(fma(R[r, 2], z, fma(R[r, 1], y, R[r, 0] * x)) + t[r]) - dst[:, r] for r in range(3)]
    return fma(d[2], d[2], fma(d[1], d[1], d[0] * d[0])), (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def threshold_between(fused, plain):
    """A max_distance whose square is the larger of the two sums of some row, so that the row counts under the smaller sum only,
    and under which the two counts differ; the first row that has one.  None: no row has."""
    for c in np.flatnonzero(fused != plain):
        hi = max(fused[c], plain[c])
        for md in (np.sqrt(hi), np.nextafter(np.sqrt(hi), 0.0), np.nextafter(np.sqrt(hi), np.inf)):
            if md * md == hi and int((fused < hi).sum()) != int((plain < hi).sum()):
                return float(md)
    return None
