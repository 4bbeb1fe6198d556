"""The stride and tile seams of sicp_feature_match, sicp_ransac_triplets and sicp_pose_refit (contracts (M), (R) and (L), DESIGN.md
sections 18 and 19): every loop of k_match, k_match_finish, k_ransac, k_pose_sweep, the folds and k_pose_best runs a second pass, every
row width of k_match is instantiated at, below and past its edge, a chunk holds several LDS tiles, and pt_fold runs two levels
with 6 and 9 terms and more than one pose.  Everything is compared bit for bit with the numpy references of tests/global_ref.py and
tests/posefit_ref.py; what the inputs must be like for a seam to matter (where the best record lies, that counts differ, that the
strided tail holds void, pruned and unmatched rows) is asserted on the reference before the device is asked."""
import contextlib
import os

import numpy as np
import pytest
import torch

import global_ref
import posefit_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# the constants of sicp_global.hip, sicp_posefit.hip and sicp_pairtree.h whose seams these tests sit on
MT_BLOCK, MT_TILE, MT_MAX_QBLOCKS, MT_MAX_CHUNKS = 256, 128, 8192, 1024
RS_WAVES, RS_MAX_BLOCKS = 4, 16384
PT_SPAN, PT_FOLD = 1024, 1024
PF_MAX_POSES_Y, PF_BLOCK, PF_BEST_BLOCKS = 32768, 256, 1024


@pytest.fixture(scope="module")
def ctx():
    from simpleicp_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


@contextlib.contextmanager
def chunked(rows):
    """A context of its own whose sicp_feature_match cuts the target into chunks of `rows` (SICP_MATCH_CHUNK is read at
    sicp_ctx_create)."""
    from simpleicp_amd import _lib
    old = os.environ.get("SICP_MATCH_CHUNK")
    os.environ["SICP_MATCH_CHUNK"] = str(rows)
    try:
        with _lib.Context(0) as other:
            yield other
    finally:
        if old is None:
            del os.environ["SICP_MATCH_CHUNK"]
        else:
            os.environ["SICP_MATCH_CHUNK"] = old


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- matching (M) ----
def check_match(ctx, q, t):
    idx, d2, st = ctx.feature_match(q, t)
    ridx, rd2, rec = global_ref.match(q, t)
    print(f"nq={len(q)} nt={len(t)} dim={q.shape[1]}: {st.as_dict()}")
    assert idx.dtype == np.int32 and np.array_equal(idx, ridx)
    assert np.array_equal(u32(d2), u32(rd2))
    assert st.as_dict() == rec
    return idx, d2


@pytest.mark.parametrize("dim", [3, 4, 5, 15, 16, 17, 35, 36, 37, 63])
def test_match_row_widths(ctx, dim):
    """Every row width (4, 16, 36, 64) at its last dim, the one before and the one past it.  The last column decides: target rows
    that would be exact hits and one query carry a NaN there, so a width that drops or mis-pads it shows in the indices."""
    nq, nt = 300, 257
    rng = np.random.default_rng(1000 * nq + nt + dim)
    q = rng.uniform(0, 200, (nq, dim)).astype(np.float32)
    t = rng.uniform(0, 200, (nt, dim)).astype(np.float32)
    t[rng.integers(0, nt, nt // 10)] = q[rng.integers(0, nq, nt // 10)]                          # exact hits, some of them repeated
    t[[3, 128, 256]] = q[[10, 20, 30]]                                # exact hits but for the NaN in the last column
    t[[3, 128, 256], dim - 1] = np.nan
    q[40, dim - 1] = np.nan
    idx, d2 = check_match(ctx, q, t)
    assert idx[40] == -1 and np.isposinf(d2[40]) and not set(idx.tolist()) & {3, 128, 256}
    assert (d2 == 0).sum() >= 10


@pytest.mark.parametrize("chunk", [300, 256, 100000])
def test_match_several_tiles_in_a_chunk(chunk):
    """Chunks of 128 + 128 + 44 rows, of exactly two tiles, and one chunk of six tiles whose last holds 60 rows: the second pass of
    the tile loop, with ties between two tiles of a chunk, across a chunk seam that is no tile seam, and into an earlier chunk."""
    rng = np.random.default_rng(700)
    q = rng.uniform(0, 1, (70, 33)).astype(np.float32)
    t = rng.uniform(0, 1, (700, 33)).astype(np.float32)
    t[127] = t[128] = q[5]
    t[299] = t[300] = q[6]
    t[600] = t[40] = q[7]
    with chunked(chunk) as other:
        idx, d2 = check_match(other, q, t)
        assert idx[5] == 127 and idx[6] == 299 and idx[7] == 40
        assert np.array_equal(u32(d2[[5, 6, 7]]), u32(np.zeros(3)))  # +0.0
        if chunk == 100000:
            dup = np.ascontiguousarray(np.tile(q[5], (700, 1)))       # every row of every tile ties: row 0
            assert np.all(check_match(other, q[5:6], dup)[0] == 0)


def test_match_more_chunks_than_the_grid():
    """Chunks of one row: 1100 of them on a grid of 1024, so the chunk stride steps once."""
    nt = MT_MAX_CHUNKS + 76
    rng = np.random.default_rng(1100)
    q = rng.uniform(0, 1, (70, 5)).astype(np.float32)
    t = rng.uniform(0, 1, (nt, 5)).astype(np.float32)
    t[MT_MAX_CHUNKS + 26] = q[3]                                      # found by the strided pass alone
    t[20] = t[20 + MT_MAX_CHUNKS] = q[9]                              # both passes of one workgroup tie
    with chunked(1) as other:
        idx, d2 = check_match(other, q, t)
        assert idx[3] == MT_MAX_CHUNKS + 26 and idx[9] == 20 and d2[3] == 0 and d2[9] == 0


def test_match_more_query_blocks_than_the_grid(ctx):
    """8192 * 256 + 77 queries under the default chunking: the query-block stride of k_match and of k_match_finish steps once, and
    the chunk comes out as 256 rows for 130 targets -- tiles of 128 and 2 rows without the environment switch."""
    nq, nt, dim = MT_MAX_QBLOCKS * MT_BLOCK + 77, 130, 2
    rng = np.random.default_rng(8192)
    q = rng.uniform(0, 1, (nq, dim)).astype(np.float32)
    t = rng.uniform(0, 1, (nt, dim)).astype(np.float32)
    t[[0, 127, 128, 129]] = q[[nq - 1, 5, nq - 70, 300000]]           # exact hits on both sides of the tile seam
    gone = np.array([7, 255, 256, 1_000_000, nq - 77 - 1, nq - 77, nq - 40, nq - 2])
    q[gone] = np.nan
    slab = 65536
    ridx, rd2, unmatched = np.empty(nq, np.int32), np.empty(nq, np.float32), 0
    for lo in range(0, nq, slab):
        ridx[lo:lo + slab], rd2[lo:lo + slab], rec = global_ref.match(q[lo:lo + slab], t)
        unmatched += rec["n_unmatched"]
    rec = dict(n_query=nq, n_target=nt, n_unmatched=unmatched)
    # the conditions: unmatched queries in the first pass and in the strided tail, matches on both tiles in both
    first, tail = ridx[:nq - 77], ridx[nq - 77:]
    assert (first == -1).sum() == 5 and (tail == -1).sum() == 3 and unmatched == 8
    assert (first >= MT_TILE).any() and (tail >= MT_TILE).any() and (tail >= 0).any() and (tail < MT_TILE).any()
    qd, td = torch.tensor(q, device=DEV), torch.tensor(t, device=DEV)
    idv = torch.full((nq,), -7, dtype=torch.int32, device=DEV)
    ddv = torch.full((nq,), -7.0, dtype=torch.float32, device=DEV)
    st = ctx.feature_match(qd.data_ptr(), td.data_ptr(), nq, nt, dim, idx_ptr=idv.data_ptr(), d2_ptr=ddv.data_ptr())
    print(f"nq={nq} nt={nt} dim={dim}: {st.as_dict()}")
    idx, d2 = idv.cpu().numpy(), ddv.cpu().numpy()
    assert np.array_equal(idx, ridx)
    assert np.array_equal(u32(d2), u32(rd2))
    assert st.as_dict() == rec
    assert np.all(idx[gone] == -1) and np.isposinf(d2[gone]).all()


# ---- RANSAC (R) ----
def check_ransac(ctx, src, dst, tri, max_distance, edge_ratio, reference=None):
    P, inl, st = ctx.ransac_triplets(src, dst, tri, max_distance, edge_ratio)
    rP, rinl, rec = reference or global_ref.ransac(src, dst, tri, max_distance, edge_ratio)
    print(f"m={len(src)} h={len(tri)} edge_ratio={edge_ratio}: {st.as_dict()}")
    assert inl.dtype == np.int32 and np.array_equal(inl, rinl)
    assert np.array_equal(u64(P), u64(rP))
    assert st.as_dict() == rec
    return P, inl, rec


def rotation(axis, angle):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


R_TRUE, T_TRUE = rotation([1.0, 2.0, 3.0], 0.7), np.array([0.3, -0.2, 0.1])


def noisy_copy(rng, m, wrong, noise):
    src = rng.uniform(-1, 1, (m, 3))
    dst = src @ R_TRUE.T + T_TRUE + rng.normal(0, noise, (m, 3))
    bad = rng.choice(m, int(wrong * m), replace=False)
    dst[bad] = rng.uniform(-1, 1, (len(bad), 3))
    return src, dst


RS_PASS = RS_MAX_BLOCKS * RS_WAVES                 # hypotheses of the first pass of k_ransac's waves
RS_MD = 0.02


@pytest.fixture(scope="module")
def ransac_tail():
    """70 matches, 30 % of them wrong, and 65536 + 300 triples whose best is the record's only through the strided pass: the best
    triple of a first draw sits at 65536 + 17 and at 65536 + 200, and whatever else reached its count is replaced."""
    m, h = 70, RS_PASS + 300
    rng = np.random.default_rng(70)
    src, dst = noisy_copy(rng, m, wrong=0.3, noise=0.008)
    tri = rng.integers(0, m, (h, 3), dtype=np.int32)
    tri[RS_PASS + 30:RS_PASS + 38] = [[4, 4, 9], [9, 4, 4], [6, 6, 6], [0, 1, m], [-1, 2, 3], [2**31 - 1, 0, 1], [5, -2**31, 6], [8, 7, 8]]
    # the first draw under the reference, at edge_ratio 0 (the count of a triple that 0.9 does not prune is the same at both)
    _, inl0, _ = global_ref.ransac(src, dst, tri, RS_MD, 0.0)
    kept9 = global_ref.poses(src, dst, tri, 0.9)[0] == 0
    top = inl0[kept9].max()
    best = tri[np.flatnonzero(kept9 & (inl0 == top))[0]].copy()
    dull = tri[np.flatnonzero(kept9 & (inl0 == inl0[kept9].min()))[0]].copy()
    assert inl0[kept9].min() < top
    tri[inl0 >= top] = dull                                           # whoever reaches the best count, at either edge_ratio
    tri[RS_PASS + 17] = tri[RS_PASS + 200] = best
    return src, dst, np.ascontiguousarray(tri)


@pytest.mark.parametrize("edge_ratio", [0.9, 0.0])
def test_ransac_more_hypotheses_than_the_grid(ctx, ransac_tail, edge_ratio):
    """16384 * 4 + 300 hypotheses: 300 waves take a second hypothesis, and their void and pruned counts and their best count join
    the first pass's.  m = 70: a full stride of the lanes over the rows and a partial one."""
    src, dst, tri = ransac_tail
    rP, rinl, rec = global_ref.ransac(src, dst, tri, RS_MD, edge_ratio)
    cut = global_ref.poses(src, dst, tri[:RS_PASS], edge_ratio)[0]
    # the conditions: the record's best lies in the strided tail, twice, and the tail's void and pruned triples count
    assert rec["best"] == RS_PASS + 17 and rinl[RS_PASS + 200] == rec["best_inliers"] > 35
    assert rec["n_void"] >= int((cut == -1).sum()) + 8                 # (the eight void triples the fixture wrote there)
    if edge_ratio > 0:
        assert rec["n_pruned"] > int((cut == -2).sum())
    else:
        assert rec["n_pruned"] == 0
    check_ransac(ctx, src, dst, tri, RS_MD, edge_ratio, reference=(rP, rinl, rec))


# ---- pose refit (L) ----
def check_refit(ctx, src, dst, poses, max_distance, rounds, reference):
    P, inl, st = ctx.pose_refit(src, dst, poses, max_distance, rounds)
    rP, rinl, rec = reference
    print(f"m={len(src)} b={len(rP)} rounds={rounds} max_distance={max_distance}: {st.as_dict()}")
    assert inl.dtype == np.int32 and np.array_equal(inl, rinl)
    assert np.array_equal(u64(P), u64(rP))
    assert st.as_dict() == rec


def perturbed(rng, degrees, shift):
    """The true motion off by `degrees` about a random axis and by a shift of about `shift`."""
    R = rotation(rng.standard_normal(3), np.radians(degrees)) @ R_TRUE
    return np.concatenate([R.ravel(), T_TRUE + rng.normal(0, shift, 3)])


@pytest.fixture(scope="module")
def two_level_rows():
    """1024 * 1024 + 2049 rows: 1027 partials per term, which pt_fold takes in two levels (1027 -> 2 -> 1)."""
    m = PT_SPAN * PT_FOLD + 2049
    rng = np.random.default_rng(2049)
    src = rng.uniform(-1, 1, (m, 3))
    dst = src @ R_TRUE.T + T_TRUE + rng.normal(0, 0.01, (m, 3))
    bad = rng.choice(m, m // 10, replace=False)
    dst[bad] = rng.uniform(-1, 1, (len(bad), 3))
    return src, dst


def test_refit_two_fold_levels_three_poses(ctx, two_level_rows):
    """Three different poses over 2^20 + 2049 rows: the second level of pt_fold with 6 and with 9 terms, and the offsets of poses 1
    and 2 into the second buffer (k * T * nb2 with nb2 = 2)."""
    src, dst = two_level_rows
    rng = np.random.default_rng(3)
    poses = np.stack([perturbed(rng, 0.1, 0.001), perturbed(rng, 0.4, 0.004), perturbed(rng, 0.8, 0.008)])
    reference = posefit_ref.refit(src, dst, poses, 0.03, 1)
    rinl = reference[1]
    print(f"the three poses end with {rinl.tolist()} inliers")
    assert len(set(rinl.tolist())) == 3 and reference[2]["n_improved"] == 3        # three different fits, none of them idle
    check_refit(ctx, src, dst, poses, 0.03, 1, reference)


def test_refit_two_fold_levels_plain_fit(ctx, two_level_rows):
    """The plain fit (poses_in NULL, every finite row) over the same rows: two levels under the mask of a pose that is not there."""
    src, dst = two_level_rows
    reference = posefit_ref.refit(src, dst, None, np.inf, 1)
    assert reference[1][0] == len(src)
    check_refit(ctx, src, dst, None, np.inf, 1, reference)


STRIDES = {
    # b: the rows of the live poses, the row of the best, the row of its copy, the seed (one that gives every live pose its own count)
    PF_MAX_POSES_Y + 5: ([0, 5, PF_MAX_POSES_Y - 1, PF_MAX_POSES_Y, PF_MAX_POSES_Y + 2], PF_MAX_POSES_Y + 2, None, 32776),
    PF_BEST_BLOCKS * PF_BLOCK + 300: ([0, 5, PF_MAX_POSES_Y - 1, PF_MAX_POSES_Y, PF_MAX_POSES_Y + 2, PF_BEST_BLOCKS * PF_BLOCK - 1,
                                       PF_BEST_BLOCKS * PF_BLOCK, PF_BEST_BLOCKS * PF_BLOCK + 10, PF_BEST_BLOCKS * PF_BLOCK + 299],
                                      PF_BEST_BLOCKS * PF_BLOCK + 10, PF_BEST_BLOCKS * PF_BLOCK + 200, 262450),
}


@pytest.mark.parametrize("b", sorted(STRIDES))
def test_refit_more_poses_than_the_grids(ctx, b):
    """32768 + 5 poses: k_pose_sweep (over blockIdx.y) and both folds take a second pose.  1024 * 256 + 300: so does k_pose_best, where
    the best and its copy 190 rows further on both lie in the strided pass.  All poses are void but a few, each of which ends with a
    count of its own."""
    rows, best_at, twin_at, seed = STRIDES[b]
    rng = np.random.default_rng(seed)
    src, dst = noisy_copy(rng, 70, wrong=0.2, noise=0.015)
    live = np.stack([perturbed(rng, d, 0.01) for d in np.linspace(0.5, 4.0, len(rows))])
    alone = posefit_ref.refit(src, dst, live, 0.03, 2)[1]             # what each live pose ends with
    assert len(set(alone.tolist())) == len(rows)
    order = np.argsort(-alone, kind="stable")                         # the best first, then by falling count
    others = [r for r in rows if r != best_at]
    poses = np.full((b, 12), np.nan)
    poses[best_at] = live[order[0]]
    poses[others] = live[order[1:]]
    n_live = len(rows)
    if twin_at is not None:
        poses[twin_at] = poses[best_at]                               # a tie inside the strided pass of k_pose_best: the lower row
        n_live += 1
    reference = posefit_ref.refit(src, dst, poses, 0.03, 2)
    rinl, rec = reference[1], reference[2]
    print(f"b={b}: the live poses end with {rinl[rinl >= 0].tolist()}")
    assert rec["best"] == best_at and rec["n_void"] == b - n_live and (rinl >= 0).sum() == n_live
    assert twin_at is None or rinl[twin_at] == rec["best_inliers"]
    check_refit(ctx, src, dst, poses, 0.03, 2, reference)
