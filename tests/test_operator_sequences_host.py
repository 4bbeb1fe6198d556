"""The call-sequence fuzz of the operators (tests/fuzz_operators.py), the parts that need no GPU: the tour takes every ordered pair of
operator kinds and both road transitions on every shared staging buffer; the driver replays the tour and random seeds on a
reference-backed context and reports nothing; and it reports faults planted in thin wrappers around that context -- a stale tail
behind a shorter staging copy, a record field that accumulates, a search that answers from the slot's previous cloud, an iteration
bounded by a match from before another operator's call -- at the move where they happen and by the operator's name."""
import numpy as np
import pytest

import fpfh_ref
import fuzz_operators as fo
import normal_angle_ref
import outlier_ref
import voxel_ref
from fuzz_operators import DEVICE, HOST, array_of, plan_move
from oracle import orc
from test_consistency_host import ConsistencyOracleContext
from test_eval_host import EvalOracleContext
from test_keypoints_host import KeypointOracleContext
from test_outlier_host import OutlierOracleContext
from test_posefit_host import PosefitOracleContext


# ---- the reference-backed context ---------------------------------------------------------------------------------------------------
class ReferenceContext(ConsistencyOracleContext, KeypointOracleContext, PosefitOracleContext, EvalOracleContext, OutlierOracleContext):
    """The host tests' stand-in contexts under one roof, and the pointer forms of their entries: an array is a numpy array (host
    memory) or a fuzz_operators.StandInArray (device memory); outputs are written in place."""

    def __init__(self):
        super().__init__()
        self.nv = {}

    def _leave(self, buffer, out, values):
        """`values` into the caller's array `out`; buffer: the staging buffer a host array would pass through (None: its own)."""
        a = array_of(out)
        a.reshape(-1)[:] = np.asarray(values).reshape(-1)

    def last_match_kernel(self):
        return "reference"

    # -- matched rows --
    def feature_match(self, query, target, nq=None, nt=None, dim=None, idx_ptr=None, d2_ptr=None, want_d2=True):
        idx, d2, rec = super().feature_match(array_of(query), array_of(target))
        self._leave("gl_idx", idx_ptr, idx)
        self._leave(None, d2_ptr, d2)
        return rec

    def ransac_triplets(self, src, dst, triples, max_distance, edge_ratio, m=None, h=None, poses_ptr=None, inliers_ptr=None,
                        want_poses=True):
        P, inl, rec = super().ransac_triplets(array_of(src), array_of(dst), array_of(triples), max_distance, edge_ratio)
        self._leave("gl_pose", poses_ptr, P)
        self._leave("gl_idx", inliers_ptr, inl)
        return rec

    def pose_refit(self, src, dst, poses, max_distance, rounds, m=None, b=None, poses_ptr=None, inliers_ptr=None):
        P, inl, rec = super().pose_refit(array_of(src), array_of(dst), None if poses is None else array_of(poses), max_distance, rounds)
        self._leave("gl_pose", poses_ptr, P)
        self._leave("gl_idx", inliers_ptr, inl)
        return rec

    def pose_robust(self, src, dst, poses, max_distance, rounds, divisor, start_scale=0.0, m=None, b=None, poses_ptr=None,
                    inliers_ptr=None, scales_ptr=None):
        P, inl, scales, rec = super().pose_robust(array_of(src), array_of(dst), None if poses is None else array_of(poses), max_distance,
                                                  rounds, divisor, start_scale)
        self._leave("gl_pose", poses_ptr, P)
        self._leave("gl_idx", inliers_ptr, inl)
        self._leave(None, scales_ptr, scales)
        return rec

    def match_consistency(self, src, dst, tolerance, min_length, m=None, degree_ptr=None, core_ptr=None):
        degree, core, rec = super().match_consistency(array_of(src), array_of(dst), tolerance, min_length)
        self._leave("gl_idx", degree_ptr, degree)
        self._leave(None, core_ptr, core)
        return rec

    # -- slots --
    def voxel_select(self, slot, voxel_size, origin=None, rows=None, keep_ptr=None):
        keep = super().voxel_select(slot, voxel_size, origin, rows)
        if keep_ptr is None:
            return keep
        self._leave(None, keep_ptr, keep)
        return int(keep.sum())

    def voxel_select_masked(self, slot, mask_ptr, n, voxel_size, origin=None, keep_ptr=None):
        self._log("voxel_select_masked")
        keep = voxel_ref.keep(self.cloud[slot][0], voxel_size, (0.0, 0.0, 0.0) if origin is None else tuple(origin), mask=array_of(mask_ptr))
        self._leave(None, mask_ptr if keep_ptr is None else keep_ptr, keep)
        return int(keep.sum())

    def outlier_statistical(self, slot, k, std_ratio, rows=None, mask_ptr=None, keep_ptr=None, mean_ptr=None):
        if mask_ptr is None:
            keep, d, rec = super().outlier_statistical(slot, k, std_ratio, rows=rows)
        else:
            self._log("outlier_statistical")
            r = outlier_ref.statistical(self.cloud[slot][0], k, std_ratio, mask=array_of(mask_ptr))
            keep, d, rec = r["keep"], r["d"], {key: r[key] for key in ("n_candidates", "n_kept", "mean", "std", "threshold")}
        if keep_ptr is None:
            return keep, d, rec
        self._leave(None, keep_ptr, keep)
        self._leave(None, mean_ptr, d)
        return rec

    def outlier_radius(self, slot, radius, min_points, rows=None, mask_ptr=None, keep_ptr=None, count_ptr=None):
        self._log("outlier_radius")
        r = outlier_ref.radius(self.cloud[slot][0], radius, min_points, rows=rows, mask=None if mask_ptr is None else array_of(mask_ptr))
        if keep_ptr is None:
            return r["keep"], r["count"], r["n_kept"]
        self._leave(None, keep_ptr, r["keep"])
        self._leave(None, count_ptr, r["count"])
        return r["n_kept"]

    def evaluate(self, query_slot, search_slot, H=None, max_distance=np.inf, rows=None):
        return super().evaluate(query_slot, search_slot, H, max_distance, None if rows is None else array_of(rows))

    def fpfh(self, slot, normals, k, radius=np.inf, viewpoint=None, fpfh_ptr=None, counts_ptr=None, want_counts=False):
        self._log("fpfh")
        r = fpfh_ref.fpfh(self.cloud[slot][0], array_of(normals), k, radius, viewpoint)
        rec = {key: r[key] for key in ("n_points", "n_pairs", "n_void_pairs", "n_empty")}
        if fpfh_ptr is None:
            return r["fpfh"], (r["counts"] if want_counts else None), rec
        self._leave(None, fpfh_ptr, r["fpfh"])
        self._leave(None, counts_ptr, r["counts"])
        return rec

    def keypoints(self, slot, k_s, salient_radius=np.inf, k_n=None, nms_radius=np.inf, gamma21=0.975, gamma32=0.975, min_neighbors=5,
                  keep_ptr=None, saliency_ptr=None, eig_ptr=None, want_saliency=False):
        keep, sal, eig, rec = super().keypoints(slot, k_s, salient_radius, k_n, nms_radius, gamma21, gamma32, min_neighbors, want_saliency=True)
        if keep_ptr is None:
            return keep, (sal if want_saliency else None), (eig if want_saliency else None), rec
        self._leave(None, keep_ptr, keep)
        self._leave(None, saliency_ptr, sal)
        self._leave(None, eig_ptr, eig)
        return rec

    # -- the movable cloud's normal columns and the rejection by them --
    def upload(self, slot, xyz, index_base=0):
        super().upload(slot, xyz, index_base)
        self.nv.pop(slot, None)

    def set_normals(self, slot, normals=None, rows=None, n_global=None):
        self._log("set_normals")
        if normals is None:
            self.nv.pop(slot, None)
        else:
            self.nv[slot] = np.array(normals, dtype=np.float32).reshape(-1, 3)

    def corr_reject_normal_angle(self, cos_max, k=10, H=None, pc2_normals=None):
        from simpleicp_amd import _lib
        self._log("corr_reject_normal_angle")
        self._need_corr()
        Hm = np.eye(4) if H is None else np.asarray(H, dtype=np.float64).reshape(4, 4)
        if pc2_normals is not None:
            n2 = np.asarray(pc2_normals, dtype=np.float32)
        elif _lib.MOV in self.nv:
            n2 = self.nv[_lib.MOV][self._idx]
        else:
            n2 = normal_angle_ref.movable_normals(self.cloud[_lib.MOV][0], self._idx, k)
        self._alive &= normal_angle_ref.verdict(self._n1, n2, Hm, cos_max)
        return int(self._alive.sum())


def clean_replay(moves, ctx=None, seed=0):
    forced = {"sweeps": ReferenceContext(), "one": ReferenceContext()}
    return fo.replay(moves, ctx or ReferenceContext(), fo.StandInMemory(), ReferenceContext, forced, seed)


# ---- the tour -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tour():
    return fo.tour()


def test_the_tour_takes_every_ordered_pair_and_every_road_transition(tour):
    kinds = [mv["kind"] for mv in tour]
    assert set(kinds) == set(fo.KINDS) and len(fo.KINDS) == 23
    pairs = set(zip(kinds, kinds[1:]))
    missing = [(a, b) for a in fo.KINDS for b in fo.KINDS if (a, b) not in pairs]
    assert not missing, missing
    # an upload to the fixed slot ends the setup: before a move that needs one it would put a setup between the two
    for a, b in zip(tour, tour[1:]):
        assert not (a["kind"] == "upload" and a["slot"] == 0 and b["kind"] in fo.NEEDS_SETUP)
    for buffer in ("gl_idx", "gl_src", "gl_dst", "gl_pose", "pf_in"):
        seen = {(fo.uses(a)[buffer], fo.uses(b)[buffer]) for a, b in zip(tour, tour[1:]) if buffer in fo.uses(a) and buffer in fo.uses(b)}
        assert {(HOST, DEVICE), (DEVICE, HOST), (HOST, HOST), (DEVICE, DEVICE)} <= seen, (buffer, seen)
    # mixed calls: arrays of one call on different roads; every size of the seam lists
    assert any(len(set(mv["roads"].values())) == 2 for mv in tour if "roads" in mv)
    assert {mv["m"] for mv in tour if "m" in mv} == set(fo.M_ROWS)
    assert {mv["b"] for mv in tour if "b" in mv} == set(fo.POSES) and {mv["h"] for mv in tour if "h" in mv} == set(fo.TRIPLES)
    assert {mv["rows"] for mv in tour if "rows" in mv} == set(fo.ROWS)
    for kind in ("voxel_select", "outlier_statistical", "outlier_radius"):
        assert {mv["form"] for mv in tour if mv["kind"] == kind} == {"rows", "mask", "whole"}
    assert {(mv["with_rows"], mv["with_H"]) for mv in tour if mv["kind"] == "evaluate"} == {(a, b) for a in (False, True) for b in (False, True)}


def test_moves_depend_on_the_seed_alone(tour):
    assert fo.tour() == tour
    assert fo.random_moves(3) == fo.random_moves(3) and fo.random_moves(3) != fo.random_moves(11)
    # a large call is mostly followed by a small one
    after = [b["m"] for a, b in zip(tour, tour[1:]) if a["big"] and "m" in b]
    assert sum(m <= 65 for m in after) > len(after) // 2
    # the scripted openings
    first = fo.random_moves(0)[:2]
    assert [mv["kind"] for mv in first] == ["match_consistency", "pose_refit"] and first[0]["m"] == 4097 and first[1]["b"] == 5
    assert set(first[0]["roads"].values()) == set(first[1]["roads"].values()) == {HOST}
    assert [mv["kind"] for mv in fo.random_moves(3)[:6]] == ["upload", "upload", "icp_setup", "icp_run", "keypoints", "fpfh"]


# ---- the clean replay -------------------------------------------------------------------------------------------------------------------
CHUNK = 54


@pytest.mark.parametrize("part", range(10))
def test_the_tour_replays_clean_on_the_reference_context(tour, part):
    moves = tour[part * CHUNK:(part + 1) * CHUNK + 1]                 # (one move of overlap: the pair across the cut)
    assert part < 9 or (part + 1) * CHUNK + 1 >= len(tour)
    bad, log, _, step = clean_replay(moves, seed=part)
    assert bad == [] and step is None, "\n".join(log[-12:] + bad)


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 9])
def test_random_seeds_replay_clean_on_the_reference_context(seed):
    bad, log, _, step = clean_replay(fo.random_moves(seed), seed=seed)
    assert bad == [] and step is None, "\n".join(log[-12:] + bad)


# ---- planted faults -----------------------------------------------------------------------------------------------------------------------
class StaleTail(ReferenceContext):
    """(a) A staging buffer whose copy is as long as the PREVIOUS call's count: the entries beyond it keep what the buffer held."""

    def __init__(self):
        super().__init__()
        self.buf, self.count = {}, {}

    def _leave(self, buffer, out, values):
        if buffer is None or not isinstance(out, np.ndarray):             # (device memory is written in place)
            return super()._leave(buffer, out, values)
        v = np.asarray(values).reshape(-1)
        old = self.buf.get(buffer, np.zeros(0, v.dtype))
        buf = np.zeros(max(len(old), len(v)), v.dtype)
        buf[:len(old)] = old.astype(v.dtype)
        fresh = len(v) if buffer not in self.count else min(len(v), self.count[buffer])
        buf[:fresh] = v[:fresh]
        self.buf[buffer], self.count[buffer] = buf, len(v)
        super()._leave(buffer, out, buf[:len(v)])


class AccumulatingRecord(ReferenceContext):
    """(b) Record fields that are added to call after call instead of starting at zero: n_void, n_valid."""

    def __init__(self):
        super().__init__()
        self.total = {"n_void": 0, "n_valid": 0}

    def _more(self, rec):
        rec = dict(rec)
        for key in self.total:
            if key in rec:
                self.total[key] += rec[key]
                rec[key] = self.total[key]
        return rec

    def pose_refit(self, *a, **kw):
        return self._more(super().pose_refit(*a, **kw))

    def ransac_triplets(self, *a, **kw):
        return self._more(super().ransac_triplets(*a, **kw))

    def match_consistency(self, *a, **kw):
        return self._more(super().match_consistency(*a, **kw))


class StaleSearch(ReferenceContext):
    """(c) A stand-alone search that answers from the cloud the slot held before its last upload."""

    def __init__(self):
        super().__init__()
        self.before = {}

    def upload(self, slot, xyz, index_base=0):
        if slot in self.cloud:
            self.before[slot] = self.cloud[slot]
        super().upload(slot, xyz, index_base)

    def knn(self, slot, q_xyz, k=1, H=None, max_dist=np.inf):
        X, base = self.before.get(slot, self.cloud[slot])
        return orc.knn(X, np.asarray(q_xyz, dtype=np.float64), k=k, H=H, max_dist=max_dist, idx_base=base)


class StaleBound(ReferenceContext):
    """(d) An iteration whose search is bounded by the match from before an interleaved keypoints or fpfh call: a query whose
    nearest point lies beyond that bound keeps the old match."""

    def __init__(self):
        super().__init__()
        self.interleaved = False
        self.old = None

    def keypoints(self, *a, **kw):
        self.interleaved = self.old is not None
        return super().keypoints(*a, **kw)

    def fpfh(self, *a, **kw):
        self.interleaved = self.old is not None
        return super().fpfh(*a, **kw)

    def icp_setup(self, *a, **kw):
        self.old, self.interleaved = None, False
        super().icp_setup(*a, **kw)

    def _iterate(self, x, obs, ow, min_planarity, w):
        from simpleicp_amd import _lib
        if not self.interleaved:
            try:
                return super()._iterate(x, obs, ow, min_planarity, w)
            finally:
                self.old = self._idx.copy()
        self.interleaved = False
        Xm = self.cloud[_lib.MOV][0]
        H = orc.params_to_H(x)
        true_idx, true_d2 = orc.knn(Xm, self._p1, k=1, H=H)
        old_d2 = ((orc.transform(H, Xm[self.old]) - self._p1) ** 2).sum(axis=1)
        stale = np.where(true_d2[:, 0] < 0.25 * old_d2, true_idx[:, 0], self.old)      # (half the old distance as the bound)
        real = orc.knn
        orc.knn = lambda *a, **kw: (stale[:, None], true_d2) if kw.get("k") == 1 and len(a[1]) == len(stale) else real(*a, **kw)
        try:
            return super()._iterate(x, obs, ow, min_planarity, w)
        finally:
            orc.knn = real


def _planned(kinds_and_fixed, seed=5):
    rng = np.random.default_rng(seed)
    return [plan_move(kind, rng, False, **fixed) for kind, fixed in kinds_and_fixed]


def _all(kind, road):
    return dict.fromkeys(fo.ARRAYS[kind], road)


def test_a_stale_tail_behind_a_shorter_copy_is_found_where_the_count_grows():
    moves = _planned([("pose_refit", dict(m=300, b=5, null_start=False, roads=_all("pose_refit", HOST))),
                      ("knn", {}),
                      ("match_consistency", dict(m=3, roads=_all("match_consistency", HOST))),        # (shorter: nothing to see)
                      ("ransac_triplets", dict(m=65, h=255, roads=_all("ransac_triplets", DEVICE))),    # (device memory: not staged)
                      ("match_consistency", dict(m=64, roads=_all("match_consistency", HOST))),
                      ("pose_refit", dict(m=64, b=1, roads=_all("pose_refit", HOST)))])
    assert clean_replay(moves)[0] == []
    bad, log, _, step = clean_replay(moves, StaleTail())
    assert step == 4 and bad[0].startswith("match_consistency m=64") and "degree differs" in bad[0], bad
    # ... and in the tour, at the first move whose staged array outgrows the one before it
    tour = fo.tour()[:120]
    bad, log, _, step = clean_replay(tour, StaleTail())
    count, expect = {}, None
    for i, mv in enumerate(tour):
        if mv["kind"] in fo.MATCHED:
            n = {"inliers": mv.get("b") if mv["kind"] != "ransac_triplets" else mv["h"], "poses": 12 * (mv.get("b") or mv.get("h") or 0),
                 "idx": mv["m"], "degree": mv["m"]}
            for buffer in ("gl_idx", "gl_pose"):
                name = fo.STAGED[buffer].get(mv["kind"])
                if name is None or mv["roads"][name] == DEVICE:             # (device memory is not staged)
                    continue
                if buffer in count and n[name] > count[buffer] and expect is None:
                    expect = i
                count[buffer] = n[name]
        if expect is not None:
            break
    assert expect is not None and step == expect and bad[0].startswith(tour[step]["kind"]), (step, expect, bad)


def test_an_accumulating_record_field_is_found_at_the_second_call():
    moves = _planned([("match_consistency", dict(m=63)), ("voxel_select", {}), ("pose_refit", dict(m=300, b=5, null_start=False)),
                      ("match_consistency", dict(m=3)), ("pose_refit", dict(m=65, b=70, null_start=False))])
    assert clean_replay(moves)[0] == []
    bad, _, _, step = clean_replay(moves, AccumulatingRecord())
    assert step == 3 and bad[0].startswith("match_consistency m=3") and "n_valid" in bad[0], bad       # 63 + 3 valid rows
    bad, _, _, step = clean_replay(moves[1:3] + moves[4:], AccumulatingRecord())
    assert step == 2 and bad[0].startswith("pose_refit m=65 b=70") and "n_void" in bad[0], bad          # one void pose a call


def test_a_search_of_the_previous_cloud_is_found_at_the_first_search_after_the_upload():
    moves = _planned([("knn", {}), ("upload", dict(slot=1)), ("fpfh", dict(slot=0)), ("knn", {}), ("knn", {})])
    assert clean_replay(moves)[0] == []
    bad, _, _, step = clean_replay(moves, StaleSearch())
    # (the replay's own two uploads are each slot's first: the move's upload is the first that leaves a cloud behind)
    assert step == 3 and bad[0].startswith("knn "), bad


def test_an_iteration_bounded_by_an_older_match_is_found_after_the_interleaved_operator():
    for between in ("keypoints", "fpfh"):
        moves = _planned([("upload", dict(slot=0, n=1500)), ("upload", dict(slot=1, n=1500)), ("icp_setup", {}), ("icp_iterate", {}),
                          ("icp_iterate", {}), (between, dict(slot=1)), ("evaluate", {}), ("icp_iterate", {}), ("icp_iterate", {})])
        assert clean_replay(moves)[0] == []
        bad, log, _, step = clean_replay(moves, StaleBound())
        assert step == 7 and bad[0].startswith("icp_iterate"), (between, step, bad, log)


def test_an_input_that_is_written_to_is_reported():
    class Scribbler(ReferenceContext):
        def pose_refit(self, src, dst, poses, *a, **kw):
            rec = super().pose_refit(src, dst, poses, *a, **kw)
            array_of(dst)[0, 0] += 1.0
            return rec
    moves = _planned([("pose_refit", dict(m=63, b=1, roads=_all("pose_refit", DEVICE)))])
    bad, _, _, step = clean_replay(moves, Scribbler())
    assert step == 0 and "the input dst was written to" in bad[0]
