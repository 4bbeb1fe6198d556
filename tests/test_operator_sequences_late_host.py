"""The second ring of the operators' call-sequence fuzz (tests/fuzz_operators_late.py), the parts that need no GPU: the late tour
takes every ordered pair of kinds with a late one in it exactly once and all four road transitions between an old and a late user
of every shared staging buffer; the driver replays the tour, the scripted openings and random seeds on a reference-backed context
and reports nothing; and it reports faults planted in thin wrappers around that context -- a stale tail in gl_pose between a pose
and a plane call, a plane record that keeps the larger of two calls' best words, an orient that answers from the lists of the
slot's previous cloud, core bytes OR-ed with the radius filter's keep bytes, a farthest that writes to its mask -- at the move
where they happen and by the operator's name."""
import numpy as np
import pytest

import cluster_ref
import fuzz_operators as fo
import fuzz_operators_late as fl
import orient_ref
from fuzz_operators import DEVICE, HOST, array_of
from test_operator_sequences_host import ReferenceContext, StaleTail

TRANSITIONS = {(HOST, HOST), (HOST, DEVICE), (DEVICE, HOST), (DEVICE, DEVICE)}


# ---- the reference-backed context ---------------------------------------------------------------------------------------------------
class LateReferenceContext(ReferenceContext):
    """ReferenceContext, and the five late entries in their host and pointer forms, answered by their references.  Outputs leave
    through _leave with the staging buffer named that a host array would pass through."""

    def _leave(self, buffer, out, values):
        if out is not None:
            super()._leave(buffer, out, values)

    def cluster(self, slot, radius, min_points, labels_ptr=None, core_ptr=None):
        self._log("cluster")
        r = fl.ref_cluster(self.cloud[slot][0], radius, min_points)
        labels, core = r["labels"].copy(), self._core(slot, r["core"].copy())
        if labels_ptr is None:
            return labels, core, cluster_ref.record(r)
        self._leave(None, labels_ptr, labels)
        self._leave(None, core_ptr, core)
        return cluster_ref.record(r)

    def _core(self, slot, core):
        return core

    def plane_triplets(self, X, triples, max_distance, mask=None, n=None, h=None, planes_ptr=None, inliers_ptr=None, want_planes=True):
        self._log("plane_triplets")
        P, inl, rec = fl.ref_triplets(array_of(X), None if mask is None else array_of(mask), array_of(triples), max_distance)
        self._leave("gl_pose", planes_ptr, P)
        self._leave("gl_idx", inliers_ptr, inl)
        return dict(rec)

    def plane_refit(self, X, planes, max_distance, rounds, mask=None, n=None, b=None, planes_ptr=None, inliers_ptr=None, keep_ptr=None,
                    want_keep=False):
        self._log("plane_refit")
        assert keep_ptr is None or b == 1
        P, inl, keep, rec = fl.ref_refit(array_of(X), None if mask is None else array_of(mask), array_of(planes), max_distance, rounds,
                                         keep_ptr is not None)
        self._leave("gl_pose", planes_ptr, P)
        self._leave("gl_idx", inliers_ptr, inl)
        self._leave("pl_keep", keep_ptr, keep)
        return dict(rec)

    def farthest(self, X, count, start=-1, mask=None, n=None, idx_ptr=None, d2_ptr=None, want_d2=True):
        self._log("farthest")
        idx, d2, rec = fl.ref_farthest(array_of(X), None if mask is None else array_of(mask), count, start)
        self._leave("fp_idx", idx_ptr, idx)
        self._leave("fp_d2", d2_ptr, d2)
        return dict(rec)

    def orient(self, slot, normals, k, reference=None, away=False, normals_ptr=None, flipped_ptr=None, want_flipped=True):
        self._log("orient")
        N = np.array(array_of(normals), dtype=np.float32)             # (a copy: normals_ptr may be the same array)
        ref = fl.ref_orient(self.cloud[slot][0], N, k, reference, away, idx=self._lists(slot, k))
        self._leave("or_out", normals_ptr, ref["normals"])
        self._leave("or_flip", flipped_ptr, ref["flipped"])
        return orient_ref.record(ref)

    def _lists(self, slot, k):
        return None                                                   # (the reference's own: of the cloud the slot holds)


def clean_replay(moves, ctx=None, seed=0, notes=None):
    return fl.replay(moves, ctx or LateReferenceContext(), fo.StandInMemory(), LateReferenceContext, LateReferenceContext(),
                     LateReferenceContext, seed, notes)


# ---- the tour -------------------------------------------------------------------------------------------------------------------------
CHUNK = 36                                                            # tests/test_gpu_operator_sequences_late.py's


@pytest.fixture(scope="module")
def tour():
    return fl.late_tour()


@pytest.fixture(scope="module")
def tour_replays(tour):
    """every chunk of the tour (one move of overlap: the pair across the cut) on the reference context, once: (problems, log, step,
    what the references saw) per chunk"""
    out = []
    for part in range((len(tour) - 1 + CHUNK - 1) // CHUNK):
        notes = []
        bad, log, _, step = clean_replay(tour[part * CHUNK:(part + 1) * CHUNK + 1], seed=part, notes=notes)
        out.append((bad, log, step, notes))
    return out


def _late(mv):
    return mv["kind"] in fl.LATE


def test_the_late_tour_takes_its_255_pairs_once_and_every_road_transition(tour):
    assert fl.KINDS_ALL == fo.KINDS + fl.LATE and len(fl.KINDS_ALL) == 28
    kinds = [mv["kind"] for mv in tour[:256]]
    pairs = list(zip(kinds, kinds[1:]))
    want = {(a, b) for a in fl.KINDS_ALL for b in fl.KINDS_ALL if a in fl.LATE or b in fl.LATE}
    assert len(pairs) == 255 == 28 * 28 - 23 * 23 and set(pairs) == want and kinds[0] == kinds[-1]
    for a, b in zip(tour, tour[1:]):
        assert not (a["kind"] == "upload" and a["slot"] == 0 and b["kind"] in fo.NEEDS_SETUP)
    # every shared buffer: all four road transitions from an old user to a late one, and from a late one to an old one
    for buffer in fl.SHARED:
        for first_late in (False, True):
            seen = {(fl.uses(a)[buffer], fl.uses(b)[buffer]) for a, b in zip(tour, tour[1:])
                    if buffer in fl.uses(a) and buffer in fl.uses(b) and _late(a) == first_late and _late(b) != first_late}
            assert TRANSITIONS <= seen, (buffer, first_late, seen)
    # every entry of every seam list; arrays of one call on different roads; the outputs that may be NULL, there and not
    for kind, lists in fl.LISTS.items():
        mine = [mv for mv in tour if mv["kind"] == kind]
        for key, values in lists.items():
            if key != "count":
                assert {mv[key] for mv in mine} >= set(values), (kind, key)
        assert any(len(set(mv["roads"].values())) == 2 for mv in mine)
        for name in fl.ARRAYS[kind]:                                  # every array on either road, by the schedule and not by a draw
            assert {mv["roads"][name] for j, mv in enumerate(mine) if j % 3 == 0 and name in mv["roads"]} == {HOST, DEVICE}, (kind, name)
    far = [mv for mv in tour if mv["kind"] == "farthest"]
    assert {mv["count"] for mv in far} >= {1, 64, 257} and any(mv["count"] == mv["n"] > 257 for mv in far)
    assert any(mv["keep"] for mv in tour if mv["kind"] == "plane_refit") and all(mv["b"] == 1 for mv in tour if mv.get("keep"))
    for kind, name in (("cluster", "core"), ("plane_triplets", "planes"), ("farthest", "d2"), ("orient", "flipped")):
        assert {name in mv["roads"] for mv in tour if mv["kind"] == kind} == {False, True}
    for road in (HOST, DEVICE):
        assert any(mv["alias"] and mv["roads"]["normals"] == road for mv in tour if mv["kind"] == "orient")
    assert any(mv["h"] >= 5 for mv in tour if mv["kind"] == "plane_triplets")


def test_late_moves_depend_on_the_seed_alone(tour):
    assert fl.late_tour() == tour
    assert fl.late_random_moves(3) == fl.late_random_moves(3) and fl.late_random_moves(6) != fl.late_random_moves(14)
    # a large call is mostly followed by a small one
    after = [b["n"] for a, b in zip(tour, tour[1:]) if a["big"] and "n" in b and _late(b)]
    assert sum(n <= 65 for n in after) > len(after) // 2
    # half the weight on the late five
    drawn = [mv for seed in (6, 7, 14, 15, 22, 23) for mv in fl.late_random_moves(seed)]
    assert 0.35 < sum(map(_late, drawn)) / len(drawn) < 0.65 and {mv["kind"] for mv in drawn if _late(mv)} == set(fl.LATE)
    # the scripted openings
    first = fl.late_random_moves(0)[:5]
    assert [mv["kind"] for mv in first] == ["pose_refit", "plane_triplets", "pose_refit", "plane_refit", "ransac_triplets"]
    assert [mv.get("b", mv.get("h")) for mv in first] == [70, 255, 5, 70, 1] and all(set(fl.uses(mv).values()) == {HOST} for mv in first)
    second = fl.late_random_moves(1)[:6]
    assert [(mv["kind"], mv.get("m", mv.get("n"))) for mv in second] == [("ransac_triplets", 1100), ("farthest", 300), ("plane_triplets", 65),
                                                                          ("pose_robust", 63), ("farthest", 2000), ("match_consistency", 64)]
    assert all(fl.uses(mv)["gl_src"] == HOST for mv in second)
    assert [mv["kind"] for mv in fl.late_random_moves(2)[:7]] == ["farthest", "ransac_triplets", "cluster", "plane_triplets", "pose_refit",
                                                                  "orient", "plane_refit"]
    fourth = fl.late_random_moves(3)[:6]
    assert [(mv["kind"], mv.get("form"), mv.get("slot")) for mv in fourth[:5]] == [("outlier_radius", "mask", 0), ("cluster", None, 0),
                                                                                   ("outlier_radius", "rows", 0), ("voxel_select", "mask", 1),
                                                                                   ("cluster", None, 1)] and fourth[5]["kind"] == "outlier_statistical"
    fifth = fl.late_random_moves(4)[:10]
    assert [mv["kind"] for mv in fifth] == ["fpfh", "orient", "estimate_normals", "orient", "upload", "orient", "transform", "orient", "keypoints",
                                            "cluster"]
    assert [mv.get("k") for mv in fifth[:4]] == [None, 33, None, 2] and fifth[4]["n"] == 250 and [mv["slot"] for mv in fifth[7:]] == [1, 1, 1]
    assert [mv["kind"] for mv in fl.late_random_moves(5)[:9]] == ["upload", "upload", "icp_setup", "icp_run", "orient", "cluster", "icp_iterate",
                                                                  "farthest", "icp_run"]
    assert fl.late_random_moves(6)[0] != fl.late_random_moves(14)[0]                                   # (no opening at 6 and 7 modulo 8)


# ---- the clean replay -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", range(8))
def test_the_late_tour_replays_clean_on_the_reference_context(tour, tour_replays, part):
    assert len(tour_replays) == 8 and 8 * CHUNK + 1 >= len(tour) > 7 * CHUNK + 1
    bad, log, step, _ = tour_replays[part]
    assert bad == [] and step is None, "\n".join(log[-12:] + bad)


def test_the_tour_shows_clusters_noise_and_border_points_and_void_planes(tour_replays):
    notes = [note for _, _, _, part in tour_replays for note in part]
    clusters = [note for note in notes if note["kind"] == "cluster"]
    assert any(note["n_clusters"] >= 2 for note in clusters) and any(note["n_noise"] > 0 for note in clusters)
    assert any(note["n_border"] > 0 for note in clusters) and any(note["n_core"] > 0 and note["n_noise"] > 0 and note["n_border"] > 0 for note in clusters)
    # ... and void planes with their -1 inliers, void start planes, rows that are no candidates, more components than one
    assert any(0 < note["n_void"] < note["n_hypotheses"] for note in notes if note["kind"] == "plane_triplets")
    assert any(note["n_void"] > 0 for note in notes if note["kind"] == "plane_refit")
    assert any(0 < note["n_selected"] <= note["n_candidates"] < note["n_points"] for note in notes if note["kind"] == "farthest")
    assert any(note["n_components"] > 2 and note["n_flipped"] > 0 for note in notes if note["kind"] == "orient")
    assert any(note["n_components_voted"] > 0 for note in notes if note["kind"] == "orient")


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4, 5, 6, 15])
def test_openings_and_random_seeds_replay_clean_on_the_reference_context(seed):
    notes = []
    bad, log, _, step = clean_replay(fl.late_random_moves(seed), seed=seed, notes=notes)
    assert bad == [] and step is None, "\n".join(log[-12:] + bad)
    if seed == 2:
        # the opening's cluster has several clusters (word 3), its plane_triplets no plane at all
        assert notes[1]["kind"] == "cluster" and notes[1]["n_clusters"] >= 2
        assert notes[2]["kind"] == "plane_triplets" and (notes[2]["best"], notes[2]["best_inliers"], notes[2]["n_void"]) == (-1, -1, 255)
    if seed == 4:
        # the opening's k are the model's draws under seeds chosen for them: the log says what they came to (the replay's two uploads first)
        assert log[2].startswith("fpfh slot=0") and " k=12 " in log[2] and log[4].startswith("estimate_normals slot=0") and log[4].endswith(" rows=64 k=8")
        assert " k=33 " in log[3] and " k=2 " in log[5] and log[6] == "upload FIX n=250"


# ---- planted faults -----------------------------------------------------------------------------------------------------------------------
class LateStaleTail(StaleTail, LateReferenceContext):
    """(a) test_operator_sequences_host.StaleTail under the late entries: a staging copy as long as the PREVIOUS call's count."""


class LargerBestWord(LateReferenceContext):
    """(b) A plane record whose best / best_inliers come from the larger of this call's and the previous call's word: a max into a
    word that was not cleared."""

    def __init__(self):
        super().__init__()
        self.word = (-1, -1)

    def ransac_triplets(self, *a, **kw):
        rec = super().ransac_triplets(*a, **kw)
        self.word = (rec["best_inliers"], rec["best"])
        return rec

    def plane_triplets(self, *a, **kw):
        rec = super().plane_triplets(*a, **kw)
        if self.word[0] > rec["best_inliers"]:
            rec["best_inliers"], rec["best"] = self.word
        self.word = (rec["best_inliers"], rec["best"])
        return rec


class StaleLists(LateReferenceContext):
    """(c) An orient that answers from the k-NN lists of the cloud the slot held before its last upload."""

    def __init__(self):
        super().__init__()
        self.before = {}

    def upload(self, slot, xyz, index_base=0):
        if slot in self.cloud:
            self.before[slot] = self.cloud[slot][0]
        super().upload(slot, xyz, index_base)

    def _lists(self, slot, k):
        if slot not in self.before:
            return None
        old, n = self.before[slot], len(self.cloud[slot][0])
        idx = np.full((n, k), -1, np.int64)                           # (a row or a neighbour the old cloud did not have: none)
        L = orient_ref.lists(old, min(k, len(old)))[:n]
        idx[:len(L), :L.shape[1]] = L
        return idx


class CoreOverKeep(LateReferenceContext):
    """(d) Core bytes OR-ed with the keep bytes of the preceding masked outlier_radius: cand_keep written over, not cleared."""

    def __init__(self):
        super().__init__()
        self.keep = np.zeros(0, np.uint8)

    def outlier_radius(self, slot, radius, min_points, rows=None, mask_ptr=None, keep_ptr=None, count_ptr=None):
        got = super().outlier_radius(slot, radius, min_points, rows=rows, mask_ptr=mask_ptr, keep_ptr=keep_ptr, count_ptr=count_ptr)
        if mask_ptr is not None:
            self.keep = np.asarray(array_of(keep_ptr) if keep_ptr is not None else got[0]).view(np.uint8).copy()
        return got

    def _core(self, slot, core):
        k = min(len(core), len(self.keep))
        core[:k] |= self.keep[:k] != 0
        return core


class MaskScribbler(LateReferenceContext):
    """(e) A farthest that writes to its mask."""

    def farthest(self, X, count, start=-1, mask=None, **kw):
        rec = super().farthest(X, count, start, mask=mask, **kw)
        if mask is not None:
            array_of(mask)[0] ^= 1
        return rec


def _planned(kinds_and_fixed, seed=5):
    rng = np.random.default_rng(seed)
    return [fl.plan_move(kind, rng, False, **fixed) for kind, fixed in kinds_and_fixed]


def _host(kind):
    """every array in host memory but the inliers: gl_pose is the buffer in view, gl_idx stays out of it"""
    return dict(dict.fromkeys(fl.ARRAYS[kind], HOST), inliers=DEVICE)


def _device(kind):
    return dict.fromkeys(fl.ARRAYS[kind], DEVICE)


def test_a_stale_tail_in_gl_pose_is_found_at_the_plane_call_where_the_doubles_grow():
    moves = _planned([("pose_refit", dict(m=300, b=70, null_start=False, roads=_host("pose_refit"))),              # 840 doubles
                      ("plane_triplets", dict(n=65, h=1, null_planes=False, mask="none", roads=_host("plane_triplets"))),  # 4: nothing to see
                      ("cluster", {}),
                      ("plane_refit", dict(n=65, b=70, mask="none", roads=_device("plane_refit"))),                 # (device memory: not staged)
                      ("pose_refit", dict(m=64, b=5, null_start=False, roads=_host("pose_refit"))),                 # 60, above 4: found if
                      ("plane_triplets", dict(n=64, h=255, null_planes=False, mask="none", roads=_host("plane_triplets")))])   # it came first
    assert clean_replay(moves)[0] == []
    bad, _, _, step = clean_replay(moves, LateStaleTail())
    assert step == 4 and bad[0].startswith("pose_refit m=64 b=5"), bad
    bad, _, _, step = clean_replay(moves[:4] + moves[5:], LateStaleTail())                              # 4 doubles, then 1 020
    assert step == 4 and bad[0].startswith("plane_triplets n=64 h=255") and "planes differs" in bad[0], bad
    # ... and the other way round: a plane call's four doubles a hypothesis, then a pose call's twelve
    moves = _planned([("plane_refit", dict(n=64, b=5, mask="none", roads=_host("plane_refit"))),
                      ("pose_refit", dict(m=63, b=5, null_start=False, roads=_host("pose_refit")))])
    assert clean_replay(moves)[0] == []
    bad, _, _, step = clean_replay(moves, LateStaleTail())
    assert step == 1 and bad[0].startswith("pose_refit m=63 b=5") and "poses differs" in bad[0], bad


def test_a_best_word_that_keeps_the_larger_of_two_calls_is_found_at_the_plane_call():
    moves = _planned([("plane_triplets", dict(n=2000, h=255, scene="plane", mask="none")), ("ransac_triplets", dict(m=1100, h=255)),
                      ("orient", {}), ("plane_triplets", dict(n=64, h=255, mask="none"))])
    assert clean_replay(moves)[0] == []
    bad, _, _, step = clean_replay(moves, LargerBestWord())
    assert step == 3 and bad[0].startswith("plane_triplets n=64 h=255") and "the record is" in bad[0] and "best_inliers" in bad[0], bad


def test_an_orient_on_the_previous_clouds_lists_is_found_at_the_first_orient_after_the_upload():
    moves = _planned([("orient", dict(slot=0, k=8)), ("upload", dict(slot=0, n=300)), ("cluster", dict(slot=0)), ("orient", dict(slot=1, k=8)),
                      ("orient", dict(slot=0, k=8)), ("orient", dict(slot=0, k=2))])
    assert clean_replay(moves)[0] == []
    bad, _, _, step = clean_replay(moves, StaleLists())
    # (the replay's own two uploads are each slot's first: the move's upload is the first that leaves a cloud behind)
    assert step == 4 and bad[0].startswith("orient slot=0"), bad


def test_core_bytes_over_the_radius_filters_keep_bytes_are_found_at_the_cluster():
    wide = fl._seed_where(0.6, [0.3, 0.6])                            # (the radius is the model's first draw: 0.6, more than 4 points)
    moves = _planned([("cluster", dict(slot=0, radius=0.6, min_points=8, null_core=False)), ("outlier_radius", dict(form="rows", slot=0, seed=wide)),
                      ("outlier_radius", dict(form="mask", slot=0, seed=wide)), ("cluster", dict(slot=0, radius=0.6, min_points=8, null_core=False))])
    assert clean_replay(moves)[0] == []
    bad, log, _, step = clean_replay(moves, CoreOverKeep())
    assert " r=0.6 " in log[3] and " r=0.6 " in log[4]
    assert step == 3 and bad[0].startswith("cluster slot=0") and "core differs" in bad[0], bad


def test_a_farthest_that_writes_to_its_mask_is_reported_as_an_input_written_to():
    for form, road in (("host", HOST), ("device", DEVICE)):
        moves = _planned([("farthest", dict(n=300, mask="none")), ("farthest", dict(n=300, mask=form))])
        assert clean_replay(moves)[0] == []
        bad, _, _, step = clean_replay(moves, MaskScribbler())
        assert step == 1 and bad[0].startswith("farthest n=300") and "the input mask was written to" in bad[0], bad
        assert moves[1]["roads"]["mask"] == road
