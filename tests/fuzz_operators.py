"""Seeded random CALL SEQUENCES over every entry of one context, the stand-alone operators included: tests/fuzz_sequence.py keeps a
model of the ICP core; the operators share far more between calls -- the eight counter words of c->cand_small with private meanings
per operator, the staging buffers gl_idx / gl_src / gl_dst / gl_pose / pf_in that are used only when the caller's array is host
memory and never shrink, the chunked k-NN's query columns and slots, the normal cache -- and each operator's own test file runs on a
context that does little else.  Here every move is held against the reference its own file uses, compared as that file compares
(bit for bit everywhere but the normals, which are also held against the same call on a context that has done nothing else).

A move is a dict drawn by plan_move from the seed alone: its kind, its sizes (from the seam lists below, a large call often
followed by a small one), the road of every array (host memory or device memory, independently) and a seed for its data.  No draw
looks at a result, so a list of moves can be replayed on any object with the entries of _lib.Context: the real one, or the
reference-backed stand-in of tests/test_operator_sequences_host.py.  Every output is prefilled with a sentinel and every input is
compared with its bytes from before the call."""
import os

import numpy as np

import consistency_ref
import eval_ref
import fpfh_ref
import fuzz_sequence
import global_ref
import iss_ref
import normal_angle_ref
import outlier_ref
import posefit_ref
import robust_ref
import voxel_ref
from fuzz_sequence import _small_H
from oracle import orc

MATCHED = ("feature_match", "ransac_triplets", "pose_refit", "pose_robust", "match_consistency")
SLOTS = ("voxel_select", "outlier_statistical", "outlier_radius", "evaluate", "fpfh", "keypoints", "estimate_normals", "select_in_range",
         "knn", "normal_angle")
STATE = ("upload", "transform", "set_planarity", "set_normals", "icp_setup", "icp_iterate", "icp_run", "operators")
KINDS = MATCHED + SLOTS + STATE
NEEDS_SETUP = ("normal_angle", "icp_iterate", "icp_run", "operators")

M_ROWS = (3, 63, 64, 65, 300, 1024, 1025, 1100)      # matched rows: a wave, a span of the pair tree, past both
M_SCRIPTED = 4097                                     # ... and past the one-launch peel's bound, in a scripted opening
POSES = (1, 5, 70, 257)
TRIPLES = (1, 255, 256, 1000)
ROWS = (1, 64, 65, 257, None)                         # selected rows of a slot; None: all
TARGETS = (1, 65, 257, 1000)                          # target rows of a descriptor match

# the arrays of a call over matched rows, and which of them passes through which shared staging buffer when it is host memory
ARRAYS = {"feature_match": ("query", "target", "idx", "d2"),
          "ransac_triplets": ("src", "dst", "triples", "poses", "inliers"),
          "pose_refit": ("src", "dst", "poses_in", "poses", "inliers"),
          "pose_robust": ("src", "dst", "poses_in", "poses", "inliers", "scales"),
          "match_consistency": ("src", "dst", "degree", "core")}
STAGED = {"gl_idx": {"feature_match": "idx", "ransac_triplets": "inliers", "pose_refit": "inliers", "pose_robust": "inliers",
                     "match_consistency": "degree"},
          "gl_src": dict.fromkeys(MATCHED[1:], "src"),
          "gl_dst": dict.fromkeys(MATCHED[1:], "dst"),
          "gl_pose": dict.fromkeys(MATCHED[1:4], "poses"),
          "pf_in": dict.fromkeys(MATCHED[2:4], "poses_in")}
HOST, DEVICE = 0, 1

# the many-queries kernels within reach of clouds of a few hundred points: 64 queries take four per wave, 512 the float32 filter
ENV = {"SICP_KNN1": "grid", "SICP_NN16_MIN_Q": "64", "SICP_NN16F_MIN_Q": "512", "SICP_ORDER_MIN_Q": "256"}
SENTINEL = -7


# ---- the two kinds of memory --------------------------------------------------------------------------------------------------------
class TorchMemory:
    """Device arrays are torch tensors on the context's GPU; what an entry takes for an address is an int."""

    def __init__(self, device="cuda:0"):
        import torch
        self.torch, self.device = torch, device

    def dev(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a).view(_plain(a.dtype))).to(self.device)
        self.torch.cuda.synchronize()                                 # (the library works on a stream of its own)
        return t

    def read(self, x, dtype):
        return (x if isinstance(x, np.ndarray) else x.cpu().numpy()).view(dtype)

    def ptr(self, x):
        return None if x is None else (x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr())

    def sync(self):
        self.torch.cuda.synchronize()


class StandInArray:
    """What stands for device memory where there is no device: an array the stand-in context reads and writes in place."""

    def __init__(self, a):
        self.a = np.array(a)
        self.shape = self.a.shape

    def data_ptr(self):
        return self


class StandInMemory:
    def dev(self, a):
        return StandInArray(a)

    def read(self, x, dtype):
        return (x if isinstance(x, np.ndarray) else x.a).view(dtype)

    def ptr(self, x):
        return x

    def sync(self):
        pass


def _plain(dtype):
    """(torch has no unsigned 16 / 32 bit tensors worth the name: such arrays travel as the signed type of their width)"""
    return {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.bool_): np.uint8}.get(np.dtype(dtype), dtype)


def array_of(x):
    """The numpy array behind a host array or a stand-in for device memory (the stand-in context's view of its arguments)."""
    return x.a if isinstance(x, StandInArray) else x


# ---- data -----------------------------------------------------------------------------------------------------------------------------
def _rotation(axis, angle):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


R_TRUE, T_TRUE = _rotation([1.0, 2.0, 3.0], 0.7), np.array([0.3, -0.2, 0.1])


def matched_rows(rng, m):
    """src, and dst = a rigid copy with a little noise, four rows in ten wrong (none of three)."""
    src = rng.uniform(-1, 1, (m, 3))
    dst = src @ R_TRUE.T + T_TRUE + rng.normal(0, 0.002, (m, 3))
    bad = rng.choice(m, int(0.4 * m) if m > 3 else 0, replace=False)
    dst[bad] = rng.uniform(-1, 1, (len(bad), 3))
    return src, dst


def start_poses(rng, b):
    """(b, 12): the true motion off by a few degrees and a little shift; where b allows, one pose that is no rotation (void)."""
    out = np.empty((b, 12))
    for k in range(b):
        R = _rotation(rng.standard_normal(3), np.radians(3.0) * rng.uniform(0.2, 1.0)) @ R_TRUE
        out[k, :9], out[k, 9:] = R.ravel(), T_TRUE + rng.normal(0, 0.01, 3)
    if b >= 5:
        out[int(rng.integers(0, b)), 0] = np.nan
    return out


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _record(st):
    return st.as_dict() if hasattr(st, "as_dict") else dict(st)


# ---- the moves' arguments, from the seed alone ----------------------------------------------------------------------------------------
def _size(rng, sizes, after_big, small=2):
    """One of `sizes`; after a large call mostly one of the `small` smallest: what the large one left behind is then in view."""
    if after_big and rng.random() < 0.7:
        return sizes[int(rng.integers(0, small))]
    return sizes[int(rng.integers(0, len(sizes)))]


def plan_move(kind, rng, after_big=False, **fixed):
    """One move of `kind`: sizes, variants and roads drawn from rng, `fixed` laid over them.  move["big"]: a large call."""
    mv = {"kind": kind, "seed": int(rng.integers(1 << 31))}
    if kind in MATCHED:
        mv["m"] = int(_size(rng, M_ROWS, after_big, 4))
        mv["roads"] = {a: int(rng.integers(0, 2)) for a in ARRAYS[kind]}
        if kind == "feature_match":
            mv["nt"] = int(_size(rng, TARGETS, after_big))
        if kind == "ransac_triplets":
            mv["h"] = int(_size(rng, TRIPLES, after_big))
        if kind in ("pose_refit", "pose_robust"):
            mv["b"] = int(POSES[int(rng.choice(4, p=[0.35, 0.35, 0.2, 0.1]))])
            if after_big and rng.random() < 0.7:
                mv["b"] = int(POSES[int(rng.integers(0, 2))])
            mv["rounds"] = int(rng.choice([1, 2, 3]))
            mv["null_start"] = bool(rng.random() < 0.5)               # (b == 1 only: poses_in is NULL)
            mv["start_scale"] = float(rng.choice([0.0, 1.5]))
        mv.update(fixed)
        if mv.get("b", 0) == 257:
            mv["rounds"] = 1                                          # (the references loop over the poses in Python)
        if mv.get("b", 1) > 1:
            mv["null_start"] = False
        mv["big"] = mv["m"] >= 1024 or mv.get("b", 0) >= 70 or mv.get("h", 0) >= 1000
        return mv
    if kind in ("voxel_select", "outlier_statistical", "outlier_radius"):
        mv["form"] = str(rng.choice(["rows", "mask", "whole"]))
    if kind in ("voxel_select", "outlier_statistical", "outlier_radius", "evaluate", "estimate_normals"):
        mv["rows"] = _size(rng, ROWS, after_big, 3)
        mv["rows_road"] = int(rng.integers(0, 2))
    if kind in ("voxel_select", "outlier_statistical", "outlier_radius", "fpfh", "keypoints", "estimate_normals", "upload"):
        mv["slot"] = int(rng.integers(0, 2))
    if kind == "evaluate":
        mv["with_rows"], mv["with_H"] = bool(rng.random() < 0.5), bool(rng.random() < 0.5)
    if kind in ("voxel_select", "outlier_statistical", "outlier_radius", "fpfh", "keypoints"):
        mv["out_road"] = int(rng.integers(0, 2))
        mv["in_road"] = int(rng.integers(0, 2))
    mv.update(fixed)
    mv["big"] = mv.get("rows", 0) is None or mv.get("form") == "whole" or kind in ("fpfh", "keypoints")
    return mv


def uses(mv):
    """{staging buffer: HOST / DEVICE} of a move over matched rows: the road of the array that would pass through each."""
    out = {}
    for buf, by_kind in STAGED.items():
        name = by_kind.get(mv["kind"])
        if name is not None and not (name == "poses_in" and mv.get("null_start")):
            out[buf] = mv["roads"][name]
    return out


def _euler_tour(n):
    """A closed walk over the complete directed graph on n nodes, loops included, that takes every edge once (Hierholzer)."""
    nxt = [list(range(n - 1, -1, -1)) for _ in range(n)]
    stack, walk = [0], []
    while stack:
        v = stack[-1]
        if nxt[v]:
            stack.append(nxt[v].pop())
        else:
            walk.append(stack.pop())
    return walk[::-1]


def tour():
    """The deterministic tour: every ordered pair (A, then B) of kinds is adjacent at least once; then moves over matched rows whose
    arrays alternate between all on the host and all on the device, so that every shared staging buffer sees both transitions."""
    rng = np.random.default_rng(20_000)
    kinds = [KINDS[i] for i in _euler_tour(len(KINDS))]
    moves, big, seen = [], False, dict.fromkeys(KINDS, 0)
    lists = {"m": M_ROWS, "nt": TARGETS, "h": TRIPLES, "b": POSES, "rows": ROWS, "form": ("rows", "mask", "whole"),
             "with_rows": (False, True, False, True), "with_H": (False, False, True, True)}
    for i, kind in enumerate(kinds):
        # every third move of a kind takes the next entry of each of its lists: no size or form is left to chance
        j, fixed = seen[kind], {}
        seen[kind] += 1
        if j % 3 == 0:
            fixed = {key: values[(j // 3) % len(values)] for key, values in lists.items() if key in plan_move(kind, np.random.default_rng(0))}
        if kind == "upload" and i + 1 < len(kinds) and kinds[i + 1] in NEEDS_SETUP:
            fixed["slot"] = 1                                         # (an upload to the fixed slot ends the setup: a setup would come between)
        moves.append(plan_move(kind, rng, big, **fixed))
        big = moves[-1]["big"]
    for i, (kind, road) in enumerate((("pose_refit", HOST), ("pose_robust", DEVICE), ("pose_refit", DEVICE), ("pose_robust", HOST),
                                      ("pose_refit", HOST), ("ransac_triplets", DEVICE), ("match_consistency", DEVICE),
                                      ("feature_match", HOST), ("match_consistency", HOST), ("ransac_triplets", HOST))):
        moves.append(plan_move(kind, rng, i % 3 == 0, roads=dict.fromkeys(ARRAYS[kind], road), b=5, null_start=False))
    return moves


# the openings aimed at one sharing each (the issue's list); a seed's opening is OPENINGS[seed % 8] where there is one
def _opening(which, rng):
    P = lambda kind, **kw: plan_move(kind, rng, False, **kw)          # noqa: E731
    host = lambda kind: dict.fromkeys(ARRAYS[kind], HOST)             # noqa: E731
    if which == 0:      # degrees, then inlier counts through gl_idx
        return [P("match_consistency", m=M_SCRIPTED, roads=host("match_consistency")),
                P("pose_refit", m=300, b=5, null_start=False, roads=host("pose_refit"))]
    if which == 1:      # the chain's three, alternating roads
        return [P("feature_match", roads=dict.fromkeys(ARRAYS["feature_match"], HOST)),
                P("ransac_triplets", roads=dict.fromkeys(ARRAYS["ransac_triplets"], DEVICE)),
                P("pose_robust", b=5, null_start=False, roads=host("pose_robust")),
                P("feature_match", roads=dict.fromkeys(ARRAYS["feature_match"], DEVICE)),
                P("ransac_triplets", roads=host("ransac_triplets")),
                P("pose_robust", b=5, null_start=False, roads=dict.fromkeys(ARRAYS["pose_robust"], DEVICE))]
    if which == 2:      # word 5 counts a mask, word 3 is preset, then the sweeps' words (more rows than the one-launch peel takes)
        return [P("outlier_radius", form="mask"), P("pose_refit", b=5, null_start=False), P("match_consistency", m=M_SCRIPTED),
                P("outlier_radius", form="mask"), P("pose_robust", b=1), P("match_consistency", m=65)]
    if which == 3:      # the run's slots and bounds against the stand-alone search's
        return [P("upload", slot=0, n=2000), P("upload", slot=1, n=2000), P("icp_setup"), P("icp_run"), P("keypoints", slot=1), P("fpfh", slot=1), P("icp_iterate"), P("icp_setup", same_size=True),
                P("evaluate"), P("operators"), P("icp_run")]
    if which == 4:      # an upload between two calls that use the normal cache
        return [P("icp_setup"), P("normal_angle"), P("estimate_normals", slot=1), P("upload", slot=1), P("normal_angle"),
                P("estimate_normals", slot=1), P("fpfh", slot=1), P("upload", slot=1), P("fpfh", slot=1), P("normal_angle")]
    return []


N_OPENINGS = 5


def random_moves(seed, steps=34):
    """The moves of a random seed: its opening, then `steps` kinds drawn evenly."""
    rng = np.random.default_rng(88_000 + seed)
    moves = _opening(seed % 8, rng)
    big = moves[-1]["big"] if moves else False
    while len(moves) < steps:
        moves.append(plan_move(KINDS[int(rng.integers(0, len(KINDS)))], rng, big))
        big = moves[-1]["big"]
    return moves


# ---- the model ------------------------------------------------------------------------------------------------------------------------
class Model(fuzz_sequence.Model):
    """fuzz_sequence's model of the clouds, the setup and the estimate, and one checked move per entry of the operators."""
    SIZES = (300, 777, 1500, 2000)        # (outlier_ref.radius holds every pair of points: 2 000 at the most)

    def __init__(self, ctx, mem, fresh, forced=None):
        """fresh(): a context like ctx that has done nothing; forced: {"sweeps": ctx, "one": ctx} for match_consistency."""
        super().__init__(ctx, None)
        self.mem, self.fresh, self.forced = mem, fresh, forced or {}
        self.nv2 = None                   # the movable cloud's normal columns
        self._inputs = []
        self._d2 = {}                     # slot -> every pair's squared distance (the radius filter's reference), by upload

    # ---- plumbing ----
    def cloud(self, slot):
        return self.F if slot == self.L.FIX else self.M

    def _in(self, name, a, road=HOST):
        """An input on its road; its bytes are remembered and looked at again after the call."""
        a = np.ascontiguousarray(a)
        x = self.mem.dev(a) if road == DEVICE else a.copy()
        self._inputs.append((name, x, a.dtype, a.tobytes()))
        return x

    def _out(self, shape, dtype, road=HOST):
        a = np.full(shape, 7 if np.dtype(dtype).kind == "u" else SENTINEL, dtype)    # (-7 as the own files have it; 7 where unsigned)
        return self.mem.dev(a) if road == DEVICE else a

    def _get(self, x, dtype, shape=None):
        a = self.mem.read(x, dtype)
        return a if shape is None else a.reshape(shape)

    def _intact(self, what):
        for name, x, dtype, before in self._inputs:
            if self.mem.read(x, dtype).tobytes() != before:
                self.bad.append(f"{what}: the input {name} was written to")
        self._inputs = []

    def _same(self, what, field, got, want):
        got, want = np.asarray(got), np.asarray(want)
        if got.shape != want.shape or got.tobytes() != want.tobytes():
            n = int(np.count_nonzero(got != want)) if got.shape == want.shape else -1
            self.bad.append(f"{what}: {field} differs from the reference in {n} entries of {want.size}")

    def _same_record(self, what, st, want, drop=()):
        got = _record(st)
        for key in drop:
            got.pop(key, None)
        if got != want:
            self.bad.append(f"{what}: the record is {got}, the reference's {want}")

    def _rows(self, rng, mv, n):
        r = mv["rows"]
        return None if r is None else rng.permutation(n)[:min(r, n)].astype(np.int64)

    # ---- matched rows ----
    def _matched(self, mv, rng):
        src, dst = matched_rows(rng, mv["m"])
        roads = mv["roads"]
        return src, dst, self._in("src", src, roads["src"]), self._in("dst", dst, roads["dst"])

    def feature_match(self, mv, rng):
        nq, nt, roads = mv["m"], mv["nt"], mv["roads"]
        q, t = rng.uniform(0, 100, (nq, 33)).astype(np.float32), rng.uniform(0, 100, (nt, 33)).astype(np.float32)
        if nq > 3:
            q[int(rng.integers(0, nq))] = np.nan                      # (a row without a finite distance: -1 / +inf)
        what = f"feature_match nq={nq} nt={nt} roads={roads}"
        self.log.append(what)
        Q, T = self._in("query", q, roads["query"]), self._in("target", t, roads["target"])
        idx, d2 = self._out(nq, np.int32, roads["idx"]), self._out(nq, np.float32, roads["d2"])
        p = self.mem.ptr
        st = self.ctx.feature_match(p(Q), p(T), nq=nq, nt=nt, dim=33, idx_ptr=p(idx), d2_ptr=p(d2))
        ridx, rd2, rec = global_ref.match(q, t)
        self._same(what, "idx", self._get(idx, np.int32), ridx)
        self._same(what, "d2", self._get(d2, np.uint32), _u32(rd2))
        self._same_record(what, st, rec)
        self._intact(what)

    def ransac_triplets(self, mv, rng):
        m, h, roads = mv["m"], mv["h"], mv["roads"]
        src, dst, S, D = self._matched(mv, rng)
        tri = rng.integers(0, m, (h, 3), dtype=np.int32)
        what = f"ransac_triplets m={m} h={h} roads={roads}"
        self.log.append(what)
        T = self._in("triples", tri, roads["triples"])
        poses, inl = self._out((h, 12), np.float64, roads["poses"]), self._out(h, np.int32, roads["inliers"])
        p = self.mem.ptr
        st = self.ctx.ransac_triplets(p(S), p(D), p(T), 0.02, 0.9, m=m, h=h, poses_ptr=p(poses), inliers_ptr=p(inl))
        rP, rinl, rec = global_ref.ransac(src, dst, tri, 0.02, 0.9)
        self._same(what, "inliers", self._get(inl, np.int32), rinl)
        self._same(what, "poses", self._get(poses, np.uint64, (h, 12)), _u64(rP))
        self._same_record(what, st, rec)
        self._intact(what)

    def _pose_call(self, mv, rng):
        b = mv["b"]
        src, dst, S, D = self._matched(mv, rng)
        start = None if mv["null_start"] else start_poses(rng, b)
        roads = mv["roads"]
        Pin = None if start is None else self._in("poses_in", start, roads["poses_in"])
        return src, dst, start, S, D, Pin, self._out((b, 12), np.float64, roads["poses"]), self._out(b, np.int32, roads["inliers"])

    def pose_refit(self, mv, rng):
        m, b, rounds = mv["m"], mv["b"], mv["rounds"]
        src, dst, start, S, D, Pin, poses, inl = self._pose_call(mv, rng)
        what = f"pose_refit m={m} b={b} rounds={rounds} start={'NULL' if start is None else 'poses'} roads={mv['roads']}"
        self.log.append(what)
        p = self.mem.ptr
        st = self.ctx.pose_refit(p(S), p(D), p(Pin), 0.05, rounds, m=m, b=b, poses_ptr=p(poses), inliers_ptr=p(inl))
        rP, rinl, rec = posefit_ref.refit(src, dst, start, 0.05, rounds)
        self._same(what, "inliers", self._get(inl, np.int32), rinl)
        self._same(what, "poses", self._get(poses, np.uint64, (b, 12)), _u64(rP))
        self._same_record(what, st, rec)
        self._intact(what)

    def pose_robust(self, mv, rng):
        m, b, rounds, s0 = mv["m"], mv["b"], mv["rounds"], mv["start_scale"]
        src, dst, start, S, D, Pin, poses, inl = self._pose_call(mv, rng)
        scales = self._out(b, np.float64, mv["roads"]["scales"])
        what = f"pose_robust m={m} b={b} rounds={rounds} start={'NULL' if start is None else 'poses'} scale={s0} roads={mv['roads']}"
        self.log.append(what)
        p = self.mem.ptr
        st = self.ctx.pose_robust(p(S), p(D), p(Pin), 0.01, rounds, 1.4, s0, m=m, b=b, poses_ptr=p(poses), inliers_ptr=p(inl),
                                  scales_ptr=p(scales))
        rP, rinl, rscales, rec = robust_ref.robust(src, dst, start, 0.01, rounds, 1.4, s0)
        self._same(what, "inliers", self._get(inl, np.int32), rinl)
        self._same(what, "poses", self._get(poses, np.uint64, (b, 12)), _u64(rP))
        self._same(what, "scales", self._get(scales, np.uint64), _u64(rscales))
        self._same_record(what, st, rec)
        self._intact(what)

    def match_consistency(self, mv, rng):
        m, roads = mv["m"], mv["roads"]
        src, dst = matched_rows(rng, m)
        want = consistency_ref.consistency(src, dst, 0.01, 0.1)
        base = f"match_consistency m={m} roads={roads}"
        self.log.append(base)
        for path, ctx in [("default", self.ctx)] + sorted(self.forced.items()):
            what = base if path == "default" else f"{base} (path {path})"
            S, D = self._in("src", src, roads["src"]), self._in("dst", dst, roads["dst"])
            degree, core = self._out(m, np.int32, roads["degree"]), self._out(m, np.int32, roads["core"])
            p = self.mem.ptr
            st = ctx.match_consistency(p(S), p(D), 0.01, 0.1, m=m, degree_ptr=p(degree), core_ptr=p(core))
            self._same(what, "degree", self._get(degree, np.int32), want[0])
            self._same(what, "core", self._get(core, np.int32), want[1])
            self._same_record(what, st, want[2], drop=("n_subrounds",))
            self._intact(what)

    # ---- slots ----
    def _candidates(self, mv, rng, n):
        """(rows, mask as it travels, mask as the reference takes it) of a call that takes rows, a device mask or the whole slot."""
        if mv["form"] == "rows":
            rows = self._rows(rng, mv, n)
            return (rows if rows is not None else np.arange(n, dtype=np.int64)), None, None
        if mv["form"] == "mask":
            mask = (rng.random(n) < 0.4).astype(np.uint8)
            mask[int(rng.integers(0, n))] = 1
            return None, self._in("mask", mask, DEVICE), mask
        return None, None, None

    def voxel_select(self, mv, rng):
        slot, X = mv["slot"], self.cloud(mv["slot"])
        n, c = len(X), float(rng.choice([0.3, 1.0]))
        origin = None if rng.random() < 0.5 else (0.1, -0.2, 0.05)
        rows, M, mask = self._candidates(mv, rng, n)
        what = f"voxel_select {mv['form']} slot={slot} n={n} c={c} rows={None if rows is None else len(rows)} out={mv['out_road']}"
        self.log.append(what)
        want = voxel_ref.keep(X, c, (0.0, 0.0, 0.0) if origin is None else origin, rows=rows, mask=mask)
        p = self.mem.ptr
        if mask is not None:
            out = self._out(n, np.uint8, DEVICE)
            kept = self.ctx.voxel_select_masked(slot, p(M), n, c, origin, keep_ptr=p(out))
            got = self._get(out, np.uint8)
        elif mv["out_road"] == DEVICE:
            out = self._out(len(want), np.uint8, DEVICE)
            kept = self.ctx.voxel_select(slot, c, origin, rows, keep_ptr=p(out))
            got = self._get(out, np.uint8)
        else:
            got = self.ctx.voxel_select(slot, c, origin, rows).view(np.uint8)
            kept = int(got.sum())
        self._same(what, "keep", got, want.view(np.uint8))
        if kept != int(want.sum()):
            self.bad.append(f"{what}: {kept} kept, the reference keeps {int(want.sum())}")
        self._intact(what)

    def outlier_statistical(self, mv, rng):
        slot, X = mv["slot"], self.cloud(mv["slot"])
        n, k = len(X), int(rng.choice([4, 8]))
        rows, M, mask = self._candidates(mv, rng, n)
        what = f"outlier_statistical {mv['form']} slot={slot} n={n} k={k} rows={None if rows is None else len(rows)} out={mv['out_road']}"
        self.log.append(what)
        ref = outlier_ref.statistical(X, k, 1.0, rows=rows, mask=mask)
        N, p = len(ref["keep"]), self.mem.ptr
        if mv["out_road"] == DEVICE:
            keep, d = self._out(N, np.uint8, DEVICE), self._out(N, np.float64, DEVICE)
            st = self.ctx.outlier_statistical(slot, k, 1.0, rows=rows, mask_ptr=p(M), keep_ptr=p(keep), mean_ptr=p(d))
            keep, d = self._get(keep, np.uint8), self._get(d, np.float64)
        else:
            keep, d, st = self.ctx.outlier_statistical(slot, k, 1.0, rows=rows, mask_ptr=p(M))
        self._same(what, "d", _u64(d), _u64(ref["d"]))
        self._same(what, "keep", np.asarray(keep).view(np.uint8), ref["keep"].view(np.uint8))
        got = _record(st)
        if (got["n_candidates"], got["n_kept"]) != (ref["n_candidates"], ref["n_kept"]) or \
                any(_u64([got[key]])[0] != _u64([ref[key]])[0] for key in ("mean", "std", "threshold")):
            self.bad.append(f"{what}: the record is {got}, the reference's {({key: ref[key] for key in got})}")
        self._intact(what)

    def outlier_radius(self, mv, rng):
        slot, X = mv["slot"], self.cloud(mv["slot"])
        n, r = len(X), float(rng.choice([0.3, 0.6]))
        rows, M, mask = self._candidates(mv, rng, n)
        what = f"outlier_radius {mv['form']} slot={slot} n={n} r={r} rows={None if rows is None else len(rows)} out={mv['out_road']}"
        self.log.append(what)
        if slot not in self._d2:
            self._d2[slot] = outlier_ref.all_d2(X)
        ref = outlier_ref.radius(X, r, 4, rows=rows, mask=mask, D2=self._d2[slot])
        N, p = len(ref["keep"]), self.mem.ptr
        if mv["out_road"] == DEVICE:
            keep, cnt = self._out(N, np.uint8, DEVICE), self._out(N, np.uint32, DEVICE)
            kept = self.ctx.outlier_radius(slot, r, 4, rows=rows, mask_ptr=p(M), keep_ptr=p(keep), count_ptr=p(cnt))
            keep, cnt = self._get(keep, np.uint8), self._get(cnt, np.uint32)
        else:
            keep, cnt, kept = self.ctx.outlier_radius(slot, r, 4, rows=rows, mask_ptr=p(M))
        self._same(what, "count", np.asarray(cnt).view(np.uint32), ref["count"])
        self._same(what, "keep", np.asarray(keep).view(np.uint8), ref["keep"].view(np.uint8))
        if kept != ref["n_kept"]:
            self.bad.append(f"{what}: {kept} kept, the reference keeps {ref['n_kept']}")
        self._intact(what)

    def evaluate(self, mv, rng):
        L = self.L
        qs, ss = (L.FIX, L.MOV) if rng.random() < 0.7 else (L.MOV, L.FIX)
        Xq, Xs = self.cloud(qs), self.cloud(ss)
        H = _small_H(rng) if mv["with_H"] else None
        d = float(rng.choice([np.inf, 0.3]))
        rows = self._rows(rng, mv, len(Xq)) if mv["with_rows"] else None
        what = f"evaluate query={'FIX' if qs == L.FIX else 'MOV'} rows={None if rows is None else len(rows)}/{mv['rows_road']} " \
               f"H={'yes' if H is not None else 'no'} d={d}"
        self.log.append(what)
        R = None if rows is None else self._in("rows", rows, mv["rows_road"])
        rec = self.ctx.evaluate(qs, ss, H, d, R)
        want = eval_ref.evaluate(Xq, Xs, H, d, rows=rows)
        sums = np.array([rec.sum_d2, *rec.sum_p, *rec.sum_pp], dtype=np.float64)
        if (rec.n_queries, rec.n_inliers) != (want["n_queries"], want["n_inliers"]):
            self.bad.append(f"{what}: {rec.n_queries} queries and {rec.n_inliers} inliers, the reference has {want['n_queries']} and "
                            f"{want['n_inliers']}")
        self._same(what, "sums", _u64(sums), _u64(want["sums"]))
        self._intact(what)

    def fpfh(self, mv, rng):
        slot, X = mv["slot"], self.cloud(mv["slot"])
        n, k = len(X), int(rng.choice([8, 12]))
        radius = float(rng.choice([np.inf, 0.8]))
        viewpoint = None if rng.random() < 0.5 else (0.0, 0.0, 10.0)
        N = rng.standard_normal((n, 3))
        N = (N / np.linalg.norm(N, axis=1, keepdims=True)).astype(np.float32)
        N[int(rng.integers(0, n))] = np.nan
        what = f"fpfh slot={slot} n={n} k={k} radius={radius} normals={mv['in_road']} out={mv['out_road']}"
        self.log.append(what)
        Nd = self._in("normals", N, mv["in_road"])
        ref = fpfh_ref.fpfh(X, N, k, radius, viewpoint)
        p = self.mem.ptr
        if mv["out_road"] == DEVICE:
            F, cnt = self._out((n, 33), np.float32, DEVICE), self._out((n, 34), np.uint16, DEVICE)
            st = self.ctx.fpfh(slot, Nd, k, radius, viewpoint, fpfh_ptr=p(F), counts_ptr=p(cnt))
            F, cnt = self._get(F, np.float32, (n, 33)), self._get(cnt, np.uint16, (n, 34))
        else:
            F, cnt, st = self.ctx.fpfh(slot, Nd, k, radius, viewpoint, want_counts=True)
        self._same(what, "counts", cnt, ref["counts"])
        self._same(what, "fpfh", _u32(F), _u32(ref["fpfh"]))
        self._same_record(what, st, {key: ref[key] for key in ("n_points", "n_pairs", "n_void_pairs", "n_empty")})
        self._intact(what)

    def keypoints(self, mv, rng):
        slot, X = mv["slot"], self.cloud(mv["slot"])
        n, k_s = len(X), int(rng.choice([8, 12]))
        k_n = None if rng.random() < 0.5 else 6
        r_s = float(rng.choice([np.inf, 1.0]))
        what = f"keypoints slot={slot} n={n} k_s={k_s} k_n={k_n} r_s={r_s} out={mv['out_road']}"
        self.log.append(what)
        ref = iss_ref.keypoints(X, k_s, r_s, k_n, np.inf, 0.975, 0.975, 5)
        p = self.mem.ptr
        if mv["out_road"] == DEVICE:
            keep, sal, eig = self._out(n, np.uint8, DEVICE), self._out(n, np.float64, DEVICE), self._out((n, 3), np.float64, DEVICE)
            st = self.ctx.keypoints(slot, k_s, r_s, k_n, np.inf, 0.975, 0.975, 5, keep_ptr=p(keep), saliency_ptr=p(sal), eig_ptr=p(eig))
            keep, sal, eig = self._get(keep, np.uint8), self._get(sal, np.float64), self._get(eig, np.float64, (n, 3))
        else:
            keep, sal, eig, st = self.ctx.keypoints(slot, k_s, r_s, k_n, np.inf, 0.975, 0.975, 5, want_saliency=True)
        self._same(what, "eig", _u64(eig), _u64(ref["eig"]))
        self._same(what, "saliency", _u64(sal), _u64(ref["saliency"]))
        self._same(what, "keep", np.asarray(keep).view(np.uint8), ref["keep"].view(np.uint8))
        self._same_record(what, st, {key: ref[key] for key in iss_ref.KEYS})

    def estimate_normals(self, mv, rng):
        slot, X = mv["slot"], self.cloud(mv["slot"])
        k = int(rng.choice([8, 10]))
        rows = self._rows(rng, mv, len(X))
        rows = np.arange(len(X), dtype=np.int64) if rows is None else rows
        what = f"estimate_normals slot={slot} n={len(X)} rows={len(rows)} k={k}"
        self.log.append(what)
        sel = self._in("rows", rows)
        nv, pl, nn = self.ctx.estimate_normals(slot, sel, k, want_nn=True)
        rnn, _ = orc.knn(X, X[rows], k=k)
        self._same(what, "neighbours", nn, rnn)
        rnv, rpl = orc.normals(X, rnn)
        # (one float32 ulp for the float64 sqrt and division: tests/test_gpu_kernels.py, tests/test_gpu_c3shape.py)
        if not (np.abs(nv - rnv).max() <= 2e-7 and np.abs(pl - rpl).max() <= 2e-6):
            self.bad.append(f"{what}: normals off by {np.abs(nv - rnv).max():.2e}, planarity by {np.abs(pl - rpl).max():.2e}")
        with self.fresh() as clean:
            clean.upload(slot, X)
            cnv, cpl, cnn = clean.estimate_normals(slot, rows, k, want_nn=True)
        self._same(what, "normals against a fresh context", _u32(nv), _u32(cnv))
        self._same(what, "planarity against a fresh context", _u32(pl), _u32(cpl))
        self._intact(what)

    def normal_angle(self, mv, rng):
        """corr_match, then the rejection by the angle between normals over its correspondences: the normals from the movable
        cloud's columns where it has some, else estimated on the device (the cache), or handed over per correspondence."""
        sel, nv, pl = self.setup
        k = 10
        H = orc.params_to_H(self.x)
        cos_max = float(np.cos(np.radians(35.0)))
        per_q = self.nv2 is None and rng.random() < 0.3
        what = f"normal_angle ({'per correspondence' if per_q else 'columns' if self.nv2 is not None else 'cache'})"
        self.log.append(what)
        idx, _ = self.ctx.corr_match(H)
        nn = orc.knn(self.M, self.F[sel], k=1, H=H)[0][:, 0]
        if not np.array_equal(idx, nn):
            self.bad.append(f"{what}: corr_match: {int(np.count_nonzero(idx != nn))} indices differ")
            return
        n2 = self.nv2[nn] if self.nv2 is not None else normal_angle_ref.movable_normals(self.M, nn, k)
        n_alive = self.ctx.corr_reject_normal_angle(cos_max, k, H, n2 if per_q else None)
        c = normal_angle_ref.cos_of(nv, n2, H)
        want = normal_angle_ref.verdict(nv, n2, H, cos_max)
        sure = ~(np.abs(np.abs(c) - cos_max) < 1e-12)                 # (the reference has no fused operations: a verdict that hangs
        alive = self.ctx.icp_state(pc2_idx=False, dist=False, residual=False)[2]   # on the last bit of c is nobody's to call)
        if not np.array_equal(alive[sure], want[sure]) or (sure.all() and n_alive != int(want.sum())):
            self.bad.append(f"{what}: {int(np.count_nonzero(alive[sure] != want[sure]))} verdicts differ, {n_alive} alive of {int(want.sum())}")

    def set_normals(self, mv, rng):
        if rng.random() < 0.3:
            self.nv2 = None
            self.ctx.set_normals(self.L.MOV, None)
        else:
            nn, _ = orc.knn(self.M, self.M, k=10)
            self.nv2 = orc.normals(self.M, nn)[0].copy()
            self.nv2[rng.random(len(self.M)) < 0.1] = np.nan
            self.ctx.set_normals(self.L.MOV, self.nv2)
        self.log.append(f"set_normals {'none' if self.nv2 is None else 'columns'}")

    # ---- fuzz_sequence's moves, as a move ----
    def upload(self, slot):
        super().upload(slot)
        self._d2.pop(slot, None)
        if slot == self.L.MOV:
            self.nv2 = None

    def transform(self):
        super().transform()
        self._d2.pop(self.L.MOV, None)

    def same_size_setup(self):
        """A new setup of the size of the one before, on other points: what lets stale slots pass for current ones."""
        sel = np.sort(self.rng.choice(len(self.F), len(self.setup[0]), replace=False))
        nv, pl = self.ctx.estimate_normals(self.L.FIX, sel, 10)
        self.ctx.icp_setup(sel, nv, pl)
        self.setup, self.x = (sel, nv, pl), np.zeros(6)
        self.log.append(f"icp_setup Q={len(sel)} (same size, other points)")

    def apply(self, mv):
        """One move.  Everything it draws comes from its own seed."""
        kind = mv["kind"]
        rng = self.rng = np.random.default_rng(mv["seed"])
        if kind in NEEDS_SETUP and self.setup is None:
            self.icp_setup()
        if kind in MATCHED or kind in SLOTS[:7] or kind in ("normal_angle", "set_normals"):
            getattr(self, kind)(mv, rng)
        elif kind == "upload":
            if "n" in mv:
                self.SIZES = (mv["n"],)                              # (this upload's size is the move's, not a draw)
            self.upload(self.L.FIX if mv["slot"] == 0 else self.L.MOV)
            self.__dict__.pop("SIZES", None)
        elif kind == "icp_setup" and mv.get("same_size") and self.setup is not None:
            self.same_size_setup()
        else:
            getattr(self, kind)()
        if kind in ("knn", "icp_iterate", "icp_run", "operators", "normal_angle", "select_in_range", "evaluate"):
            self.kernels.add(self.ctx.last_match_kernel())


def replay(moves, ctx, mem, fresh, forced=None, seed=0):
    """The moves on ctx, after an upload to either slot.  Returns (problems, log, kernels seen, the index of the move that failed or
    None).  Empty problems: every call agreed with its reference."""
    m = Model(ctx, mem, fresh, forced)
    m.rng = np.random.default_rng(99_000 + seed)
    m.upload(m.L.FIX)
    m.upload(m.L.MOV)
    for step, mv in enumerate(moves):
        m.apply(mv)
        mem.sync()
        if m.bad:
            return m.bad, m.log, m.kernels, step
    return m.bad, m.log, m.kernels, None


# ---- on the real library --------------------------------------------------------------------------------------------------------------
def library_context(flavour="near", **more):
    """A _lib.Context created under ENV (the thresholds are read at sicp_ctx_create)."""
    from simpleicp_amd import _lib
    env = dict(ENV, SICP_NN16=flavour, **more)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return _lib.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def run_on_library(moves, seed=0):
    """The moves on a fresh context of the real library, match_consistency also on a context forced to either peeling path."""
    flavour = "far" if seed % 2 else "near"
    ctx = library_context(flavour)
    forced = {}
    try:
        if any(mv["kind"] == "match_consistency" for mv in moves):
            forced = {path: library_context(flavour, SICP_CONSISTENCY=path) for path in ("sweeps", "one")}
        return replay(moves, ctx, TorchMemory(), lambda: library_context(flavour), forced, seed)
    finally:
        for c in [ctx] + list(forced.values()):
            c.close()
