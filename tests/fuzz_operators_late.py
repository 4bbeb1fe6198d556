"""A second ring of call sequences beside tests/fuzz_operators.py, for the five entries that came after it -- sicp_cluster,
sicp_plane_triplets, sicp_plane_refit, sicp_farthest, sicp_orient -- and what they share with the older ones: the counter words of
c->cand_small (word 2 is POSE_BEST1 for the pose and plane operators, the bits of a double for farthest, CL_NOISE, OR_COMPONENTS;
word 3 is POSE_BEST behind a preset of all ones, CL_CLUSTERS, OR_FLIPPED; word 4 is OL_KEPT, CL_BEST, OR_VOTED), the staging buffers
gl_src / gl_tri / gl_pose / gl_idx / pf_in that the plane and the pose operators use with different strides, cand_keep and ol_cnt
that cluster takes from the candidate intake and the radius filter, and the k-NN buffers that orient reads behind rows_knn.

fuzz_operators.KINDS, tour() and random_moves() stay what they are: the first ring takes every ordered pair of the old kinds.  Here
late_tour() takes every ordered pair in which at least one kind is a late one, and late_random_moves() draws from all of them.  A
move of a late kind is a dict from the seed alone, like the old ones; Model adds one checked move per late entry, each compared as
that entry's own GPU test file compares it: bit for bit, every record field, outputs prefilled, inputs looked at again."""
import numpy as np

import cluster_ref
import farthest_ref
import fuzz_operators as fo
import orient_ref
import plane_ref
from fuzz_operators import DEVICE, HOST, _u64

LATE = ("cluster", "plane_triplets", "plane_refit", "farthest", "orient")
KINDS_ALL = fo.KINDS + LATE

RADII = (0.3, 0.6)                                    # the radius filter's, on the same clouds
MIN_POINTS = (4, 8)
PLANE_ROWS = (3, 64, 65, 1025, 2000)                  # the least, a wave, past a workgroup's span, the model's largest
REFIT_PLANES = (1, 5, 70)
FAR_ROWS = (1, 64, 65, 300, 1025, 2000)
COUNTS = (1, 64, None, 257)                           # None: as many as there are rows; a count above n is n
ORIENT_K = (2, 8, 17, 33)
MASKS = ("none", "host", "device")
REFERENCES = ("none", "towards", "away")

ARRAYS = dict(fo.ARRAYS, cluster=("labels", "core"), plane_triplets=("X", "mask", "triples", "planes", "inliers"),
              plane_refit=("X", "mask", "planes_in", "planes", "inliers", "keep"), farthest=("X", "mask", "idx", "d2"),
              orient=("normals", "normals_out", "flipped"))
# which array of which kind passes through which shared staging buffer when it is host memory (the stage_in / stage_out calls of
# sicp_plane.hip and sicp_farthest.hip beside the older operators')
STAGED = {"gl_idx": dict(fo.STAGED["gl_idx"], plane_triplets="inliers", plane_refit="inliers"),
          "gl_src": dict(fo.STAGED["gl_src"], plane_triplets="X", plane_refit="X", farthest="X"),
          "gl_dst": dict(fo.STAGED["gl_dst"]),
          "gl_tri": {"ransac_triplets": "triples", "plane_triplets": "triples"},
          "gl_pose": dict(fo.STAGED["gl_pose"], plane_triplets="planes", plane_refit="planes"),
          "pf_in": dict(fo.STAGED["pf_in"], plane_refit="planes_in")}
SHARED = ("gl_src", "gl_tri", "gl_pose", "gl_idx", "pf_in")

# the late entries' switches: orient's lists cross chunk boundaries and the plane scores take several spans at these sizes
ENV_LATE = {"SICP_ORIENT_CHUNK": "64", "SICP_PLANE_SPAN": "128"}
ENV_STEPPED = {"SICP_FARTHEST_ONE_MAX": "0", "SICP_FARTHEST_SPAN": "128"}

# the seam lists of a late kind: every third move of the kind in the tour takes the next entry of each
LISTS = {"cluster": {"slot": (0, 1, 1), "radius": RADII, "min_points": (4, 4, 8, 8), "null_core": (False, True, False)},
         "plane_triplets": {"n": PLANE_ROWS, "h": fo.TRIPLES, "mask": MASKS, "scene": ("plane", "uniform"), "null_planes": (False, False, True)},
         "plane_refit": {"n": PLANE_ROWS[::-1], "b": REFIT_PLANES, "rounds": (1, 2, 3), "mask": MASKS[::-1], "keep": (False, True)},
         "farthest": {"n": FAR_ROWS, "count": COUNTS, "mask": MASKS, "start": ("lowest", "row"), "null_d2": (False, True, False)},
         "orient": {"slot": (0, 1, 1), "k": ORIENT_K, "reference": REFERENCES, "alias": (False, True, False, False, False),
                    "null_flipped": (False, False, True)}}
OLD_LISTS = {"m": fo.M_ROWS, "nt": fo.TARGETS, "h": fo.TRIPLES, "b": fo.POSES, "rows": fo.ROWS, "form": ("rows", "mask", "whole"),
             "with_rows": (False, True, False, True), "with_H": (False, False, True, True)}


# ---- the moves' arguments, from the seed alone ----------------------------------------------------------------------------------------
def plan_move(kind, rng, after_big=False, **fixed):
    """One move of any kind; an old kind is fuzz_operators.plan_move's.  A late kind: sizes, variants and roads drawn from rng,
    `fixed` laid over them.  move["roads"] holds the arrays that are there: an output that is NULL and a mask that is none are not."""
    if kind not in LATE:
        return fo.plan_move(kind, rng, after_big, **fixed)
    pick = lambda values: values[int(rng.integers(0, len(values)))]   # noqa: E731
    coin = lambda p: bool(rng.random() < p)                           # noqa: E731
    mv = {"kind": kind, "seed": int(rng.integers(1 << 31))}
    mv["roads"] = {a: int(rng.integers(0, 2)) for a in ARRAYS[kind]}
    if kind == "cluster":
        mv.update(slot=int(rng.integers(0, 2)), radius=float(pick(RADII)), min_points=int(pick(MIN_POINTS)), null_core=coin(0.3))
    elif kind == "plane_triplets":
        mv.update(n=int(fo._size(rng, PLANE_ROWS, after_big, 3)), h=int(fo._size(rng, fo.TRIPLES, after_big)), mask=pick(MASKS),
                  scene=pick(("plane", "uniform")), null_planes=coin(0.3), all_void=False)
    elif kind == "plane_refit":
        mv.update(n=int(fo._size(rng, PLANE_ROWS, after_big, 3)), b=int(fo._size(rng, REFIT_PLANES, after_big)), rounds=int(pick((1, 2, 3))),
                  mask=pick(MASKS), scene=pick(("plane", "uniform")), keep=coin(0.5))
    elif kind == "farthest":
        mv.update(n=int(fo._size(rng, FAR_ROWS, after_big, 3)), count=pick(COUNTS), mask=pick(MASKS), start=pick(("lowest", "row")),
                  null_d2=coin(0.3))
    elif kind == "orient":
        mv.update(slot=int(rng.integers(0, 2)), k=int(pick(ORIENT_K)), reference=pick(REFERENCES), alias=coin(0.25), null_flipped=coin(0.3))
    mv.update(fixed)
    roads = mv["roads"] = dict(mv["roads"])
    if "mask" in ARRAYS[kind]:
        if mv["mask"] == "none":
            roads.pop("mask", None)
        else:
            roads["mask"] = HOST if mv["mask"] == "host" else DEVICE
    if kind == "plane_refit":
        mv["keep"] = bool(mv["keep"] and mv["b"] == 1)                # (keep_out requires b == 1: contract (Q))
    if kind == "farthest":
        mv["count"] = mv["n"] if mv["count"] is None else min(int(mv["count"]), mv["n"])
    for flag, name in (("null_core", "core"), ("null_planes", "planes"), ("null_d2", "d2"), ("null_flipped", "flipped")):
        if mv.get(flag):
            roads.pop(name, None)
    if kind == "plane_refit" and not mv["keep"]:
        roads.pop("keep", None)
    if kind == "orient" and mv["alias"]:
        roads["normals_out"] = roads["normals"]                       # (the same array)
    mv["big"] = kind in ("cluster", "orient") or mv["n"] >= 1025 or mv.get("h", 0) >= 1000 or mv.get("b", 0) >= 70
    return mv


def uses(mv):
    """{staging buffer: HOST / DEVICE} of a move, old or late: the road of the array that would pass through each."""
    out = {}
    for buf, by_kind in STAGED.items():
        name = by_kind.get(mv["kind"])
        if name is not None and name in mv.get("roads", {}) and not (name == "poses_in" and mv.get("null_start")):
            out[buf] = mv["roads"][name]
    return out


def _late_euler_tour():
    """A closed walk over KINDS_ALL (as indices) that takes every ordered pair with a late kind in it exactly once, loops of the
    late kinds included: 28 * 28 - 23 * 23 edges.  In that edge set every node has as many edges in as out and every old node
    borders a late one, so Hierholzer's walk from a late node closes."""
    n, first = len(KINDS_ALL), len(fo.KINDS)
    nxt = [[w for w in range(n - 1, -1, -1) if v >= first or w >= first] for v in range(n)]
    stack, walk = [first], []
    while stack:
        v = stack[-1]
        if nxt[v]:
            stack.append(nxt[v].pop())
        else:
            walk.append(stack.pop())
    return walk[::-1]


def _all(kind, road):
    return dict.fromkeys(ARRAYS[kind], road)


def _roads(kind, turn):
    """The roads of a late move by turns: all host, all device, host and device array by array, device and host."""
    return {a: (HOST, DEVICE, i % 2, 1 - i % 2)[turn % 4] for i, a in enumerate(ARRAYS[kind])}


def late_tour():
    """The deterministic tour of the second ring: every ordered pair (A, then B) of kinds with a late one in it is adjacent exactly
    once; then three runs of an old and a late user of the shared staging buffers in turn, all arrays of a move on one road, the
    roads in an order that gives both (old, late) and (late, old) all four transitions."""
    rng = np.random.default_rng(21_000)
    kinds = [KINDS_ALL[i] for i in _late_euler_tour()]
    moves, big, seen = [], False, dict.fromkeys(KINDS_ALL, 0)
    for i, kind in enumerate(kinds):
        # every third move of a kind takes the next entry of each of its lists, a late kind the next pattern of roads too: no
        # size, form or road is left to chance
        j, fixed = seen[kind], {}
        seen[kind] += 1
        if j % 3 == 0 and kind in LATE:
            fixed = {key: values[(j // 3) % len(values)] for key, values in LISTS[kind].items()}
            fixed["roads"] = _roads(kind, j // 3)
        elif j % 3 == 0:
            fixed = {key: values[(j // 3) % len(values)] for key, values in OLD_LISTS.items() if key in fo.plan_move(kind, np.random.default_rng(0))}
        if kind == "upload" and i + 1 < len(kinds) and kinds[i + 1] in fo.NEEDS_SETUP:
            fixed["slot"] = 1                                         # (an upload to the fixed slot ends the setup: a setup would come between)
        moves.append(plan_move(kind, rng, big, **fixed))
        big = moves[-1]["big"]
    # roads of nine moves, old and late in turn: (old, late) sees HH HD DH DD, (late, old) HH DD HD DH
    turn = (HOST, HOST, HOST, DEVICE, DEVICE, HOST, DEVICE, DEVICE, HOST)
    for old, late in (("pose_refit", "plane_refit"), ("ransac_triplets", "plane_triplets"), ("pose_robust", "farthest")):
        for i, road in enumerate(turn):
            if i % 2 == 0:
                moves.append(plan_move(old, rng, i % 3 == 0, roads=_all(old, road), b=5, null_start=False))
                continue
            fixed = {"plane_refit": dict(b=5), "plane_triplets": dict(null_planes=False), "farthest": dict(null_d2=False)}[late]
            moves.append(plan_move(late, rng, i % 3 == 0, roads=_all(late, road), mask=("none", "device", "host", "device")[i // 2], **fixed))
    return moves


def _seed_where(first_draw, values):
    """A move's seed under which the model's first draw, rng.choice(values), is first_draw (fpfh's and estimate_normals' k)."""
    return next(s for s in range(1000) if np.random.default_rng(s).choice(values) == first_draw)


# the openings aimed at one sharing each; a seed's opening is LATE_OPENINGS[seed % 8] where there is one
def _late_opening(which, rng):
    P = lambda kind, **kw: plan_move(kind, rng, False, **kw)          # noqa: E731
    host = lambda kind: _all(kind, HOST)                              # noqa: E731
    if which == 0:      # gl_pose / gl_idx with 12 and 4 doubles a hypothesis
        return [P("pose_refit", b=70, null_start=False, roads=host("pose_refit")),
                P("plane_triplets", h=255, null_planes=False, roads=host("plane_triplets")),
                P("pose_refit", b=5, null_start=False, roads=host("pose_refit")),
                P("plane_refit", b=70, roads=host("plane_refit")),
                P("ransac_triplets", h=1, roads=host("ransac_triplets"))]
    if which == 1:      # gl_src: matched rows, farthest's rows, a plane's rows
        return [P("ransac_triplets", m=1100, roads=host("ransac_triplets")), P("farthest", n=300, roads=host("farthest")),
                P("plane_triplets", n=65, roads=host("plane_triplets")), P("pose_robust", m=63, b=5, null_start=False, roads=host("pose_robust")),
                P("farthest", n=2000, roads=host("farthest")), P("match_consistency", m=64, roads=host("match_consistency"))]
    if which == 2:      # words 2 and 3: a double's bits, POSE_BEST1 / POSE_BEST behind their preset, CL_CLUSTERS, OR_FLIPPED
        return [P("farthest", n=300, count=64), P("ransac_triplets"), P("cluster", radius=0.3, min_points=4),
                P("plane_triplets", h=255, all_void=True), P("pose_refit", b=5, null_start=False), P("orient"), P("plane_refit")]
    if which == 3:      # cand_keep / ol_cnt: the radius filter's, the candidate intake's, cluster's
        return [P("outlier_radius", form="mask", slot=0), P("cluster", slot=0), P("outlier_radius", form="rows", rows=1, slot=0),
                P("voxel_select", form="mask", slot=1), P("cluster", slot=1), P("outlier_statistical")]
    if which == 4:      # the k-NN buffers and the slot's freshness
        return [P("fpfh", slot=0, seed=_seed_where(12, [8, 12])), P("orient", slot=0, k=33),
                P("estimate_normals", slot=0, rows=64, seed=_seed_where(8, [8, 10])), P("orient", slot=0, k=2), P("upload", slot=0, n=250),
                P("orient", slot=0), P("transform"), P("orient", slot=1), P("keypoints", slot=1), P("cluster", slot=1)]
    if which == 5:      # behind a run
        return [P("upload", slot=0, n=2000), P("upload", slot=1, n=2000), P("icp_setup"), P("icp_run"), P("orient", slot=0), P("cluster", slot=1),
                P("icp_iterate"), P("farthest"), P("icp_run")]
    return []


N_LATE_OPENINGS = 6


def late_random_moves(seed, steps=34):
    """The moves of a random seed: its opening, then kinds drawn from all of them, half the weight on the late five."""
    rng = np.random.default_rng(188_000 + seed)
    moves = _late_opening(seed % 8, rng)
    big = moves[-1]["big"] if moves else False
    while len(moves) < steps:
        late = rng.random() < 0.5
        kind = LATE[int(rng.integers(0, len(LATE)))] if late else fo.KINDS[int(rng.integers(0, len(fo.KINDS)))]
        moves.append(plan_move(kind, rng, big))
        big = moves[-1]["big"]
    return moves


# ---- the references, computed once per input ------------------------------------------------------------------------------------------
_MEMO = {}


def memo(key, compute):
    """compute() under `key`; the last few results are kept (a stand-in context and the model ask for the same ones in turn)."""
    if key not in _MEMO:
        if len(_MEMO) >= 8:
            _MEMO.pop(next(iter(_MEMO)))
        _MEMO[key] = compute()
    return _MEMO[key]


def _bytes(a):
    return None if a is None else np.ascontiguousarray(a).tobytes()


def ref_cluster(X, radius, min_points, A=None):
    return memo(("cluster", _bytes(X), float(radius), int(min_points)), lambda: cluster_ref.cluster(X, radius, min_points, A=A))


def ref_triplets(X, mask, tri, md):
    return memo(("triplets", _bytes(X), _bytes(mask), _bytes(tri), float(md)), lambda: plane_ref.triplets(X, mask, tri, md))


def ref_refit(X, mask, planes, md, rounds, want_keep):
    return memo(("refit", _bytes(X), _bytes(mask), _bytes(planes), float(md), int(rounds), bool(want_keep)),
                lambda: plane_ref.refit(X, mask, planes, md, rounds, want_keep=want_keep))


def ref_farthest(X, mask, count, start):
    return memo(("farthest", _bytes(X), _bytes(mask), int(count), int(start)), lambda: farthest_ref.farthest(X, mask, count, start))


def ref_orient(X, N, k, reference, away, idx=None):
    kw = {} if reference is None else {"away_from": reference} if away else {"viewpoint": reference}
    return memo(("orient", _bytes(X), _bytes(N), int(k), _bytes(reference), bool(away), _bytes(idx)),
                lambda: orient_ref.orient(X, N, k, idx=idx, **kw))


def start_planes(rng, X, mask, md, b):
    """(b, 4): the best plane of sixteen triples of the reference, each copy a little off; where b allows, one that is not finite."""
    tri = rng.integers(0, len(X), (16, 3), dtype=np.int32)
    P, _, rec = plane_ref.triplets(X, mask, tri, md)
    base = P[rec["best"]] if rec["best"] >= 0 else np.array([0.0, 0.0, 1.0, 0.0])
    out = np.empty((b, 4))
    for k in range(b):
        nrm = base[:3] + rng.normal(0, 0.02, 3)
        out[k, :3], out[k, 3] = nrm / np.linalg.norm(nrm), base[3] + rng.normal(0, 0.01)
    if b >= 5:
        out[int(rng.integers(0, b)), int(rng.integers(0, 4))] = (np.nan, np.inf)[int(rng.integers(0, 2))]
    return out


# ---- the model ------------------------------------------------------------------------------------------------------------------------
class Model(fo.Model):
    """fuzz_operators' model, and one checked move per late entry."""

    def __init__(self, ctx, mem, fresh, stepped=None, one=None, notes=None):
        """stepped: a context forced to farthest's stepped path and to match_consistency's sweeps (None: the default context
        alone); one(): a context forced to match_consistency's one launch, opened for such a move and closed behind it; notes: a
        list that gets what the references saw, one dict per late move."""
        super().__init__(ctx, mem, fresh)
        self.stepped, self.one = stepped, one
        self.notes = [] if notes is None else notes
        self._rel = {}                    # (slot, radius) -> the dense neighbour relation (cluster's reference), by upload

    def upload(self, slot):
        super().upload(slot)
        self._rel = {key: A for key, A in self._rel.items() if key[0] != slot}

    def transform(self):
        super().transform()
        self._rel = {key: A for key, A in self._rel.items() if key[0] != self.L.MOV}

    def cluster(self, mv, rng):
        slot, X, roads = mv["slot"], self.cloud(mv["slot"]), mv["roads"]
        n, r, mp = len(X), mv["radius"], mv["min_points"]
        what = f"cluster slot={slot} n={n} r={r} min_points={mp} roads={roads}"
        self.log.append(what)
        if (slot, r) not in self._rel:
            self._rel[(slot, r)] = cluster_ref.relation(X, r)
        ref = ref_cluster(X, r, mp, self._rel[(slot, r)])
        self.notes.append(dict(kind="cluster", **cluster_ref.record(ref)))
        p = self.mem.ptr
        if roads == {"labels": HOST, "core": HOST}:
            labels, core, st = self.ctx.cluster(slot, r, mp)          # (the binding's own arrays)
        else:
            L = self._out(n, np.int32, roads["labels"])
            K = self._out(n, np.uint8, roads["core"]) if "core" in roads else None
            st = self.ctx.cluster(slot, r, mp, labels_ptr=p(L), core_ptr=p(K))
            labels, core = self._get(L, np.int32), None if K is None else self._get(K, np.uint8)
        self._same(what, "labels", labels, ref["labels"])
        if core is not None:
            self._same(what, "core", np.asarray(core).view(np.uint8), ref["core"].view(np.uint8))
        self._same_record(what, st, cluster_ref.record(ref))
        self._intact(what)

    # ---- rows of their own ----
    def _plane_rows(self, mv, rng):
        """(X, mask, max_distance) of a plane call: a plane with noise in clutter or uniform rows; the mask drops a fifth."""
        n = mv["n"]
        if mv["scene"] == "plane":
            X, md = plane_ref.plane_scene(int(rng.integers(1 << 30)), (3 * n) // 5, n - (3 * n) // 5)[0], 0.05
        else:
            X, md = rng.uniform(-10.0, 10.0, (n, 3)), 1.0
        mask = None
        if mv["mask"] != "none":
            mask = np.where(rng.random(n) < 0.2, 0, rng.choice([1, 7], n)).astype(np.uint8)
        return X, mask, md

    def _rows_in(self, mv, X, mask):
        roads = mv["roads"]
        return self._in("X", X, roads["X"]), None if mask is None else self._in("mask", mask, roads["mask"])

    def plane_triplets(self, mv, rng):
        n, h, roads = mv["n"], mv["h"], mv["roads"]
        X, mask, md = self._plane_rows(mv, rng)
        tri = rng.integers(0, n, (h, 3), dtype=np.int32)
        if mv["all_void"]:
            tri[:, 1] = tri[:, 0]                                     # every triple repeats a row: best = -1
        elif h >= 5:
            k = rng.choice(h, max(1, h // 8), replace=False)
            tri[k, 2] = tri[k, 0]
        what = f"plane_triplets n={n} h={h} mask={mv['mask']} scene={mv['scene']} all_void={mv['all_void']} roads={roads}"
        self.log.append(what)
        want = ref_triplets(X, mask, tri, md)
        self.notes.append(dict(kind="plane_triplets", **want[2]))
        Xd, Md = self._rows_in(mv, X, mask)
        T = self._in("triples", tri, roads["triples"])
        planes = self._out((h, 4), np.float64, roads["planes"]) if "planes" in roads else None
        inl = self._out(h, np.int32, roads["inliers"])
        p = self.mem.ptr
        st = self.ctx.plane_triplets(p(Xd), p(T), md, mask=p(Md), n=n, h=h, planes_ptr=p(planes), inliers_ptr=p(inl))
        self._same(what, "inliers", self._get(inl, np.int32), want[1])
        if planes is not None:
            self._same(what, "planes", self._get(planes, np.uint64, (h, 4)), _u64(want[0]))
        self._same_record(what, st, want[2])
        self._intact(what)

    def plane_refit(self, mv, rng):
        n, b, rounds, roads = mv["n"], mv["b"], mv["rounds"], mv["roads"]
        X, mask, md = self._plane_rows(mv, rng)
        start = start_planes(rng, X, mask, md, b)
        what = f"plane_refit n={n} b={b} rounds={rounds} mask={mv['mask']} scene={mv['scene']} keep={mv['keep']} roads={roads}"
        self.log.append(what)
        want = ref_refit(X, mask, start, md, rounds, mv["keep"])
        self.notes.append(dict(kind="plane_refit", **want[3]))
        Xd, Md = self._rows_in(mv, X, mask)
        Pin = self._in("planes_in", start, roads["planes_in"])
        planes, inl = self._out((b, 4), np.float64, roads["planes"]), self._out(b, np.int32, roads["inliers"])
        keep = self._out(n, np.uint8, roads["keep"]) if mv["keep"] else None
        p = self.mem.ptr
        st = self.ctx.plane_refit(p(Xd), p(Pin), md, rounds, mask=p(Md), n=n, b=b, planes_ptr=p(planes), inliers_ptr=p(inl), keep_ptr=p(keep))
        self._same(what, "inliers", self._get(inl, np.int32), want[1])
        self._same(what, "planes", self._get(planes, np.uint64, (b, 4)), _u64(want[0]))
        if keep is not None:
            self._same(what, "keep", self._get(keep, np.uint8), want[2].view(np.uint8))
        self._same_record(what, st, want[3])
        self._intact(what)

    def farthest(self, mv, rng):
        n, count, roads = mv["n"], mv["count"], mv["roads"]
        X = rng.uniform(-10.0, 10.0, (n, 3))
        if n >= 64:                                                   # rows that are no candidates, mask or not
            rows = rng.choice(n, 2, replace=False)
            X[rows[0], 0], X[rows[1], 2] = np.nan, np.inf
        mask = None
        if mv["mask"] != "none":
            mask = np.where(rng.random(n) < 0.3, 0, rng.choice([1, 7, 255], n)).astype(np.uint8)
        cand = np.flatnonzero(farthest_ref.candidates(X, mask))
        start = int(rng.choice(cand)) if mv["start"] == "row" and len(cand) else -1
        base = f"farthest n={n} count={count} start={start} mask={mv['mask']} roads={roads}"
        self.log.append(base)
        want = ref_farthest(X, mask, count, start)
        self.notes.append(dict(kind="farthest", **want[2]))
        bits = lambda rec: dict(rec, cover_d2=int(_u64([rec["cover_d2"]])[0]))    # noqa: E731  (+0.0 is not -0.0)
        p = self.mem.ptr
        for path, ctx in [("default", self.ctx)] + ([] if self.stepped is None else [("stepped", self.stepped)]):
            what = base if path == "default" else f"{base} (path {path})"
            Xd, Md = self._rows_in(mv, X, mask)
            idx = self._out(count, np.int64, roads["idx"])
            d2 = self._out(count, np.float64, roads["d2"]) if "d2" in roads else None
            st = ctx.farthest(p(Xd), count, start, mask=p(Md), n=n, idx_ptr=p(idx), d2_ptr=p(d2))
            self._same(what, "idx", self._get(idx, np.int64), want[0])
            if d2 is not None:
                self._same(what, "d2", self._get(d2, np.uint64), _u64(want[1]))
            self._same_record(what, bits(fo._record(st)), bits(want[2]))
            self._intact(what)

    def orient(self, mv, rng):
        slot, X, k, roads = mv["slot"], self.cloud(mv["slot"]), mv["k"], mv["roads"]
        n = len(X)
        N = rng.standard_normal((n, 3)).astype(np.float32)
        N[rng.integers(0, 2, n).astype(bool)] *= np.float32(-1.0)
        rows = rng.choice(n, 2, replace=False)
        N[rows[0]], N[rows[1]] = (np.nan, 0.0, 1.0), 0.0
        reference = None if mv["reference"] == "none" else (X.min(axis=0) + X.max(axis=0)) * 0.5 + np.array([0.0, 0.0, 10.0])
        away = mv["reference"] == "away"
        what = f"orient slot={slot} n={n} k={k} reference={mv['reference']} alias={mv['alias']} roads={roads}"
        self.log.append(what)
        ref = ref_orient(X, N, k, reference, away)
        self.notes.append(dict(kind="orient", **orient_ref.record(ref)))
        if mv["alias"]:
            Nin = out = self.mem.dev(N) if roads["normals"] == DEVICE else N.copy()    # (expected to hold the result, not its old bytes)
        else:
            Nin, out = self._in("normals", N, roads["normals"]), self._out((n, 3), np.float32, roads["normals_out"])
        flipped = self._out(n, np.uint8, roads["flipped"]) if "flipped" in roads else None
        p = self.mem.ptr
        st = self.ctx.orient(slot, Nin, k, reference=reference, away=away, normals_ptr=p(out), flipped_ptr=p(flipped))
        self._same(what, "normals", self._get(out, np.uint32, (n, 3)), ref["normals"].view(np.uint32))
        if flipped is not None:
            self._same(what, "flipped", self._get(flipped, np.uint8), ref["flipped"].view(np.uint8))
        self._same_record(what, st, orient_ref.record(ref))
        self._intact(what)

    def match_consistency(self, mv, rng):
        """fuzz_operators' move, the forced paths on the context that steps and on one opened for this move: with the context of
        an estimate_normals move, never more than three are open."""
        if self.one is None:
            return super().match_consistency(mv, rng)
        with self.one() as one:
            self.forced = {"one": one, "sweeps": self.stepped}
            try:
                super().match_consistency(mv, rng)
            finally:
                self.forced = {}

    def apply(self, mv):
        if mv["kind"] not in LATE:
            return super().apply(mv)
        rng = self.rng = np.random.default_rng(mv["seed"])
        getattr(self, mv["kind"])(mv, rng)


def replay(moves, ctx, mem, fresh, stepped=None, one=None, seed=0, notes=None):
    """fuzz_operators.replay with the late model: (problems, log, kernels seen, the index of the move that failed or None).  The
    two clouds of the start take their sizes in turn by the seed (cluster and orient run on them: no size is left to chance)."""
    m = Model(ctx, mem, fresh, stepped, one, notes)
    m.rng = np.random.default_rng(99_000 + seed)
    for slot, turn in ((m.L.FIX, seed), (m.L.MOV, seed + seed // 4)):
        m.SIZES = (fo.Model.SIZES[turn % 4],)
        m.upload(slot)
    del m.SIZES
    for step, mv in enumerate(moves):
        m.apply(mv)
        mem.sync()
        if m.bad:
            return m.bad, m.log, m.kernels, step
    return m.bad, m.log, m.kernels, None


# ---- on the real library --------------------------------------------------------------------------------------------------------------
def run_on_library(moves, seed=0):
    """The moves on a fresh context of the real library, farthest also on a context forced to the stepped path, match_consistency
    on one forced to either peeling path.  Three contexts at the most: the default one; the one that steps, which is also the one
    that sweeps, opened where the moves hold either kind; and the one a single move opens and closes again -- match_consistency its
    one-launch context, estimate_normals its fresh one."""
    flavour = "far" if seed % 2 else "near"
    kinds = {mv["kind"] for mv in moves}
    ctx, stepped = fo.library_context(flavour, **ENV_LATE), None
    try:
        if kinds & {"farthest", "match_consistency"}:
            stepped = fo.library_context(flavour, SICP_CONSISTENCY="sweeps", **ENV_LATE, **ENV_STEPPED)
        return replay(moves, ctx, fo.TorchMemory(), lambda: fo.library_context(flavour, **ENV_LATE), stepped,
                      lambda: fo.library_context(flavour, SICP_CONSISTENCY="one", **ENV_LATE), seed)
    finally:
        for c in (ctx, stepped):
            if c is not None:
                c.close()
