"""What the six plane calls refuse, and with which words: gg_fuse_states, gg_track_clusters, gg_route_planes, gg_match_planes,
gg_footprint_planes and gg_route_headings through the raw C calls, and the six GroundSegmentation methods over them.

Per call one valid baseline (a 20 x 20 map, n_slots = 4, n = 3, every optional buffer given) and a list of named mistakes in the source
order of the checks.  The cases: every single mistake, every adjacent pair, the first with the last, n = n_slots + 2 alone and with each
other mistake, n = 0 with garbage, and every (output, input) and (output, output) pair of buffers laid over each other at the first word,
at the last word of the last plane, and one word past it (which is accepted).  observe_*() return, per case, [rc, gg_last_error text] of
the C call or [exception type name, message] of the method; `python -m tests.plane_refusals --record` writes them to
tests/golden/plane_refusals_{cpu,gpu}.json, and tests/test_plane_refusals_{cpu,gpu}.py hold the code to the recording.  Buffers are
places in one device arena, so no address appears in a message.  Not collected by pytest (no test_ prefix)."""
import ctypes as C
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from groundgrid_amd import _lib, api  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
SIDE, N_SLOTS, N = 20, 4, 3
GEOMETRY = (7.0, 0.35)     # (length, resolution) of a 20 x 20 map
CELLS = SIDE * SIDE
STRIDE = CELLS + 16        # of every plane buffer of the C table: larger than the plane, so a range ends before n * stride
OVER = N_SLOTS + 2
ROW = _lib.GG_PLANES_ROWMAJOR
NULL, GARBAGE = "null", "garbage"   # places of a buffer other than a word offset into the arena


def i32(rows):
    return np.ascontiguousarray(np.asarray(rows, dtype=np.int32))


def changed(base, *edits):
    """a copy of the host array with a[index] = value for every (index, value)"""
    a = base.copy()
    for index, value in edits:
        a[index] = value
    return a


# ---------------------------------------------------------------- the C calls

SHIFTS = i32([[0, 0], [25, -25], [1, 1], [0, 0], [0, 0], [0, 0]])          # (host arrays hold OVER rows: n = n_slots + 2 reads none of them,
PIVOTS = i32([[10, 10]] * OVER)                                            # and if it did, it would stay inside)
ROTATIONS = i32([[16384, 0], [0, 16384]])
ROUTE_STARTS = i32([0, -1, 5, 0, 0, 0])
SPANS = i32([[[0, 0], [0, 0], [0, 0]], [[1, 0], [-1, 1], [1, 0]]])          # K = 2, R = 1
MOVES = np.zeros((2, 8, 4), np.int32)
MOVES[0, 0], MOVES[1, 0], MOVES[0, 6], MOVES[1, 6] = (1, 0, 0, 10), (0, 1, 1, 10), (0, 0, 1, 5), (0, 0, 0, 5)
POSES = i32([[0, 0], [-1, 0], [5, 1], [0, 0], [0, 0], [0, 0]])
MAX_PATH = 4


def planes(stride_field, words=CELLS):
    return lambda v: (v["n"] - 1) * v[stride_field] + words


def rows_of(words):
    return lambda v: v["n"] * words


# per call: the struct, the baseline values, the buffers (field, words of its range, is an output) in the order of the call's range table,
# and the mistakes (name, {field: value, "@buffer": place}) in the order of the call's checks; the overlap mistake is added behind them
C_CALLS = {
    "gg_fuse_states": dict(
        struct=_lib.GGStateFusion,
        values=dict(n=N, state_stride=STRIDE, shifts=SHIFTS, hit=4, miss=1, decay=0, e_min=-16, e_max=32, free_threshold=-2, occ_threshold=4, order=ROW,
                    plane_stride=STRIDE),
        buffers=[("d_state", planes("state_stride"), False), ("d_evidence_in", planes("plane_stride"), False), ("d_evidence_out", planes("plane_stride"), True),
                 ("d_fused", planes("plane_stride"), True), ("d_frontier", planes("plane_stride"), True), ("d_counts", rows_of(4), True)],
        mistakes=[("n < 0", {"n": -1}), ("no d_evidence_out", {"@d_evidence_out": NULL}), ("state_stride", {"state_stride": CELLS - 1}),
                  ("plane_stride", {"plane_stride": CELLS - 1}), ("order", {"order": 7}), ("hit", {"hit": -1}), ("e_max", {"e_max": -1}),
                  ("free_threshold", {"free_threshold": 0}), ("occ_threshold", {"occ_threshold": 0})]),
    "gg_track_clusters": dict(
        struct=_lib.GGClusterTracks,
        values=dict(n=N, cells_stride=STRIDE, prev_stride=STRIDE, shifts=SHIFTS, max_clusters=8, gate=1, order=ROW, track_stride=STRIDE),
        buffers=[("d_cells", planes("cells_stride"), False), ("d_cells_prev", planes("prev_stride"), False), ("d_tracks_in", rows_of(8 * 8), False),
                 ("d_heads_in", rows_of(4), False), ("d_tracks_out", rows_of(8 * 8), True), ("d_heads_out", rows_of(4), True),
                 ("d_cell_track", planes("track_stride"), True)],
        mistakes=[("n < 0", {"n": -1}), ("no d_heads_out", {"@d_heads_out": NULL}), ("half a prior", {"@d_heads_in": NULL}),
                  ("cells_stride", {"cells_stride": CELLS - 1}), ("prev_stride", {"prev_stride": CELLS - 1}), ("track_stride", {"track_stride": CELLS - 1}),
                  ("order", {"order": 7}), ("max_clusters", {"max_clusters": 0}), ("gate", {"gate": 5})]),
    "gg_route_planes": dict(
        struct=_lib.GGPlaneRoutes,
        values=dict(n=N, blocked_stride=STRIDE, cost_stride=STRIDE, goal_stride=STRIDE, connectivity=8, straight=5, diagonal=7, cost_max=252, max_cost=0,
                    order=ROW, plane_stride=STRIDE, starts=ROUTE_STARTS, max_path=MAX_PATH),
        buffers=[("d_blocked", planes("blocked_stride"), False), ("d_cost", planes("cost_stride"), False), ("d_goals", planes("goal_stride"), False),
                 ("d_dist", planes("plane_stride"), True), ("d_next", planes("plane_stride"), True), ("d_counts", rows_of(3), True),
                 ("d_paths", rows_of(MAX_PATH), True), ("d_path_len", rows_of(1), True)],
        mistakes=[("n < 0", {"n": -1}), ("no d_dist", {"@d_dist": NULL}), ("blocked_stride", {"blocked_stride": CELLS - 1}),
                  ("cost_stride", {"cost_stride": CELLS - 1}), ("goal_stride", {"goal_stride": CELLS - 1}), ("plane_stride", {"plane_stride": CELLS - 1}),
                  ("order", {"order": 7}), ("connectivity", {"connectivity": 6}), ("straight", {"straight": 0}), ("cost_max", {"cost_max": 0}),
                  ("max_cost", {"max_cost": -1}), ("limit", {"straight": 65535, "cost_max": 2 ** 31 - 1}), ("no d_paths", {"@d_paths": NULL}),
                  ("start outside", {"starts": changed(ROUTE_STARTS, (1, CELLS))})]),
    "gg_match_planes": dict(
        struct=_lib.GGPlaneMatches,
        values=dict(n=N, scan_stride=STRIDE, field_stride=STRIDE, field_max=32, shifts=SHIFTS, pivots=PIVOTS, rotations=ROTATIONS, n_rotations=2, window=1,
                    order=ROW, score_stride=20),
        buffers=[("d_scan", planes("scan_stride"), False), ("d_field", planes("field_stride"), False), ("d_best", rows_of(6), True),
                 ("d_scores", planes("score_stride", 2 * 3 * 3), True)],
        mistakes=[("n < 0", {"n": -1}), ("no d_best", {"@d_best": NULL}), ("scan_stride", {"scan_stride": CELLS - 1}), ("field_stride", {"field_stride": CELLS - 1}),
                  ("order", {"order": 7}), ("window", {"window": 33}), ("n_rotations", {"n_rotations": 0}),
                  ("rotation word", {"rotations": changed(ROTATIONS, ((1, 0), 16385))}), ("field_max", {"field_max": 0}), ("score_stride", {"score_stride": 17}),
                  ("pivot outside", {"pivots": changed(PIVOTS, ((2, 0), SIDE))})]),
    "gg_footprint_planes": dict(
        struct=_lib.GGPlaneFootprints,
        values=dict(n=N, blocked_stride=STRIDE, spans=SPANS, n_headings=2, radius=1, min_fit=2, outside_free=0, order=ROW, mask_stride=STRIDE, fit_stride=STRIDE),
        buffers=[("d_blocked", planes("blocked_stride"), False), ("d_mask", planes("mask_stride"), True), ("d_fit", planes("fit_stride"), True),
                 ("d_counts", rows_of(3), True)],
        mistakes=[("n < 0", {"n": -1}), ("no d_blocked", {"@d_blocked": NULL}), ("no spans", {"spans": None}),
                  ("no output", {"@d_mask": NULL, "@d_fit": NULL, "@d_counts": NULL}), ("blocked_stride", {"blocked_stride": CELLS - 1}),
                  ("mask_stride", {"mask_stride": CELLS - 1}), ("fit_stride", {"fit_stride": CELLS - 1}), ("order", {"order": 7}), ("n_headings", {"n_headings": 0}),
                  ("radius", {"radius": 33}), ("min_fit", {"min_fit": 0}), ("outside_free", {"outside_free": 2}),
                  ("span beyond radius", {"spans": changed(SPANS, ((1, 1, 0), -2))}), ("not column-convex", {"spans": changed(SPANS, ((0, 1), (1, 0)))})]),
    "gg_route_headings": dict(
        struct=_lib.GGHeadingRoutes,
        values=dict(n=N, mask_stride=STRIDE, cost_stride=STRIDE, goal_stride=STRIDE, goal_headings=0xFFFFFFFF, n_headings=2, moves=MOVES, cost_max=252, max_cost=0,
                    order=ROW, dist_stride=2 * STRIDE + 8, plane_stride=STRIDE, next_stride=2 * STRIDE + 8, next_plane_stride=STRIDE, best_stride=STRIDE,
                    best_heading_stride=STRIDE, starts=POSES, path_stride=2 * MAX_PATH + 2, max_len=MAX_PATH),
        buffers=[("d_mask", planes("mask_stride"), False), ("d_cost", planes("cost_stride"), False), ("d_goals", planes("goal_stride"), False),
                 ("d_dist", lambda v: (v["n"] - 1) * v["dist_stride"] + v["plane_stride"] + CELLS, True),
                 ("d_next", lambda v: (v["n"] - 1) * v["next_stride"] + v["next_plane_stride"] + CELLS, True),
                 ("d_best", planes("best_stride"), True), ("d_best_heading", planes("best_heading_stride"), True), ("d_counts", rows_of(3), True),
                 ("d_paths", planes("path_stride", 2 * MAX_PATH), True), ("d_path_len", rows_of(1), True)],
        mistakes=[("n < 0", {"n": -1}), ("no d_goals", {"@d_goals": NULL}), ("no moves", {"moves": None}), ("n_headings", {"n_headings": 0}),
                  ("mask_stride", {"mask_stride": CELLS - 1}), ("cost_stride", {"cost_stride": CELLS - 1}), ("goal_stride", {"goal_stride": CELLS - 1}),
                  ("dist_stride", {"dist_stride": STRIDE}), ("next_plane_stride", {"next_plane_stride": CELLS - 1}), ("best_stride", {"best_stride": CELLS - 1}),
                  ("best_heading_stride", {"best_heading_stride": CELLS - 1}), ("order", {"order": 7}), ("cost_max", {"cost_max": 0}), ("max_cost", {"max_cost": -1}),
                  ("move cost", {"moves": changed(MOVES, ((0, 0, 3), 40000))}), ("move length", {"moves": changed(MOVES, ((1, 0, 1), 4))}),
                  ("move heading", {"moves": changed(MOVES, ((1, 6, 2), 2))}), ("move to itself", {"moves": changed(MOVES, ((0, 6, 2), 0))}),
                  ("limit", {"moves": changed(MOVES, ((0, 0, 3), 32767)), "cost_max": 2 ** 31 - 1}), ("no d_path_len", {"@d_path_len": NULL}),
                  ("path_stride", {"path_stride": 2 * MAX_PATH - 1}), ("start cell", {"starts": changed(POSES, ((2, 0), CELLS))}),
                  ("start heading", {"starts": changed(POSES, ((2, 1), 2))})]),
}


def _extents(call):
    return {field: words(call["values"]) for field, words, _ in call["buffers"]}


def _layout(call):
    """the baseline place (word offset) of every buffer, and the spare region two buffers are laid into to meet each other"""
    place, at = {}, 0
    for field, words in _extents(call).items():
        place[field] = at
        at += words + 64
    return place, at, at + 2 * max(_extents(call).values()) + 64


ARENA_WORDS = max(_layout(call)[2] for call in C_CALLS.values())


def c_cases(name):
    """[(case, {field: value, "@buffer": place})] of one C call"""
    call = C_CALLS[name]
    ext, (_, spare, _) = _extents(call), _layout(call)
    bufs = call["buffers"]
    meets = []   # (case, overrides): the output `a` against every buffer `b` before it in the table, and every input behind it
    for (a, _, a_out), (b, _, b_out) in itertools.permutations(bufs, 2):
        if a_out and (not b_out or [f for f, _, _ in bufs].index(b) < [f for f, _, _ in bufs].index(a)):
            for how, delta in (("first word", 0), ("last word", ext[b] - 1), ("one past", ext[b])):
                meets.append((f"{a} on {b}: {how}", {"@" + b: spare, "@" + a: spare + delta}))
    mistakes = call["mistakes"] + [("overlap", meets[0][1])]
    cases = [("baseline", {}), ("null struct", None)]
    cases += [(m, o) for m, o in mistakes]
    cases += [(f"{m1} + {m2}", {**o1, **o2}) for (m1, o1), (m2, o2) in zip(mistakes, mistakes[1:])]
    cases.append((f"{mistakes[0][0]} + {mistakes[-1][0]}", {**mistakes[0][1], **mistakes[-1][1]}))
    cases.append(("n > n_slots", {"n": OVER}))
    cases += [(f"n > n_slots + {m}", {**o, "n": OVER}) for m, o in mistakes if "n" not in o]
    garbage = {"@" + f: GARBAGE for f, _, _ in bufs}
    cases.append(("n = 0 + garbage", {**garbage, "n": 0, "order": 99, **{k: -7 for k in call["values"] if k.endswith("_stride")}}))
    return cases + meets


class Device:
    """one context of the baseline size and one zeroed device arena"""

    def __init__(self, words=None):
        import torch

        self.torch = torch
        self.seg = api.GroundSegmentation().init(*GEOMETRY, n_slots=N_SLOTS, max_points=4096)
        assert self.seg.rows == self.seg.cols == SIDE
        self.arena = torch.zeros(ARENA_WORDS if words is None else words, dtype=torch.int32, device="cuda")

    def close(self):
        self.torch.cuda.synchronize()
        self.seg.close()


def observe_c(dev, name, overrides):
    """[rc, gg_last_error text] of one raw call ("" with GG_OK); the arena is zero before it and the device idle after it"""
    call, L, ctx = C_CALLS[name], dev.seg._L, dev.seg._ctx
    dev.arena.zero_()
    dev.torch.cuda.synchronize()
    if overrides is None:
        rc = getattr(L, name)(ctx, None, None)
    else:
        place, _, end = _layout(call)
        assert end <= ARENA_WORDS
        x, keep = call["struct"](), []
        for field, value in {**call["values"], **{k: v for k, v in overrides.items() if not k.startswith("@")}}.items():
            if isinstance(value, np.ndarray):
                keep.append(value)
                value = value.ctypes.data_as(C.POINTER(C.c_int32))
            setattr(x, field, value)
        for field, at in {**place, **{k[1:]: v for k, v in overrides.items() if k.startswith("@")}}.items():
            setattr(x, field, None if at == NULL else 0x10 if at == GARBAGE else dev.arena.data_ptr() + 4 * at)
        rc = getattr(L, name)(ctx, C.byref(x), None)
    dev.torch.cuda.synchronize()
    return [int(rc), "" if rc == _lib.GG_OK else L.gg_last_error(ctx).decode()]


# ---------------------------------------------------------------- the Python methods

class NoLibrary:
    """in place of the loaded library: any call through it fails"""

    def __getattr__(self, name):
        raise AssertionError(f"the library was reached: {name}")


def host_seg():
    seg = api.GroundSegmentation()
    seg._L, seg.rows, seg.cols, seg.device, seg.n_slots = NoLibrary(), SIDE, SIDE, 0, N_SLOTS
    return seg


def _planes(torch, device, b=N, dtype=None, shape=(SIDE, SIDE)):
    return torch.zeros((b,) + shape, dtype=dtype or torch.int32, device=device)


def py_baseline(name, torch, device, b=N):
    """the keyword arguments of one valid call of method `name` with its tensors on `device`: every optional input and output asked for"""
    t = lambda: _planes(torch, device, b)  # noqa: E731
    rows = lambda a: np.concatenate([a, a])[:b]  # noqa: E731
    return {
        "fuse_states": lambda: dict(states=t(), evidence=t(), shifts=rows(SHIFTS)),
        "route_planes": lambda: dict(goals=t(), blocked=t(), cost=t(), starts=rows(ROUTE_STARTS), max_path=MAX_PATH),
        "match_planes": lambda: dict(scan=t(), field=t(), shifts=rows(SHIFTS), pivots=rows(PIVOTS), rotations=ROTATIONS, window=1, scores=True),
        "footprint_planes": lambda: dict(blocked=t(), spans=SPANS),
        "route_headings": lambda: dict(mask=t(), goals=t(), moves=MOVES, cost=t(), starts=rows(POSES), max_len=MAX_PATH),
        "track_clusters": lambda: dict(cell_cluster=t(), previous=api.TrackOutputs(tracks=_planes(torch, device, b, shape=(8, 8)),
                                                                                   heads=_planes(torch, device, b, shape=(4,)), cell_cluster=t()),
                                       shifts=rows(SHIFTS), max_clusters=8, cell_track=True),
    }[name]()


# the parameter mistakes, which a host tensor reaches (name, {keyword: value}), in the order of the method's checks
PY_PARAMETER_MISTAKES = {
    "fuse_states": [("order", {"order": "fortran"}), ("miss is no integer", {"miss": 1.5}), ("hit", {"hit": -1}), ("e_min", {"e_min": 1}),
                    ("free_threshold", {"free_threshold": 0})],
    "route_planes": [("order", {"order": "fortran"}), ("diagonal is no integer", {"diagonal": True}), ("connectivity", {"connectivity": 6}),
                     ("straight", {"straight": 0}), ("cost_max", {"cost_max": 0}), ("max_cost", {"max_cost": -1}), ("max_path", {"max_path": -1}),
                     ("limit", {"straight": 65535, "cost_max": 2 ** 31})],
    "match_planes": [("order", {"order": "fortran"}), ("field_max is no integer", {"field_max": 1.5}), ("window", {"window": 33}), ("field_max", {"field_max": 0}),
                     ("rotations shape", {"rotations": [1, 2, 3]}), ("rotations count", {"rotations": np.zeros((65, 2), np.int32)}),
                     ("rotation word", {"rotations": [[16385, 0]]})],
    "footprint_planes": [("order", {"order": "fortran"}), ("outside_free", {"outside_free": 1}), ("spans shape", {"spans": np.zeros((2, 2, 2), np.int32)}),
                         ("spans inexact", {"spans": np.full((2, 3, 2), 0.5)}), ("spans count", {"spans": np.zeros((33, 3, 2), np.int32)}), ("min_fit", {"min_fit": 0}),
                         ("no output", {"mask": False, "fit": False, "counts": False})],
    "route_headings": [("order", {"order": "fortran"}), ("max_cost is no integer", {"max_cost": True}), ("goal_headings", {"goal_headings": -1}),
                       ("cost_max", {"cost_max": 0}), ("max_cost", {"max_cost": -1}), ("max_len", {"max_len": -1}), ("moves shape", {"moves": np.zeros((2, 7, 4), np.int32)}),
                       ("move cost", {"moves": changed(MOVES, ((0, 0, 3), 40000))}), ("move length", {"moves": changed(MOVES, ((1, 0, 1), 4))}),
                       ("move heading", {"moves": changed(MOVES, ((1, 6, 2), 2))}), ("move to itself", {"moves": changed(MOVES, ((0, 6, 2), 0))}),
                       ("limit", {"moves": changed(MOVES, ((0, 0, 3), 32767)), "cost_max": 2 ** 31 - 1})],
    "track_clusters": [("order", {"order": "fortran"}), ("gate is no integer", {"gate": 1.5}), ("max_clusters", {"max_clusters": 0}), ("gate", {"gate": 5})],
}


def _alias(torch, kw, key, shape):
    """a tensor of `shape` at the first word of the input kw[key]"""
    return kw[key].view(-1)[:int(np.prod(shape))].view(shape)


def py_tensor_mistakes(name, torch):
    """the tensor, `out` and host-array mistakes of one method, (name, edit of the keyword arguments), in the order of its checks"""
    cpu = lambda key: lambda kw: kw.update({key: kw[key].cpu()})  # noqa: E731
    other_b = lambda key: lambda kw: kw.update({key: _planes(torch, "cuda", N + 1)})  # noqa: E731
    floats = lambda key: lambda kw: kw.update({key: kw[key].float()})  # noqa: E731
    put = lambda **edits: lambda kw: kw.update(edits)  # noqa: E731

    def out(cls, flags, **fields):
        """the edit that sets fields of the call's `out` (made when the call has none yet): a tensor, the name of the input to alias, or a function of kw"""
        def edit(kw):
            kw.update(flags)
            res = kw.setdefault("out", cls())
            for field, v in fields.items():
                setattr(res, field, kw[v] if isinstance(v, str) else v(kw) if callable(v) else v)
        return edit

    plane, small = lambda: _planes(torch, "cuda"), lambda *shape: _planes(torch, "cuda", shape=shape)  # noqa: E731
    return {
        "fuse_states": [
            ("states on the host", cpu("states")), ("states shape", put(states=small(SIDE, SIDE + 1))), ("evidence of another B", other_b("evidence")),
            ("shifts shape", put(shifts=np.zeros((N, 3), np.int32))), ("shifts inexact", put(shifts=np.full((N, 2), 0.5))),
            ("out.state not asked for", out(api.FusionOutputs, dict(fused=False), state=plane())),
            ("out.frontier shape", out(api.FusionOutputs, {}, evidence=plane(), frontier=small(SIDE, SIDE + 1))),
            ("out.evidence is states", out(api.FusionOutputs, {}, evidence="states"))],
        "route_planes": [
            ("goals on the host", cpu("goals")), ("goals shape", put(goals=small(SIDE, SIDE + 1))), ("blocked of another B", other_b("blocked")),
            ("cost of another dtype", floats("cost")), ("starts shape", put(starts=np.zeros((N, 2), np.int32))), ("starts inexact", put(starts=np.full(N, 0.5))),
            ("start outside", put(starts=changed(ROUTE_STARTS[:N], (1, CELLS)))), ("starts without max_path", put(max_path=0)),
            ("out.next not asked for", out(api.RouteOutputs, dict(next=False), next=plane())),
            ("out.paths shape", out(api.RouteOutputs, {}, dist=plane(), paths=small(MAX_PATH + 1))),
            ("out.dist is cost", out(api.RouteOutputs, {}, dist="cost"))],
        "match_planes": [
            ("scan on the host", cpu("scan")), ("field of another B", other_b("field")), ("shifts shape", put(shifts=np.zeros((N, 3), np.int32))),
            ("pivots inexact", put(pivots=np.full((N, 2), 0.5))), ("pivot outside", put(pivots=changed(PIVOTS[:N], ((2, 1), SIDE)))),
            ("out.scores not asked for", out(api.MatchOutputs, dict(scores=False), scores=small(2, 3, 3))),
            ("out.scores shape", out(api.MatchOutputs, {}, best=small(6), scores=small(2, 3, 4))),
            ("out.best is field", out(api.MatchOutputs, {}, best=lambda kw: _alias(torch, kw, "field", (N, 6)))),
            ("out.scores is scan", out(api.MatchOutputs, {}, scores=lambda kw: _alias(torch, kw, "scan", (N, 2, 3, 3))))],
        "footprint_planes": [
            ("blocked on the host", cpu("blocked")), ("blocked shape", put(blocked=small(SIDE, SIDE + 1))),
            ("out.fit not asked for", out(api.FootprintOutputs, dict(fit=False), fit=plane())),
            ("out.counts shape", out(api.FootprintOutputs, {}, mask=plane(), counts=small(4))),
            ("out.fit is blocked", out(api.FootprintOutputs, {}, fit="blocked"))],
        "route_headings": [
            ("mask on the host", cpu("mask")), ("goals of another B", other_b("goals")), ("cost of another dtype", floats("cost")),
            ("starts shape", put(starts=np.zeros((N,), np.int32))), ("start cell", put(starts=changed(POSES[:N], ((2, 0), CELLS)))),
            ("start heading", put(starts=changed(POSES[:N], ((2, 1), 2)))), ("starts without max_len", put(max_len=0)),
            ("out.best not asked for", out(api.HeadingOutputs, dict(best=False), best=plane())),
            ("out.dist shape", out(api.HeadingOutputs, {}, dist=plane(), best=plane())),
            ("out.best_heading is goals", out(api.HeadingOutputs, {}, best=plane(), best_heading="goals"))],
        "track_clusters": [
            ("cell_cluster on the host", cpu("cell_cluster")), ("out is previous", lambda kw: kw.update(out=kw["previous"])),
            ("previous of another order", lambda kw: setattr(kw["previous"], "order", "col")),
            ("previous of another max_clusters", lambda kw: setattr(kw["previous"], "tracks", small(9, 8))),
            ("shifts shape", put(shifts=np.zeros((N, 3), np.int32))),
            ("out.cell_track not asked for", out(api.TrackOutputs, dict(cell_track=False), cell_track=plane())),
            ("out.heads shape", out(api.TrackOutputs, {}, tracks=small(8, 8), heads=small(3))),
            ("out.cell_track is cell_cluster", out(api.TrackOutputs, {}, cell_track="cell_cluster")),
            ("out.heads is previous.heads", out(api.TrackOutputs, {}, heads=lambda kw: kw["previous"].heads))],
    }[name]


def _combined(mistakes):
    """every single mistake, every adjacent pair, the first with the last"""
    return [(m, [e]) for m, e in mistakes] + [(f"{a} + {b}", [ea, eb]) for (a, ea), (b, eb) in zip(mistakes, mistakes[1:])] + [
        (f"{mistakes[0][0]} + {mistakes[-1][0]}", [mistakes[0][1], mistakes[-1][1]])]


def observe_py(seg, name, kw):
    """[exception type name, message] of one method call, ["", ""] when it returns"""
    try:
        getattr(seg, name)(**kw)
    except Exception as e:  # noqa: BLE001 (whatever is raised is what is recorded)
        return [type(e).__name__, str(e)]
    return ["", ""]


def observe_cpu():
    """{case: [exception type name, message]} of the parameter mistakes, on host tensors and without the library"""
    import torch

    seen, seg = {}, host_seg()
    for name, mistakes in PY_PARAMETER_MISTAKES.items():
        for case, edits in [("baseline on the host", [])] + _combined(mistakes):
            kw = py_baseline(name, torch, "cpu")
            for edit in edits:
                kw.update(edit)
            seen[f"{name}: {case}"] = observe_py(seg, name, kw)
    return seen


def observe_gpu():
    """{case: [rc, text]} of the C table and {case: [exception type name, message]} of the methods' tensor mistakes, on the device"""
    import torch

    seen, dev = {}, Device()
    try:
        for name in C_CALLS:
            for case, overrides in c_cases(name):
                seen[f"{name}: {case}"] = observe_c(dev, name, overrides)
        for name in PY_PARAMETER_MISTAKES:
            tensor = py_tensor_mistakes(name, torch)
            # (a parameter mistake comes before a tensor mistake: the last of the one list with the first of the other)
            lists = [("baseline", [])] + _combined(tensor) + [(f"{PY_PARAMETER_MISTAKES[name][-1][0]} + {tensor[0][0]}", [PY_PARAMETER_MISTAKES[name][-1][1], tensor[0][1]])]
            for case, edits in lists:
                kw = py_baseline(name, torch, "cuda")
                for edit in edits:
                    kw.update(edit) if isinstance(edit, dict) else edit(kw)
                seen[f"{name}: {case}"] = observe_py(dev.seg, name, kw)
                torch.cuda.synchronize()
            seen[f"{name}: B > n_slots"] = observe_py(dev.seg, name, py_baseline(name, torch, "cuda", OVER))
    finally:
        dev.close()
    return seen


def recorded(which, name="plane_refusals"):
    with open(os.path.join(GOLDEN, f"{name}_{which}.json")) as f:
        return json.load(f)


def first_difference(seen, want):
    """None, or a line that names the first case of the recording the observation differs in (or a case of only one of the two)"""
    for case in want:
        if case not in seen:
            return f"{case}: recorded, not observed"
        if seen[case] != want[case]:
            return f"{case}: recorded {want[case]}, observed {seen[case]}"
    extra = [case for case in seen if case not in want]
    return f"{extra[0]}: observed, not recorded" if extra else None


def record_main(name, observe_cpu, observe_gpu):
    """`python -m tests.NAME --record [--out DIR]`: the CPU table, and on a machine with a device the GPU table, into NAME_{cpu,gpu}.json"""
    import torch

    if "--record" not in sys.argv[1:]:
        sys.exit(f"usage: python -m tests.{name} --record [--out DIR]")
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else GOLDEN
    tables = {"cpu": observe_cpu()}
    if torch.cuda.is_available():
        tables["gpu"] = observe_gpu()
    for which, seen in tables.items():
        with open(os.path.join(out, f"{name}_{which}.json"), "w") as f:
            json.dump(seen, f, indent=0, sort_keys=False)
            f.write("\n")
        print(f"recorded {len(seen)} {which} cases")


if __name__ == "__main__":
    record_main("plane_refusals", observe_cpu, observe_gpu)
