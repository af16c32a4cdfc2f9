"""What gg_fuse_states must write, restated in numpy from the text of include/groundgrid_hip.h alone: prior (the shifted, clamped evidence of
the previous call), decay, observation, fused state, frontier, counts.  Every array here is LOGICAL, [rows, cols] indexed (row, col);
`lay` puts one where `order` puts it in memory.  The arithmetic runs in int64 and is checked to fit an int32, so an overflow of the code
under test cannot be shared.  The frontier loops over cells and their neighbours; nothing is pooled, tiled or shifted as a whole.

WorldEvidence is a second reference that is built differently: one large array indexed by ABSOLUTE cell, updated in place, through which the
window moves by the running sum of the shifts.  It never shifts anything, so it does not share the sign convention of `prior_of`."""
import numpy as np

FREE, UNKNOWN, OCCUPIED = -1, 0, 1
LIMIT = (1 << 30) - 1
DEFAULTS = dict(hit=4, miss=1, decay=0, e_min=-16, e_max=32, free_threshold=-2, occ_threshold=4)  # those of GroundSegmentation.fuse_states


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    assert all(0 <= p[k] <= LIMIT for k in ("hit", "miss", "decay")) and -LIMIT <= p["e_min"] <= 0 <= p["e_max"] <= LIMIT
    assert p["e_min"] <= p["free_threshold"] <= -1 and 1 <= p["occ_threshold"] <= p["e_max"]
    return p


def lay(a, order):
    """a logical [rows, cols] array as the plane of `order`: [rows, cols] row-major, [cols, rows] column-major"""
    return np.ascontiguousarray(a if order == "row" else a.T)


def prior_of(evidence, shift, p):
    """rule 1: P[r, c] = clamp(in[r + s0, c + s1]) where that cell exists, 0 elsewhere; evidence None: 0 everywhere"""
    rows, cols = evidence.shape if evidence is not None else (0, 0)
    s0, s1 = int(shift[0]), int(shift[1])
    P = np.zeros((rows, cols), np.int64)
    for r in range(rows):
        rr = r + s0
        if rr < 0 or rr >= rows:
            continue
        for c in range(cols):
            cc = c + s1
            if 0 <= cc < cols:
                P[r, c] = min(max(int(evidence[rr, cc]), p["e_min"]), p["e_max"])
    return P


def frontier_of(F):
    """rule 5, cell by cell: 0 on a FREE cell with an UNKNOWN cell among its neighbours inside the map, -1 elsewhere.  Walked from the
    UNKNOWN cells: each marks the FREE cells among its own neighbours inside the map (being a neighbour is mutual)"""
    rows, cols = F.shape
    out = np.full((rows, cols), -1, np.int32)
    for r, c in np.argwhere(F == UNKNOWN):
        for a in (-1, 0, 1):
            for b in (-1, 0, 1):
                rr, cc = r + a, c + b
                if (a or b) and 0 <= rr < rows and 0 <= cc < cols and F[rr, cc] == FREE:
                    out[rr, cc] = 0
    return out


def expected_fusion(state, evidence, shift, p):
    """the six rules for one map: state [rows, cols] (any int32 words), evidence [rows, cols] or None, shift (s0, s1) or None.
    Returns dict(evidence, fused, frontier: int32 [rows, cols]; counts: int32 [4] free, unknown, occupied, frontier)"""
    state = np.asarray(state).astype(np.int64)
    shift = (0, 0) if shift is None else shift
    P = prior_of(np.asarray(evidence), shift, p) if evidence is not None else np.zeros(state.shape, np.int64)
    D = np.where(P > 0, np.maximum(P - p["decay"], 0), np.minimum(P + p["decay"], 0))
    S = D + np.where(state > 0, p["hit"], np.where(state < 0, -p["miss"], 0))
    assert np.abs(S).max(initial=0) < (1 << 31)  # (the limits of the header keep every sum inside an int32)
    E = np.clip(S, p["e_min"], p["e_max"])
    F = np.where(E >= p["occ_threshold"], OCCUPIED, np.where(E <= p["free_threshold"], FREE, UNKNOWN)).astype(np.int32)
    front = frontier_of(F)
    counts = np.array([(F == FREE).sum(), (F == UNKNOWN).sum(), (F == OCCUPIED).sum(), (front == 0).sum()], np.int32)
    assert int(counts[:3].sum()) == state.size
    return dict(evidence=E.astype(np.int32), fused=F, frontier=front, counts=counts)


class WorldEvidence:
    """The second reference: evidence per ABSOLUTE cell of a world large enough for the whole drive, updated in place.  The window's cell
    (r, c) is the absolute cell (r + o0, c + o1), (o0, o1) being the sum of the shifts so far: no plane is ever shifted.  A cell that left
    the window keeps its evidence here and loses it in the definition, so `comparable` names the window cells that have been inside without
    interruption since they first entered."""

    def __init__(self, rows, cols, shifts, p):
        self.rows, self.cols, self.p = rows, cols, p
        path = np.cumsum(np.asarray(shifts, np.int64).reshape(-1, 2), axis=0)
        lo, hi = np.minimum(path.min(axis=0), 0), np.maximum(path.max(axis=0), 0)
        self.base = -lo  # absolute cell 0 of the window's start lies here in the arrays
        shape = (int(hi[0] - lo[0]) + rows, int(hi[1] - lo[1]) + cols)
        self.E = np.zeros(shape, np.int64)
        self.seen = np.zeros(shape, bool)   # was inside the window at some frame
        self.left = np.zeros(shape, bool)   # ... and outside it at a later one
        self.at = np.zeros(2, np.int64)

    def window(self):
        r0, c0 = (self.at + self.base).tolist()
        return slice(r0, r0 + self.rows), slice(c0, c0 + self.cols)

    def step(self, shift, state):
        p = self.p
        self.at += np.asarray(shift, np.int64)
        w = self.window()
        inside = np.zeros(self.E.shape, bool)
        inside[w] = True
        self.left |= self.seen & ~inside
        self.seen |= inside
        state = np.asarray(state).astype(np.int64)
        P = self.E[w]
        D = np.where(P > 0, np.maximum(P - p["decay"], 0), np.minimum(P + p["decay"], 0))
        self.E[w] = np.clip(D + np.where(state > 0, p["hit"], np.where(state < 0, -p["miss"], 0)), p["e_min"], p["e_max"])

    def evidence(self):
        return self.E[self.window()].astype(np.int32)

    def comparable(self):
        return ~self.left[self.window()]
