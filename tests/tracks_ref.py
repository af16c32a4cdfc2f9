"""gg_track_clusters in numpy: a restatement of the definition in include/groundgrid_hip.h, one map at a time, everything in (row, col)
terms on planes of shape [rows, cols].  Two independent formulations of the overlap matrix: `overlap_vectorised` (np.add.at on a padded
previous plane) and `overlap_loop` (a plain loop over cells and offsets with a dict); tests/test_track_clusters_cpu.py holds them together."""
import numpy as np

TRACK_DTYPE = np.dtype([("track_id", "<i4"), ("age", "<i4"), ("prev", "<i4"), ("overlap", "<i4"), ("still", "<i4"), ("cells", "<i4"),
                        ("sum_row", "<i4"), ("sum_col", "<i4")])
INT32_MAX = 2 ** 31 - 1


def cluster_counts(cur, prev, heads_in, M):
    """(Kc, Kp, next_id) of a map; prev is None without a prior"""
    top = int(cur.max()) if cur.size else -1
    Kc = 0 if top < 0 else min(top + 1, M)
    if prev is None:
        return Kc, 0, 0
    return Kc, min(max(int(heads_in[1]), 0), M), int(heads_in[0])


def overlap_vectorised(cur, prev, Kc, Kp, M, shift, g):
    """O[c][p] and its offset-(0, 0) part S[c][p], int64 [Kc, Kp]"""
    rows, cols = cur.shape
    s0, s1 = int(shift[0]), int(shift[1])
    O, S = np.zeros((Kc, Kp), np.int64), np.zeros((Kc, Kp), np.int64)
    if Kc == 0 or Kp == 0 or abs(s0) >= rows or abs(s1) >= cols:
        return O, S
    P = g + max(abs(s0), abs(s1))
    padded = np.full((rows + 2 * P, cols + 2 * P), -1, np.int64)
    padded[P:P + rows, P:P + cols] = np.where((prev >= 0) & (prev < Kp), prev, -1)
    r, q = np.nonzero((cur >= 0) & (cur < M))
    c = cur[r, q].astype(np.int64)
    for a in range(-g, g + 1):
        for b in range(-g, g + 1):
            p = padded[r + s0 + a + P, q + s1 + b + P]
            hit = p >= 0
            np.add.at(O, (c[hit], p[hit]), 1)
            if a == 0 and b == 0:
                np.add.at(S, (c[hit], p[hit]), 1)
    return O, S


def overlap_loop(cur, prev, Kc, Kp, M, shift, g):
    """the same by a plain loop over cells and offsets with a dict"""
    rows, cols = cur.shape
    s0, s1 = int(shift[0]), int(shift[1])
    pairs, exact = {}, {}
    if not (abs(s0) >= rows or abs(s1) >= cols):
        for r in range(rows):
            for q in range(cols):
                c = int(cur[r, q])
                if c < 0 or c >= M:
                    continue
                for a in range(-g, g + 1):
                    for b in range(-g, g + 1):
                        rr, qq = r + s0 + a, q + s1 + b
                        if rr < 0 or rr >= rows or qq < 0 or qq >= cols:
                            continue
                        p = int(prev[rr, qq])
                        if p < 0 or p >= Kp:
                            continue
                        pairs[(c, p)] = pairs.get((c, p), 0) + 1
                        if a == 0 and b == 0:
                            exact[(c, p)] = exact.get((c, p), 0) + 1
    O, S = np.zeros((Kc, Kp), np.int64), np.zeros((Kc, Kp), np.int64)
    for (c, p), v in pairs.items():
        O[c, p] = v
    for (c, p), v in exact.items():
        S[c, p] = v
    return O, S


def track_map(cur, prev=None, tracks_in=None, heads_in=None, shift=(0, 0), M=256, g=1, overlap=overlap_vectorised):
    """One map.  cur, prev: int32 [rows, cols]; tracks_in: TRACK_DTYPE records (at least Kp of them); heads_in: four ints.  Returns
    (records TRACK_DTYPE [Kc], heads int32 [4], cell_track int32 [rows, cols])."""
    cur = np.asarray(cur)
    rows, cols = cur.shape
    Kc, Kp, next_id = cluster_counts(cur, prev, heads_in, M)
    O, S = overlap(cur, prev, Kc, Kp, M, shift, g) if prev is not None else (np.zeros((Kc, 0), np.int64),) * 2
    # candidate: the p of the largest O[c][p] > 0, the smallest among equals (np.argmax returns the first maximum)
    pstar = [int(np.argmax(O[c])) if Kp and O[c].max() > 0 else -1 for c in range(Kc)]
    # winner of p: the c with p*(c) = p of the largest O[c][p], the smallest among equals
    winner = {}
    for c in range(Kc):
        p = pstar[c]
        if p >= 0 and (p not in winner or O[c, p] > O[winner[p], p]):
            winner[p] = c
    inside = (cur >= 0) & (cur < M)
    rr, qq = np.nonzero(inside)
    ids = cur[rr, qq]
    rec = np.zeros(Kc, TRACK_DTYPE)
    rec["cells"] = np.bincount(ids, minlength=Kc)[:Kc]
    rec["sum_row"] = np.bincount(ids, weights=rr, minlength=Kc)[:Kc].astype(np.int64)
    rec["sum_col"] = np.bincount(ids, weights=qq, minlength=Kc)[:Kc].astype(np.int64)
    born = inherited = 0
    for c in range(Kc):
        p = pstar[c]
        if p >= 0 and winner[p] == c:
            rec[c]["track_id"] = tracks_in[p]["track_id"]
            rec[c]["age"] = min(int(tracks_in[p]["age"]), INT32_MAX - 1) + 1
            rec[c]["prev"], rec[c]["overlap"], rec[c]["still"] = p, O[c, p], S[c, p]
            inherited += 1
        else:
            rec[c]["track_id"] = (next_id + born) & 0x7FFFFFFF
            rec[c]["age"], rec[c]["prev"], rec[c]["overlap"], rec[c]["still"] = 0, -1, 0, 0
            born += 1
    heads = np.array([(next_id + born) & 0x7FFFFFFF, Kc, born, Kp - inherited], np.int32)
    cell_track = np.full((rows, cols), -1, np.int32)
    cell_track[rr, qq] = rec["track_id"][ids]
    return rec, heads, cell_track


def label_plane(occupied):
    """an id plane as gg_cluster_clouds writes it from a boolean occupancy [rows, cols]: the 8-connected components numbered by their
    smallest row-major cell (scipy.ndimage.label's raster order), -1 elsewhere"""
    from scipy import ndimage

    labels, _ = ndimage.label(np.asarray(occupied, bool), structure=np.ones((3, 3), int))
    return labels.astype(np.int32) - 1


def random_scene(rng, side, density):
    return label_plane(rng.random((side, side)) < density)


def first_records(cur, M, first_id=0):
    """(tracks int32 [M, 8], heads [4]) of a call without a prior on `cur`: what a chain starts from"""
    rec, heads, _ = track_map(cur, M=M)
    rec["track_id"] = (rec["track_id"].astype(np.int64) + first_id) & 0x7FFFFFFF
    heads[0] = (int(heads[0]) + first_id) & 0x7FFFFFFF
    full = np.zeros(M, TRACK_DTYPE)
    full[:len(rec)] = rec
    return full.view(np.int32).reshape(M, 8), heads


def as_row_col(plane, order):
    """a plane as the call stores it ([rows, cols] with order "row", [cols, rows] with "col") in (row, col) terms"""
    return plane if order == "row" else plane.T


def track_maps(cells, prev_cells=None, tracks_in=None, heads_in=None, shifts=None, M=256, g=1, order="row", overlap=overlap_vectorised):
    """Many maps, with the shapes of the device call.  cells / prev_cells: int32 [n, rows, cols] ([n, cols, rows] with order "col");
    tracks_in: int32 [n, M, 8]; heads_in: int32 [n, 4]; shifts: [n, 2] or None.  Returns (list of TRACK_DTYPE records per map, heads int32
    [n, 4], cell_track int32 in the shape and order of `cells`)."""
    n = cells.shape[0]
    recs, heads, planes = [], np.zeros((n, 4), np.int32), np.empty_like(cells)
    for i in range(n):
        prior = prev_cells is not None
        rec, heads[i], ct = track_map(as_row_col(cells[i], order), as_row_col(prev_cells[i], order) if prior else None,
                                      np.ascontiguousarray(tracks_in[i]).view(TRACK_DTYPE).reshape(-1) if prior else None,
                                      heads_in[i] if prior else None, (0, 0) if shifts is None else shifts[i], M, g, overlap)
        recs.append(rec)
        planes[i] = as_row_col(ct, order)
    return recs, heads, planes
