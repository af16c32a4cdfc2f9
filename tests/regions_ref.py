"""What gg_cluster_planes is expected to give, in numpy and without the library (a helper, not a test): cluster_ref.label_plane on the
member mask, the sizes by bincount, the drop of the small components, the renumbering by smallest linear index and the records.
tests/test_cluster_planes_cpu.py holds it against scipy.ndimage.label with a size filter and a sequential relabelling."""
import numpy as np

from tests import cluster_ref

INT32_MAX, INT32_MIN = 0x7FFFFFFF, -(1 << 31)
FIELDS = ["cells", "row_min", "row_max", "col_min", "col_max", "first_cell", "value_cell", "value_min", "sum_row", "sum_col"]
REGION_DTYPE = np.dtype([("cells", "<i4"), ("row_min", "<i4"), ("row_max", "<i4"), ("col_min", "<i4"), ("col_max", "<i4"), ("first_cell", "<i4"),
                         ("value_cell", "<i4"), ("value_min", "<i4"), ("sum_row", "<i8"), ("sum_col", "<i8")])


def members(seeds, lo=0, hi=INT32_MAX):
    seeds = np.asarray(seeds, dtype=np.int64)
    return (seeds >= lo) & (seeds <= hi)


def regions_of_labels(labels, min_cells=1, order="row", values=None):
    """labels: int32 [rows, cols], -1 or the id of the cell's component, the ids ascending in the components' smallest linear index of
    `order` (cluster_ref.label_plane).  Returns (plane int32 [rows, cols], sizes int32 [rows, cols], heads int32 [4], records
    REGION_DTYPE [K])"""
    labels = np.asarray(labels, dtype=np.int64)
    rows, cols = labels.shape
    member = labels >= 0
    n_all = int(labels.max()) + 1 if member.any() else 0
    size_of = np.bincount(labels[member], minlength=n_all)
    sizes = np.zeros((rows, cols), dtype=np.int32)
    sizes[member] = size_of[labels[member]]
    keep = size_of >= min_cells
    new_id = np.where(keep, np.cumsum(keep) - 1, -1)  # (the order of the smallest indices survives the drop)
    K = int(keep.sum())
    plane = np.full((rows, cols), -1, dtype=np.int32)
    plane[member] = new_id[labels[member]]
    heads = np.array([K, n_all - K, int(member.sum()), int((plane >= 0).sum())], dtype=np.int32)
    rec = np.zeros(K, dtype=REGION_DTYPE)
    rr, cc = np.nonzero(plane >= 0)
    of = plane[rr, cc].astype(np.int64)
    L = cluster_ref.linear_index(rr, cc, rows, cols, order).astype(np.int64)
    rec["cells"] = np.bincount(of, minlength=K)
    lo_r, lo_c, first = np.full(K, rows), np.full(K, cols), np.full(K, rows * cols)
    hi_r, hi_c = np.full(K, -1), np.full(K, -1)
    np.minimum.at(lo_r, of, rr)
    np.maximum.at(hi_r, of, rr)
    np.minimum.at(lo_c, of, cc)
    np.maximum.at(hi_c, of, cc)
    np.minimum.at(first, of, L)
    rec["row_min"], rec["row_max"], rec["col_min"], rec["col_max"], rec["first_cell"] = lo_r, hi_r, lo_c, hi_c, first
    sum_r, sum_c = np.zeros(K, dtype=np.int64), np.zeros(K, dtype=np.int64)
    np.add.at(sum_r, of, rr)
    np.add.at(sum_c, of, cc)
    rec["sum_row"], rec["sum_col"] = sum_r, sum_c
    rec["value_min"], rec["value_cell"] = INT32_MAX, -1
    if values is not None and K:
        v = np.asarray(values, dtype=np.int64)[rr, cc]
        by = np.lexsort((L, v, of))  # by region, then value, then L: the first of every region is the lexicographic minimum of (value, L)
        head = by[np.r_[True, of[by][1:] != of[by][:-1]]]
        rec["value_min"][of[head]] = v[head]
        rec["value_cell"][of[head]] = L[head]
    return plane, sizes, heads, rec


def expected_regions(seeds, lo=0, hi=INT32_MAX, connectivity=8, min_cells=1, order="row", values=None):
    """seeds: int [rows, cols].  The answer of gg_cluster_planes for one map, as regions_of_labels gives it"""
    return regions_of_labels(cluster_ref.label_plane(members(seeds, lo, hi), connectivity, order), min_cells, order, values)


def words_of(rec):
    """REGION_DTYPE [K] as int32 [K, 12], the words of the records"""
    return np.ascontiguousarray(rec).view(np.int32).reshape(len(rec), 12)
