"""CPU guard for tests/edge_scenes.py: every hostile scene still reaches the branch it is named for, checked with the oracle.  An
edit of a generator that quietly drops a case (a long cell that shrinks under RCAP, a tile that no longer holds exactly 512
records) fails here, without a GPU."""
import numpy as np
import pytest

from groundgrid_amd import api
from oracle import oracle
from tests import edge_scenes as es


def _run(scene, frames=None):
    ref = oracle.OracleMap(scene.length, scene.resolution, pos=scene.pos, odom_z=scene.odom_z)
    if scene.cfg_edit:
        scene.cfg_edit(ref.cfg)
    rs = [ref.filter_cloud(scene.cloud, scene.origin, scene.base_z) for _ in range(frames or scene.frames)]
    return ref, rs


def _records(ref, r):
    """points per cell and records per 16 x 16 tile (every point inside the map is a record of its cell's tile)"""
    inside = r["cls"] != oracle.OUTSIDE
    cell = r["cell"][inside]
    per_cell = np.bincount(cell, minlength=ref.rows * ref.cols)
    tile = (cell % ref.rows) // es.TILE + ((cell // ref.rows) // es.TILE) * ((ref.rows + es.TILE - 1) // es.TILE)
    per_tile = np.bincount(tile) if len(tile) else np.zeros(1, np.int64)
    return per_cell, per_tile


def test_long_cells_hold_more_than_the_reciprocal_table():
    for scene in (es.dense_single_cells_and_ties(), es.reduce_tile_classes_long_cells_and_quotient_fallbacks(), es.exact_tile_records()):
        ref, rs = _run(scene, 1)
        per_cell, _ = _records(ref, rs[0])
        assert per_cell.max() > es.RCAP, scene.name
    ref, rs = _run(es.exact_tile_records(), 1)
    assert (_records(ref, rs[0])[0] == es.RCAP + 1).sum() == 1


def test_tiles_of_exactly_512_and_513_records():
    scene = es.exact_tile_records()
    ref, rs = _run(scene, 1)
    _, per_tile = _records(ref, rs[0])
    for count, tiles in scene.extra["tile_records"].items():
        assert (per_tile == count).sum() == tiles, count
    assert (per_tile == es.K2_LIGHT_MAX).sum() == 1 and (per_tile == es.K2_LIGHT_MAX + 1).sum() == 1


def test_constant_tiny_and_huge_heights_reach_k_reduce():
    scene = es.reduce_tile_classes_long_cells_and_quotient_fallbacks()
    z = scene.cloud["z"]
    assert (np.abs(z[(z != 0) & (np.abs(z) < 1e-30)]) > 0).sum() >= 250
    assert (np.abs(z) > 1e25).sum() >= 250
    assert (z == np.float32(-1.5)).sum() >= 700


def test_recurrence_scene_holds_zero_means_and_non_numbers():
    z = es.reduce_recurrence_rare_cases().cloud["z"]
    assert np.isnan(z).sum() == 3 * 10 and np.isposinf(z).sum() == 3 and np.isneginf(z).sum() == 3  # (three regions)
    assert (np.signbit(z) & (z == 0)).sum() >= 2


def test_ring_and_outlier_scenes_produce_ignored_and_outlier_points():
    _, rs = _run(es.edge_cases())
    assert (rs[-1]["cls"] == oracle.IGNORED).sum() > 0
    assert (rs[-1]["cls"] == oracle.OUTSIDE).sum() >= 4       # NaN / inf / 500 m / -1e30
    for scene in (es.line_of_sight_walk(), es.corrupt_z()):
        _, rs = _run(scene)
        assert (rs[-1]["cls"] == oracle.OUTLIER).sum() > 0, scene.name
    assert (es.edge_cases().cloud["ring"] > oracle.default_config().max_ring).sum() == 1


def test_signalling_nan_heights_are_signalling():
    z = es.signalling_nan_heights().cloud["z"].view(np.uint32)
    for k in (1, 3):
        assert (z[k] & 0x7F800000) == 0x7F800000 and (z[k] & 0x007FFFFF) != 0 and not (z[k] & 0x00400000), hex(z[k])


@pytest.mark.parametrize("cfg", es.LABEL_TOLERANCE_CONFIGS)
def test_label_tolerance_configs_give_two_labels(cfg):
    _, rs = _run(es.label_tolerance(*cfg))
    assert len(np.unique(rs[-1]["label"])) >= 2


def test_empty_and_all_outside_scenes():
    assert len(es.empty().cloud) == 0
    _, rs = _run(es.all_outside())
    assert (rs[0]["cls"] == oracle.OUTSIDE).all()


def test_border_and_utm_scenes_reach_the_border_and_land_inside():
    for pos in es.MAP_BORDER_POSITIONS[:3]:
        _, rs = _run(es.map_border(pos), 1)
        cls = rs[0]["cls"]
        assert (cls != oracle.OUTSIDE).sum() > 0 and (cls == oracle.OUTSIDE).sum() > 0, pos
    for k, pos in enumerate(es.UTM_POSITIONS):
        _, rs = _run(es.utm_drive(pos, 40 + k), 1)
        assert (rs[0]["cls"] == oracle.KEPT).sum() > 1000, pos


def test_sized_scenes_have_exactly_their_size():
    for n in es.BATCH_SIZES + [4095, 4096]:
        assert len(es.sized(n).cloud) == n


def test_special_bits_survive_both_point_formats():
    """api.pack16 and the raw 32-byte records keep the exact bits of NaN payloads, subnormals and -0.0"""
    c = es.special_bits().cloud
    k = es.special_bits().extra["n_specials"]
    raw32 = np.frombuffer(c.tobytes(), dtype=np.uint8).reshape(-1, 32)
    p16 = api.pack16(c)
    for name, off in (("x", 0), ("y", 4), ("z", 8)):
        want = c[name].view(np.uint32)
        assert np.array_equal(p16[name].view(np.uint32), want), name
        assert np.array_equal(raw32[:, off : off + 4].copy().view(np.uint32)[:, 0], want), name
    assert np.array_equal(p16["ring"], c["ring"])
    bits = np.concatenate([c[n].view(np.uint32)[:k] for n in ("x", "y", "z")])
    assert 0x80000000 in bits and 0x00000001 in bits and 0x7F800001 in bits and 0xFFA00001 in bits
    # the signalling NaNs of edge_scenes.signalling_nan_heights go through pack16 unchanged too
    s = es.signalling_nan_heights().cloud
    assert np.array_equal(api.pack16(s)["z"].view(np.uint32), s["z"].view(np.uint32))


def test_adversarial_scenes_share_the_batch_geometry():
    names = [s.name for s in es.adversarial_scenes()]
    assert len(names) == len(set(names))
    for s in es.adversarial_scenes():
        assert (s.length, s.resolution) == (120.0, 0.33) and s.cfg_edit is None, s.name
