"""FRESH maps by the sign tag on the device: k_patch stores its confidences with bit 31 set, k_sweep<FRESH> takes a loaded cell as it is iff
the bit is set and the slot's reset pair otherwise (groundgrid_amd/csrc/sweep_core.h sw_untag) -- so the layer's memory, which gg_reset_maps
leaves as the slot's LAST USE left it, must never show through.  Every case re-uses its slots: a second reset and filter meets the first
filter's finished layer as stale memory.  Bit-exact against the oracle on ground, groundpatch, labels, index and counts; after every filter
and after the last reset no confidence of any slot has its sign bit set.

The launches have 17 to 24 clouds of a few thousand points (above the 16 clouds of the pair sweep, which fills fresh maps first).  A launch
that small would by default give every ring group a work-group of its own WITH split steps, and split steps fill fresh maps first as well:
the tests switch split steps off (tuning sweep_split = 2), which leaves the launch shapes under test -- one work-group per cloud on the
map of one ring group (67 x 67, odd), two and three work-groups per cloud (k_sweep<PARTS, FRESH>) on 244 x 244 and 364 x 364 (even), and two
work-groups per cloud on 135 x 135: odd AND in parts, so k_patch's cells in ring c keep their tag while only the last part's work-group
looks at the border and its last wavefront clears the tags.  These are shapes a production launch of this size does not pick by itself;
launches that do pick them (100 and more clouds) are the fresh-map cases of test_gpu_parity.py.

The check for sign bits that counts is the one after each filter: a getter on a fresh map fills it first, so after a reset it cannot fail."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from groundgrid_amd import api  # noqa: E402
from oracle import oracle  # noqa: E402
from tests.test_gpu_parity import ORIGIN0, _batch_inputs, _rotated_clouds, assert_same_state, nan_equal  # noqa: E402

# (length, resolution, clouds per launch, azimuth steps of a cloud): the maps of the fresh-map parity cases of test_gpu_parity.py; the last
# of those is swept by three work-groups per cloud; (27.0, 0.2) = 135 x 135, 65 rings: the smallest odd map with two ring groups
MAPS = [(22.0, 0.33, 19, 100), (61.0, 0.25, 17, 100), (120.0, 0.33, 24, 120), (27.0, 0.2, 18, 100)]


def sign_bits(a):
    return (np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) >> 31) != 0


class Rig:
    def __init__(self, length, resolution, batch, n_az, seed=61):
        import torch

        self.torch = torch
        self.length, self.resolution, self.batch = length, resolution, batch
        self.clouds = _rotated_clouds(batch, length, seed=seed, n_az=n_az)
        assert all(2000 <= len(c) <= 12000 for c in self.clouds), [len(c) for c in self.clouds][:3]
        self.stride = (max(len(c) for c in self.clouds) + 63) // 64 * 64
        self.seg = api.GroundSegmentation().init(length, resolution, n_slots=batch, max_points=self.stride)
        self.seg.debug_set_tuning("sweep_split", 2)
        self.out = None
        self.border_patched = 0  # maps in which k_patch wrote a cell of ring >= c (by the oracle): the cells whose tag outlives the chains

    def filter(self, refs, shift, base_z, tag):
        """cloud (b + shift) mod batch on slot b; everything the call returns and the two persistent layers of EVERY slot against the oracle"""
        torch, batch = self.torch, self.batch
        clouds = [self.clouds[(b + shift) % batch] for b in range(batch)]
        pts = _batch_inputs(16, clouds, self.stride)
        self.out = self.seg.filter_batch(pts, [len(c) for c in clouds], np.zeros((batch, 3), np.float32), np.full(batch, base_z), out=self.out)
        torch.cuda.synchronize()
        labels, index, counts = self.out.labels.cpu().numpy(), self.out.out_index.cpu().numpy(), self.out.counts.cpu().numpy()
        for b, c in enumerate(clouds):
            r = refs[b].filter_cloud(c, ORIGIN0, base_z)
            n = len(c)
            assert np.array_equal(labels[b, :n], r["label"]), (tag, b, "labels")
            assert np.array_equal(index[b, :n], r["index"]), (tag, b, "index")
            assert counts[b, 0] == len(r["out_points"]) and counts[b, 3] == (r["cls"] == oracle.OUTLIER).sum(), (tag, b, "counts")
            w = self.seg.map(b)["groundpatch"]
            assert not sign_bits(w).any(), (tag, b, "a confidence with its sign bit set", np.argwhere(sign_bits(w))[:3].tolist())
            assert nan_equal(w, refs[b].layer("groundpatch")), (tag, b, "groundpatch", np.argwhere(w != refs[b].layer("groundpatch"))[:3].tolist())
            g = self.seg.map(b)["ground"]
            assert nan_equal(g, refs[b].layer("ground")), (tag, b, "ground", np.argwhere(g != refs[b].layer("ground"))[:3].tolist())
            if b in (0, batch - 1):
                assert_same_state(self.seg.map(b), refs[b], f"{tag} cloud {b}")
            rows = refs[b].rows
            i, j = np.indices((rows, rows))
            border = np.maximum(np.abs(i - (rows // 2 - 1)), np.abs(j - (rows // 2 - 1))) >= rows // 2 - 1
            self.border_patched += bool((refs[b].layer("groundpatch")[border] != np.float32(0.0000001)).any())

    def reset(self, odom_z):
        self.seg.reset_maps(odom_z=odom_z, on_torch_stream=True)
        return [oracle.OracleMap(self.length, self.resolution, odom_z=odom_z) for _ in range(self.batch)]

    def no_sign_bits_anywhere(self, tag):
        for b in range(self.batch):
            assert not sign_bits(self.seg.map(b)["groundpatch"]).any(), (tag, b)

    def close(self):
        self.seg.close()


@pytest.mark.parametrize("shift", [0, 5], ids=["same_slots", "rotated"])
@pytest.mark.parametrize("length,resolution,batch,n_az", MAPS)
def test_second_filter_meets_the_first_ones_layer(length, resolution, batch, n_az, shift):
    """reset, filter, reset, filter: the second filter's fresh maps hold the first one's finished layer (other clouds; or the same clouds
    rotated over the slots) -- none of it may be taken for a cell written in the second call"""
    rig = Rig(length, resolution, batch, n_az)
    refs = rig.reset(0.25)
    rig.filter(refs, 0, -1.73, "first call")
    refs = rig.reset(-0.5)
    rig.filter(refs, shift if shift else batch // 2 + 1, -1.7, "second call")
    if shift == 0:  # ... and the same clouds on the same slots once more: the stale layer is the one the call would write itself
        refs = rig.reset(0.125)
        rig.filter(refs, batch // 2 + 1, -1.7, "third call")
    if rig.seg.rows % 2:
        assert rig.border_patched > 0, "the case is meant to have k_patch write cells of ring c"
    rig.reset(0.0)
    rig.no_sign_bits_anywhere("after the last reset")
    rig.close()


@pytest.mark.parametrize("length,resolution,batch,n_az", [MAPS[0], MAPS[2], MAPS[3]])
def test_caller_planes_with_sign_bits_take_the_fill(length, resolution, batch, n_az):
    """gg_set_layer of groundpatch with negative and NaN entries: the slot's next reset fills every cell (once), and a filter on it equals the
    oracle's cold result; the slots next to it stay fresh"""
    rig = Rig(length, resolution, batch, n_az)
    refs = rig.reset(0.25)
    rig.filter(refs, 0, -1.73, "first call")
    rng = np.random.default_rng(7)
    rows = rig.seg.rows
    for b in (1, batch - 2):
        plane = rng.uniform(-1.0, 1.0, (rows, rows)).astype(np.float32)
        plane[rng.random((rows, rows)) < 0.05] = np.float32(-0.0)
        nan_neg = np.array([0xFFC00000], dtype=np.uint32).view(np.float32)[0]
        plane[rng.random((rows, rows)) < 0.05] = nan_neg
        plane[rng.random((rows, rows)) < 0.05] = np.float32("nan")
        rig.seg.map(b).set("groundpatch", plane)
        assert sign_bits(rig.seg.map(b)["groundpatch"]).any()  # (the caller's values, as the caller put them)
    refs = rig.reset(-0.5)
    rig.filter(refs, 3, -1.7, "after set_layer and reset")
    refs = rig.reset(0.5)  # (the flag is spent: fresh again, on the layer the last call left)
    rig.filter(refs, 7, -1.75, "one reset later")
    rig.close()


def test_fresh_and_warm_maps_in_one_launch():
    """a launch that mixes fresh and warm maps fills the fresh ones first, as before"""
    length, resolution, batch, n_az = MAPS[0]
    rig = Rig(length, resolution, batch, n_az)
    refs = rig.reset(0.25)
    rig.filter(refs, 0, -1.73, "first call")
    for b in range(0, batch - 1, 4):
        rig.seg.reset_maps(first_slot=b, n_slots=2, odom_z=-0.25, on_torch_stream=True)
        refs[b] = oracle.OracleMap(length, resolution, odom_z=-0.25)
        refs[b + 1] = oracle.OracleMap(length, resolution, odom_z=-0.25)
    rig.filter(refs, 2, -1.7, "mixed launch")
    refs = rig.reset(0.0)
    rig.filter(refs, 4, -1.73, "all fresh again")
    rig.close()
