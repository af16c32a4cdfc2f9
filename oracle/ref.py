"""Python side of the reference build (TEST INFRASTRUCTURE): writes scenario files, runs oracle/_ref/gg_ref_run -- the reference's
own GroundSegmentation translation unit compiled against the stand-ins of oracle/ref_shim/, one process per scenario -- under a
time limit, and reads its raw results as numpy arrays.  The file formats are described at the top of oracle/ref_driver.cpp.

Nothing here touches libgg_oracle.so or the HIP library: the two sides of a comparison share no object code.
"""
from __future__ import annotations

import os
import struct
import subprocess
import tempfile

import numpy as np

from . import ref_build

LAYERS = ["points", "ground", "groundpatch", "minGroundHeight", "maxGroundHeight", "groundCandidates", "planeDist", "m2",
          "meanVariance", "pointsRaw", "variance"]
CONFIG_INTS = ["point_count_cell_variance_threshold", "max_ring", "thread_count"]
CONFIG_DOUBLES = ["groundpatch_detection_minimum_threshold", "distance_factor", "minimum_distance_factor",
                  "miminum_point_height_threshold", "minimum_point_height_obstacle_threshold", "outlier_tolerance",
                  "ground_patch_detection_minimum_point_count_threshold", "patch_size_change_distance",
                  "occupied_cells_decrease_factor", "occupied_cells_point_count_factor", "min_outlier_detection_ground_confidence"]
# What GroundGrid::initGroundGrid leaves in a new map (src/GroundGrid.cpp:55, :71-75), as data: the five layers that exist and the
# value each is filled with (None: the odometry height).  The values reach the layers as floats, as a double literal reaches a float matrix.
INITIAL_LAYERS = {"points": 0.0, "ground": None, "groundpatch": 0.0000001, "minGroundHeight": 100.0, "maxGroundHeight": -100.0}
OP_FILTER, OP_INSERT, OP_DETECT_SECTION, OP_SPIRAL, OP_PATCH, OP_INTERPOLATE, OP_INIT = 1, 2, 3, 4, 5, 6, 7
POINT_BYTES = 32
TIME_LIMIT_S = 120.0


class Config:
    """the fields of gg_config with the defaults of gg_default_config, as plain numbers"""

    def __init__(self):
        for k, v in zip(CONFIG_INTS, (10, 1024, 1)):
            setattr(self, k, v)
        for k, v in zip(CONFIG_DOUBLES, (0.01, 0.0001, 0.0005, 0.3, 0.1, 0.1, 0.25, 20.0, 5.0, 20.0, 1.25)):
            setattr(self, k, v)


def default_config() -> Config:
    return Config()


def single_thread(cfg) -> Config:
    """a copy of any gg_config-shaped object with thread_count = 1: the caller's statement that the run is single-threaded"""
    c = Config()
    for k in CONFIG_INTS + CONFIG_DOUBLES:
        setattr(c, k, getattr(cfg, k))
    c.thread_count = 1
    return c


class ReferenceFailed(RuntimeError):
    """the reference process did not run to the end: .returncode (None after the time limit), .stderr"""

    def __init__(self, msg, returncode, stderr):
        super().__init__(msg)
        self.returncode, self.stderr = returncode, stderr


def _cloud_bytes(cloud) -> bytes:
    b = np.ascontiguousarray(cloud).tobytes()
    assert len(b) % POINT_BYTES == 0
    return b


class Scenario:
    """One process of gg_ref_run: geometry, map position, initial layers, configuration, steps.

    cfg: any object with the fields of gg_config (oracle.Config, a namespace).  Its thread_count must be 1, the only value at which the
    reference is deterministic (more insertion threads race on shared cells, src/GroundSegmentation.cpp:101-106): anything else is a
    ValueError; single_thread(cfg) makes the copy that says so.  layers: None = the map as GroundGrid::initGroundGrid leaves it (src/GroundGrid.cpp:71-75), or a
    dict / sequence of all 11 layers as (rows, cols) arrays."""

    def __init__(self, length, resolution, pos=(0.0, 0.0), odom_z=0.0, cfg=None, layers=None, quaternion=(0.0, 0.0, 0.0, 1.0)):
        self.length, self.resolution, self.pos, self.odom_z = float(length), float(resolution), tuple(pos), float(odom_z)
        if cfg is not None and int(cfg.thread_count) != 1:
            raise ValueError(f"thread_count = {int(cfg.thread_count)}: the reference build is run with one thread only (see single_thread)")
        self.cfg, self.layers, self.quaternion = cfg, layers, tuple(quaternion)
        self.steps = []   # (payload bytes, (op, dump))

    def _add(self, op, dump, payload):
        self.steps.append((struct.pack("<ii", op, 1 if dump else 0) + payload, (op, dump)))
        return self

    def filter_cloud(self, cloud, origin=(0.0, 0.0, 0.0), base_z=0.0, dump=True):
        b = _cloud_bytes(cloud)
        return self._add(OP_FILTER, dump, struct.pack("<Q4fd", len(b) // POINT_BYTES, *[float(v) for v in origin], 0.0, float(base_z)) + b)

    def insert_cloud(self, cloud, origin=(0.0, 0.0, 0.0), start=0, end=None, dump=True):
        b = _cloud_bytes(cloud)
        n = len(b) // POINT_BYTES
        return self._add(OP_INSERT, dump, struct.pack("<QQQ4f", n, start, n if end is None else end, *[float(v) for v in origin], 0.0) + b)

    def detect_ground_patches(self, section, dump=True):
        return self._add(OP_DETECT_SECTION, dump, struct.pack("<i", section))

    def spiral_ground_interpolation(self, base_z=0.0, dump=True):
        return self._add(OP_SPIRAL, dump, struct.pack("<d", float(base_z)))

    def detect_ground_patch(self, S, i, j, dump=True):
        return self._add(OP_PATCH, dump, struct.pack("<iQQ", S, i, j))

    def interpolate_cell(self, x, y, dump=True):
        return self._add(OP_INTERPOLATE, dump, struct.pack("<QQ", x, y))

    def init(self):
        return self._add(OP_INIT, False, b"")

    def to_bytes(self) -> bytes:
        cfg = self.cfg if self.cfg is not None else Config()
        ints = [int(getattr(cfg, k)) for k in CONFIG_INTS]
        doubles = [float(getattr(cfg, k)) for k in CONFIG_DOUBLES]
        head = b"GGREFSC1" + struct.pack("<ff2d3ii11d4d", np.float32(self.length), np.float32(self.resolution), *self.pos,
                                         *ints, len(self.steps), *doubles, *self.quaternion)
        parts = [head]
        for k, name in enumerate(LAYERS):
            if self.layers is None:   # the map as initGroundGrid leaves it: five layers, each one value
                if name in INITIAL_LAYERS:
                    v = INITIAL_LAYERS[name]
                    parts.append(b"\x02" + struct.pack("<f", np.float32(self.odom_z if v is None else v)))
                else:
                    parts.append(b"\x00")
            else:
                a = self.layers[name] if isinstance(self.layers, dict) else self.layers[k]
                parts.append(b"\x01" + np.asfortranarray(a, dtype=np.float32).tobytes(order="F"))
        parts += [s[0] for s in self.steps]
        return b"".join(parts)


def _read_layers(buf, off, rows, cols):
    (mask,) = struct.unpack_from("<I", buf, off)
    off += 4
    out = {}
    for k, name in enumerate(LAYERS):
        if mask & (1 << k):
            out[name] = np.frombuffer(buf, dtype="<f4", count=rows * cols, offset=off).reshape((rows, cols), order="F")
            off += 4 * rows * cols
    return out, off


def _read_pairs(buf, off):
    (n,) = struct.unpack_from("<Q", buf, off)
    off += 8
    rec = np.frombuffer(buf, dtype=np.dtype([("i", "<u8"), ("row", "<i4"), ("col", "<i4")]), count=n, offset=off)
    return rec, off + 16 * n


def run(scenario: Scenario, binary: str = "gg_ref_run", time_limit: float = TIME_LIMIT_S):
    """Runs the scenario in a fresh process; returns one dict per step: "layers" (name -> (rows, cols) array) where dumped, and
    "out_points" (raw (n, 32) bytes of the returned cloud) / "kept", "ignored" (records i, row, col), "outliers" / "expected_points"."""
    exe = ref_build.binary(binary)
    with tempfile.TemporaryDirectory(prefix="gg_ref_") as tmp:
        sc, rs = os.path.join(tmp, "scenario.bin"), os.path.join(tmp, "results.bin")
        with open(sc, "wb") as f:
            f.write(scenario.to_bytes())
        try:
            p = subprocess.run([exe, sc, rs], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=time_limit)
        except subprocess.TimeoutExpired as e:
            raise ReferenceFailed(f"{binary} did not end within {time_limit:g} s", None, (e.stderr or b"").decode(errors="replace"))
        if p.returncode != 0:
            raise ReferenceFailed(f"{binary} ended with status {p.returncode}: {p.stderr.decode(errors='replace').strip()}", p.returncode,
                                  p.stderr.decode(errors="replace"))
        with open(rs, "rb") as f:
            buf = f.read()
    if buf[:8] != b"GGREFRS1" or buf[-8:] != b"GGREFEND":
        raise ReferenceFailed(f"{binary} left incomplete results", p.returncode, "")
    rows, cols = struct.unpack_from("<ii", buf, 8)
    off, results = 16, []
    for _, (op, dump) in scenario.steps:
        r = {"rows": rows, "cols": cols}
        if op == OP_FILTER:
            (n,) = struct.unpack_from("<Q", buf, off)
            r["out_points"] = np.frombuffer(buf, dtype=np.uint8, count=n * POINT_BYTES, offset=off + 8).reshape(n, POINT_BYTES)
            off += 8 + n * POINT_BYTES
        elif op == OP_INSERT:
            r["kept"], off = _read_pairs(buf, off)
            r["ignored"], off = _read_pairs(buf, off)
            (n,) = struct.unpack_from("<Q", buf, off)
            r["outliers"] = np.frombuffer(buf, dtype="<u8", count=n, offset=off + 8)
            off += 8 + 8 * n
        elif op == OP_INIT:
            r["expected_points"] = np.frombuffer(buf, dtype="<f4", count=rows * cols, offset=off).reshape((rows, cols), order="F")
            off += 4 * rows * cols
        if dump:
            r["layers"], off = _read_layers(buf, off, rows, cols)
        results.append(r)
    assert off == len(buf) - 8, (off, len(buf))
    return results
