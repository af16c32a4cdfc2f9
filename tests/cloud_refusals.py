"""What the nine map and cloud calls refuse, and with which words: gg_export_layers, gg_import_layers, gg_export_slopes, gg_export_images,
gg_split_clouds, gg_rasterize_clouds, gg_cluster_clouds, gg_clearance_clouds (cloud mode and seed mode) and gg_visibility_clouds through the
raw C calls, and the ten GroundSegmentation methods over them.  The scheme, the shapes and the shared parts are those of
tests/plane_refusals.py: a 20 x 20 map, n_slots = 4, n = 3; three zero-filled POINT16 clouds of 40, 0 and 64 points with cloud_stride = 64;
per call a valid baseline with every optional output asked for and a list of named mistakes in the source order of the checks.  The cases:
every single mistake, every adjacent pair, the first with the last, n = n_slots + 2 alone and with each other mistake, n = 0 with garbage,
the null struct.  `python -m tests.cloud_refusals --record` writes tests/golden/cloud_refusals_{cpu,gpu}.json, and
tests/test_cloud_refusals_{cpu,gpu}.py hold the code to the recording.  Not collected by pytest (no test_ prefix)."""
import ctypes as C
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from groundgrid_amd import _lib, api  # noqa: E402
from tests.plane_refusals import (CELLS, GARBAGE, N, N_SLOTS, NULL, OVER, ROW, SIDE, STRIDE, Device, _combined, changed, first_difference,  # noqa: E402,F401
                                  host_seg, i32, observe_py, record_main, recorded as _recorded)

MAX_POINTS, CLOUD_STRIDE = 4096, 64
N_POINTS = i32([40, 0, 64, 40, 0, 64])                    # (host arrays hold OVER rows, as in plane_refusals)
TRANSFORMS = np.ascontiguousarray(np.tile(np.eye(3, 4).reshape(12), (OVER, 1)))
ORIGINS = np.zeros((OVER, 3), np.float32)
ALL_LAYERS, ALL_SLOPES, ALL_RASTER = (1 << len(_lib.LAYERS)) - 1, (1 << len(_lib.SLOPE_CHANNELS)) - 1, (1 << len(_lib.RASTER_CHANNELS)) - 1
TERRAIN_STRIDE = 3 * CELLS + 16
MAX_CLUSTERS = 8


# ---------------------------------------------------------------- the C calls

# the slot list of a call, through slots[] and through first_slot
SLOT_MISTAKES = [("slots[]: n > n_slots", {"n": OVER, "slots": i32([0, 1, 2, 3, 4, 5])}), ("slots[]: a slot outside", {"slots": i32([0, N_SLOTS, 2, 0, 0, 0])}),
                 ("slots[]: a slot twice", {"slots": i32([0, 1, 1, 0, 0, 0])}), ("first_slot: n > n_slots", {"n": OVER}),
                 ("first_slot: a slot outside", {"first_slot": N_SLOTS - N + 1}), ("first_slot < 0", {"first_slot": -1})]

CLOUD_VALUES = dict(n=N, first_slot=0, slots=None, point_format=_lib.GG_POINT16, cloud_stride=CLOUD_STRIDE, n_points=N_POINTS, transforms=TRANSFORMS)
CLOUD_BUFFERS = [("d_points", N * CLOUD_STRIDE * 16), ("d_labels", N * CLOUD_STRIDE), ("d_label_masks", N * CLOUD_STRIDE // 4)]
NOT_GIVEN = {"@d_label_masks": NULL}   # of the baseline: labels are given
WITH_MASKS = {"@d_labels": NULL, "@d_label_masks": "d_label_masks"}
# the checks the five cloud calls share (labelled_clouds_begin), in their order
CLOUD_MISTAKES = [("no d_points", {"@d_points": NULL}), ("no n_points", {"n_points": None}), ("point_format", {"point_format": 7}),
                  ("labels and masks", {"@d_label_masks": "d_label_masks"}), ("neither labels nor masks", {"@d_labels": NULL}),
                  ("masks with cloud_stride = 62", {**WITH_MASKS, "cloud_stride": 62}), ("cloud_stride > max_points", {"cloud_stride": MAX_POINTS + 4}),
                  *SLOT_MISTAKES, ("n_points[1] < 0", {"n_points": changed(N_POINTS, (1, -1))}),
                  ("n_points[1] > max_points", {"n_points": changed(N_POINTS, (1, MAX_POINTS + 1))}),
                  ("n_points[1] > cloud_stride", {"n_points": changed(N_POINTS, (1, CLOUD_STRIDE + 1))})]
PLANE = N * STRIDE * 4   # bytes of N planes of 4-byte words, STRIDE apart
OCCUPANCY = dict(min_points=1, min_height=-math.inf, max_height=math.inf)
OCCUPANCY_MISTAKES = [("min_points", {"min_points": 0}), ("min_height is NaN", {"min_height": math.nan})]


def _transfer(name, mask_bits, all_mask):
    """one of the three transfers: positional arguments, no struct"""
    return dict(struct=None, args=("n", "slots", "first_slot", "mask", "order", "@d_planes", "plane_stride"),
                values=dict(n=N, slots=None, first_slot=0, mask=all_mask, order=ROW, plane_stride=STRIDE), absent={},
                buffers=[("d_planes", N * mask_bits * STRIDE * 4)],
                mistakes=[("n < 0", {"n": -1}), ("mask zero", {"mask": 0}), ("mask bit beyond the last", {"mask": 1 << mask_bits}), ("order", {"order": 7}),
                          ("null planes", {"@d_planes": NULL}), ("plane_stride", {"plane_stride": CELLS - 1}), *SLOT_MISTAKES])


C_CALLS = {
    "gg_export_layers": _transfer("gg_export_layers", len(_lib.LAYERS), ALL_LAYERS),
    "gg_import_layers": _transfer("gg_import_layers", len(_lib.LAYERS), ALL_LAYERS),
    "gg_export_slopes": _transfer("gg_export_slopes", len(_lib.SLOPE_CHANNELS), ALL_SLOPES),
    "gg_export_images": dict(
        struct=_lib.GGImageExport, absent={},
        values=dict(n=N, first_slot=0, slots=None, layer_mask=ALL_LAYERS, image_stride=STRIDE, terrain_stride=TERRAIN_STRIDE, terrain_layout=_lib.GG_TERRAIN_HWC),
        buffers=[("d_images", N * len(_lib.LAYERS) * STRIDE), ("d_bounds", N * len(_lib.LAYERS) * 8), ("d_terrain", N * TERRAIN_STRIDE * 4)],
        mistakes=[("n < 0", {"n": -1}), ("mask bit beyond the last", {"layer_mask": 1 << len(_lib.LAYERS)}), ("mask without d_images", {"@d_images": NULL}),
                  ("neither a layer nor the terrain image", {"layer_mask": 0, "@d_terrain": NULL}), ("image_stride", {"image_stride": CELLS - 1}),
                  ("terrain_stride", {"terrain_stride": 3 * CELLS - 1}), ("terrain_layout", {"terrain_layout": 7}), *SLOT_MISTAKES]),
    "gg_split_clouds": dict(
        struct=_lib.GGCloudSplit, absent=NOT_GIVEN, values=dict(CLOUD_VALUES),
        buffers=CLOUD_BUFFERS + [(f"{s}.d_{k}", N * CLOUD_STRIDE * w) for s in ("ground", "nonground") for k, w in (("points", 16), ("height", 4), ("source", 4))] + [
            ("d_counts", N * 8)],
        mistakes=[("n < 0", {"n": -1}), ("no d_counts", {"@d_counts": NULL}), *CLOUD_MISTAKES]),
    "gg_rasterize_clouds": dict(
        struct=_lib.GGCloudRaster, absent=NOT_GIVEN, values=dict(CLOUD_VALUES, channel_mask=ALL_RASTER, order=ROW, plane_stride=STRIDE),
        buffers=CLOUD_BUFFERS + [("d_dst", len(_lib.RASTER_CHANNELS) * PLANE)],
        mistakes=[("n < 0", {"n": -1}), ("no d_dst", {"@d_dst": NULL}), ("mask zero", {"channel_mask": 0}),
                  ("mask bit beyond the last", {"channel_mask": 1 << len(_lib.RASTER_CHANNELS)}), ("order", {"order": 7}), ("plane_stride", {"plane_stride": CELLS - 1}),
                  *CLOUD_MISTAKES]),
    "gg_cluster_clouds": dict(
        struct=_lib.GGCloudClusters, absent=NOT_GIVEN, values=dict(CLOUD_VALUES, **OCCUPANCY, connectivity=8, order=ROW, plane_stride=STRIDE, max_clusters=MAX_CLUSTERS),
        buffers=CLOUD_BUFFERS + [("d_cell_cluster", PLANE), ("d_point_cluster", N * CLOUD_STRIDE * 4), ("d_n_clusters", N * 4), ("d_clusters", N * MAX_CLUSTERS * 32)],
        mistakes=[("n < 0", {"n": -1}), ("no d_n_clusters", {"@d_n_clusters": NULL}), *OCCUPANCY_MISTAKES, ("connectivity", {"connectivity": 6}), ("order", {"order": 7}),
                  ("plane_stride", {"plane_stride": CELLS - 1}), ("max_clusters < 0", {"max_clusters": -1}), ("d_clusters without max_clusters", {"max_clusters": 0}),
                  *CLOUD_MISTAKES]),
    "gg_clearance_clouds": dict(
        struct=_lib.GGCloudClearance, absent={**NOT_GIVEN, "@d_seeds": NULL}, values=dict(CLOUD_VALUES, **OCCUPANCY, seed_stride=0, max_cells=0, order=ROW, plane_stride=STRIDE),
        buffers=CLOUD_BUFFERS + [("d_seeds", PLANE), ("d_dist2", PLANE), ("d_nearest", PLANE), ("d_distance", PLANE), ("d_n_occupied", N * 4)],
        mistakes=[("n < 0", {"n": -1}), ("d_points and d_seeds", {"@d_seeds": "d_seeds"}), ("no d_dist2", {"@d_dist2": NULL}), ("plane_stride", {"plane_stride": CELLS - 1}),
                  ("order", {"order": 7}), ("max_cells", {"max_cells": -1}), *OCCUPANCY_MISTAKES, *CLOUD_MISTAKES[1:]]),
    # (seed mode: the same call, no cloud member set; the slot list is 0 .. n - 1)
    "gg_clearance_clouds, seeds": dict(
        call="gg_clearance_clouds", struct=_lib.GGCloudClearance,
        absent={"@d_points": NULL, "@d_labels": NULL, "@d_label_masks": NULL},
        values=dict(n=N, seed_stride=STRIDE, max_cells=0, order=ROW, plane_stride=STRIDE),
        buffers=CLOUD_BUFFERS + [("d_seeds", PLANE), ("d_dist2", PLANE), ("d_nearest", PLANE), ("d_distance", PLANE), ("d_n_occupied", N * 4)],
        mistakes=[("n < 0", {"n": -1}), ("neither d_points nor d_seeds", {"@d_seeds": NULL}), ("n_points with d_seeds", {"n_points": N_POINTS}),
                  ("transforms with d_seeds", {"transforms": TRANSFORMS}), ("d_labels with d_seeds", {"@d_labels": "d_labels"}),
                  ("d_label_masks with d_seeds", {"@d_label_masks": "d_label_masks"}), ("slots with d_seeds", {"slots": i32([0, 1, 2, 3, 0, 0])}),
                  ("seed_stride", {"seed_stride": CELLS - 1}), ("no d_dist2", {"@d_dist2": NULL}), ("plane_stride", {"plane_stride": CELLS - 1}), ("order", {"order": 7}),
                  ("max_cells", {"max_cells": -1})]),
    "gg_visibility_clouds": dict(
        struct=_lib.GGCloudVisibility, absent=NOT_GIVEN, values=dict(CLOUD_VALUES, **OCCUPANCY, origins=ORIGINS, max_cells=0, order=ROW, plane_stride=STRIDE),
        buffers=CLOUD_BUFFERS + [("d_state", PLANE), ("d_counts", N * 12)],
        mistakes=[("n < 0", {"n": -1}), ("no origins", {"origins": None}), ("no d_state", {"@d_state": NULL}), ("plane_stride", {"plane_stride": CELLS - 1}),
                  ("order", {"order": 7}), ("max_cells", {"max_cells": -1}), *OCCUPANCY_MISTAKES, *CLOUD_MISTAKES]),
}


def _layout(call):
    """the place (word offset into the arena, 256-byte aligned) of every buffer, and the words of them all"""
    place, at = {}, 0
    for field, nbytes in call["buffers"]:
        place[field] = at
        at += (nbytes + 255) // 256 * 64
    return place, at


ARENA_WORDS = max(_layout(call)[1] for call in C_CALLS.values())


def c_cases(name):
    """[(case, {field: value, "@buffer": place})] of one C call; None: the null struct"""
    call = C_CALLS[name]
    mistakes = call["mistakes"]
    cases = [("baseline", {})]
    if call["absent"].get("@d_label_masks") == NULL and "@d_points" not in call["absent"]:   # (the calls that read clouds)
        cases.append(("baseline with masks", dict(WITH_MASKS)))
    if call["struct"] is not None:
        cases.append(("null struct", None))
    cases += [(m, o) for m, o in mistakes]
    cases += [(f"{m1} + {m2}", {**o1, **o2}) for (m1, o1), (m2, o2) in zip(mistakes, mistakes[1:])]
    cases.append((f"{mistakes[0][0]} + {mistakes[-1][0]}", {**mistakes[0][1], **mistakes[-1][1]}))
    cases.append(("n > n_slots", {"n": OVER}))
    cases += [(f"n > n_slots + {m}", {**o, "n": OVER}) for m, o in mistakes if "n" not in o]
    garbage = {"@" + f: GARBAGE for f, _ in call["buffers"]}
    garbage.update({k: GARBAGE for k in ("slots", "n_points", "transforms", "origins") if (k == "slots" if call["struct"] is None else hasattr(call["struct"], k))})
    cases.append(("n = 0 + garbage", {**garbage, "n": 0, "order": 99, **{k: -7 for k in call["values"] if k.endswith("_stride")}}))
    return cases


def _set(x, field, value):
    for part in field.split(".")[:-1]:
        x = getattr(x, part)
    setattr(x, field.split(".")[-1], value)


def observe_c(dev, name, overrides):
    """[rc, gg_last_error text] of one raw call ("" with GG_OK); the arena is zero before it and the device idle after it"""
    call, L, ctx = C_CALLS[name], dev.seg._L, dev.seg._ctx
    fn = getattr(L, call.get("call", name))
    dev.arena.zero_()
    dev.torch.cuda.synchronize()
    if overrides is None:
        rc = fn(ctx, None, None)
    else:
        place, end = _layout(call)
        assert end <= dev.arena.numel()
        at = {**{"@" + f: f for f in place}, **call["absent"], **{k: v for k, v in overrides.items() if k.startswith("@")}}
        v = {**call["values"], **{k: w for k, w in overrides.items() if not k.startswith("@")}}
        v.update({k: None if w == NULL else 0x10 if w == GARBAGE else dev.arena.data_ptr() + 4 * place[w] for k, w in at.items()})
        host = lambda a, pointer: C.cast(0x10 if isinstance(a, str) else a.ctypes.data, pointer) if a is not None else None  # noqa: E731
        if call["struct"] is None:
            rc = fn(ctx, v["n"], host(v["slots"], C.POINTER(C.c_int32)), v["first_slot"], v["mask"], v["order"], v["@d_planes"], v["plane_stride"], None)
        else:
            x = call["struct"]()
            for field, value in v.items():
                if isinstance(value, (np.ndarray, str)):   # (a host array, or GARBAGE in its place)
                    value = host(value, type(getattr(x, field)))
                _set(x, field.lstrip("@"), value)
            rc = fn(ctx, C.byref(x), None)
    dev.torch.cuda.synchronize()
    return [int(rc), "" if rc == _lib.GG_OK else L.gg_last_error(ctx).decode()]


# ---------------------------------------------------------------- the Python methods

LAYERS, SLOPES, RASTER = list(_lib.LAYERS), list(_lib.SLOPE_CHANNELS), list(_lib.RASTER_CHANNELS)
CLOUD_METHODS = ("split_clouds", "rasterize_clouds", "cluster_clouds", "clearance_clouds", "visibility_clouds")


def _zeros(torch, device, dtype, *shape):
    return torch.zeros(shape, dtype=dtype, device=device)


def py_baseline(name, torch, device, b=N, host_out=False):
    """the keyword arguments of one valid call of method `name` with its tensors on `device`: every optional output asked for.  host_out: the
    outputs of the methods that would allocate before they look at a tensor are given, on `device`, so that no case depends on a device"""
    z = lambda dtype, *shape: _zeros(torch, device, dtype, *shape)  # noqa: E731
    clouds = lambda: dict(points=z(torch.uint8, b, CLOUD_STRIDE, 16), n_points=[int(v) for v in N_POINTS[:b]], labels=z(torch.uint8, b, CLOUD_STRIDE))  # noqa: E731
    kw = {
        "export_layers": lambda: dict(n=b), "export_slopes": lambda: dict(n=b),
        "import_layers": lambda: dict(planes=z(torch.float32, b, len(LAYERS), SIDE, SIDE), n=b),
        "export_images": lambda: dict(n=b, terrain=True),
        "split_clouds": clouds, "rasterize_clouds": lambda: dict(clouds(), channels=RASTER), "cluster_clouds": lambda: dict(clouds(), max_clusters=MAX_CLUSTERS),
        "clearance_clouds": clouds, "clearance_planes": lambda: dict(seeds=z(torch.int32, b, SIDE, SIDE)),
        "visibility_clouds": lambda: dict(clouds(), origins=ORIGINS[:b].copy()),
    }[name]()
    if host_out and name in ("export_layers", "export_slopes"):
        kw["out"] = z(torch.float32, b, len(LAYERS if name == "export_layers" else SLOPES), SIDE, SIDE)
    if host_out and name == "export_images":
        kw["out"] = api.ImageExport(images=z(torch.uint8, b, len(LAYERS), SIDE, SIDE), bounds=z(torch.float32, b, len(LAYERS), 2), terrain=z(torch.float32, b, SIDE, SIDE, 3))
    return kw


def _names(key, known):
    return [(f"{key} unknown", {key: ["nope"]}), (f"{key} duplicated", {key: [known[0], known[0]]}), (f"{key} out of order", {key: [known[1], known[0]]}),
            (f"{key} empty", {key: []})]


_MAX_CELLS = [("max_cells < 0", {"max_cells": -1}), ("max_cells is no integer", {"max_cells": 1.5})]
_OCCUPANCY = [("min_points", {"min_points": 0}), ("min_height is NaN", {"min_height": math.nan})]
# the parameter mistakes (name, {keyword: value}), in the order of the method's checks
PY_PARAMETER_MISTAKES = {
    "export_layers": _names("names", LAYERS),
    "export_slopes": _names("names", SLOPES),
    "import_layers": _names("names", LAYERS),
    "export_images": _names("names", LAYERS)[:3] + [("no layer and no terrain", {"names": [], "terrain": False}), ("no layer, the terrain", {"names": []})],
    "split_clouds": [],
    "rasterize_clouds": _names("channels", RASTER) + [("order", {"order": "fortran"})],
    "cluster_clouds": [("connectivity", {"connectivity": 6}), ("order", {"order": "fortran"}), ("max_clusters", {"max_clusters": -1})],
    "clearance_clouds": [("order", {"order": "fortran"})] + _MAX_CELLS + _OCCUPANCY,
    "clearance_planes": [("order", {"order": "fortran"})] + _MAX_CELLS,
    "visibility_clouds": [("order", {"order": "fortran"})] + _MAX_CELLS + _OCCUPANCY + [
        ("origins [B, 2]", {"origins": np.zeros((N, 2), np.float32)}), ("origins of another B", {"origins": np.zeros((N + 1, 3), np.float32)})],
}

# the structured `out` of a method: (its class, the flags that turn one field off, that field, two other fields)
OUTS = {
    "export_images": (api.ImageExport, dict(terrain=False), "terrain", "images", "bounds"),
    "split_clouds": (api.SplitOutputs, dict(heights=False), "ground_height", "counts", "ground_points"),
    "cluster_clouds": (api.ClusterOutputs, dict(point_clusters=False), "point_cluster", "cell_cluster", "n_clusters"),
    "clearance_clouds": (api.ClearanceOutputs, dict(nearest=False), "nearest", "dist2", "distance"),
    "clearance_planes": (api.ClearanceOutputs, dict(nearest=False), "nearest", "dist2", "distance"),
    "visibility_clouds": (api.VisibilityOutputs, dict(counts=False), "counts", "state", "counts"),
}


def _spoilt(torch, t):
    """(name, what stands in place of the valid output tensor t) for every mistake of one output"""
    wider = tuple(t.shape[:-1]) + (t.shape[-1] + 1,)
    return [("of another shape", lambda: torch.zeros(wider, dtype=t.dtype, device=t.device)),
            ("of another dtype", lambda: torch.zeros(tuple(t.shape), dtype=torch.float32 if t.dtype == torch.int32 else torch.int32, device=t.device)),
            ("on the host", lambda: t.cpu()),
            ("not contiguous", lambda: torch.zeros(tuple(t.shape[:-1]) + (2 * t.shape[-1],), dtype=t.dtype, device=t.device)[..., ::2]),
            ("no tensor", lambda: 5)]


def py_tensor_mistakes(name, torch, good):
    """the tensor and `out` mistakes of one method, (name, edit of the keyword arguments), in the order of its checks.  good: what the method
    returned for its baseline"""
    put = lambda **edits: lambda kw: kw.update(edits)  # noqa: E731
    u8 = lambda *shape: _zeros(torch, "cuda", torch.uint8, *shape)  # noqa: E731
    found = []
    if name in CLOUD_METHODS:
        found += [("points on the host", lambda kw: kw.update(points=kw["points"].cpu())), ("points of another dtype", lambda kw: kw.update(points=kw["points"].float())),
                  ("points of 24-byte records", put(points=u8(N, CLOUD_STRIDE, 24))), ("labels of another shape", put(labels=u8(N, CLOUD_STRIDE + 1))),
                  ("labels and masks", put(masks=u8(N, CLOUD_STRIDE // 4))), ("neither labels nor masks", put(labels=None)),
                  ("masks with a stride of 62", put(points=u8(N, 62, 16), n_points=[40, 0, 62], labels=None, masks=u8(N, 16)))]
    if name == "import_layers":
        found += [(f"planes {m}", (lambda make: lambda kw: kw.update(planes=make()))(make)) for m, make in _spoilt(torch, good["planes"])]
    if name == "clearance_planes":
        found += [("seeds of another shape", put(seeds=_zeros(torch, "cuda", torch.int32, N, SIDE, SIDE + 1))), ("seeds on the host", lambda kw: kw.update(seeds=kw["seeds"].cpu())),
                  ("seeds are out.dist2", lambda kw: setattr(kw.setdefault("out", api.ClearanceOutputs()), "dist2", kw["seeds"]))]
    if name in OUTS:
        cls, flags, off, a, b = OUTS[name]

        def field(f, make):
            return lambda kw: setattr(kw.setdefault("out", cls()), f, make())

        def not_asked(kw):
            kw.update(flags)
            setattr(kw.setdefault("out", cls()), off, getattr(good, off).clone())

        found.append((f"out.{off} not asked for", not_asked))
        # (the two fields take turns, so that an adjacent pair holds two mistaken fields)
        for k in range(5):
            f = (a, b)[k % 2]
            m, make = _spoilt(torch, getattr(good, f))[k]
            found.append((f"out.{f} {m}", field(f, make)))
    elif name in ("export_layers", "export_slopes", "rasterize_clouds"):
        found += [(f"out {m}", (lambda make: lambda kw: kw.update(out=make()))(make)) for m, make in _spoilt(torch, good)]
    if name in ("export_layers", "export_slopes", "import_layers"):
        K, flat = len(SLOPES if name == "export_slopes" else LAYERS), "planes" if name == "import_layers" else "out"
        found += [("flat, plane_stride = cells + 16", put(plane_stride=CELLS + 16, **{flat: _zeros(torch, "cuda", torch.float32, N * K * (CELLS + 16))})),
                  ("flat, the dense tensor", put(plane_stride=CELLS + 16, **{flat: _zeros(torch, "cuda", torch.float32, N, K, SIDE, SIDE)}))]
    return found


def _apply(kw, edits):
    for edit in edits:
        kw.update(edit) if isinstance(edit, dict) else edit(kw)
    return kw


def _lists(mistakes):
    return _combined(mistakes) if mistakes else []


def observe_cpu():
    """{case: [exception type name, message]} of the parameter mistakes, on host tensors and without the library"""
    import torch

    seen, seg = {}, host_seg()
    for name, mistakes in PY_PARAMETER_MISTAKES.items():
        for case, edits in [("baseline on the host", [])] + _lists(mistakes):
            seen[f"{name}: {case}"] = observe_py(seg, name, _apply(py_baseline(name, torch, "cpu", host_out=True), edits))
    return seen


def observe_gpu():
    """{case: [rc, text]} of the C table and {case: [exception type name, message]} of the methods' parameter, tensor and `out` mistakes, on
    the device"""
    import torch

    seen, dev = {}, Device(ARENA_WORDS)
    try:
        for name in C_CALLS:
            for case, overrides in c_cases(name):
                seen[f"{name}: {case}"] = observe_c(dev, name, overrides)
        for name, parameter in PY_PARAMETER_MISTAKES.items():
            base = py_baseline(name, torch, "cuda")
            good = base if name == "import_layers" else getattr(dev.seg, name)(**base)
            tensor = py_tensor_mistakes(name, torch, good)
            lists = [("baseline", [])] + _lists(parameter) + _lists(tensor)
            if name in CLOUD_METHODS:
                lists.append(("baseline with masks", [dict(labels=None, masks=_zeros(torch, "cuda", torch.uint8, N, CLOUD_STRIDE // 4))]))
            if parameter and tensor:  # (a parameter mistake comes before a tensor mistake: the last of the one list with the first of the other)
                lists.append((f"{parameter[-1][0]} + {tensor[0][0]}", [parameter[-1][1], tensor[0][1]]))
            for case, edits in lists:
                seen[f"{name}: {case}"] = observe_py(dev.seg, name, _apply(py_baseline(name, torch, "cuda"), edits))
                torch.cuda.synchronize()
            seen[f"{name}: B > n_slots"] = observe_py(dev.seg, name, py_baseline(name, torch, "cuda", OVER))
            torch.cuda.synchronize()
    finally:
        dev.close()
    return seen


def recorded(which):
    return _recorded(which, "cloud_refusals")


if __name__ == "__main__":
    record_main("cloud_refusals", observe_cpu, observe_gpu)
