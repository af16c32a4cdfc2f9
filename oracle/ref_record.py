"""Records tests/golden/ref_build_digests.json (TEST INFRASTRUCTURE): every scene of tests/ref_scenes.py through oracle/_ref/gg_ref_run
-- the reference's own translation unit compiled against stand-ins -- and NOTHING ELSE: neither libgg_oracle.so nor the HIP library
computes a result here.  Two INPUTS do come by way of the oracle, and only inputs: the generators of tests/edge_scenes.py ask it for a
map's length and resolution when they place points on cell borders, and the four golden/* scenes take their clouds and parameters
out of tests/golden/*.npz, files the oracle wrote (the arrays of results in them are not read here).  Per scene: a digest of its inputs (so that a drifting generator is named as such) and, per frame, digests of the
labels, the order and the bytes of the returned cloud and of each of the 11 layers.

    python -m oracle.ref_record          (needs the reference on this machine: oracle/ref_build.py)

The file is data: results the reference build wrote while it ran.  It travels to machines without the reference, where the
oracle (CPU) and the HIP path (GPU) are held to it.
"""
from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_build  # noqa: E402


def record() -> dict:
    from tests import ref_scenes as rs

    ref_build.build()
    scenes = {}
    for name in rs.names():
        scene = rs.scene(name)
        # (rs.run_reference: the configuration goes to the scenario as plain numbers -- ref.Scenario's defaults edited, no oracle involved --
        # and a scene that carries a pair of the two compile-time constants runs through the binary compiled with that pair)
        frames = [rs.frame_digest(out, layers) for out, layers in rs.run_reference(scene)]
        scenes[name] = {"input": rs.input_digest(scene), "points": int(len(scene.cloud)), "frames": frames}
        print(f"{name}: {len(scene.cloud)} points, {len(frames)} frames", flush=True)
    return {
        "what": "SHA-256 (first 16 hex digits) of what oracle/_ref/gg_ref_run returned and left in the map, per scene and frame (one line per "
                "frame; a later frame lists only what differs from the frame before); written by oracle/ref_record.py from the "
                "reference build alone",
        "conventions": {"eigen": "GG_EIGEN_33", "rotation": "kdl"},
        "excluded": rs.EXCLUDED,
        "scenes": scenes,
    }


if __name__ == "__main__":
    from tests import ref_scenes

    doc = record()
    ref_scenes.dump_digests(doc)
    print(f"wrote {ref_scenes.DIGESTS}: {len(doc['scenes'])} scenes, {sum(len(s['frames']) for s in doc['scenes'].values())} frames")
