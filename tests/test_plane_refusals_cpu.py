"""The parameter refusals of the six plane methods (fuse_states, route_planes, match_planes, footprint_planes, route_headings,
track_clusters) against their recording, tests/golden/plane_refusals_cpu.json: which check answers and with which words, for every single
mistake, every adjacent pair and the first with the last (tests/plane_refusals.py).  Host tensors and no library: nothing reaches a device."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from groundgrid_amd import build  # noqa: E402
from tests import plane_refusals  # noqa: E402


def test_the_methods_refuse_what_the_recording_says_in_its_words():
    build.build()  # (GroundSegmentation() loads the library; no case calls into it)
    want = plane_refusals.recorded("cpu")
    assert len(want) >= 90 and all(v[0] == "ValueError" for v in want.values())
    assert plane_refusals.first_difference(plane_refusals.observe_cpu(), want) is None
