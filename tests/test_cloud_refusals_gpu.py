"""The refusals of the nine map and cloud calls on the device against their recording, tests/golden/cloud_refusals_gpu.json: the return
code and gg_last_error text of every raw C call of the table (single mistakes, adjacent pairs, n beyond n_slots with each, n = 0 with
garbage, the null struct), and the exception and message of the methods' parameter, tensor and `out` mistakes (tests/cloud_refusals.py).
One 20 x 20 context with 4 slots."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import cloud_refusals  # noqa: E402

pytestmark = pytest.mark.gpu


def test_the_calls_refuse_what_the_recording_says_in_its_words():
    want = cloud_refusals.recorded("gpu")
    codes = {v[0] for v in want.values()}
    assert len(want) >= 800 and {0, -1, -5, "", "ValueError", "AssertionError", "GroundGridError"} <= codes
    assert cloud_refusals.first_difference(cloud_refusals.observe_gpu(), want) is None
