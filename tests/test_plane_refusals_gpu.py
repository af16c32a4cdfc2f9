"""The refusals of the six plane calls on the device against their recording, tests/golden/plane_refusals_gpu.json: the return code and
gg_last_error text of every raw C call of the table (single mistakes, adjacent pairs, n beyond n_slots with each, n = 0 with garbage,
every pair of buffers laid over each other at the first word, the last word and one word past it), and the exception and message of the
methods' tensor, `out` and host-array mistakes (tests/plane_refusals.py).  One 20 x 20 context with 4 slots."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import plane_refusals  # noqa: E402

pytestmark = pytest.mark.gpu


def test_the_calls_refuse_what_the_recording_says_in_its_words():
    want = plane_refusals.recorded("gpu")
    codes = {v[0] for v in want.values()}
    assert len(want) >= 700 and {0, -1, -5, "", "ValueError", "GroundGridError"} <= codes
    assert plane_refusals.first_difference(plane_refusals.observe_gpu(), want) is None
