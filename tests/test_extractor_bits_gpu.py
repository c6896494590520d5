"""The control extractors reproduce their recorded output bits (pytest -m gpu): car_hed, car_depth and car_lineart on the inputs and synthetic weights
of the committed fixtures, both arithmetic modes, map and control tensor, against the SHA-256 digests of tests/golden/extractor_bits.json
(minted by tests/golden/make_extractor_bits.py).  The parity tests bound the distance to the reference; this one pins the bits, so that a change which
is meant to leave the arithmetic alone can show that it did."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_every_extractor_output_reproduces_its_recorded_digest():
    sys.path.insert(0, GOLDEN)
    try:
        import make_extractor_bits as mk
    finally:
        sys.path.remove(GOLDEN)
    with open(os.path.join(GOLDEN, "extractor_bits.json")) as f:
        want = json.load(f)
    got = mk.digests()
    assert sorted(got) == sorted(want)
    assert len(want) == 2 * 2 * (len(mk.HED_CASES) + len(mk.LINEART_CASES) + len(mk.DEPTH_CASES))
    differ = [k for k in sorted(want) if got[k] != want[k]]
    assert not differ, differ
