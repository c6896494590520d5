"""The entries that run the host side's batched attention reproduce their recorded output bits (pytest -m gpu): car_encode_control, car_t5_encode, both
CLIP towers, car_score and car_generate (teacher-forced) on synthetic weights, both arithmetic modes, against the SHA-256 digests of
tests/golden/encoder_bits.json (minted by tests/golden/make_encoder_bits.py; two mints in separate processes agreed on every key).  The parity tests
bound the distance to the reference; this one pins the bits, so that a change which is meant to leave the arithmetic alone — moving host code between
files, for one — can show that it did.  car_depth's attention is pinned by test_extractor_bits_gpu.py."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_every_encoder_output_reproduces_its_recorded_digest():
    sys.path.insert(0, GOLDEN)
    try:
        import make_encoder_bits as mk
    finally:
        sys.path.remove(GOLDEN)
    with open(os.path.join(GOLDEN, "encoder_bits.json")) as f:
        want = json.load(f)
    got = mk.digests()
    assert sorted(got) == sorted(want)
    assert len(want) == mk.N_KEYS == 48
    assert {k.split("/")[0] for k in want} == {"encode_control", "t5_encode", "clip_encode_image", "clip_encode_text", "score", "generate"}
    differ = [k for k in sorted(want) if got[k] != want[k]]
    assert not differ, differ
