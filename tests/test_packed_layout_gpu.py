"""The packed weight images reproduce their recorded bits (pytest -m gpu): every entry car_export_packed writes for three contexts (fp32 and bf16 with
every model family, bf16 + decode_weight_fp8 with the GPT alone) against tests/golden/packed_digests.json, which tests/golden/make_packed_digests.py
minted on the build of the commit recorded in the file.  No other test looks at a weight image directly: a wrong index in car_load_tensor would
otherwise only show as a parity failure three stages later."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_every_packed_entry_reproduces_its_recorded_digest():
    sys.path.insert(0, GOLDEN)
    try:
        import make_packed_digests as mk
    finally:
        sys.path.remove(GOLDEN)
    with open(os.path.join(GOLDEN, "packed_digests.json")) as f:
        golden = json.load(f)
    assert len(golden["parent"]) == 40
    want = golden["contexts"]
    got = mk.digests()
    assert sorted(got) == sorted(want) == sorted(mk.CONTEXTS)
    for ctx in sorted(want):
        assert sorted(got[ctx]) == sorted(want[ctx]), (ctx, sorted(set(got[ctx]) ^ set(want[ctx])))
        differ = {k: (got[ctx][k], want[ctx][k]) for k in sorted(want[ctx]) if got[ctx][k] != want[ctx][k]}      # kind, shape, numel, bytes, sha256[:16]
        assert not differ, (ctx, differ)
