"""The token encoder computes the recorded bits: SHA-256 digests of y, dx and the parameter gradient of a 2-layer stack
(tools/token_encoder_dump.py: its cases, inputs and parameters) against tests/golden/token_encoder_bits.json, which was
recorded on the MI355X from the commit before the encoder's formulas moved into csrc/token_math.h (two dumps there gave
the same digests).  Eval mode and train mode (dropout 0.1), the one-launch kernels and the launch-per-operation path.
Neither path has atomics and both sum in fixed orders: exact equality, no tolerance."""
import json
import os

import pytest

from tools import token_encoder_dump as D

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "token_encoder_bits.json")


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def test_fixture_covers_every_case_mode_and_path():
    gold = _golden()
    assert sorted(gold) == sorted(D.case_id(B, S) for B, S in D.CASES)
    for case in gold.values():
        assert sorted(case) == sorted(D.MODES)
        for mode in case.values():
            assert sorted(mode) == sorted(D.PATHS)
            for path in mode.values():
                assert sorted(path) == ["dx", "grad", "y"] and all(len(v) == 64 for v in path.values())


@pytest.mark.parametrize("B,S", D.CASES)
def test_reproduces_the_recorded_digests(B, S):
    want = _golden()[D.case_id(B, S)]
    got = D.run_case(B, S)
    bad = [(mode, path, k) for mode in want for path in want[mode] for k in want[mode][path]
           if got[mode][path][k] != want[mode][path][k]]
    assert not bad, bad
