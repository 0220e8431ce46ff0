"""The two augmentation kernels compute the recorded bits: SHA-256 digests of every output tensor of
torch.ops.mi355ppo.image_pair_augment and tactile_augment (tools/augment_dump.py: its cases and inputs) against
tests/golden/augment_bits.json, which was recorded on the MI355X from the commit before the per-pixel chain moved into
csrc/aug_pixel.h (two dumps there gave the same digests).  Neither kernel has atomics and the tactile mean is summed in a
fixed order: exact equality, no tolerance."""
import json
import os

import pytest
import torch

from tools import augment_dump as D

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment_bits.json")


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def test_fixture_covers_every_case():
    gold = _golden()
    assert sorted(gold) == sorted(D.CASES)
    for name, case in gold.items():
        assert sorted(case) == (["img", "seg"] if name in D.CAMERA else ["out"]) and all(len(v) == 64 for v in case.values())


def test_the_cases_are_the_existing_tests_inputs():
    """the camera angles are tests/img_augment_ref.py's; every tactile case with its stages on holds all four kinds of
    image (asserted where the inputs are built)"""
    from tests import img_augment_ref as R
    assert torch.equal(D.camera_inputs("cam_54x96_on")[4], R.rot_angles())
    for name, (_, _, on, _) in D.TACTILE.items():
        jitter, angles = D.tactile_inputs(name)[3:5]
        assert bool((jitter[:, 0] != 0).any()) == bool((angles != 0).any()) == on


@pytest.mark.parametrize("name", D.CASES)
def test_reproduces_the_recorded_digests(name):
    assert D.run_case(name) == _golden()[name]
