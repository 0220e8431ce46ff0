"""The augmentation transforms keep their random stream: SHA-256 digests (dtype, shape and bytes) of every tensor, and
the seed, that ``SyncTransform.draw(3, 2)``, ``SyncEvalTransform.draw(3, 2)`` and ``TactileAugment.draw(18)`` (train and
eval) return from ``torch.Generator().manual_seed(k)``, stages on and each stage off in turn, against
tests/golden/augment_draws.json, recorded (tools/augment_dump.py --draws) from the commit before the draws moved into
module-level helpers.  The number the generator gives after each ``draw`` is recorded too: an extra or a missing draw
moves it.  Exact equality."""
import json
import os

import pytest

from tools import augment_dump as D

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment_draws.json")


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def test_fixture_covers_every_configuration_and_seed():
    gold = _golden()
    assert sorted(gold) == sorted(D.draw_configs())
    for name, case in gold.items():
        assert sorted(case) == sorted(str(k) for k in D.DRAW_SEEDS)
        assert all(len(v["draws"]) == (4 if name.startswith("sync") else 5) for v in case.values())


@pytest.mark.parametrize("name", sorted(_golden()))
def test_draws_and_the_generator_state_are_the_recorded_ones(name):
    assert D.run_draw(D.draw_configs()[name]) == _golden()[name]


def test_a_stage_that_is_off_draws_nothing():
    """the recorded streams themselves: evaluation leaves the generator where it was, and so does a train transform without
    a stage to draw for"""
    import torch
    gold = _golden()
    for k in D.DRAW_SEEDS:
        untouched = torch.rand(1, generator=torch.Generator().manual_seed(k), dtype=torch.float64).item().hex()
        assert gold["sync_eval"][str(k)]["next"] == gold["tactile_eval"][str(k)]["next"] == untouched
        assert gold["sync_on"][str(k)]["next"] != untouched and gold["tactile_on"][str(k)]["next"] != untouched
