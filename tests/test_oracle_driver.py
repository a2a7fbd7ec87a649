"""The oracle's batch driver (oracle/orc_batch.h: reset(mask), step and rollout in NEXT_STEP, SAME_STEP and DISABLED, final_obs,
invalid actions, episode statistics across resets) against tests/golden/oracle_driver.json, the recording that
tests/golden/gen/gen_oracle_driver.py took from the eight per-file drivers before they became one header (no GPU).  The script of
a run is the generator's record_run(); every call's outputs are compared through one digest, whole lists at a time, so a mismatch
names the case, the mode and the first differing call."""
import importlib.util
import os

import pytest

from conftest import golden
from test_oracle_hash_rollout import CASES

_spec = importlib.util.spec_from_file_location("_gen_oracle_driver", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gen", "gen_oracle_driver.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def recorded():
    return golden("oracle_driver.json")


def test_the_recording_has_all_51_runs(recorded):
    assert sorted(recorded) == sorted(f"{case}/{mode}" for case in CASES for mode in gen.MODES) and len(recorded) == 51


@pytest.mark.parametrize("mode", gen.MODES)
@pytest.mark.parametrize("case", list(CASES))
def test_driver_replays_the_recording(oracle, recorded, case, mode):
    calls, done = gen.record_run(oracle, case, mode)
    if mode != "DISABLED":
        assert done.min() >= 2, "every env finishes at least two episodes within the stepped part"
    want = recorded[f"{case}/{mode}"]
    first = next((k for k, (a, b) in enumerate(zip(calls, want)) if a != b), min(len(calls), len(want)))
    assert calls == want, f"{case}/{mode}: first differing call #{first}: got {calls[first:first + 1]}, recorded {want[first:first + 1]}"
