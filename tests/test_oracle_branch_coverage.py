"""Which branches of the oracles' dynamics do the GPU tests' action streams reach?  (No GPU.)

Every kernel is pinned to its oracle, but only along the trajectories the tests' actions produce; a dynamics branch no stream enters
is a branch where the kernel could be wrong unnoticed.  This test builds a copy of oracle/ with gcc --coverage, replays on the
oracles alone every stream of tests/_action_streams.py, every reference fixture the GPU tests replay and every directed scenario
(tests/_directed_scenarios.py) in one child process, and runs `gcov -b -c` on the counters.  Every line of env_step, write_obs, the
per-env reset and their static helpers in the eight orc_<env>.c that was never executed, or has a branch outcome never taken, must
be on tests/golden/oracle_unreachable.json, where each entry says why no test can reach it: the device refuses the configuration,
the line handles a failed allocation, another test reaches it by state injection, or arithmetic makes the arm impossible (with the
argument); one entry is a stated probability bound, marked as such.  A new unreached line means: write a scenario for it (test_directed_scenarios_gpu.py), or argue it onto the list.
profiles/oracle_branch_coverage.txt records the list under the streams alone, before the scenarios existed, and after them."""
import json
import os
import shutil

import pytest

import _oracle_coverage as cov

# the four kinds of reason, and one more that is not a reason of those kinds and is kept apart so that "arithmetic" keeps meaning
# impossible: an arm whose probability per step is bounded, with the bound derived in the entry, that no seed search can find and no
# state injection can reach yet (climate has no set_state)
KINDS = {"device_refuses", "resource_failure", "state_injection", "arithmetic", "probability_bound"}


def _allowed():
    with open(os.path.join(cov.HERE, "golden", "oracle_unreachable.json")) as f:
        return json.load(f)


def test_unreachable_list_is_well_formed():
    entries = _allowed()
    keys = [(e["file"], e["function"], e["line"]) for e in entries]
    assert len(set(keys)) == len(keys), "an entry is listed twice"
    for e in entries:
        assert e["kind"] in KINDS, e
        assert len(e["reason"].split()) >= 8, ("a reason is an argument, not a label", e)
        assert cov.is_dynamics(e["function"]), e
        with open(os.path.join(cov.ROOT, "oracle", e["file"])) as f:
            assert any(ln.strip() == e["line"] for ln in f), ("the listed line is no longer in the source", e)
        if e["kind"] == "device_refuses":
            assert ".hip:" in e["reason"], ("cite the refusing line", e)
        if e["kind"] == "probability_bound":
            assert "p <" in e["reason"] and "sigma" in e["reason"], ("state the bound", e)
        assert isinstance(e["outcomes"], int) and e["outcomes"] >= 1, e
        if e["kind"] == "state_injection":
            assert "::test_" in e["reason"], ("name the test", e)


@pytest.mark.skipif(shutil.which("gcc") is None or shutil.which("gcov") is None, reason="needs gcc and gcov on PATH (neither is a Python package)")
def test_every_unreached_dynamics_line_is_argued_unreachable(tmp_path):
    work = str(tmp_path)
    cov.build_copy(work)
    cov.replay(work)                                           # streams, fixtures, scenarios; the scenarios assert their events
    unreached = cov.unreached(work)
    allowed = {(e["file"], e["function"], e["line"]) for e in _allowed()}
    extra = {k: v for k, v in unreached.items() if k not in allowed}
    assert not extra, "dynamics lines no stream, fixture or scenario reaches, and not argued unreachable:\n" + cov.format_lines(extra)
    # keys are lines, so a listed line could lose a further outcome unnoticed: each entry also records how many outcomes were unreached
    listed = {(e["file"], e["function"], e["line"]): e["outcomes"] for e in _allowed()}
    grown = {k: v for k, v in unreached.items() if v[1] > listed[k]}
    assert not grown, "listed lines with more unreached outcomes than the list records:\n" + cov.format_lines(grown)
    stale = allowed - set(unreached)
    assert not stale, "listed as unreachable, but reached: take them off tests/golden/oracle_unreachable.json\n" + "\n".join(map(str, sorted(stale)))
