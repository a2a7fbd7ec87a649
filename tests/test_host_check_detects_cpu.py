"""Would the record-lane host checks report a wrong fixture?  (No GPU.)

tools/probes/{airline,emergency,space_station,farm}_host_check.cpp are the only check of csrc/<type>_env.hpp that runs without a GPU,
and every other test only sees them print `0 mismatching steps` on the right files.  Here one fixture of each type is written with one
bit of one element flipped, once for every field the type records (and once with the last recorded reset row dropped, from
`reset_index` and `reset_obs` alike so that the other rows keep their numbers), and the program must exit 1 with a summary line that
counts a mismatching step.  A poke table that names a field the type does not have must end the run with status 2.  The unedited files
give status 0.  The files are edited through the `edit` hook of tools/probes/lane_host_check.py::write_fixture."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "probes"))

# kind -> (fixture, [n, T], recorded resets, the fields it records beyond the common ones)
CASES = {
    "airline": ("airline_cancel", (16, 60), 58, ()),
    "emergency": ("emergency_timeout", (16, 150), 18, ()),
    "space_station": ("station_evacuate", (8, 80), 12, ("info0", "truncated")),
    "farm": ("farm_bankrupt", (8, 100), 8, ("info0",)),
}
COMMON = ("obs0", "obs_xor", "reward", "terminated", "info", "reset_obs", "reset_index")
POKED = {"space_station": "station_poked", "farm": "farm_poked"}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """program(kind) -> (the kind's host check module, its program, a directory for its files); each program is built once"""
    built = {}

    def get(kind):
        if kind not in built:
            hc = importlib.import_module(kind + "_host_check")
            d = str(tmp_path_factory.mktemp(kind))
            built[kind] = (hc, hc.build(d), d)
        return built[kind]
    return get


def flip(field):
    """edit(arrays): one bit of one element of the field, in the middle of the array"""
    def edit(z):
        if field == "reset_index":                                  # the last recorded reset row is gone
            z["reset_index"], z["reset_obs"] = z["reset_index"][:-1], z["reset_obs"][:-1]
            return
        a = np.ascontiguousarray(z[field])
        bits = a.reshape(-1).view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
        bits[bits.size // 2] ^= 1
        z[field] = a
    return edit


def run(program, kind, name, edit=None):
    hc, exe, d = program(kind)
    out = subprocess.run([exe, hc.write_fixture(name, d, edit=edit)], capture_output=True, text=True)
    return out.returncode, out.stdout.strip().split("\n")[-1]


@pytest.mark.parametrize("kind", list(CASES))
def test_unedited_fixture_passes(program, kind):
    name, (n, T), resets, _ = CASES[kind]
    seen = {}
    status, summary = run(program, kind, name, edit=lambda z: seen.update(shape=z["reward"].shape, resets=len(z["reset_index"]), fields=set(z)))
    assert seen["shape"] == (n, T) and seen["resets"] == resets
    assert {"info0", "truncated"} & seen["fields"] == set(CASES[kind][3]), "every field the fixture records has a case below"
    assert status == 0 and summary.endswith(f": {n} envs x {T} steps, 0 mismatching steps"), summary


@pytest.mark.parametrize("kind,field", [(kind, field) for kind, case in CASES.items() for field in COMMON + case[3]])
def test_one_flipped_bit_is_reported(program, kind, field):
    status, summary = run(program, kind, CASES[kind][0], edit=flip(field))
    assert status == 1, (status, summary)
    assert summary.endswith(" mismatching steps") and not summary.endswith(" 0 mismatching steps"), summary


@pytest.mark.parametrize("kind", list(POKED))
def test_unknown_poke_name_is_refused(program, kind):
    def rename(z):
        names = json.loads(str(z["poke_fields"]))
        names[int(z["pokes"][0, 2])] = "no_such_field"              # a name that the first poke uses
        z["poke_fields"] = np.array(json.dumps(names))
    assert run(program, kind, POKED[kind])[0] == 0
    status, summary = run(program, kind, POKED[kind], edit=rename)
    assert status == 2 and summary == "no field no_such_field", (status, summary)
