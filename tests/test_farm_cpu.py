"""CPU-side checks of the agricultural-farm env: the model (tests/farm_model.py) reproduces, bit for bit, what the unmodified reference
recorded (tests/golden/farm_*.npz, written by tests/golden/gen/gen_farm.py), the autoreset observations and the stepping past
termination included; the kernels' own dynamics code, built for the host, does too, sums its means in NumPy's order, carries Python's
stage durations and draws the two streams as NumPy and CPython do; the C ABI is declared, exported and bound; there is no CPU path;
the spaces are the reference's; no kernel of the type uses scratch."""
import json
import os
import random
import re
import subprocess
import sys
import types

import numpy as np
import pytest

import _lane_kit as kit
import farm_model as fm
from _lane_kit import bits
from conftest import ROOT, golden

OLD_FIXTURES = ["farm_hash.npz", "farm_bankrupt.npz", "farm_orchard.npz", "farm_chores.npz", "farm_overrun.npz", "farm_two_years.npz"]
FIXTURES = OLD_FIXTURES + ["farm_soil.npz", "farm_poked.npz"]
SPEC = types.SimpleNamespace(
    m=fm, kind="farm", env="AgriculturalFarmVectorEnv", model=fm.FarmModel, model_kw=dict(width=fm.LIVE), limit="max_years", actions=45,
    fixtures=FIXTURES, poked="farm_poked.npz", recorded=fm.LIVE,
    info_keys=list(fm.INFO) + [f"{k}_{f}" for k in fm.FIELD_INFO for f in range(4)],      # the eleven values and field_status
    config=("FarmConfig", 16, ["autoreset_mode", "max_years", "compact_obs", "reserved"]), abi=kit.ABI, mangled="3cge4farm")
HOST_CHECK = kit.host_check(SPEC)


@pytest.mark.parametrize("name", FIXTURES)
def test_model_reproduces_the_reference(name):
    kit.model_reproduces_the_reference(SPEC, name)


def test_model_pads_the_row_with_zeros():
    m = fm.FarmModel([3, 4])
    row = m.reset()
    assert row.shape == (2, 620) and row.dtype == np.float32 and not row[:, 134:].any() and row[:, :134].any()
    assert np.array_equal(bits(row[:, :134]), bits(fm.FarmModel([3, 4], width=134).reset()))


def test_fixtures_cover_what_they_are_for():
    h, b, o, c, ov, ty = (golden(f) for f in OLD_FIXTURES)
    ev = {f: json.loads(str(z["events"])) for f, z in zip(OLD_FIXTURES, (h, b, o, c, ov, ty))}
    assert h["reward"].shape == (8, 400) and b["reward"].shape == (8, 100) and o["reward"].shape == (4, 400) and c["reward"].shape == (4, 400)
    assert ov["reward"].shape == (4, 400) and ty["reward"].shape == (4, 730)
    assert h["actions"].min() == 0 and h["actions"].max() == 44 and (b["actions"] == 40).all()
    assert int(ty["max_years"]) == 2 and all(int(z["max_years"]) == 1 for z in (h, b, o, c, ov))
    # farm_hash: an end at day 360 followed by an autoreset, a random.choice in every planting season, frost, a long drought, a
    # negative observed health, a reset observation that carries a changed water_quality
    hv = ev["farm_hash.npz"]
    assert hv["year_end"] >= 1 and min(hv["choice_spring"], hv["choice_summer"], hv["choice_fall"]) >= 1 and hv["plant_winter"] >= 1
    assert hv["frost_high"] >= 1 and hv["drought_long"] >= 1 and hv["negative_health"] >= 1 and hv["invalid_fifth_field"] >= 1
    assert hv["year_end"] + hv["bankrupt"] == len(h["reset_index"]) == int(h["terminated"].sum()) and hv["soil_end"] == 0
    ends = h["info"][h["terminated"].astype(bool)]
    assert (ends[ends[:, 2] == 2][:, 0] == 360).all() and (ends[:, 2] == 2).sum() == hv["year_end"]      # year 2 begins at day 360
    hobs = fm.fixture_obs(h)
    assert (hobs[..., 2:60:15] < 0).any() and (hobs[..., 65] > 0.5).any() and (hobs[..., 66] > np.float32(20 / 30.0)).any()
    assert (h["reset_obs"][:, 122] != np.float32(0.9)).sum() == hv["carried_water_quality"] >= 1
    assert (h["reset_obs"][:, 69] == 0).all() and (h["reset_obs"][:, 125] == 0.5).all()    # day 0, cash 50000 / 100000
    # farm_bankrupt: action 40 only; every env bankrupt at day 80 or 81 with -5000 and reset once; water_quality, which action 40
    # never changes, is the constructor's in the reset observation
    bv = ev["farm_bankrupt.npz"]
    assert bv["bankrupt"] == 8 == len(b["reset_index"]) and sorted(set(b["reset_index"][:, 0])) == list(range(8))
    assert set(b["reset_index"][:, 1]) <= {79, 80}                                         # the step that makes the day 80 or 81
    at = b["terminated"].astype(bool)
    assert (b["reward"][at] <= -5000).all() and (b["info"][at][:, 3] < -50000).all() and (b["reset_obs"][:, 122] == np.float32(0.9)).all()
    # farm_orchard: field 3 planted and harvested by hand and by the automatic harvest, replanted with and without the rotation bonus
    ov_ = ev["farm_orchard.npz"]
    assert min(ov_["harvest_action"], ov_["harvest_auto"], ov_["replant_bonus"], ov_["replant_no_bonus"], ov_["replant_after_wheat"]) >= 1
    assert set(np.unique(o["actions"])) == {3, 8} and (o["actions"][:, 0:100:2] == 3).all() and (o["actions"][:, 1:100:2] == 8).all() and (o["actions"][:, 100:200] == 3).all()
    # farm_chores: refusals, over-fertilisation, a sale taken and one refused, action 43 with and without three truthy crop types.
    # Nothing is ever repaired in these six: maintenance_needed stays below 0.5 in the reference (0.2 at most, plus 0.02 for each of
    # the at most ten operations a tank allows); farm_poked.npz sets it from outside.
    cv = ev["farm_chores.npz"]
    assert min(cv["fert_refused"], cv["over_fertilised"], cv["pest_refused"], cv["equipment_refused"], cv["sale_taken"], cv["sale_refused"],
               cv["rotation_three"], cv["rotation_fewer"]) >= 1 and cv["year_end"] >= 1 and cv["carried_water_quality"] >= 1
    assert all((fm.fixture_obs(z)[..., 73:110:5] < 0.5).all() for z in (h, b, o, c, ov, ty))
    chores = {10, 11, 12, 13, 15, 16, 17, 18, 20, 21, 22, 23, 25, 26, 27, 28, 29, 30, 31, 32, 33, 35, 36, 37, 38, 39, 41, 42, 43, 44}
    assert set(np.unique(c["actions"])) == chores | {3} and (c["actions"][:, [31, 211]] == 3).all() and (c["actions"][:, 0:30:2] == np.array(sorted(chores))[:15]).all()
    # farm_overrun: stepped on past termination
    assert ov["terminated"].any() and len(ov["reset_index"]) == 0 and not ov["terminated"][:, 0].any() and (ov["terminated"].sum(1) >= 30).all()
    # farm_two_years: the second year's climate shift, an end at day 720
    tv = ev["farm_two_years.npz"]
    assert tv["climate_temperature"] >= 1 and tv["year_end"] >= 1
    ends = ty["info"][ty["terminated"].astype(bool)]
    assert (ends[ends[:, 2] == 3][:, 0] == 720).all() and (ends[:, 2] == 3).sum() == tv["year_end"] and (ty["info"][..., 2] == 2).any()
    for z in (h, b, o, c, ov, ty):
        assert not z["terminated"][:, 0].any() and z["reward"].dtype == np.float64 and np.array_equal(z["reward"], np.round(z["reward"]))
        assert np.abs(z["reward"]).max() < 2 ** 24                                         # integers a float32 holds exactly
    # farm_soil: field 3 planted, organic matter driven to its floor by action 42 (a mean below 0.02), then biodiversity above 0.7
    so, pk = golden("farm_soil.npz"), golden("farm_poked.npz")
    sv, pv = json.loads(str(so["events"])), json.loads(str(pk["events"]))
    assert so["reward"].shape == (4, 64) and "pokes" not in so and sv["soil_low"] >= 1 and sv["biodiversity_high"] >= 1 and sv["soil_end"] == 0
    assert (so["actions"][:, 0] == 3).all() and (so["actions"][:, 1:41] == 42).all() and (so["actions"][:, 41:] == 41).all()
    sobs = fm.fixture_obs(so)
    om = sobs[..., 11:60:15].astype(np.float64) / 10                                       # the observed organic matter of the four fields
    assert (om.mean(-1) < 0.0199).sum() >= 1 and (om >= np.float32(0.1) / 10 - 1e-9).all() and (so["info"][..., 9] > 0.7).sum() == sv["biodiversity_high"]
    assert ((so["reward"] <= -1500) & (so["info"][..., 9] <= 0.7)).any()                   # the -2000 of a mean below 0.02, before the +500 of action 41
    # farm_poked: what the reference's own arithmetic keeps out of reach from reset(), set on its env object between steps: two
    # machines above 0.5 and 0.8 maintenance_needed (one refused, both paid for, both repaired), a spray at a pest level above 1,
    # excessive_rain_days held at 7 under action 40, and field 3 harvested by hand in all four arms of the yield ratio
    assert pk["reward"].shape == (4, 80) and pk["pokes"].shape[1] == 4 and len(pk["pokes"]) >= 4 * (2 + 1 + 12)
    assert min(pv[k] for k in ("maintenance_repair", "maintenance_refused", "maintenance_cost", "rain_protection", "excessive_rain_penalty", "severe_pest",
                               "harvest_5000", "harvest_2000", "harvest_1000", "harvest_poor")) >= 1
    assert pv["harvest_action"] == pv["harvest_field_3"] == 4 and pv["maintenance_repair"] == 8 and pv["soil_end"] == 0
    names = json.loads(str(pk["poke_fields"]))
    assert set(names) == {"f1.pest", "f3.health", "f3.yp", "maint0", "maint1", "rain_days"}
    assert (pk["pokes"][:, 0] < 4).all() and (pk["pokes"][:, 1] < 80).all() and (pk["pokes"][:, 2] < len(names)).all()
    pobs = fm.fixture_obs(pk)
    assert (pobs[:, 10:12, 73] > 0.5).all() and (pobs[:, 10:12, 78] > 0.8).all() and (pobs[:, 12, 73:110:5] < 0.5).all()      # repaired at step 12
    assert (pk["reward"][:, 12] >= 60 - 600).all() and (pobs[..., 67] > 0.5).sum() == pv["excessive_rain"]
    assert (pk["actions"] == 8).sum() == 4 and ((pk["actions"] == 8).sum(1) == 1).all()   # one harvest by hand per env
    # the older files hold none of this
    assert all(v["maintenance_repair"] == 0 and v["excessive_rain"] == 0 and v["soil_end"] == 0 for v in ev.values())
    for f in FIXTURES:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) < 1 << 20


def test_hash_actions_equal_the_shared_hash():
    kit.hash_actions_equal_the_shared_hash(SPEC)


def test_kernel_dynamics_replay_the_fixtures_on_the_host():
    """csrc/<type>_env.hpp compiled for the CPU and replayed over every fixture, bit for bit (tools/probes/<type>_host_check.py): the test
    fails, it does not skip, where no host compiler is there"""
    kit.kernel_dynamics_replay_the_fixtures_on_the_host(SPEC)


def test_mean_of_four_is_summed_in_numpys_order():
    """np.mean over the four fields' organic matter and compaction: below eight values a plain loop.  The host build of mean4 and the
    model's against np.mean on 5,000 random vectors, every one bit for bit."""
    rng = np.random.default_rng(4)
    v = 0.04 + rng.uniform(-0.03, 0.06, (5000, 4)) * rng.uniform(0.0, 1.0, (5000, 1))
    v[:200] = 0.045 + rng.uniform(-1e-16, 1e-16, (200, 4))
    want = np.array([np.mean(list(row)) for row in v])
    tree = np.array([((row[0] + row[1]) + (row[2] + row[3])) / 4.0 for row in v])
    assert (tree != want).sum() > 100                                                      # the order matters for these vectors
    assert np.array_equal(bits(np.array([fm.mean4(list(row)) for row in v])), bits(want))
    out = subprocess.run([sys.executable, HOST_CHECK, "--mean"], input=v.tobytes(), capture_output=True)
    assert out.returncode == 0, out.stderr.decode()
    got = np.frombuffer(out.stdout, np.float64)
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want))


def test_stage_durations_equal_pythons_int():
    """int(growth_cycle_days * percentage) for the five crops and the eight stages (0.1 where a stage is not listed), in Python's float
    arithmetic: int(365 * 0.01) is 3, int(90 * 0.35) is 31"""
    want = [[int(fm.CYCLE[c] * p) for p in fm.STAGE_PCT[c]] for c in range(5)]
    assert want[3][0] == int(365 * 0.01) == 3 and want[0][2] == int(90 * 0.35) == 31 and want[3][7] == int(365 * 0.14) == 51 and want[0][7] == 9
    assert [list(r) for r in fm.STAGE_DAYS] == want and min(min(r) for r in want) >= 3      # never a modulus of zero
    out = subprocess.run([sys.executable, HOST_CHECK, "--stage-days"], capture_output=True)
    assert out.returncode == 0, out.stderr.decode()
    assert np.frombuffer(out.stdout, np.int32).reshape(5, 8).tolist() == want


@pytest.mark.parametrize("seed", [0, 7, 123456])
def test_draws_equal_numpy_and_cpython(seed):
    """the legacy randint(0, 25) of the equipment's locations (one masked word per attempt) and random.choice's _randbelow(5 | 3 | 1)
    (the top k bits of a word; _randbelow(1) draws until a zero bit), host build against NumPy and CPython"""
    out = subprocess.run([sys.executable, HOST_CHECK, "--randint", str(seed), "2000"], capture_output=True)
    assert out.returncode == 0, out.stderr.decode()
    rs = np.random.RandomState(seed)
    assert np.frombuffer(out.stdout, np.uint32).tolist() == [int(rs.randint(0, 25)) for _ in range(2000)]
    for n in (5, 3, 1):
        out = subprocess.run([sys.executable, HOST_CHECK, "--randbelow", str(seed), str(n), str(n.bit_length()), "1000"], capture_output=True)
        assert out.returncode == 0, out.stderr.decode()
        py = random.Random(seed)
        want = [py.choice(range(n)) for _ in range(1000)]
        assert np.frombuffer(out.stdout, np.uint32).tolist() == want
        py2 = random.Random(seed)
        assert [py2._randbelow(n) for _ in range(1000)] == want


def test_host_record_equals_the_model():
    """the float64 record after 64 hashed steps — the Gaussians of 320 prices, the one place libm's log enters — host build against
    the model, which draws NumPy's own normal(), bit for bit"""
    n, k = 16, 64
    acts = fm.hash_actions(9, k, n, envs=np.arange(n))
    out = subprocess.run([sys.executable, HOST_CHECK, "--record", "2000", str(n), str(k)], input=np.ascontiguousarray(acts, np.int32).tobytes(), capture_output=True)
    assert out.returncode == 0, out.stderr.decode()
    got = np.frombuffer(out.stdout, np.float64).reshape(n, 89)
    m = fm.FarmModel(2000 + np.arange(n), fm.SAME_STEP)
    m.reset()
    for t in range(k):
        m.step(acts[t])
    for j, e in enumerate(m.envs):
        want = [x for f in e.fields for x in (f.health, f.yp, f.moisture, f.ph, f.n, f.p, f.k, f.compaction, f.om, f.pest, f.disease)]
        want += e.fuel + e.maint + [e.temp, e.hum, e.rain, e.wind, e.frost] + e.price + e.pred
        want += [e.reservoir, e.water_quality, e.cash, e.costs, e.margin, e.revenue, e.expenses, e.carbon, e.wcs, e.bio, e.trend, e.climate]
        assert np.array_equal(bits(got[j, :87]), bits(np.array(want, np.float64))), j
        assert got[j, 88] == e.ep_ret


def test_poke_helper_changes_exactly_the_named_field():
    """tests/_lane_env_pokes.py, which the GPU test of farm_poked.npz uses: on a snapshot-shaped blob (32-byte header, 32-bit columns
    [word][env]) made from the host packer's records, a poke changes the named field of the named env and nothing else; the name is
    the field the model's record holds at that place"""
    import _lane_env_pokes as lp
    n, k = 5, 3
    acts = fm.hash_actions(9, k, n, envs=np.arange(n))
    out = subprocess.run([sys.executable, HOST_CHECK, "--record", "2000", str(n), str(k)], input=np.ascontiguousarray(acts, np.int32).tobytes(), capture_output=True)
    assert out.returncode == 0, out.stderr.decode()
    rec = np.frombuffer(out.stdout, np.float64).reshape(n, 89)
    table = lp.layout("farm")
    assert len({w for w, _ in table.values()}) == len(table) and all(0 <= w < 208 for w, _ in table.values())
    assert all((w < 178 and w % 2 == 0) == (fmt == "f64") for w, fmt in table.values())   # W_INT = 178: doubles below, whole-word integers from there
    words = np.zeros((208, n), np.uint32)
    words[:178] = rec.view(np.uint32).reshape(n, 178).T
    blob = np.concatenate([np.zeros(32, np.uint8), words.reshape(-1).view(np.uint8)])
    order = [f"f{j}.{m}" for j in range(4) for m in ("health", "yp", "moisture", "ph", "n", "p", "k", "compaction", "om", "pest", "disease")]
    order += [f"fuel{q}" for q in range(8)] + [f"maint{q}" for q in range(8)] + ["temp", "hum", "rain", "wind", "frost"]      # as test_host_record_equals_the_model
    for name, env, value in (("f1.pest", 2, 1.5), ("f3.yp", 0, 1.4), ("maint1", 4, 0.9), ("maint0", 1, 0.6), ("f3.health", 3, 0.25), ("rain_days", 2, 7)):
        poked = blob.copy()
        lp.poke_blob(poked, n, table, env, name, value)
        assert np.array_equal(poked[:32], blob[:32])
        got = poked[32:].view(np.uint32).reshape(208, n)
        changed = np.argwhere(got != words)
        assert len(changed) and (changed[:, 1] == env).all(), name
        if name == "rain_days":
            assert changed.tolist() == [[table[name][0], env]] and got[table[name][0], env] == 7 and table[name][0] >= 178
            continue
        after = np.ascontiguousarray(got[:178].T).view(np.float64).reshape(n, 89)
        diff = np.argwhere(bits(after) != bits(rec))
        assert diff.tolist() == [[env, order.index(name)]] and after[env, order.index(name)] == value, name
    with pytest.raises(KeyError):
        lp.poke_blob(blob.copy(), n, table, 0, "no_such_field", 1.0)
    # what the helper takes from the host glue by hand: the snapshot's header and magic, and the record as the first array behind it
    host = open(os.path.join(ROOT, "custom_gymnasium_environments_amd", "csrc", "cge_host.hpp")).read()
    assert "struct SnapHeader { uint64_t magic; int64_t n; uint32_t tag, extra; uint64_t reserved; };" in host and lp.HEADER_BYTES == 8 + 8 + 4 + 4 + 8
    assert int(re.search(r"constexpr uint64_t SNAP_MAGIC = (0x[0-9a-f]+)ull;", host).group(1), 16) == lp.SNAP_MAGIC
    for kind, words in (("farm", "farm::REC_WORDS"), ("space_station", "station::REC_WORDS")):
        hip = open(os.path.join(ROOT, "custom_gymnasium_environments_amd", "csrc", kind + ".hip")).read()
        first = re.search(r"alloc\((\w+), ([^;]*?), (true|false), (true|false)\)\);", hip)
        assert first.group(1) == "state" and first.group(2) == f"(size_t){words} * n * sizeof(uint32_t)" and first.group(4) == "true", first.group(0)


def test_abi_is_declared_exported_and_bound():
    kit.abi_is_declared_exported_and_bound(SPEC)


def test_no_cpu_path():
    kit.no_cpu_path(SPEC)


def test_spaces_equal_the_reference():
    rec = json.loads(str(golden("farm_hash.npz")["spaces"]))
    from custom_gymnasium_environments_amd import farm
    from custom_gymnasium_environments_amd._spaces import Box, Discrete, batch_space
    assert rec["action"] == {"kind": "Discrete", "n": 45} and farm.NUM_ACTIONS == 45
    o = rec["observation"]
    assert o["kind"] == "Box" and o["dtype"] == "float32" and o["low"] == -np.inf and o["high"] == np.inf
    assert o["shape"] == [620] == [farm.OBS_DIM] and o["live"] == 134 == farm.COMPACT_OBS_DIM
    sp = Box(-np.inf, np.inf, (farm.OBS_DIM,), np.float32)
    assert tuple(batch_space(sp, 6).shape) == (6, 620) and [int(v) for v in batch_space(Discrete(45), 6).nvec] == [45] * 6
    assert tuple(farm.REFERENCE_INFO_KEYS) == fm.INFO and tuple(farm.FIELD_INFO_KEYS) == fm.FIELD_INFO
    assert list(farm.INFO_FIELDS)[:11] == list(fm.INFO) and [farm.INFO_FIELDS[k] for k in fm.FIELD_INFO] == [11, 15, 19, 23]
    assert farm.RECORD_BYTES == 832 and farm.GENERATOR_BYTES == 5120 and len(farm.CROPS) == 5 and len(farm.SEASONS) == 4


def test_no_kernel_uses_scratch(tmp_path):
    """the condition of DESIGN.md §3.18: the record stays in registers.  The private-segment size of every cge::farm kernel, read from the
    built library's code-object notes as tests/test_kernel_occupancy.py reads the register counts"""
    kit.no_kernel_uses_scratch(SPEC, tmp_path)
