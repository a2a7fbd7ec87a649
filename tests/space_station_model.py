"""Model of the reference's SpaceStationEnv (space_station_env/station_env.py:1-797) in plain Python, in the form the kernels keep it
(csrc/space_station_env.hpp): float64 state in the reference's operation order, the three np.mean reductions written out in NumPy's
summation order, the orbit as an index into tables of 18 values, the draws taken from an `np.random.RandomState` per env.

What reset() leaves alone is kept across episodes, as the reference keeps it: `episode_reward`, `last_emergency_time`, the crew's
modules (one bit: after action 38 everybody is in Docking for good), `solar_angle`, `radiation_level`, `total_power_consumption`.
A task is one bit per crew member: only "emergency_response" is ever read.  `crew.x` / `crew.y`, `nitrogen`, `medical_supplies` and
`fuel` never change.  The radiation's effect on health is dead (the level reaches 0.5 and the test is `> 0.5`; a solar storm's 0.8 is
overwritten before the crew update of the next step) and is kept as written.

tests/test_space_station_cpu.py pins the model to fixtures recorded from the unmodified reference; the GPU tests use it where the
fixtures cannot reach.  Test infrastructure only: the product never imports it.
"""
import math
import re

import numpy as np

import _lane_model
from _lane_model import DISABLED, NEXT_STEP, SAME_STEP, LaneModel, clip, fixture_obs, fixture_pokes  # noqa: F401

INFO = ("time_step", "day", "crew_alive", "system_failures", "emergency_count", "mission_success", "episode_reward", "battery_level", "avg_crew_health")
OBS, NUM_ACTIONS, NM, NC, NS = 120, 40, 8, 6, 12
POWER_DRAW = (500.0, 300.0, 400.0, 0.0, 600.0, 200.0, 100.0, 350.0, 50.0, 800.0, 250.0, 1000.0)           # :175-244
CRITICAL = (True, True, True, True, True, True, False, False, True, True, False, False)
CREW_XY = ((1.5, 1.5), (5.0, 3.0), (9.5, 2.0), (1.5, 5.5), (5.0, 8.0), (8.5, 5.5))                          # :151-171, module centres
DOCKING = 6
O2_GEN, CO2_SCRUB, WATER_REC, THERMAL, WASTE = 0, 1, 2, 4, 7
# the orbit advances by exactly 20.0 degrees a step (:403-404): 18 phases
COS_PHASE = tuple(math.cos(math.radians(20.0 * k)) for k in range(18))
SOLAR_EFF = tuple(0.0 if 180 < 20.0 * k < 270 else max(0, COS_PHASE[k]) for k in range(18))
RADIATION = tuple(0.3 + 0.2 * math.sin(math.radians(20.0 * k - 90)) if 90 < 20.0 * k < 270 else 0.2 for k in range(18))


def hash_actions(a_seed, k, n, t0=0, env0=0, envs=None):
    """int32 [k, n]: the actions `rollout(k, action_seed=a_seed, t0=t0)` stands for: hash_action(a_seed, env0 + i, t0 + t, 40, 0)"""
    return _lane_model.hash_actions(a_seed, k, n, NUM_ACTIONS, t0, env0, envs)


def mean6(v):
    """np.mean of 6 float64: below eight values NumPy's pairwise sum is a plain loop"""
    return (((((v[0] + v[1]) + v[2]) + v[3]) + v[4]) + v[5]) / 6.0


def sum8(v):
    return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]))


def mean8(v):
    """np.mean of 8 float64: the unrolled block of NumPy's pairwise sum, combined as a tree"""
    return sum8(v) / 8.0


def mean12(v):
    """np.mean of 12 float64: the tree over the first eight, then the other four in turn"""
    return ((((sum8(v) + v[8]) + v[9]) + v[10]) + v[11]) / 12.0


class _Env:
    def __init__(self, seed, max_steps=8640):
        self.max_steps = max_steps
        self.seed(seed)

    def seed(self, seed):
        """np.random.seed(seed); SpaceStationEnv(): the constructor draws nothing and sets what reset() will not touch"""
        self.rng = np.random.RandomState(int(seed))
        self.ret = 0.0                                                # episode_reward: never reset
        self.last_emergency = 0
        self.evacuated = False
        self.angle = 0                                                # index of solar_angle; radiation_level = 0.2 = RADIATION[0]
        self.storm_level = False                                      # radiation_level is a solar storm's 0.8
        self.total_power = 0.0
        self.needs_reset = False
        self.ep_r, self.ep_l = 0.0, 0
        self.t = 0
        self.ep_ret = 0.0

    def reset(self):                                                  # :247-308
        r = self.rng
        self.t = 0
        self.o2, self.co2, self.pres, self.temp = [0.0] * NM, [0.0] * NM, [0.0] * NM, [0.0] * NM
        for m in range(NM):
            self.o2[m] = 21.0 + r.normal(0, 0.5)
            self.co2[m] = 400.0 + r.normal(0, 50)
            self.pres[m] = 101.3 + r.normal(0, 1)
            self.temp[m] = 22.0 + r.normal(0, 1)
        self.health, self.oxy, self.fatigue, self.task = [100.0] * NC, [100.0] * NC, [0.0] * NC, [False] * NC
        self.eff, self.maint, self.last_maint = [0.0] * NS, [0.0] * NS, [0] * NS
        for s in range(NS):
            self.eff[s] = 100.0 - r.uniform(0, 5)
            self.maint[s] = r.uniform(0, 10)
        self.water, self.food, self.tanks, self.spare, self.waste = 1000.0, 500.0, 20.0, 50.0, 100.0
        self.battery, self.backup = 100.0, True
        self.phase = 0
        self.alerts = [False] * 6                                     # fire, depressurization, radiation_storm, power_failure, life_support_critical, medical
        self.success, self.casualties, self.failures, self.failure_mask, self.emergencies = False, 0, 0, 0, 0
        self.needs_reset = False
        self.ep_ret = 0.0                                             # the episode's own return (the statistics'), not the reference's episode_reward

    def radiation(self):
        return 0.8 if self.storm_level else RADIATION[self.angle]

    def step(self, a):
        """-> (reward float64, terminated, truncated, invalid)"""
        r = self.rng
        self.t += 1
        invalid = not 0 <= a < NUM_ACTIONS
        if invalid:                                                   # :351-398
            pass
        elif a < 12:
            v = self.eff[a] + 10.0
            self.eff[a] = v if v < 100.0 else 100.0
        elif a < 24:
            s = a - 12
            if self.spare > 0:
                v = self.maint[s] - 20.0
                self.maint[s] = v if v > 0 else 0.0
                self.last_maint[s] = self.t
                self.spare -= 0.5
        elif a < 30:
            self.task[a - 24] = True
        elif a < 36:
            m = a - 30
            self.temp[m] = clip(self.temp[m] + r.uniform(-1, 1), 18, 26)
            self.pres[m] = clip(self.pres[m] + r.uniform(-0.5, 0.5), 95, 108)
        elif a == 36:                                                 # :623-638
            for s in range(NS):
                if CRITICAL[s]:
                    v = self.eff[s] + 20
                    self.eff[s] = v if v < 100 else 100.0
            if self.tanks > 0:
                for m in range(NM):
                    v = self.o2[m] + 2
                    self.o2[m] = v if v < 25 else 25.0
                self.tanks -= 0.5
            self.task = [True] * NC
        elif a == 37:
            if self.backup:
                v = self.battery + 20.0
                self.battery = v if v < 100.0 else 100.0
                self.backup = False
        elif a == 38:                                                 # :640-651; the task "evacuation" is never read
            self.evacuated = True
            self.task = [False] * NC
            self.pres[DOCKING], self.o2[DOCKING], self.temp[DOCKING] = 101.3, 21.0, 22.0
        self.phase = (self.phase + 1) % 18                            # :400-420
        self.angle, self.storm_level = self.phase, False
        total = 0                                                     # :422-443, sum() from int 0
        for s in range(NS):
            total = total + POWER_DRAW[s] * (self.eff[s] / 100.0)
        self.total_power = total
        balance = 5000.0 * SOLAR_EFF[self.phase] - total
        self.battery = clip(self.battery + (balance / 5000.0) * 10, 0, 100)
        if self.battery < 10:
            self.alerts[3] = True
            self.eff = [e * 0.8 for e in self.eff]
        for m in range(NM):                                           # :445-479
            crew = (NC if m == DOCKING else 0) if self.evacuated else (1 if m < NC else 0)
            if self.eff[O2_GEN] > 50:
                self.o2[m] += (self.eff[O2_GEN] / 100.0) * 0.05
            self.o2[m] -= crew * 0.01
            if self.eff[CO2_SCRUB] > 50:
                self.co2[m] -= (self.eff[CO2_SCRUB] / 100.0) * 10
            self.co2[m] += crew * 5
            self.o2[m] = clip(self.o2[m], 0, 30)
            self.co2[m] = clip(self.co2[m], 0, 10000)
            if self.eff[THERMAL] > 50:
                self.temp[m] += (22.0 - self.temp[m]) * 0.1 * (self.eff[THERMAL] / 100.0)
            else:
                self.temp[m] += r.uniform(-0.5, 0.5)
            self.temp[m] = clip(self.temp[m], 10, 35)
        rad = self.radiation()
        for c in range(NC):                                           # :481-523
            m = DOCKING if self.evacuated else c
            if self.o2[m] < 19:
                self.oxy[c] -= 2.0
            elif self.o2[m] > 19:
                v = self.oxy[c] + 1.0
                self.oxy[c] = v if v < 100 else 100.0
            if self.co2[m] > 1000:
                self.health[c] -= 0.5
            if self.co2[m] > 5000:
                self.health[c] -= 2.0
            if self.temp[m] < 15 or self.temp[m] > 30:
                self.health[c] -= 0.3
            self.fatigue[c] += 0.1
            if self.fatigue[c] > 80:
                self.health[c] -= 0.2
            if self.task[c]:
                v = self.fatigue[c] - 5
                self.fatigue[c] = v if v > 0 else 0.0
                self.task[c] = False
            if rad > 0.5:
                self.health[c] -= rad * 0.1
            self.health[c] = clip(self.health[c], 0, 100)
            self.oxy[c] = clip(self.oxy[c], 0, 100)
            self.fatigue[c] = clip(self.fatigue[c], 0, 100)
            if self.health[c] <= 0 or self.oxy[c] <= 0:
                self.casualties += 1
        alive = sum(1 for h in self.health if h > 0)                  # :525-556
        used = alive * 0.02
        if self.eff[WATER_REC] > 50:
            self.water -= used - used * (self.eff[WATER_REC] / 100.0) * 0.9
        else:
            self.water -= used
        self.food -= alive * 0.01
        if self.alerts[4]:
            self.tanks -= 0.1
        made = alive * 0.05
        if self.eff[WASTE] > 50:
            self.waste -= (made - made * (self.eff[WASTE] / 100.0)) * 0.1
        else:
            self.waste -= made * 0.2
        self.water, self.food, self.tanks, self.spare, self.waste = (v if v > 0 else 0.0 for v in (self.water, self.food, self.tanks, self.spare, self.waste))
        if r.random_sample() < 0.001:                                 # :558-601; choice() is randint(0, len)
            kind = int(r.randint(0, 4))
            if kind == 0:
                self.pres[int(r.randint(0, NM))] -= 10
                self.alerts[1] = True
            elif kind == 1:
                s = int(r.randint(0, NS))
                self.eff[s] = 0.0
                self.failures += 1
                self.failure_mask |= 1 << s
                if CRITICAL[s]:
                    self.alerts[4] = True
            elif kind == 2:
                self.health[int(r.randint(0, NC))] -= 30
                self.alerts[5] = True
            else:
                self.storm_level = True
                self.alerts[2] = True
            self.emergencies += 1
        if mean8(self.o2) < 18:
            self.alerts[4] = True
        if self.battery < 5:
            self.alerts[3] = True
        for s in range(NS):                                           # :603-621
            self.eff[s] -= 0.01
            self.maint[s] += 0.05
            if self.t - self.last_maint[s] > 200:
                self.eff[s] -= 0.1
                self.maint[s] += 0.2
            if r.random_sample() < 0.001:
                v = self.eff[s] - 20
                self.eff[s] = v if v > 0 else 0.0
            self.eff[s] = clip(self.eff[s], 0, 100)
            self.maint[s] = clip(self.maint[s], 0, 100)
        alive = sum(1 for h in self.health if h > 0)                  # :653-712
        reward = 0.0 + alive * 10
        avg_o2, avg_co2, avg_eff = mean8(self.o2), mean8(self.co2), mean12(self.eff)
        if 19 < avg_o2 < 23:
            reward += 50
        if avg_co2 < 1000:
            reward += 30
        if avg_eff > 90:
            reward += 200
        elif avg_eff > 70:
            reward += 50
        if self.water > 20 and self.food > 20 and self.tanks > 20:
            reward += 100
        if any(self.alerts):
            if self.t - self.last_emergency > 10:
                self.last_emergency = self.t
            elif alive == NC:
                reward += 500
        if self.casualties > 0:
            reward -= 5000 * self.casualties
        for k in range(6):
            if self.alerts[k]:
                reward -= 2000 if k in (1, 4) else 500
        for v in (self.water, self.food, self.tanks, self.spare, self.waste):    # nitrogen, medical_supplies and fuel stay at 100, 100, 200
            if v < 10:
                reward -= 100
        if self.battery > 50 and avg_eff > 80 and alive == NC and not any(self.alerts):
            reward += 500
        self.ret += reward
        self.ep_ret += reward
        if self.t >= self.max_steps:                                  # :714-737
            self.success = True
            term = True
        elif all(h <= 0 for h in self.health):
            term = True
        elif sum(1 for s in range(NS) if CRITICAL[s] and self.eff[s] < 10) >= 3:
            term = True
        else:
            term = mean8(self.o2) < 15 or mean8(self.pres) < 80
        return float(reward), bool(term), self.t >= self.max_steps, invalid

    def obs(self):                                                    # :739-783
        o = []
        for c in range(NC):
            o += [CREW_XY[c][0], CREW_XY[c][1], self.health[c], self.oxy[c]]
        for s in range(NS):
            o += [self.eff[s], POWER_DRAW[s], self.maint[s]]
        for m in range(NM):
            o += [self.o2[m], self.co2[m], self.pres[m], self.temp[m]]
        o += [SOLAR_EFF[self.phase], self.battery, self.total_power, float(self.backup), 5000.0, 0.0, 0.0, 0.0, 0.0, 0.0]
        o += [self.water, self.food, self.tanks, 100.0, 100.0, self.spare, 200.0, self.waste]
        o += [20.0 * self.phase / 360.0, COS_PHASE[self.angle], float(180 < 20.0 * self.phase < 270), self.radiation()]
        o += [float(a) for a in self.alerts]
        return np.array(o, dtype=np.float32)

    def info(self):
        """the nine values in the reference's order (system_failures as its length), then the 12-bit mask of the failed systems"""
        return [self.t, (self.t * 5) // 1440, sum(1 for h in self.health if h > 0), self.failures, self.emergencies, float(self.success), self.ret,
                self.battery, mean6(self.health), self.failure_mask]


def poke(env, name, value):
    """set the plain state field that csrc/space_station_env.hpp calls `name` (a fixture's `pokes` table;
    tools/probes/space_station_host_check.cpp --layout lists the names): o2 / co2 / pres / temp of module m, health / oxy / fatigue of
    crew member c, eff / maint of system s, a resource or the battery"""
    m = re.fullmatch(r"(o2|co2|pres|temp|health|oxy|fatigue|eff|maint)(\d+)", name)
    if m:
        getattr(env, m.group(1))[int(m.group(2))] = float(value)
    else:
        assert name in ("water", "food", "tanks", "spare", "waste", "battery"), name
        setattr(env, name, float(value))


class SpaceStationModel(LaneModel):
    """SpaceStationModel(seeds, mode, max_steps=8640); the info rows are the reference's nine values and the failure mask"""
    ENV, INFO_COLUMNS = _Env, len(INFO) + 1

    def _step_env(self, e, a):
        return e.step(a)
