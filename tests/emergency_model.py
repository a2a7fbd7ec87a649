"""Collapsed-state model of the reference's EmergencyResponseEnv (emergency_response_env/emergency_env.py) in plain Python.

Only what an observation, a reward, a flag or an info value can see is kept, in the form the kernels keep it (csrc/emergency_env.hpp):
  network    the twenty station coordinates of units 30..39.  `population_density` (900 draws) feeds only `incident.casualties`, which
             nothing reads; the hospitals' four capacities (32 draws) are overwritten at reset and only ever raised to their cap, so
             both capacity ratios of the observation are the constant 1.0.  The draws are consumed.
  incidents  at most 20 in dict insertion order, compacted in place: x, y, type, severity, start time, the fire-truck and police-car
             requirement and the requirement's sum AS COMPUTED AT CREATION OR AT THE LAST ESCALATION (work lowers the severity
             without touching them), the mask of units ever dispatched to it.  `escalation_risk` is recomputed for every incident in
             every step before the reward reads it, and new incidents carry 0.0: a per-step mask.
  units      0..19 (fire trucks 0..11, police cars 12..19 — all that actions 0..19 reach): x, y, busy, the incident's slot, travel
             time, fatigue.  Readiness is `max(0.3, 1.0 - fatigue)` whenever a unit works (it was busy at its last update), plus
             the bonus of action 44 / 47 of the same step.  A freed unit stays at the incident's cell.  Units 20..39 never move;
             mutual-aid and National-Guard units cost four `randint(0, 29)` each and are never seen.
  the rest   25 traffic values, visibility / precipitation / wind (road conditions follow from precipitation), cascade multiplier,
             broadcast reach, cellular coverage, the counters and their `_prev_*` copies (which survive reset()), the sum, count
             and last value of `response_times`.
Dead branches, left out: `cellular_coverage < 0.7` (it only rises from 0.95), "three busy unit types" (two types can be busy), a busy
unit whose incident has gone (an incident goes only when contained, which frees its units).

tests/test_emergency_cpu.py pins the model to fixtures recorded from the unmodified reference; the GPU tests use it where the fixtures
cannot reach.  Test infrastructure only: the product never imports it.

Env i draws from `random.Random(seeds[i])`: the network at seeding (the constructor does not reset), every reset() after it.
"""
import math
import random

import numpy as np

import _lane_model
from _lane_model import DISABLED, NEXT_STEP, SAME_STEP, LaneModel, fixture_obs  # noqa: F401

INFO = ("active_emergencies", "total_casualties", "lives_saved", "emergencies_resolved", "avg_response_time", "termination_reason")
OBS, NUM_ACTIONS, MAX_INC, NU = 276, 50, 20, 20
FIRE, ACCIDENT, CHEMICAL, FLOOD, QUAKE, GAS, MEDICAL, UNREST = range(8)
FIRE_STATIONS = [(5, 5), (25, 5), (5, 25), (25, 25)]
POLICE_STATIONS = [(10, 10), (20, 10), (15, 20)]
AMBULANCE_STATIONS = [(8, 8), (22, 8), (8, 22), (22, 22), (15, 15)]
HOME = [FIRE_STATIONS[k % 4] for k in range(12)] + [POLICE_STATIONS[k % 3] for k in range(12, 20)] + [AMBULANCE_STATIONS[k % 5] for k in range(20, 30)]
HOSPITALS = [(7, 7), (23, 7), (7, 23), (23, 23), (15, 10), (10, 15), (20, 20), (15, 25)]
ZONE_TYPES = {0: [(FIRE, 0.3), (MEDICAL, 0.4), (GAS, 0.2), (UNREST, 0.1)],                   # residential :311
              1: [(FIRE, 0.25), (ACCIDENT, 0.3), (MEDICAL, 0.25), (UNREST, 0.2)],            # commercial :318
              2: [(CHEMICAL, 0.3), (FIRE, 0.2), (GAS, 0.25), (ACCIDENT, 0.25)]}              # industrial :325
CASCADE_TYPE = {FIRE: FIRE, ACCIDENT: ACCIDENT, CHEMICAL: GAS, QUAKE: FIRE, GAS: FIRE}       # :440, the others MEDICAL


def hash_actions(a_seed, k, n, t0=0, env0=0, envs=None):
    """int32 [k, n]: the actions `rollout(k, action_seed=a_seed, t0=t0)` stands for: hash_action(a_seed, env0 + i, t0 + t, 50, 0)"""
    return _lane_model.hash_actions(a_seed, k, n, NUM_ACTIONS, t0, env0, envs)


def pairwise_mean25(v):
    """np.mean of 25 float64: eight strided partial sums over the first 24, combined as a tree, then the 25th; divided by 25"""
    r = [(v[j] + v[8 + j]) + v[16 + j] for j in range(8)]
    return ((((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))) + v[24]) / 25.0


def required(kind, sev):
    """(fire trucks, police cars, sum over all unit types) of _get_required_units :358-399"""
    if kind == FIRE:
        return min(4, max(2, sev // 3)), 0, min(4, max(2, sev // 3)) + min(2, max(1, sev // 5)) + (1 if sev > 7 else 0)
    if kind == ACCIDENT:
        return (1 if sev > 6 else 0), min(3, max(1, sev // 4)), min(3, max(1, sev // 4)) + min(4, max(1, sev // 3)) + (1 if sev > 6 else 0)
    if kind == CHEMICAL:
        return 1, 0, min(2, max(1, sev // 5)) + 2
    if kind == GAS:
        return min(2, max(1, sev // 4)), 0, min(2, max(1, sev // 4)) + 1
    if kind == MEDICAL:
        return 0, 0, min(3, max(1, sev // 4))
    assert kind == UNREST                                             # floods and earthquakes are never created
    return 0, min(5, max(2, sev // 2)), min(5, max(2, sev // 2)) + 1


class _Inc:
    __slots__ = ("x", "y", "kind", "sev", "start", "rf", "rp", "rs", "mask")

    def __init__(self, x, y, kind, sev, start):
        self.x, self.y, self.kind, self.sev, self.start, self.mask = x, y, kind, sev, start, 0
        self.rf, self.rp, self.rs = required(kind, sev)


class _Env:
    def __init__(self, seed, max_timesteps=1440):
        self.max_timesteps = max_timesteps
        self.seed(seed)

    def seed(self, seed):
        """random.seed(seed); EmergencyResponseEnv(): _initialize_city :192-218, _initialize_units :220-265, _initialize_hospitals :267-283"""
        r = self.rng = random.Random(int(seed))
        for i in range(30):
            for _ in range(30):
                if i < 10 or i > 20:
                    r.randint(100, 300)
                elif i <= 15:
                    r.randint(50, 500)
                else:
                    r.randint(20, 100)
        self.station = [(r.randint(5, 25), r.randint(5, 25)) for _ in range(10)]
        for _ in range(8):
            r.randint(50, 150); r.randint(10, 30); r.randint(80, 200); r.randint(15, 40)
        self.prev_resolved = self.prev_lives = self.prev_casualties = 0
        self.needs_reset = False
        self.ep_r, self.ep_l = 0.0, 0
        self.inc = []
        self.t = 0

    def _create(self):                                                # :303-356
        r = self.rng
        x, y = r.randint(0, 29), r.randint(0, 29)
        zone = 0 if x < 10 or x > 20 else 1 if x <= 15 else 2
        v = r.random()
        cumulative, kind = 0, ZONE_TYPES[zone][0][0]
        for k, p in ZONE_TYPES[zone]:
            cumulative += p
            if v <= cumulative:
                kind = k
                break
        self.inc.append(_Inc(x, y, kind, r.randint(1, 10), self.t))

    def reset(self):                                                  # :829-881
        self.t = 0
        self.inc = []
        self.casualties = self.resolved = self.lives = 0
        self.rt_sum = self.rt_count = self.rt_last = 0
        self.soe = self.mutual = self.guard = False
        self.cm = 1.0
        self.ux, self.uy = [h[0] for h in HOME[:NU]], [h[1] for h in HOME[:NU]]
        self.busy, self.slot, self.travel, self.fatigue = [False] * NU, [0] * NU, [0] * NU, [0.0] * NU
        self.evac = [False] * 6
        self.traffic = [0.3] * 25
        self.vis, self.precip, self.wind = 1.0, 0.0, 0.0
        self.cell, self.reach = 0.95, 0.90
        for _ in range(self.rng.randint(1, 3)):
            self._create()
        self.needs_reset = False
        self.ret = 0.0
        self.reason = 0

    def road(self):
        return max(0.5, 1.0 - self.precip * 0.5)                      # :777; 1.0 after reset (precipitation 0.0)

    def _dispatch(self, u):                                           # :692-736
        if self.busy[u]:
            return
        best, best_d = None, float("inf")
        for s, inc in enumerate(self.inc):
            need = inc.rf if u < 12 else inc.rp                      # 0: the type is not in required_units
            have = bin(inc.mask & (0xFFF if u < 12 else 0xFF000)).count("1")
            if need == 0 or have >= need:
                continue
            d = math.sqrt((self.ux[u] - inc.x) ** 2 + (self.uy[u] - inc.y) ** 2)
            if d < best_d:
                best, best_d = s, d
        if best is not None:
            self.busy[u], self.slot[u] = True, best
            self.travel[u] = max(1, int(best_d * (2.0 - self.road())))
            self.inc[best].mask |= 1 << u

    def step(self, a):
        """-> (reward float64, terminated, invalid)"""
        r = self.rng
        invalid = not 0 <= a < NUM_ACTIONS
        bonus44 = False
        if invalid:                                                   # :648-690
            pass
        elif a < 20:
            self._dispatch(a)
        elif a < 26:
            self.evac[a - 20] = True
        elif a < 32:
            if not self.mutual:
                self.mutual = True
                for _ in range(20):
                    r.randint(0, 29)
        elif a < 38:
            pass                                                      # beds_available is at its cap already
        elif a < 44:
            self.traffic[a - 38] *= 0.7
        elif a == 44:
            if not self.soe:
                self.soe = bonus44 = True
        elif a == 45:
            self.reach = min(1.0, self.reach + 0.1)
        elif a == 46:
            if not self.guard and self.soe:
                self.guard = True
                for _ in range(40):
                    r.randint(0, 29)
        elif a == 48:
            self.cell = min(1.0, self.cell + 0.05)
        rate = 0.02 * self.cm                                         # :285-301
        if self.precip > 0.7:
            rate *= 1.5
        if self.wind > 0.8:
            rate *= 1.3
        if r.random() < rate and len(self.inc) < MAX_INC:
            self._create()
        risky = 0                                                     # :401-419; bit s: escalation_risk > 0.8
        for s in range(len(self.inc)):                                # (incidents a cascade adds are not visited)
            inc = self.inc[s]
            tf = (self.t - inc.start) / 60
            sf = inc.sev / 10.0
            rf = bin(inc.mask).count("1") / max(1, inc.rs)
            risk = min(1.0, tf * sf * (1.0 - rf))
            if risk > 0.8:
                risky |= 1 << s
                if r.random() < 0.1:                                  # :421-428
                    inc.sev = min(10, inc.sev + 1)
                    r.randint(1, 5)
                    self.casualties += r.randint(1, 5)
                    inc.rf, inc.rp, inc.rs = required(inc.kind, inc.sev)
            if risk > 0.6 and r.random() < 0.05 and len(self.inc) < MAX_INC:   # :430-463
                nx = max(0, min(29, inc.x + r.randint(-3, 3)))
                ny = max(0, min(29, inc.y + r.randint(-3, 3)))
                sev = r.randint(3, 7)
                r.randint(0, 3)
                self.inc.append(_Inc(nx, ny, CASCADE_TYPE.get(inc.kind, MEDICAL), sev, self.t))
                self.cm = min(3.0, self.cm + 0.1)
        road = self.road()
        for u in range(NU):                                           # :465-522
            if self.busy[u]:
                if self.travel[u] > 0:
                    self.travel[u] -= 1
                else:
                    inc = self.inc[self.slot[u]]
                    self.ux[u], self.uy[u] = inc.x, inc.y
                    ready = max(0.3, 1.0 - self.fatigue[u])
                    if bonus44:
                        ready = min(1.0, ready + 0.2)
                    if a == 47 and u < 12:
                        ready = min(1.0, ready + 0.1)
                    if r.random() < ready * self.vis * road * 0.1:
                        inc.sev = max(0, inc.sev - 1)
                        if r.random() < 0.3:
                            self.lives += 1
                    if inc.sev <= 0:
                        self.resolved += 1
                        self.rt_last = self.t - inc.start
                        self.rt_sum += self.rt_last
                        self.rt_count += 1
                        for k in range(NU):
                            if inc.mask >> k & 1:
                                self.busy[k] = False
            if self.busy[u]:
                self.fatigue[u] = min(1.0, self.fatigue[u] + 0.01)
            else:
                self.fatigue[u] = max(0.0, self.fatigue[u] - 0.005)
        self.vis = max(0.3, min(1.0, self.vis + r.uniform(-0.1, 0.1)))            # :768-780
        self.precip = max(0.0, min(1.0, self.precip + r.uniform(-0.05, 0.05)))
        self.wind = max(0.0, min(1.0, self.wind + r.uniform(-0.1, 0.1)))
        hour = (self.t // 60) % 24                                    # :782-806
        base = 0.7 if 7 <= hour <= 9 or 17 <= hour <= 19 else 0.1 if hour >= 22 or hour <= 5 else 0.3
        ec, wc = len(self.inc) * 0.05, self.precip * 0.3              # a contained incident still counts
        for i in range(25):
            target = base + ec + wc
            target += r.uniform(-0.1, 0.1)
            target = max(0.0, min(1.0, target))
            self.traffic[i] = self.traffic[i] * 0.8 + target * 0.2
        keep = [s for s, inc in enumerate(self.inc) if inc.sev > 0]   # :894-898; contained is severity 0
        if len(keep) != len(self.inc):
            new = {s: j for j, s in enumerate(keep)}
            self.slot = [new.get(s, 0) for s in self.slot]
            risky = sum((risky >> s & 1) << j for j, s in enumerate(keep))
            self.inc = [self.inc[s] for s in keep]
        reward = 0.0                                                  # :589-646
        if self.resolved - self.prev_resolved > 0:
            reward += 2000 * (self.resolved - self.prev_resolved)
        if self.lives - self.prev_lives > 0:
            reward += 5000 * (self.lives - self.prev_lives)
        if self.rt_count and self.rt_last <= 15:
            reward += 1000
        if self.cm < 1.2:
            reward += 300
        if self.casualties - self.prev_casualties > 0:
            reward -= 10000 * (self.casualties - self.prev_casualties)
        reward -= 2000 * bin(risky).count("1")
        reward -= 1000 * sum(bin(inc.mask).count("1") > inc.rs * 1.5 for inc in self.inc)
        if pairwise_mean25(self.traffic) > 0.8:
            reward -= 500
        self.prev_resolved, self.prev_lives, self.prev_casualties = self.resolved, self.lives, self.casualties
        if not self.inc and self.t > 60:                              # :808-827
            self.reason = 1
        elif self.casualties > 50:
            self.reason = 2
        elif self.avg_rt() > 45:
            self.reason = 3
        elif self.t >= self.max_timesteps:
            self.reason = 4
        else:
            self.reason = 0
        self.t += 1
        return float(reward), self.reason != 0, invalid

    def avg_rt(self):
        return self.rt_sum / self.rt_count if self.rt_count else 0.0

    def obs(self):                                                    # :524-587
        o = np.zeros(OBS, np.float32)
        for s, inc in enumerate(self.inc):
            o[4 * s:4 * s + 4] = [inc.x / 30, inc.y / 30, inc.kind / 7.0, inc.sev / 10.0]
        for u in range(40):
            if u < NU:
                x, y, b = self.ux[u], self.uy[u], self.busy[u]
            else:
                (x, y), b = (HOME[u] if u < 30 else self.station[u - 30]), False
            o[80 + 3 * u:83 + 3 * u] = [x / 30, y / 30, 1.0 if b else 0.0]
        o[200:225] = self.traffic
        for h, (hx, hy) in enumerate(HOSPITALS):
            total = 0
            for inc in self.inc:
                total = total + math.sqrt((inc.x - hx) ** 2 + (inc.y - hy) ** 2)
            o[225 + 3 * h:228 + 3 * h] = [1.0, 1.0, min(1.0, total / 100.0)]
        o[249:254] = [self.vis, self.road(), self.wind, self.precip, 0.5]
        for z in range(6):
            o[254 + 2 * z] = 1.0 if self.evac[z] else 0.0
        o[266:276] = [8 / 10.0, self.cell, self.reach, float(self.soe), float(self.mutual), float(self.guard), len(self.inc) / 20, sum(self.busy) / 40,
                      self.casualties / 100.0, self.t / self.max_timesteps]
        return o

    def info(self):
        return [len(self.inc), self.casualties, self.lives, self.resolved, self.avg_rt(), self.reason]


class EmergencyModel(LaneModel):
    """EmergencyModel(seeds, mode, max_timesteps=1440); no truncation"""
    ENV, INFO_COLUMNS, RETURN = _Env, len(INFO), "ret"

    def extra(self):
        """timestep, needs_reset, busy_units, mutual_aid_requested, national_guard_active, state_of_emergency per env"""
        return np.array([[e.t, e.needs_reset, sum(e.busy), e.mutual, e.guard, e.soe] for e in self.envs], np.float64)

    def _step_env(self, e, a):
        reward, term, bad = e.step(a)
        e.ret += reward
        return reward, term, False, bad
