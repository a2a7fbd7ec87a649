"""Collapsed-state model of the reference's AirlineOperationsEnv (airline_operations_env/airline_env.py) in plain Python.

Only what an observation, a reward or a flag can see is kept, in the form the kernels keep it (csrc/airline_env.hpp):
  aircraft   current airport, destination, in flight, steps flown, delay minutes, fuel level, maintenance hours (float64).  The airport
             and the destination survive reset(); `passengers_onboard` is zeroed before it is paid (:562, :569), so revenue stays 0.0.
  airports   gate availability, fuel price, weather severity; x / y are constants of the network.
  flights    origin, destination, passengers, the quarter hour at which the flight comes due (`current_hour >= scheduled_time` is
             `4 * hour >= ceil(4 * scheduled)`, both exact: the hour is a multiple of 0.25), whether `scheduled + 0.25` still counts as
             on time after float64 rounding (:623-625), a status and the boarding aircraft.  A flight leaves "scheduled" at most once.
  crew       nothing: `assigned_flight` is never set, crews only rest; their draws are consumed.
  weather    up to three systems (x, y, radius, movement); the distance is sqrt(dx*dx + dy*dy), not the reference's dx**2 + dy**2
             through libm pow — the one stated departure, invisible in every recorded float32 observation.
`priority` is 1.0 for every flight and sorted() is stable: the ten "priority" flights are flights 0..9.

tests/test_airline_cpu.py pins the model to fixtures recorded from the unmodified reference; the GPU tests use it where the fixtures
cannot reach.  Test infrastructure only: the product never imports it.

Env i draws from `random.Random(seeds[i])`: the network and the constructor's discarded reset() at seeding, every reset() after it.
"""
import math
import random

import numpy as np

import _lane_model
from _lane_model import DISABLED, NEXT_STEP, SAME_STEP, LaneModel, fixture_obs  # noqa: F401

INFO = ("on_time_performance", "passenger_satisfaction", "daily_revenue", "daily_costs", "current_hour")
NA, NP, NF, NC = 25, 15, 150, 40
ARRIVE = 0
_p = 0.0
while _p < 1.0:                                                       # flight_progress += 0.05 from 0.0 until >= 1.0 (:555-557), in float64
    _p += 0.05
    ARRIVE += 1
FUEL_USE = [2.0] * 8 + [1.0] * 12 + [0.5] * 5                          # :64-79
MAX_PAX = [300] * 8 + [150] * 12 + [70] * 5
# airport positions (:196-219): the hub, four regional hubs, ten spokes on an ellipse (700 + 400 cos, 500 + 300 sin), as float64
_SPOKES = """0x1.1300000000000p+10 0x1.f400000000000p+8 0x1.ffcdab8c75b92p+9 0x1.522af424e617ap+9 0x1.9bcdab8c75b92p+9 0x1.88a891fa504e6p+9
0x1.203254738a46fp+9 0x1.88a891fa504e7p+9 0x1.7864a8e7148dep+8 0x1.522af424e617ap+9 0x1.2c00000000000p+8 0x1.f400000000001p+8
0x1.7864a8e7148dcp+8 0x1.43aa17b633d0ep+8 0x1.203254738a46ep+9 0x1.ad5db816bec66p+7 0x1.9bcdab8c75b91p+9 0x1.ad5db816bec64p+7
0x1.ffcdab8c75b91p+9 0x1.43aa17b633d0cp+8""".split()
AIRPORT_XY = [(700.0, 500.0), (300.0, 300.0), (1100.0, 300.0), (300.0, 700.0), (1100.0, 700.0)] + [
    (float.fromhex(_SPOKES[2 * i]), float.fromhex(_SPOKES[2 * i + 1])) for i in range(10)]
SCHEDULED, BOARDING, DEPARTED, CANCELLED, DELAYED_ACTION, DELAYED_NO_AIRCRAFT = range(6)


def hash_actions(a_seed, k, n, t0=0, env0=0, envs=None):
    """int32 [k, n]: the actions `rollout(k, action_seed=a_seed, t0=t0)` stands for: hash_action(a_seed, env0 + i, t0 + t, 45, 0)"""
    return _lane_model.hash_actions(a_seed, k, n, 45, t0, env0, envs)


class _Env:
    def __init__(self, seed):
        self.seed(seed)

    def seed(self, seed):
        """random.seed(seed); AirlineOperationsEnv(): _initialize_network :221-272, then the constructor's own reset() (:190)"""
        r = self.rng = random.Random(int(seed))
        self.ap, self.dest = [0] * NA, [0] * NA
        for a in range(NA):
            lo = 0 if a < 20 else 5
            self.ap[a] = r.randint(0, 4) if a < 8 else r.randint(lo, 14)
            self.dest[a] = r.randint(lo, 14)
            r.uniform(0, 1)                                           # maintenance_status: overwritten by reset()
        self.f_org, self.f_dst, self.f_s, self.f_pax = [], [], [], []
        for _ in range(NF):
            o = r.randint(0, 14)
            d = r.randint(0, 14)
            while d == o:
                d = r.randint(0, 14)
            self.f_org.append(o); self.f_dst.append(d)
            self.f_s.append(r.uniform(6, 22)); self.f_pax.append(r.randint(50, 250))
        self.f_due = [math.ceil(s * 4.0) for s in self.f_s]
        self.f_ontime = [abs((s + 0.25) - s) < 0.25 for s in self.f_s]
        for _ in range(NC):
            r.choice([0, 1, 2]); r.randint(0, 14); r.uniform(8, 12)
        self.needs_reset = False
        self.ep_r, self.ep_l = 0.0, 0
        self.reset()

    def reset(self):                                                  # :274-336
        r = self.rng
        self.h4, self.t = 24, 0
        self.sat, self.costs, self.fuel_costs, self.comp = 1.0, 0.0, 0.0, 0.0
        self.disruption = False
        self.fly, self.prog, self.delay = [False] * NA, [0] * NA, [0] * NA
        self.fuel, self.maint = [0.0] * NA, [0.0] * NA
        for a in range(NA):
            self.fuel[a] = r.uniform(0.7, 1.0)
            self.maint[a] = r.uniform(50, 200)
        self.gate, self.price, self.sev = [0.0] * NP, [0.0] * NP, [0.0] * NP
        for p in range(NP):
            self.gate[p] = r.uniform(0.7, 1.0)
            r.randint(100, 1000)
            self.price[p] = r.uniform(2.0, 3.0)
        self.f_st, self.f_ac = [SCHEDULED] * NF, [0] * NF
        self.left = self.ontime = 0
        for _ in range(NC):
            r.uniform(8, 12)
        self.wx = []
        for _ in range(r.randint(0, 3)):
            x, y, rad = r.uniform(100, 1300), r.uniform(100, 900), r.uniform(100, 300)
            r.choice([1, 2, 3, 5])
            self.wx.append([x, y, rad, r.uniform(-20, 20), r.uniform(-20, 20)])
        self.needs_reset = False
        self.ret = 0.0

    def _leave(self, f, status):
        self.f_st[f] = status
        self.left += 1
        self.ontime += status in (BOARDING, CANCELLED) or (status == DELAYED_NO_AIRCRAFT and self.f_ontime[f])

    def otp(self):
        return self.ontime / self.left if self.left else 0.95         # keeps 0.95 while no flight has left "scheduled" (:622)

    def step(self, a):
        """-> (reward float64, terminated, invalid)"""
        r = self.rng
        reward = 0.0
        invalid = not 0 <= a < 45
        if invalid:
            pass
        elif a < 25:                                                  # :449-461
            if not self.fly[a]:
                d = r.randint(0, 14)
                if d != self.ap[a]:
                    self.dest[a], self.fly[a], self.prog[a] = d, True, 0
                    r.randint(50, MAX_PAX[a])
                    reward += 100
        elif a < 35:                                                  # :463-478
            f = r.randint(0, 50)
            if self.f_st[f] == SCHEDULED:
                if a < 30:
                    self._leave(f, CANCELLED)
                    self.sat *= 0.9
                    self.comp += self.f_pax[f] * 200
                    reward -= 5000
                else:
                    self._leave(f, DELAYED_ACTION)
                    reward -= 100
        elif a < 40:
            self.gate[a - 35] = min(1.0, self.gate[a - 35] + 0.2)
            reward += 50
        elif a == 40:
            self.disruption = True
            reward -= 200
        elif a == 41:
            if self.costs < 500000:
                self.costs += 50000
                reward += 200
        elif a == 42:
            self.comp += 10000
            self.sat = min(1.0, self.sat + 0.05)
            reward -= 100
        elif a == 43:
            for k in range(NA):
                if not self.fly[k]:
                    self.delay[k] += 30
            reward -= 500
        else:
            self.disruption = False
            reward += 50
        self.h4 += 1                                                  # :406-408
        if self.h4 >= 96:
            self.h4 -= 96
        self.t += 1
        for w in self.wx:                                             # :513-548
            w[0] += w[3] * 0.1
            w[1] += w[4] * 0.1
        for p in range(NP):
            self.sev[p] = 0.0
            for x, y, rad, _, _ in self.wx:
                dx, dy = AIRPORT_XY[p][0] - x, AIRPORT_XY[p][1] - y
                dist = math.sqrt(dx * dx + dy * dy)
                if dist < rad:
                    self.sev[p] = 1.0 - (dist / rad)
        for k in range(NA):                                           # :550-576
            if self.fly[k]:
                self.prog[k] += 1
                if self.prog[k] >= ARRIVE:
                    self.fly[k], self.ap[k], self.prog[k] = False, self.dest[k], 0
                    self.fuel[k] = max(0.1, self.fuel[k] - 0.1 * FUEL_USE[k])
            self.maint[k] -= 0.5
            if self.maint[k] <= 0:
                self.delay[k] += 120
                self.maint[k] = 100.0
                self.costs += 10000
        for f in range(NF):                                           # :578-599
            if self.f_st[f] == SCHEDULED:
                if self.h4 >= self.f_due[f]:
                    free = [k for k in range(NA) if not self.fly[k] and self.ap[k] == self.f_org[f]]
                    if free:
                        self.f_ac[f] = free[0]
                        self._leave(f, BOARDING)
                        self.dest[free[0]] = self.f_dst[f]
                    else:
                        self._leave(f, DELAYED_NO_AIRCRAFT)
            elif self.f_st[f] == BOARDING:
                self.f_st[f] = DEPARTED
                self.fly[self.f_ac[f]] = True
        total = 0                                                     # :628-630: sum() from int 0, left to right
        for k in range(NA):
            if not self.fly[k]:
                total = total + FUEL_USE[k] * self.price[self.ap[k]]
        self.fuel_costs = total * 100
        self.costs += self.fuel_costs + self.comp + 0.0
        otp = self.otp()                                              # :632-666
        reward += (500 if otp > 0.95 else 200 if otp > 0.90 else -500 if otp < 0.70 else 0)
        reward += (300 if self.sat > 0.9 else -1000 if self.sat < 0.6 else 0)
        reward += -500 if 0.0 - self.costs < -100000 else 0
        reward += 100 if all(v > 0.2 for v in self.fuel) else 0
        return float(reward), self.h4 >= 95 or self.sat < 0.6, invalid

    def obs(self):                                                    # :354-396
        o = np.zeros(160, np.float32)
        for k in range(NA):
            o[4 * k:4 * k + 4] = [self.ap[k] / 15, self.fuel[k], self.delay[k] / 240.0, self.maint[k] / 200.0]
        for p in range(NP):
            o[100 + 2 * p:102 + 2 * p] = [self.sev[p], self.gate[p]]
        for f in range(10):
            s = self.f_s[f]
            actual = s + 0.5 if self.f_st[f] == DELAYED_ACTION else s + 0.25 if self.f_st[f] == DELAYED_NO_AIRCRAFT else s
            o[130 + 2 * f:132 + 2 * f] = [(actual - s) / 4.0, self.f_pax[f] / 300.0]
        o[150:160] = [self.otp(), self.sat, (self.h4 * 0.25) / 24.0, sum(self.fly) / 25, 0.0, self.costs / 1000000.0, self.fuel_costs / 100000.0,
                      self.comp / 100000.0, 1.0 if self.disruption else 0.0, len(self.wx) / 5.0]
        return o

    def info(self):
        return [self.otp(), self.sat, 0.0, self.costs, self.h4 * 0.25]


class AirlineModel(LaneModel):
    """no truncation, and no other info than info(): step() returns zeros and those rows"""
    ENV, INFO_COLUMNS, RETURN = _Env, len(INFO), "ret"

    def extra(self):
        """timestep, needs_reset, flights_in_air, delay_compensation, fuel_costs per env"""
        return np.array([[e.t, e.needs_reset, sum(e.fly), e.comp, e.fuel_costs] for e in self.envs], np.float64)

    def _step_env(self, e, a):
        reward, term, bad = e.step(a)
        e.ret += reward
        return reward, term, False, bad
