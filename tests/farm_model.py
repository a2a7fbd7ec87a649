"""Model of the reference's AgriculturalFarmEnv (agricultural_farm_env/farm_env.py:116-935 and crops/crop_data.py) in plain Python,
in the form the kernels keep it (csrc/farm_env.hpp): float64 state in the reference's operation order, crops, stages and seasons as
small integers (-1 is the reference's None), the two np.mean reductions written out in NumPy's summation order, the draws taken from
an `np.random.RandomState` (the process-global NumPy legacy stream of the reference) and a `random.Random` (its `random.choice`) per env.

What reset() leaves alone is kept across episodes, as the reference keeps it: `water_quality` (`irrigation_capacity` and `water_costs`
never change at all), and both streams with the legacy Gaussian's cached second value.  `operation_field` is never set, so an operating
machine compacts nothing; `last_irrigated_day`, `debt_level`, `groundwater_level` and `solar_radiation` are never read or never change.
The soil termination (:619-621) is written as the reference writes it; the clip of :388 keeps every fixture out of it
(tests/golden/lane_env_unreachable.json).  The excessive-rain penalty (:879-881) and the repair of action 44 are entered by
farm_poked.npz, whose `pokes` table poke() applies.

tests/test_farm_cpu.py pins the model to fixtures recorded from the unmodified reference; the GPU tests use it where the fixtures
cannot reach.  Test infrastructure only: the product never imports it.
"""
import random

import numpy as np

import _lane_model
from _lane_model import DISABLED, NEXT_STEP, SAME_STEP, LaneModel, clip, fixture_obs, fixture_pokes  # noqa: F401

INFO = ("day", "season", "year", "cash_flow", "total_revenue", "total_expenses", "profit_margin", "carbon_sequestered",
        "water_conservation_score", "biodiversity_index", "soil_health_trend")
FIELD_INFO = ("field_crop", "field_stage", "field_health", "field_yield_potential")
INFO_COLUMNS = len(INFO) + 4 * len(FIELD_INFO)
OBS, LIVE, NUM_ACTIONS, NF, NE, NCROP = 620, 134, 45, 4, 8, 5
WHEAT, CORN, TOMATOES, APPLES, SOYBEANS = range(5)
HARVEST_READY, HARVESTED, DORMANT = 5, 6, 7
# crops/crop_data.py:57-167
CYCLE = (90, 120, 60, 365, 100)
TEMP_RANGE = ((10.0, 25.0), (18.0, 32.0), (18.0, 29.0), (4.0, 24.0), (20.0, 30.0))
PH_RANGE = ((6.0, 7.5), (5.8, 7.0), (6.0, 6.8), (6.0, 7.0), (6.0, 7.0))
NEEDS = ((120, 60, 40), (180, 80, 90), (100, 120, 140), (80, 40, 100), (40, 60, 80))
BASE_PRICE = (250.0, 200.0, 800.0, 600.0, 400.0)
YIELD_HA = (3.5, 10.0, 80.0, 40.0, 3.0)
CARBON = (0.8, 1.2, 0.5, 2.5, 1.0)
SUITABLE = ((0, 1, 2, 3, 4), (1, 2, 4), (0,), ())                                       # planting_seasons, by season
STAGE_PCT = ((0.05, 0.10, 0.35, 0.25, 0.20, 0.05, 0.1, 0.1), (0.04, 0.08, 0.40, 0.25, 0.18, 0.05, 0.1, 0.1),
             (0.05, 0.12, 0.33, 0.30, 0.15, 0.05, 0.1, 0.1), (0.01, 0.02, 0.40, 0.15, 0.20, 0.08, 0.1, 0.14),
             (0.05, 0.10, 0.35, 0.30, 0.15, 0.05, 0.1, 0.1))                            # crop_data.py:178-223, 0.1 where a stage is not listed
STAGE_DAYS = tuple(tuple(int(CYCLE[c] * p) for p in STAGE_PCT[c]) for c in range(NCROP))
SEASON_MULT = ((1.0, 0.9, 1.2, 1.1, 1.0), (1.1, 1.0, 0.8, 0.9, 1.0), (0.9, 1.2, 1.3, 1.2, 1.1), (1.2, 1.3, 1.5, 1.0, 1.2))
# farm_env.py:242-274: temperature, humidity, rainfall, wind_speed, frost_risk by season
WEATHER = (((10.0, 22.0), (0.4, 0.7), (0.0, 15.0), (5.0, 20.0), (0.0, 0.2)), ((20.0, 35.0), (0.3, 0.6), (0.0, 10.0), (3.0, 15.0), (0.0, 0.0)),
           ((8.0, 20.0), (0.5, 0.8), (0.0, 20.0), (8.0, 25.0), (0.0, 0.3)), ((-5.0, 10.0), (0.6, 0.9), (0.0, 25.0), (10.0, 30.0), (0.2, 0.7)))
FIELD_SIZE = (156, 156, 156, 157)
INITIAL_CROP = (WHEAT, CORN, TOMATOES, -1)


def hash_actions(a_seed, k, n, t0=0, env0=0, envs=None):
    """int32 [k, n]: the actions `rollout(k, action_seed=a_seed, t0=t0)` stands for: hash_action(a_seed, env0 + i, t0 + t, 45, 0)"""
    return _lane_model.hash_actions(a_seed, k, n, NUM_ACTIONS, t0, env0, envs)


def mean4(v):
    """np.mean of 4 float64: below eight values NumPy's pairwise sum is a plain loop"""
    return (((v[0] + v[1]) + v[2]) + v[3]) / 4.0


def yield_modifier(crop, moisture, ph, npk, temperature, pest, disease):   # crop_data.py:226-282
    m = 1.0
    lo, hi = TEMP_RANGE[crop]
    if lo <= temperature <= hi:
        m *= 1.0
    elif temperature < lo:
        m *= max(0.3, 1.0 - (lo - temperature) * 0.05)
    else:
        m *= max(0.3, 1.0 - (temperature - hi) * 0.05)
    lo, hi = PH_RANGE[crop]
    if not lo <= ph <= hi:
        m *= max(0.5, 1.0 - min(abs(ph - lo), abs(ph - hi)) * 0.15)
    if not 0.4 <= moisture <= 0.8:
        m *= max(0.4, 1.0 - abs(moisture - 0.6))
    for have, need in zip(npk, NEEDS[crop]):
        ratio = have / need
        if 0.8 <= ratio <= 1.2:
            m *= 1.0
        elif ratio < 0.8:
            m *= max(0.5, ratio)
        else:
            m *= max(0.7, 2.0 - ratio)
    m *= (1.0 - pest * 0.5)
    m *= (1.0 - disease * 0.5)
    return max(0.1, min(1.5, m))


class _Field:
    pass


class _Env:
    def __init__(self, seed, max_years=1):
        self.max_years = max_years
        self.seed(seed)

    def seed(self, seed):
        """random.seed(seed); np.random.seed(seed); AgriculturalFarmEnv(): the constructor draws the fields, the equipment and the
        market (:141-155) and sets what reset() will not touch"""
        self.rng = np.random.RandomState(int(seed))
        self.py = random.Random(int(seed))
        self.water_quality = 0.9
        self.needs_reset = False
        self.ep_r, self.ep_l = 0.0, 0
        self._draw_episode()

    def _draw_episode(self):
        r = self.rng
        self.day, self.season, self.year = 0, 0, 1
        self.fields = []
        for k in range(NF):                                           # :194-220
            f = _Field()
            f.crop, f.stage, f.health, f.yp, f.dth, f.since, f.last_crop = INITIAL_CROP[k], DORMANT, 1.0, 1.0, 0, 0, -1
            f.pest, f.disease, f.last_fert, f.last_pest = 0.0, 0.0, -100, -100
            f.moisture = r.uniform(0.3, 0.7)
            f.ph = r.uniform(6.0, 7.0)
            f.n = r.uniform(80, 120)
            f.p = r.uniform(40, 60)
            f.k = r.uniform(40, 60)
            f.compaction = r.uniform(0.2, 0.4)
            f.om = r.uniform(0.03, 0.05)
            self.fields.append(f)
        self.loc, self.fuel, self.maint, self.operating = [], [], [], [False] * NE
        for _ in range(NE):                                           # :222-232
            self.loc.append((int(r.randint(0, 25)), int(r.randint(0, 25))))
            self.fuel.append(r.uniform(0.7, 1.0))
            self.maint.append(r.uniform(0.0, 0.2))
        self.temp, self.hum, self.rain, self.wind, self.frost, self.drought, self.rain_days = 20.0, 0.5, 0.0, 10.0, 0.0, 0, 0
        self.climate = 0.0
        self.price, self.pred = [0.0] * NCROP, [0.0] * NCROP
        for c in range(NCROP):                                        # :234-240
            self.price[c] = BASE_PRICE[c] * r.uniform(0.9, 1.1)
            self.pred[c] = BASE_PRICE[c] * r.uniform(0.85, 1.15)
        self.reservoir = 0.8
        self.cash, self.costs, self.margin, self.revenue, self.expenses = 50000.0, 0.0, 0.0, 0.0, 0.0
        self.carbon, self.wcs, self.bio, self.trend = 0.0, 0.0, 0.5, 0.0
        self.ep_ret = 0.0

    def reset(self):                                                  # :520-566
        self._draw_episode()
        self.needs_reset = False

    def _harvest(self, f, size):                                      # :802-845
        if f.crop < 0:
            return 0.0
        base = YIELD_HA[f.crop] * (size / 625.0)
        actual = base * f.yp * f.health
        price = self.price[f.crop]
        revenue = actual * price
        self.cash += revenue
        self.revenue += revenue
        ratio = actual / base
        reward = 5000 if ratio > 1.2 else 2000 if ratio > 0.9 else 1000 if ratio > 0.7 else -1000
        avg = BASE_PRICE[f.crop]
        if price > avg * 1.2:
            reward += 800
        elif price < avg * 0.8:
            reward -= 400
        f.last_crop, f.crop, f.stage, f.since, f.health, f.yp = f.crop, -1, DORMANT, 0, 1.0, 1.0
        return reward

    def _act(self, a):                                                # :629-800
        reward = 0.0
        if a <= 4:
            if a < NF:
                f = self.fields[a]
                if f.crop < 0 or f.stage == HARVESTED:
                    suitable = SUITABLE[self.season]
                    if suitable:
                        f.crop = suitable[self.py._randbelow(len(suitable))]   # random.choice
                        f.stage, f.since, f.health, f.yp = 0, 0, 1.0, 1.0
                        self.cash -= 500
                        reward += 50
                        if f.last_crop > 0 and f.last_crop != f.crop:     # `if field.last_crop`: wheat is false
                            reward += 100
        elif a <= 9:
            if a - 5 < NF:
                f = self.fields[a - 5]
                if f.stage == HARVEST_READY:
                    reward += self._harvest(f, FIELD_SIZE[a - 5])
        elif a <= 14:
            if a - 10 < NF:
                f = self.fields[a - 10]
                if self.day - f.last_fert > 14:
                    f.n += 30
                    f.p += 20
                    f.k += 20
                    f.last_fert = self.day
                    self.cash -= 300
                    reward += 20
                    if f.n > 150:
                        reward -= 100
                        self.water_quality -= 0.02
        elif a <= 19:
            if a - 15 < NF:
                f = self.fields[a - 15]
                if self.reservoir > 0.1:
                    amount = min(0.05, self.reservoir)
                    f.moisture += amount * 2
                    f.moisture = min(1.0, f.moisture)
                    self.reservoir -= amount
                    self.cash -= 10.0 * amount * 100
                    if f.moisture < 0.3:
                        reward += 50
        elif a <= 24:
            if a - 20 < NF:
                f = self.fields[a - 20]
                if self.day - f.last_pest > 21:
                    f.pest = float(max(0, f.pest - 0.5))
                    f.disease = float(max(0, f.disease - 0.3))
                    f.last_pest = self.day
                    self.cash -= 400
                    self.bio -= 0.02
                    self.water_quality -= 0.01
                    reward -= 50
                    if f.pest > 0.5:
                        reward += 200
        elif a <= 29:
            q = a - 25
            if self.fuel[q] > 0.1 and self.maint[q] < 0.8:
                self.operating[q] = True
                self.fuel[q] -= 0.1
                self.maint[q] += 0.02
                reward += 10
            else:
                reward -= 20
        elif a <= 34:
            if a - 30 < NF:
                f = self.fields[a - 30]
                reward += 15
                self.cash -= 100
                f.compaction = float(max(0, f.compaction - 0.1))
        elif a <= 39:
            if self.cash < 10000:
                revenue = self.price[a - 35] * 10
                self.cash += revenue
                self.revenue += revenue
                reward += 100
        elif a == 40:
            for f in self.fields:
                if self.frost > 0.5 or self.rain_days > 3:
                    f.health = max(f.health - 0.05, 0.5)
                    reward += 50
            self.cash -= 1000
        elif a == 41:
            self.bio += 0.01
            self.trend += 0.02
            self.carbon += 1.0
            reward += 500
        elif a == 42:
            for f in self.fields:
                if f.crop > 0:
                    f.yp *= 1.1
                    f.om -= 0.001
            reward += 100
        elif a == 43:
            if len({f.crop for f in self.fields if f.crop > 0}) >= 3:
                reward += 200
        elif a == 44:
            for q in range(NE):
                if self.maint[q] > 0.5:
                    self.maint[q] = 0.0
                    self.fuel[q] = 1.0
                    self.cash -= 500
                    reward += 30
        return reward

    def step(self, a):
        """-> (reward float64, terminated, invalid)"""
        r = self.rng
        invalid = not 0 <= a < NUM_ACTIONS
        reward = 0.0
        if not invalid:
            reward += self._act(a)
        w = WEATHER[self.season]                                      # :276-316
        shift = self.climate * 2.0
        self.temp = 0.7 * self.temp + (1 - 0.7) * r.uniform(w[0][0] + shift, w[0][1] + shift)
        self.hum = 0.7 * self.hum + (1 - 0.7) * r.uniform(*w[1])
        self.rain = r.uniform(*w[2]) if r.random_sample() < 0.3 else 0.0
        self.wind = r.uniform(*w[3])
        self.frost = r.uniform(*w[4]) if self.temp < 5 else 0.0
        if self.rain < 2.0:
            self.drought += 1
            self.rain_days = 0
        elif self.rain > 15.0:
            self.rain_days += 1
            self.drought = 0
        else:
            self.drought = max(0, self.drought - 1)
            self.rain_days = max(0, self.rain_days - 1)
        for f in self.fields:                                         # :318-356
            if f.crop >= 0 and f.stage != HARVESTED:
                f.since += 1
                if f.since % STAGE_DAYS[f.crop][f.stage] == 0 and f.stage < HARVEST_READY:
                    f.stage += 1
                f.dth = max(0, CYCLE[f.crop] - f.since)
                f.yp = yield_modifier(f.crop, f.moisture, f.ph, (f.n, f.p, f.k), self.temp, f.pest, f.disease)
                f.health = max(0.0, min(1.0, f.health - 0.01 * (f.pest + f.disease)))
                if r.random_sample() < 0.05:
                    f.pest = min(1.0, f.pest + r.uniform(0.01, 0.05))
                if self.hum > 0.7 and self.temp > 15:
                    f.disease = min(1.0, f.disease + 0.02)
        for f in self.fields:                                         # :358-388
            f.moisture += self.rain * 0.01
            f.moisture -= (self.temp / 100.0) * (1.0 - self.hum)
            f.moisture = clip(f.moisture, 0.0, 1.0)
            if f.crop >= 0:
                f.n -= NEEDS[f.crop][0] * 0.001
                f.p -= NEEDS[f.crop][1] * 0.001
                f.k -= NEEDS[f.crop][2] * 0.001
                if f.crop == SOYBEANS:
                    f.n += 0.5
            f.compaction = max(0.0, f.compaction - 0.001)             # operation_field is never set
            if f.last_crop >= 0:
                f.om += 0.0001
            f.om = clip(f.om, 0.01, 0.1)
        for c in range(NCROP):                                        # :390-411
            base = BASE_PRICE[c]
            new = self.price[c] + r.normal(0, 0.1 * base)
            new = 0.9 * new + 0.1 * (base * SEASON_MULT[self.season][c])
            self.price[c] = max(base * 0.5, min(base * 2.0, new))
            self.pred[c] = new * r.uniform(0.9, 1.1)
        self.reservoir += self.rain * 0.001                           # :581-589
        self.reservoir -= 0.01
        self.reservoir = clip(self.reservoir, 0.0, 1.0)
        costs = 0.0                                                   # :413-433
        for q in range(NE):
            if self.operating[q]:
                costs += 50.0
        costs += 200.0
        costs += 10.0 * (1.0 - self.reservoir) * 10
        for q in range(NE):
            if self.maint[q] > 0.5:
                costs += 100.0
        self.costs = costs
        self.expenses += costs
        self.cash -= costs
        for k, f in enumerate(self.fields):                           # :591-596
            if f.stage == HARVEST_READY and f.dth <= 0:
                reward += self._harvest(f, FIELD_SIZE[k])
        avg_om = mean4([f.om for f in self.fields])                   # :847-883
        if avg_om > 0.045:
            reward += 500
        elif avg_om < 0.02:
            reward -= 2000
        if self.reservoir > 0.5 and self.drought > 10:
            reward += 300
        if self.bio > 0.7:
            reward += 200
        elif self.bio < 0.3:
            reward -= 300
        for f in self.fields:
            if f.crop > 0:
                if self.frost > 0.5 and f.stage in (1, 3):
                    f.health -= 0.2
                    reward -= 300
                if self.drought > 20 and f.moisture < 0.2:
                    f.health -= 0.15
                    reward -= 300
                if self.rain_days > 5:
                    f.disease += 0.1
                    reward -= 200
        for f in self.fields:                                         # :885-909
            if f.crop > 0:
                self.carbon += CARBON[f.crop] * 0.01
        if 1.0 - self.reservoir < 0.3:
            self.wcs = min(1.0, self.wcs + 0.01)
        else:
            self.wcs = max(0.0, self.wcs - 0.01)
        self.trend = (mean4([f.om for f in self.fields]) * 10 - mean4([f.compaction for f in self.fields])) / 2
        self.margin = (self.revenue - self.expenses) / self.revenue if self.revenue > 0 else -1.0
        self.day += 1                                                 # :604-621
        if self.day % 90 == 0:
            self.season = (self.season + 1) % 4
            if self.season == 0:
                self.year += 1
                self.climate += 0.05
        term = False
        if self.year > self.max_years:
            term = True
        elif self.cash < -50000:
            term = True
            reward -= 5000
        elif all(f.om < 0.01 for f in self.fields):
            term = True
            reward -= 3000
        self.ep_ret += reward
        return float(reward), term, invalid

    def obs(self, width=OBS):                                         # :435-518
        o = []
        for f in self.fields:
            o += [f.crop if f.crop > 0 else -1, f.stage, f.health, f.yp, f.dth, f.moisture, f.ph, f.n / 200.0, f.p / 100.0, f.k / 100.0, f.compaction,
                  f.om * 10, f.pest, f.disease, f.since / 365.0]
        o += [self.temp / 40.0, self.hum, self.rain / 30.0, self.wind / 40.0, 15.0 / 30.0, self.frost, self.drought / 30.0, self.rain_days / 10.0,
              self.season / 3.0, self.day / 365.0]
        for q in range(NE):
            o += [self.loc[q][0] / 25, self.loc[q][1] / 25, self.fuel[q], self.maint[q], float(self.operating[q])]
        for c in range(NCROP):
            o += [self.price[c] / 1000.0, self.pred[c] / 1000.0]
        o += [self.reservoir, 1.0, self.water_quality, 0.7, 10.0 / 50.0]
        o += [self.cash / 100000.0, self.costs / 1000.0, 0.0 / 100000.0, self.margin, (self.revenue - self.expenses) / 100000.0]
        o += [self.carbon / 100.0, self.wcs, self.bio, self.trend]
        assert len(o) == LIVE
        row = np.zeros(width, np.float32)
        row[:LIVE] = np.array(o, dtype=np.float32)
        return row

    def info(self):
        """the eleven scalar values of _get_info in its order (:911-924), then field_status as crop (-1 for "None", which wheat prints
        too), stage, health and yield_potential of the four fields"""
        return ([self.day, self.season, self.year, self.cash, self.revenue, self.expenses, self.margin, self.carbon, self.wcs, self.bio, self.trend]
                + [f.crop if f.crop > 0 else -1 for f in self.fields] + [f.stage for f in self.fields] + [f.health for f in self.fields]
                + [f.yp for f in self.fields])


def poke(env, name, value):
    """set the plain state field that csrc/farm_env.hpp calls `name` (a fixture's `pokes` table; tools/probes/farm_host_check.cpp
    --layout lists the names): f<k>.<member> of a field, fuel<q> / maint<q> of a machine, a scalar"""
    head, _, member = name.partition(".")
    if member:
        assert head[0] == "f" and member in ("health", "yp", "moisture", "ph", "n", "p", "k", "compaction", "om", "pest", "disease"), name
        setattr(env.fields[int(head[1:])], member, float(value))
    elif name[:-1] in ("fuel", "maint"):
        getattr(env, name[:-1])[int(name[-1])] = float(value)
    elif name in ("day", "drought", "rain_days"):
        setattr(env, name, int(value))
    else:
        attr = {"quality": "water_quality"}.get(name, name)
        assert attr in ("temp", "hum", "rain", "wind", "frost", "reservoir", "water_quality", "cash", "bio", "trend", "climate"), name
        setattr(env, attr, float(value))


class FarmModel(LaneModel):
    """FarmModel(seeds, mode, max_years=1, width=OBS): on the two streams of seeds[i]; rows of `width` columns; no truncation"""
    ENV, INFO_COLUMNS, LENGTH = _Env, INFO_COLUMNS, "day"

    def __init__(self, seeds, mode=SAME_STEP, max_years=1, width=OBS):
        super().__init__(seeds, mode, max_years)
        self.width = width

    def _obs(self, e):
        return e.obs(self.width)

    def _step_env(self, e, a):
        reward, term, bad = e.step(a)
        return reward, term, False, bad
