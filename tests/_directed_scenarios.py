"""Directed scenarios: action policies that drive the oracles into the dynamics branches random actions never reach.

tests/test_oracle_branch_coverage.py found those branches (profiles/oracle_branch_coverage.txt holds the baseline).  A scenario is
an env type, constructor kwargs, a seed and a policy; the policy may be closed-loop on the oracle's state (its observation,
`o.info`), which is legitimate because the device must equal the oracle at every step: test_directed_scenarios_gpu.py feeds the
actions the loop produced to the device and compares every step.  Each scenario names an observable event and `hit()` says, from
the oracle's own outputs, in which envs it happened; the CPU coverage test and the GPU test both assert that it did.
"""
import random

import numpy as np

N_ENVS, ENV0 = 65, 3          # one full wave plus one lane, at env_index0 = 3

# env type -> the device constructor's name for the time limit
LIMIT_KW = {"snake": "max_steps", "crypto": "max_steps", "traffic": "max_steps", "parking": "max_steps", "climate": "episode_minutes",
            "fleet": "max_timesteps", "manufacturing": "max_steps", "hospital": "max_episode_length"}
# env type -> the info fields compared at the end of a run (oracle name == device name)
INFO = {"snake": ["score", "snake_length", "steps", "direction", "food_r", "food_c", "episodes", "head_r", "head_c", "needs_reset"],
        "crypto": ["cash", "holdings", "market_psychology", "trend_strength", "regime", "step", "episodes", "needs_reset", "cash_kind"],
        "traffic": ["timestep", "num_vehicles", "episodes", "needs_reset"],
        "parking": ["timestep", "total_customers", "rejected", "satisfied", "total_wait_time", "queue_length", "episodes", "needs_reset"],
        "climate": ["num_people", "step", "comfort_time", "episodes", "needs_reset", "room_temp", "outside_temp", "energy_usage", "total_reward"],
        "fleet": ["timestep", "missed_deadlines", "completed_deliveries", "num_requests", "weather_effect", "total_reward", "episodes",
                  "needs_reset", "fuel0", "fuel1", "fuel2"],
        "manufacturing": ["raw_material", "energy_consumption", "total_reward", "in_system", "completed", "scrapped", "product_ids", "history_len",
                          "oee_availability", "oee_performance", "oee_quality", "timestep", "episodes", "needs_reset", "overflow"],
        "hospital": ["deaths", "patients_treated", "total_wait_time", "time", "outbreak_active", "mass_casualty_event", "next_patient_id",
                     "queue0", "queue1", "queue2", "queue3", "queue4", "queue5", "occupied_beds", "medicine_total", "episodes", "needs_reset",
                     "overflow"]}
# the snake oracle's info() takes field numbers (oracle/orc_snake.c: orc_snake_info)
SNAKE_FIELD = {"score": 0, "snake_length": 1, "steps": 2, "direction": 3, "food_r": 4, "food_c": 5, "board_full": 6, "episodes": 7, "head_r": 8,
               "head_c": 9, "needs_reset": 10}


def oracle_info(o, env, field):
    return o.info(SNAKE_FIELD[field]) if env == "snake" else o.info(field)


# the float64 info fields that existing tests compare within a tolerance (rtol, atol): test_crypto_gpu.py::test_step_matches_oracle and
# test_climate_gpu.py::test_step_matches_oracle_all_modes; every other field is compared exactly
INFO_TOL = {"crypto": ({"cash", "holdings", "market_psychology", "trend_strength"}, 1e-9, 1e-12),
            "climate": ({"room_temp", "outside_temp", "energy_usage", "total_reward"}, 1e-10, 1e-9)}


class Scenario:
    def __init__(self, name, env, ctor, seed, T, policy, event, hit, line):
        self.name, self.env, self.ctor, self.seed, self.T = name, env, ctor, seed, T      # ctor: oracle kwargs (max_steps = the time limit)
        self.policy, self.event, self.hit, self.line = policy, event, hit, line

    def device_kwargs(self):
        kw = dict(self.ctor)
        if "grid" in kw:
            kw["grid_size"] = kw.pop("grid")
        if "max_steps" in kw:
            kw[LIMIT_KW[self.env]] = kw.pop("max_steps")
        return kw


def run_oracle(oracle, scn, mode, n=N_ENVS, env0=ENV0):
    """The scenario on the oracle alone: the actions the policy produced and everything the oracle returned.  `hit[i]` says whether
    the event happened in env i; it is judged on the step's own observation (the terminal row where the episode ended)."""
    import _action_streams as S
    o = S.make_oracle(oracle, scn.env, scn.ctor, n, mode)
    seeds = np.arange(n, dtype=np.uint64) + np.uint64(env0 + scn.seed)
    o.seed(seeds)
    obs = o.reset()
    pol = scn.policy(o, n, seeds, obs)
    same = mode == oracle.SAME_STEP
    run = dict(obs0=obs, actions=[], obs=[], rew=[], rew64=[], te=[], tr=[], fin=[], hit=np.zeros(n, bool), oracle=o)
    idle = np.zeros(n, bool)                                   # NEXT_STEP: this step slot only resets the env, the action is ignored
    for t in range(scn.T):
        a = pol.act(t, obs)
        res = S.orc_step(o, a, want_final=same)
        new, rew, te, tr = res[:4]
        done = (te | tr).astype(bool)
        sobs = np.where(done.reshape((n,) + (1,) * (new.ndim - 1)), res[4], new) if same else new
        run["hit"] |= scn.hit(dict(t=t, a=a, obs=sobs, prev=obs, rew=rew, te=te.astype(bool), tr=tr.astype(bool), o=o)) & ~idle
        idle = done if mode == oracle.NEXT_STEP else idle
        run["actions"].append(a); run["obs"].append(new); run["rew"].append(rew); run["te"].append(te); run["tr"].append(tr)
        run["fin"].append(res[4] if same else None)
        run["rew64"].append(o.last_reward64.copy() if o._reward64 else rew)   # what a rollout sums: the unrounded rewards (snake: float32)
        obs = new
        pol.after(t, obs, done)
    return run


class Policy:
    def __init__(self, o, n, seeds, obs0):
        self.o, self.n, self.seeds = o, n, seeds

    def after(self, t, obs, done):
        pass


def fixed(fn):
    """an open-loop policy: fn(t, n) -> actions"""
    class P(Policy):
        def act(self, t, obs):
            return fn(t, self.n)
    return P


# ------------------------------------------------------------------------------------------------------------------ snake
_CYCLE = [(0, 0), (0, 1), (0, 2), (0, 3), (1, 3), (1, 2), (1, 1), (2, 1), (2, 2), (2, 3), (3, 3), (3, 2), (3, 1), (3, 0), (2, 0), (1, 0)]
_DIR = {(-1, 0): 0, (0, 1): 1, (1, 0): 2, (0, -1): 3}
_NEXT_DIR = np.zeros((4, 4), np.int32)
for _k, (_r, _c) in enumerate(_CYCLE):
    _nr, _nc = _CYCLE[(_k + 1) % 16]
    _NEXT_DIR[_r, _c] = _DIR[(_nr - _r, _nc - _c)]


class HamiltonianCycle(Policy):
    """The head follows one Hamiltonian cycle of the 4 x 4 board (it passes the start cell (2, 2) heading right, the reset direction),
    so the snake never meets itself and eats every food until it covers all 16 cells; the next move runs into its own tail."""

    def act(self, t, obs):
        return _NEXT_DIR[self.o.info(8), self.o.info(9)]


# ------------------------------------------------------------------------------------------------------------------ traffic
def _traffic_caps(s):
    ni, ob = 2, s["obs"]
    qlen, avg = ob[:, 4 * ni:8 * ni], ob[:, 8 * ni:12 * ni]
    tot = ob[:, 12 * ni + 1:14 * ni:2]
    return (qlen.max(1) == 20) & (avg.max(1) == 100) & (tot.max(1) == 1000) & (ob[:, 14 * ni + 1] == 100) & (ob[:, 14 * ni + 2] == 50)


# ------------------------------------------------------------------------------------------------------------------ crypto
_CLIP = np.array([[2.5, 0.0], [0.0, 1.5], [-2.0, 1.0], [1.0, -3.0], [1.0, 1.0], [0.0, 0.0], [0.5, 7.0], [-0.0, 0.25]], np.float32)


def _crypto_clip_actions(t, n):
    return _CLIP[(t + np.arange(n)) % len(_CLIP)] if t else np.tile(_CLIP[0], (n, 1))


# ------------------------------------------------------------------------------------------------------------------ hospital
def _doc_dept(obs):
    x, y = np.rint(obs[:, 0:45:3] * 20).astype(int), np.rint(obs[:, 1:45:3] * 20).astype(int)
    return np.where(y < 5, np.where(x < 5, 0, np.where(x < 9, 1, 2)), np.where(x < 7, 3, np.where(x < 10, 4, 5)))


class NursesExhausted(Policy):
    """Every doctor to the ICU (action 7 until none is elsewhere), so the emergency and general queues only grow; then every nurse
    to the general ward (action 3), where a queue above 5 tires them; once all 25 are at fatigue >= 80 the same action finds no
    available nurse."""

    def act(self, t, obs):
        dept = _doc_dept(obs)
        return np.where((dept != 1).any(1), 7, 3).astype(np.int32)


def _nurses_hit(s):
    return (s["prev"][:, 213:238] >= 0.8).all(1) & (s["a"] >= 0) & (s["a"] <= 5)


class DoctorsExhausted(Policy):
    """Every doctor into a department that admits patients (emergency, ICU, general ward; quotas 6 / 3 / 6), then mass-casualty mode
    once, which doubles arrivals and keeps all fifteen busy until every one is above fatigue 95."""
    QUOTA = np.array([6, 3, 0, 6, 0, 0])

    def act(self, t, obs):
        dept = _doc_dept(obs)
        cnt = np.stack([(dept == d).sum(1) for d in range(6)], 1)
        bad = cnt[:, [2, 4, 5]].sum(1) > 0
        target = np.argmax(self.QUOTA[None, :] - cnt, 1)
        a = np.where(bad, 6 + target, np.where(obs[:, 242] == 0, 33, 12))
        return a.astype(np.int32)


def _doctors_hit(s):
    ob = s["obs"]
    return s["te"] & ~s["tr"] & (ob[:, 198:213] > 0.95).all(1) & (ob[:, 238] < 0.25)


# ------------------------------------------------------------------------------------------------------------------ manufacturing
class AllTargetsMet(Policy):
    """Meets every production target.  Quality decays by the station's degradation at every processing step, and a station's
    degradation grows by 0.005 per step while its operation count is a multiple of 100 (so from the start until its first product is
    through); products of the longer types only survive the quality gates if that growth is stopped early.  So: one type-A product is
    processed up to its last step, station 0 is maintained (degradation and count back to 0), and the product's last step then ends
    with count 1 and degradation 0.  Quality mode (x 1.02 per step) from step 1.  Each later station is maintained so that it comes
    back just before its first product arrives.  Products are started whenever station 0 is up and its queue is empty."""
    T = [10, 15, 20, 25, 30, 18]
    REQ = [1, 2, 3, 4, 5, 3]

    def __init__(self, o, n, seeds, obs0):
        super().__init__(o, n, seeds, obs0)
        self.sched = [dict() for _ in range(n)]           # step -> station to maintain
        self.fresh = [set() for _ in range(n)]            # stations whose first product is on its way or through
        self.out = [[] for _ in range(n)]                 # (type, step by which it has left the system)
        self.busy_until = np.zeros(n, int)
        self.alive = np.ones(n, bool)

    def act(self, t, obs):
        a = np.full(self.n, 19, np.int32)                  # 19: no effect
        for i in range(self.n):
            if not self.alive[i]:
                continue
            ob = obs[i]
            if t == 0:
                a[i] = 0
            elif t == 1:
                a[i] = 23
            elif t == 10:
                a[i] = 11
            elif t <= 30:
                pass
            else:
                due = [s for tt, s in self.sched[i].items() if tt <= t]
                up0, q0, raw = ob[30] == 1, ob[45], ob[56]
                if due and ob[30 + 3 * due[0]] == 1:
                    a[i] = 11 + due[0]
                    self.sched[i] = {tt: s for tt, s in self.sched[i].items() if s != due[0]}
                elif up0 and q0 == 0 and raw >= 10:
                    self.out[i] = [(k, tt) for k, tt in self.out[i] if tt > t]
                    need = ob[57:63].copy()
                    for k, _ in self.out[i]:
                        need[k] -= 1
                    order = [k for k in (1, 2, 5, 3, 4, 0) if need[k] > 0]
                    if order:
                        k = order[0]
                        a[i] = k
                        start = max(t, int(self.busy_until[i]))
                        self.busy_until[i] = start + self.T[k]
                        self.out[i].append((k, start + self.T[k] + 30))
                        for s in range(1, self.REQ[k]):
                            if s not in self.fresh[i]:
                                self.fresh[i].add(s)
                                self.sched[i][max(t + 1, start + self.T[k] + s - 23)] = s
        return a

    def after(self, t, obs, done):
        self.alive &= ~done                                 # only the first episode of an env follows the script


def _all_met_hit(s):
    return s["te"] & ~s["tr"] & (s["obs"][:, 57:63] == 0).all(1) & (s["obs"][:, 31:45:3] == 0).all(1)


# ------------------------------------------------------------------------------------------------------------------ fleet
def fleet_requests(seed):
    """generate_requests (fleet_env.py:450-514) of the first episode after reset(seed=seed), drawn as the reference draws it"""
    L, P = np.random.RandomState(int(seed) & 0xFFFFFFFF), random.Random(int(seed))

    def cell(zone, k):
        i, j = divmod(k, 12)
        return (13 + i if zone in (1, 3) else i), (13 + j if zone in (2, 3) else j)
    out = []
    for _ in range(L.randint(8, 13)):
        pz, dz = L.randint(0, 4), L.randint(0, 4)
        px, py = cell(pz, P.randrange(144))
        dx, dy = cell(dz, P.randrange(144))
        while (px, py) == (dx, dy):
            dx, dy = cell(dz, P.randrange(144))
        urg = int(L.choice(4, p=[0.3, 0.4, 0.2, 0.1]))
        req = 1 if dz == 3 else (2 if dz == 2 and L.random_sample() < 0.6 else 0)
        t0, t1 = (0, 10**6)
        if dz == 1:
            t0 = L.randint(50, 200)
            t1 = min(t0 + 300, 600)
        out.append(dict(px=px, py=py, dx=dx, dy=dy, urg=urg, req=req, t0=t0, t1=t1, done=False, by=None))
    return out


class DeliverEverything(Policy):
    """A greedy courier: every idle vehicle takes the nearest open request it may carry (urgent ones first), drives there, picks up,
    drives to the destination and drops off; a vehicle refuels at the nearest station before a leg it could not finish.  The
    destinations are not observable, so the requests are drawn again as the reference draws them and checked against the reset
    observation."""
    STATIONS = [(5, 5), (20, 5), (5, 20)]
    CONS = [1.0, 0.5, 2.0]

    def __init__(self, o, n, seeds, obs0):
        super().__init__(o, n, seeds, obs0)
        self.req = [fleet_requests(s) for s in seeds]
        self.alive = np.ones(n, bool)
        for i, rq in enumerate(self.req):
            px = np.full(12, -1.0); py = np.full(12, -1.0)
            px[:len(rq)] = [d["px"] for d in rq]; py[:len(rq)] = [d["py"] for d in rq]
            assert np.array_equal(obs0[i, 15:39:2], px) and np.array_equal(obs0[i, 16:39:2], py), "fleet_requests() left the reference's draws"
        self.target = [[None] * 3 for _ in range(n)]

    @staticmethod
    def _toward(x, y, tx, ty):
        if x != tx:
            return 4 if tx > x else 3
        return 2 if ty > y else 1

    def act(self, t, obs):
        a = np.zeros((self.n, 3), np.int32)
        info = {f: self.o.info(f) for f in (4, 8, 9, 10) + tuple(range(11, 23))}
        for i in np.nonzero(self.alive)[0]:
            rq = self.req[i]
            for k in range(3):
                x, y, asg = int(info[11 + 4 * k][i]), int(info[12 + 4 * k][i]), int(info[14 + 4 * k][i])
                fuel, rate = info[8 + k][i], self.CONS[k] * info[4][i] * 1.7
                if asg >= 0:
                    rq[asg]["by"] = k
                    self.target[i][k] = asg
                    goal = (rq[asg]["dx"], rq[asg]["dy"])
                else:
                    j = self.target[i][k]
                    if j is not None and (rq[j]["done"] or rq[j]["by"] not in (None, k) or t > rq[j]["t1"]):
                        j = None
                    if j is None:
                        open_ = [(-(d["urg"] >= 2), max(abs(d["px"] - x) + abs(d["py"] - y), d["t0"] - t), jj) for jj, d in enumerate(rq)
                                 if not d["done"] and d["by"] is None and d["req"] in (0, k) and t <= d["t1"]
                                 and all(self.target[i][kk] != jj for kk in range(3) if kk != k)]
                        j = min(open_)[2] if open_ else None
                    self.target[i][k] = j
                    if j is None:
                        continue
                    goal = (rq[j]["px"], rq[j]["py"])
                dist = abs(goal[0] - x) + abs(goal[1] - y)
                st = min(self.STATIONS, key=lambda s: abs(s[0] - goal[0]) + abs(s[1] - goal[1]))
                if fuel < rate * (dist + abs(st[0] - goal[0]) + abs(st[1] - goal[1]) + 1):
                    st = min(self.STATIONS, key=lambda s: abs(s[0] - x) + abs(s[1] - y))
                    if (x, y) == st:
                        a[i, k] = 7
                        continue
                    if fuel >= rate * (abs(st[0] - x) + abs(st[1] - y)) or fuel < rate * dist:
                        a[i, k] = self._toward(x, y, *st)
                        continue
                if dist:
                    a[i, k] = self._toward(x, y, *goal)
                elif asg >= 0:
                    a[i, k] = 6
                    rq[asg]["done"] = True
                    self.target[i][k] = None
                elif t >= rq[j]["t0"]:
                    a[i, k] = 5
        return a

    def after(self, t, obs, done):
        self.alive &= ~done


def _all_done_hit(s):
    return s["te"] & ~s["tr"] & (s["obs"][:, 15:39] == -1).all(1) & (s["obs"][:, 6:9].max(1) > 0)


# ------------------------------------------------------------------------------------------------------------------ the table
def _parking_actions(t, n):
    return np.array([8, 1, -1, 2, 100, 3, 9, 5, -(2**31), 2**31 - 1], np.int64)[(t + np.arange(n)) % 10].astype(np.int32)


def _fleet_actions(t, n):
    if t == 0:
        return np.full((n, 3), -1, np.int32)
    return (np.array([-1, 4, 2, -5, 5, 1, -(2**31), 7, 3, 6], np.int64)[(t + np.arange(3 * n).reshape(n, 3)) % 10]).astype(np.int32)


def _hospital_actions(t, n):
    return np.array([-1, 33, 3, -35, 7, -(2**31), 31, 0, 12, 30], np.int64)[(t + np.arange(n)) % 10].astype(np.int32)


SCENARIOS = [
    Scenario("snake_fills_the_board", "snake", dict(grid=4, max_steps=300), 2, 110, HamiltonianCycle,
             "the snake's length equals G * G = 16: every cell of the observation is body and there is no food", lambda s: (s["obs"] == 1).all((1, 2)),
             "orc_snake.c place_food: len >= G * G (reached before only by stepping dead envs in Disabled mode and by injected state)"),
    Scenario("traffic_hold_one_phase", "traffic", dict(grid_size=(1, 2), num_intersections=2, max_vehicles=127, spawn_rate=1.0, max_steps=210), 5, 215,
             fixed(lambda t, n: np.ones((n, 2), np.int32)),
             "all five observation caps at once: a queue length 20, a queue's average wait 100, an intersection's total wait 1000, the "
             "global average wait 100 and average queue 50", _traffic_caps, "orc_traffic.c write_obs: the five caps"),
    Scenario("crypto_actions_beyond_the_box", "crypto", dict(action_type="continuous", max_steps=40), 12, 60, fixed(_crypto_clip_actions),
             "a buy fraction of 2.5 is clipped to 1.0: cash / initial_balance == 0.9 after the first step",
             lambda s: (s["t"] == 0) & (s["obs"][:, 250] == np.float32(0.9)), "orc_crypto.c execute_action: a_cont > 1.0f"),
    Scenario("crypto_negative_balance", "crypto", dict(action_type="discrete", max_steps=50, config=dict(initial_balance=-1000.0)), 12, 25,
             fixed(lambda t, n: ((t + np.arange(n)) % 5).astype(np.int32)),
             "a buy with negative cash is refused: reward exactly -1, the no-trade penalty (every step also terminates, but by `pv <= 0` and "
             "`pv >= 10 * initial_balance` alike: for a balance <= 0 the second subsumes the first, so that arm is not discriminated here)",
             lambda s: ((s["a"] == 1) | (s["a"] == 2)) & (s["rew"] == -1) & s["te"],
             "orc_crypto.c do_buy: amount <= 0 (and, for gcov only, env_step: pv <= 0)"),
    Scenario("climate_cold_night", "climate", dict(max_occupancy=1, max_steps=190), 328, 200,
             fixed(lambda t, n: (np.full((n, 1), 10.0, np.float32), np.zeros((n, 4), np.int8))),
             "room temperature below 16", lambda s: s["obs"][:, 0] < 16, "orc_climate.c env_step: 16 <= T false"),
    Scenario("parking_actions_outside_discrete8", "parking", dict(max_steps=40), 7, 60, fixed(_parking_actions),
             "a step with an action above 7 and reward 0", lambda s: (s["a"] > 7) & (s["rew"] == 0), "orc_parking.c process_action: a <= 7 false"),
    Scenario("fleet_negative_actions", "fleet", dict(max_steps=40), 7, 60, fixed(_fleet_actions),
             "three negative actions at the first step: reward 3 * (-2 - 10)", lambda s: (s["t"] == 0) & (s["rew"] == -36),
             "orc_fleet.c vehicle_action: a >= 1 false below 0"),
    Scenario("hospital_negative_actions", "hospital", dict(max_steps=40), 7, 60, fixed(_hospital_actions),
             "a step with a negative action", lambda s: s["a"] < 0, "orc_hospital.c process_action: action < 0"),
    Scenario("hospital_nurses_exhausted", "hospital", dict(max_steps=400), 1, 400, NursesExhausted,
             "a nurse-assignment action while all 25 nurses are at fatigue >= 80", _nurses_hit, "orc_hospital.c process_action: if (na) false"),
    Scenario("hospital_doctors_exhausted", "hospital", dict(max_steps=1440), 1, 300, DoctorsExhausted,
             "terminated before the time limit with fewer than 3 deaths and all 15 doctors above fatigue 95", _doctors_hit,
             "orc_hospital.c env_step: tired == NDOC"),
    Scenario("manufacturing_all_targets_met", "manufacturing", dict(max_steps=1500), 1, 600, AllTargetsMet,
             "terminated before the time limit with no target left and no station broken", _all_met_hit, "orc_manufacturing.c env_step: all_met"),
    Scenario("fleet_deliver_everything", "fleet", dict(max_steps=800), 1, 330, DeliverEverything,
             "terminated before the time limit with every request delivered and fuel left", _all_done_hit, "orc_fleet.c env_step: all_done"),
]
