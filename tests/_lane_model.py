"""What the plain-Python models of the env types share (tests/<type>_model.py): the explicit actions a hash-action rollout stands for,
the readers of a recorded fixture, and the batch of n envs with gymnasium's three autoreset modes that the record-lane types (airline,
emergency, space station, farm) step their `_Env` in.  Test infrastructure only: the product never imports it."""
import json

import numpy as np

NEXT_STEP, SAME_STEP, DISABLED = 0, 1, 2


def hash_actions(a_seed, k, n, nvec, t0=0, env0=0, envs=None):
    """The actions `rollout(k, action_seed=a_seed, t0=t0)` stands for.  nvec an int: int32 [k, n], hash_action(a_seed, env0 + i, t0 + t,
    nvec, 0).  nvec a sequence: int32 [k, n, len(nvec)], component c is hash_action(a_seed, env0 + i, t0 + t, nvec[c], c).
    envs: global env indices instead of env0 .. env0 + n - 1."""
    from _hash_actions import common
    env = np.arange(env0, env0 + n, dtype=np.uint64) if envs is None else np.asarray(envs, dtype=np.uint64)
    if isinstance(nvec, (int, np.integer)):
        return np.stack([common.hash_actions_np(a_seed, env, t0 + t, nvec, 0) for t in range(k)])
    return np.stack([np.stack([common.hash_actions_np(a_seed, env, t0 + t, nv, c) for c, nv in enumerate(nvec)], axis=-1) for t in range(k)])


def fixture_obs(z):
    """float32 [n, T, width] of a fixture (tests/golden/gen/gen_<type>.py stores uint32 [n, width, T] XORed along time)"""
    return np.ascontiguousarray(np.bitwise_xor.accumulate(z["obs_xor"], axis=2).transpose(0, 2, 1)).view(np.float32)


def fixture_pokes(z):
    """{step: [(env, field name, value)]} of a fixture's `pokes` table (empty for a fixture without one)"""
    out = {}
    if "pokes" in z:
        names = json.loads(str(z["poke_fields"]))
        for i, t, k, value in z["pokes"]:
            out.setdefault(int(t), []).append((int(i), names[int(k)], float(value)))
    return out


def clip(x, lo, hi):
    """np.clip of a scalar: min(max(x, lo), hi) with C's `a > b ? a : b` and `a < b ? a : b`"""
    t = x if x > lo else float(lo)
    return t if t < hi else float(hi)


class LaneModel:
    """n envs, env i on the stream(s) of seeds[i]; step() follows gymnasium's three autoreset modes.  A type sets ENV (its `_Env`; the
    constructor's further arguments, a step limit, go on to it), INFO_COLUMNS, RETURN (the attribute of the episode's running return)
    and LENGTH (that of its step count), and says in _step_env() how one env steps."""
    ENV = INFO_COLUMNS = None
    RETURN, LENGTH = "ep_ret", "t"

    def __init__(self, seeds, mode=SAME_STEP, *limit, **limits):
        self.envs = [self.ENV(s, *limit, **limits) for s in seeds]
        self.n, self.mode = len(self.envs), mode
        self.invalid = 0

    def _step_env(self, e, a):
        """-> (reward float64, terminated, truncated, invalid) of env e under action a, the running return kept"""
        raise NotImplementedError

    def _obs(self, e):
        return e.obs()

    def obs(self):
        return np.stack([self._obs(e) for e in self.envs])

    def reset(self, mask=None):
        for i, e in enumerate(self.envs):
            if mask is None or mask[i]:
                e.reset()
        return self.obs()

    def info(self):
        return np.array([e.info() for e in self.envs], np.float64)

    def step(self, actions):
        """-> (obs, reward float64, terminated, truncated, final_obs, info); final_obs / info are those before any SameStep reset"""
        reward, term, trunc = np.zeros(self.n, np.float64), np.zeros(self.n, bool), np.zeros(self.n, bool)
        final, info = [None] * self.n, np.zeros((self.n, self.INFO_COLUMNS), np.float64)
        for i, e in enumerate(self.envs):
            if self.mode == NEXT_STEP and e.needs_reset:
                e.reset()
                final[i], info[i] = self._obs(e), e.info()
                continue
            reward[i], term[i], trunc[i], bad = self._step_env(e, int(actions[i]))
            self.invalid += bad
            final[i], info[i] = self._obs(e), e.info()
            if term[i]:
                e.ep_r, e.ep_l = getattr(e, self.RETURN), getattr(e, self.LENGTH)
                if self.mode == SAME_STEP:
                    e.reset()
                elif self.mode == NEXT_STEP:
                    e.needs_reset = True
        return self.obs(), reward, term, trunc, np.stack(final), info
