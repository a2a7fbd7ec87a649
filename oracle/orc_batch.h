/* oracle/orc_batch.h — the batch driver of every orc_<env>.c, written once (TEST INFRASTRUCTURE ONLY, see orc_rng.h).
 *
 * An include-template: orc_<env>.c defines its handle (orc_<env>: int64_t n; int mode; <env> *e; orc_eps eps; ...), its dynamics
 * and the hooks below, then includes this file once.  The hooks stay direct, inlinable calls.  This file defines
 *   batch_create   n / mode checks, the zeroed handle and envs, default seeds i (what all orc_<env>_create share)
 *   orc_<env>_destroy, _seed, _reset, _step, _rollout, _set_max_steps, _episode_stats
 *
 * Hooks (macros unless said otherwise):
 *   ORC_NAME                 <env>; the handle type is orc_<env>
 *   ORC_ENV                  the per-env state type; needs `int needs_reset, episodes`
 *   ORC_OBS_T, ORC_OBS_LEN(h)   element type and length of one observation row
 *   ORC_FLOAT_REWARD         optional (snake): env_step yields a float and rollout sums floats in step order; otherwise both are
 *                            double and step() has a `double *reward64` (nullable) for the unrounded reward
 *   ORC_MAX_STEPS(h)         the handle's time-limit field
 *   ORC_SEED(e, s)           seed env e's private stream(s) from uint64 s
 *   ORC_RESET(h, e), ORC_WRITE_OBS(h, e, row)
 *   ORC_STEP_PARAMS          step()'s action parameter(s)
 *   ORC_STEP(h, e, i, r)     one reference step of env i with its action from ORC_STEP_PARAMS; *r = reward; returns the flags
 *                            terminated | truncated << 1 (the episode ends on either)
 *   ORC_ACTION_OK(h, i)      optional: step() returns the number of envs whose action fails it (the reference raises ValueError)
 *   hash_step(h, e, a_seed, env, t, r)   a function: ORC_STEP with the counter-hash action of (a_seed, env, t) (rollout)
 *   ORC_SCRATCH              optional, a row capacity: rollout assembles the observation of EVERY step into a scratch row while
 *                            obs != NULL, as the reference does (its cost is part of bench.py's cpu_baseline for those types);
 *                            the row is discarded (at a SAME_STEP episode end it is the reset observation, not the terminal one)
 *
 * Batch / autoreset semantics (the build's own; the reference has no vector API).  They mirror include/cge_amd.h so the parity
 * tests drive both sides with the same calls:
 *   mode 0 NEXT_STEP : a done env returns its terminal obs; the NEXT step() ignores the action, resets it (no reseed, the stream
 *                      continues) and returns (reset obs, reward 0, flags 0).  That step belongs to no episode.
 *   mode 1 SAME_STEP : a done env is reset inside the same step(); obs = reset obs, the terminal obs goes to final_obs (if not NULL).
 *   mode 2 DISABLED  : no reset at all; stepping a finished env does what the reference does.
 * Episode statistics (orc_epstats.h): every stepped env adds its reward, a finished episode is published at its last step, and
 * the accumulators restart wherever the env is re-initialised (batch_reset_env is the only caller of ORC_RESET).
 */
#include <stdint.h>
#include <stdlib.h>

#include "orc_epstats.h"

#define ORC_CAT_(a, b) a##b
#define ORC_CAT(a, b) ORC_CAT_(a, b)
#define ORC_H ORC_CAT(orc_, ORC_NAME)
#define ORC_FN(f) ORC_CAT(ORC_H, _##f)

static ORC_H *batch_create(int64_t n, int mode) {
    if (n <= 0 || mode < 0 || mode > 2) return NULL;
    ORC_H *h = (ORC_H *)calloc(1, sizeof(*h));
    h->n = n; h->mode = mode;
    h->e = (ORC_ENV *)calloc((size_t)n, sizeof(ORC_ENV));
    eps_init(&h->eps, n);
    for (int64_t i = 0; i < n; ++i) ORC_SEED(&h->e[i], (uint64_t)i);
    return h;
}

void ORC_FN(destroy)(ORC_H *h) { if (h) { free(h->e); eps_free(&h->eps); free(h); } }

/* env i's private stream(s) := the reference's reset(seed=seeds[i]) seeding */
void ORC_FN(seed)(ORC_H *h, const uint64_t *seeds) { for (int64_t i = 0; i < h->n; ++i) ORC_SEED(&h->e[i], seeds[i]); }

/* Time-limit override for the short-horizon parity tests (the reference's limit is a constructor constant / config value; the
 * device ABI takes it in its config struct).  Call before reset(). */
void ORC_FN(set_max_steps)(ORC_H *h, int v) { ORC_MAX_STEPS(h) = v; }

/* return and length of each env's last finished episode (orc_epstats.h) */
void ORC_FN(episode_stats)(const ORC_H *h, double *ret, int32_t *len) { eps_get(&h->eps, h->n, ret, len); }

static inline void batch_reset_env(ORC_H *h, ORC_ENV *e, int64_t i) { ORC_RESET(h, e); eps_clear(&h->eps, i); }

void ORC_FN(reset)(ORC_H *h, const uint8_t *mask, ORC_OBS_T *obs) {
    for (int64_t i = 0; i < h->n; ++i) {
        if (!mask || mask[i]) batch_reset_env(h, &h->e[i], i);
        if (obs) ORC_WRITE_OBS(h, &h->e[i], obs + i * ORC_OBS_LEN(h));   /* every row is written, like the device ABI */
    }
}

/* NEXT_STEP: an env that finished at its previous step is reset now, and this step slot is spent on that */
static inline int batch_reset_due(ORC_H *h, ORC_ENV *e, int64_t i) {
    if (h->mode != 0 || !e->needs_reset) return 0;
    batch_reset_env(h, e, i);
    return 1;
}

/* after env i was stepped (reward r, flags f; the episode ended if f != 0): episode statistics, autoreset, and the observation
 * row o (skipped if NULL).  (NEXT_STEP flags the env before its terminal row is written; no ORC_WRITE_OBS reads the flag.) */
static inline void batch_settle(ORC_H *h, ORC_ENV *e, int64_t i, double r, int f, ORC_OBS_T *o, ORC_OBS_T *final_o) {
    eps_add(&h->eps, i, r);
    if (f) {
        e->episodes += 1; eps_done(&h->eps, i);
        if (h->mode == 1) {
            if (final_o) ORC_WRITE_OBS(h, e, final_o);
            batch_reset_env(h, e, i);
        } else if (h->mode == 0) e->needs_reset = 1;
    }
    if (o) ORC_WRITE_OBS(h, e, o);
}

#ifdef ORC_FLOAT_REWARD
#define ORC_REWARD_T float
#define ORC_REWARD64_PARAM
#define ORC_REWARD64_SET(i, v)
#else
#define ORC_REWARD_T double
#define ORC_REWARD64_PARAM double *reward64,
#define ORC_REWARD64_SET(i, v) do { if (reward64) reward64[i] = (v); } while (0)
#endif
#define ORC_IDLE_OUT(i) do { reward[i] = 0.0f; ORC_REWARD64_SET(i, 0.0); terminated[i] = 0; truncated[i] = 0; } while (0)

#ifdef ORC_ACTION_OK
int
#else
void
#endif
ORC_FN(step)(ORC_H *h, ORC_STEP_PARAMS, ORC_OBS_T *obs, float *reward, ORC_REWARD64_PARAM uint8_t *terminated,
             uint8_t *truncated, ORC_OBS_T *final_obs) {
    const int64_t len = ORC_OBS_LEN(h);
#ifdef ORC_ACTION_OK
    int bad = 0;
#endif
    for (int64_t i = 0; i < h->n; ++i) {
        ORC_ENV *e = &h->e[i];
        ORC_OBS_T *o = obs + i * len;
        if (batch_reset_due(h, e, i)) { ORC_WRITE_OBS(h, e, o); ORC_IDLE_OUT(i); continue; }
#ifdef ORC_ACTION_OK
        if (!ORC_ACTION_OK(h, i)) { ++bad; ORC_WRITE_OBS(h, e, o); ORC_IDLE_OUT(i); continue; }   /* the env is left untouched */
#endif
        ORC_REWARD_T r;
        int f = ORC_STEP(h, e, i, &r);
        reward[i] = (float)r; ORC_REWARD64_SET(i, r);
        terminated[i] = (uint8_t)(f & 1); truncated[i] = (uint8_t)((f >> 1) & 1);
        batch_settle(h, e, i, (double)r, f, o, final_obs ? final_obs + i * len : NULL);
    }
#ifdef ORC_ACTION_OK
    return bad;
#endif
}

/* K fused steps per env with the shared counter-hash action source (a NEXT_STEP reset consumes step slot t without hashing an
 * action); per-env reward sums and done counts are accumulated and the observation after the LAST step is written; each of obs,
 * reward_sum and done_count may be NULL.  bench.py's cpu_baseline leg, and the check of the device's rollout entry point. */
void ORC_FN(rollout)(ORC_H *h, int k_steps, uint64_t a_seed, int64_t t0, int64_t env0, ORC_OBS_T *obs, ORC_REWARD_T *reward_sum,
                     int32_t *done_count) {
#ifdef ORC_SCRATCH
    ORC_OBS_T scratch[ORC_SCRATCH], *each = obs ? scratch : NULL;
#else
    ORC_OBS_T *each = NULL;
#endif
    for (int64_t i = 0; i < h->n; ++i) {
        ORC_ENV *e = &h->e[i];
        ORC_REWARD_T rs = 0;
        int dc = 0;
        for (int t = 0; t < k_steps; ++t) {
            if (batch_reset_due(h, e, i)) continue;
            ORC_REWARD_T r;
            int f = hash_step(h, e, a_seed, (uint64_t)(env0 + i), (uint64_t)(t0 + t), &r);
            rs += r;
            if (f) ++dc;
            batch_settle(h, e, i, (double)r, f, each, NULL);
        }
        if (obs) ORC_WRITE_OBS(h, e, obs + i * ORC_OBS_LEN(h));
        if (reward_sum) reward_sum[i] = rs;
        if (done_count) done_count[i] = dc;
    }
}
