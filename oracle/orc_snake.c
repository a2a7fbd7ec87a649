/* oracle/orc_snake.c — CPU restatement of SnakeEnvClassic over a batch of independent envs.
 *
 * TEST INFRASTRUCTURE ONLY (see orc_rng.h).  Follows, line by line in behaviour:
 *   reset             /root/reference/snake_env_classic/snake_env.py:49-65
 *   step              snake_env.py:67-119
 *   _place_food       snake_env.py:121-129
 *   _get_observation  snake_env.py:131-143
 * Parity pins: tests/golden/snake_*.npz + snake_kat.json (produced by tests/golden/gen/gen_snake.py
 * running the reference itself) — checked by tests/test_oracle_snake.py.
 *
 * The batch driver (seed / reset / step / rollout, the autoreset modes, episode statistics) is orc_batch.h.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "orc_rng.h"
#include "orc_epstats.h"

#define SNAKE_MAX_G 32

typedef struct {
    orc_mt rng;               /* family P: CPython global `random`, one private stream per env */
    int len, head;            /* ring buffer of cells, head at ring[head], tail at ring[(head+len-1)%cap] */
    int dir, score, steps;
    int food_r, food_c;       /* -1 when the board is full (reference would spin forever) */
    int needs_reset, board_full;
    int episodes;
    uint16_t ring[SNAKE_MAX_G * SNAKE_MAX_G];
    uint8_t occ[SNAKE_MAX_G * SNAKE_MAX_G];
} snake_env;

typedef struct {
    int64_t n;
    int G, mode, max_steps;
    snake_env *e; orc_eps eps;
} orc_snake;

static void place_food(orc_snake *h, snake_env *e) {      /* snake_env.py:121-129 */
    int G = h->G;
    if (e->len >= G * G) {          /* reference: infinite loop; reported, never silently skipped */
        e->food_r = e->food_c = -1;
        e->board_full = 1;
        return;
    }
    for (;;) {
        int r = orc_py_randint(&e->rng, 0, G - 1);   /* row first ... */
        int c = orc_py_randint(&e->rng, 0, G - 1);   /* ... then column */
        if (!e->occ[r * G + c]) { e->food_r = r; e->food_c = c; return; }
    }
}

static void env_reset(orc_snake *h, snake_env *e) {       /* snake_env.py:49-65 */
    int G = h->G, center = G / 2;
    memset(e->occ, 0, (size_t)G * G);
    e->len = 1; e->head = 0;
    e->ring[0] = (uint16_t)(center * G + center);
    e->occ[center * G + center] = 1;
    e->dir = 1; e->score = 0; e->steps = 0;
    e->needs_reset = 0;
    place_food(h, e);
}

static void write_obs(const orc_snake *h, const snake_env *e, int8_t *obs) {   /* :131-143 */
    int G = h->G;
    for (int i = 0; i < G * G; ++i) obs[i] = (int8_t)e->occ[i];
    if (e->food_r >= 0) obs[e->food_r * G + e->food_c] = 2;
}

/* one reference step(); returns terminated */
static int env_step(orc_snake *h, snake_env *e, int action, float *reward) {   /* :67-119 */
    int G = h->G, cap = G * G;
    int d = action - e->dir;
    if (d != 2 && d != -2) e->dir = action;                                   /* :73-74 */
    int hr = e->ring[e->head] / G, hc = e->ring[e->head] % G;
    int nr = hr, nc = hc;
    if (e->dir == 0) nr = hr - 1; else if (e->dir == 1) nc = hc + 1;          /* :77-85 */
    else if (e->dir == 2) nr = hr + 1; else nc = hc - 1;
    if (nr < 0 || nr >= G || nc < 0 || nc >= G) { *reward = -10.0f; return 1; }   /* :88-90 */
    if (e->occ[nr * G + nc]) { *reward = -10.0f; return 1; }                  /* :93-94 (tail cell counts) */
    e->head = (e->head + cap - 1) % cap;                                      /* :97 insert(0, new_head) */
    e->ring[e->head] = (uint16_t)(nr * G + nc);
    e->occ[nr * G + nc] = 1;
    e->len += 1;
    *reward = 0.0f;
    if (nr == e->food_r && nc == e->food_c) {                                 /* :101-104 */
        e->score += 1;
        *reward = 10.0f;
        place_food(h, e);
    } else {                                                                  /* :107 pop() */
        int tail = e->ring[(e->head + e->len - 1) % cap];
        e->occ[tail] = 0;
        e->len -= 1;
    }
    e->steps += 1;                                                            /* :109 */
    return e->steps >= h->max_steps;                                          /* :113-114 */
}

/* env i's private stream := CPython random.seed(seeds[i]).  step() returns the number of invalid actions (the reference raises
 * ValueError, snake_env.py:69-70).  rollout() does not assemble per-step observations. */
static inline int hash_step(orc_snake *h, snake_env *e, uint64_t a_seed, uint64_t env, uint64_t t, float *r) {
    return env_step(h, e, (int)orc_hash_action(a_seed, env, t, 4, 0), r);
}
#define ORC_NAME snake
#define ORC_ENV snake_env
#define ORC_OBS_T int8_t
#define ORC_OBS_LEN(h) ((h)->G * (h)->G)
#define ORC_FLOAT_REWARD
#define ORC_MAX_STEPS(h) (h)->max_steps
#define ORC_SEED(e, s) orc_py_seed(&(e)->rng, s)
#define ORC_RESET(h, e) env_reset(h, e)
#define ORC_WRITE_OBS(h, e, o) write_obs(h, e, o)
#define ORC_STEP_PARAMS const int32_t *actions
#define ORC_ACTION_OK(h, i) (actions[i] >= 0 && actions[i] <= 3)
#define ORC_STEP(h, e, i, r) env_step(h, e, actions[i], r)
#include "orc_batch.h"

orc_snake *orc_snake_create(int64_t n, int grid, int mode) {
    if (grid < 2 || grid > SNAKE_MAX_G) return NULL;
    orc_snake *h = batch_create(n, mode);
    if (h) { h->G = grid; h->max_steps = 1000; }                             /* :47 */
    return h;
}

/* field: 0 score, 1 snake_length, 2 steps, 3 direction, 4 food_r, 5 food_c, 6 board_full, 7 episodes,
 *        8 head_r, 9 head_c, 10 needs_reset */
void orc_snake_info(const orc_snake *h, int field, int32_t *out) {
    for (int64_t i = 0; i < h->n; ++i) {
        const snake_env *e = &h->e[i];
        int v = 0;
        switch (field) {
            case 0: v = e->score; break;
            case 1: v = e->len; break;
            case 2: v = e->steps; break;
            case 3: v = e->dir; break;
            case 4: v = e->food_r; break;
            case 5: v = e->food_c; break;
            case 6: v = e->board_full; break;
            case 7: v = e->episodes; break;
            case 8: v = e->ring[e->head] / h->G; break;
            case 9: v = e->ring[e->head] % h->G; break;
            case 10: v = e->needs_reset; break;
        }
        out[i] = v;
    }
}

/* Canonical per-env state record shared with the device library's get/set_state
 * (include/cge_amd.h: cge_snake_state): all little-endian int32 unless noted.
 *   [0] len [1] dir [2] food_r [3] food_c [4] score [5] steps [6] needs_reset [7] mt_idx
 *   then uint32 mt[624], then uint16 body[G*G] (head first, unused = 0xFFFF), padded to 4 bytes. */
size_t orc_snake_state_bytes(const orc_snake *h) {
    size_t b = 8 * 4 + 624 * 4 + (size_t)h->G * h->G * 2;
    return (b + 3) & ~(size_t)3;
}

void orc_snake_get_state(const orc_snake *h, void *buf) {
    size_t rec = orc_snake_state_bytes(h);
    int cap = h->G * h->G;
    for (int64_t i = 0; i < h->n; ++i) {
        const snake_env *e = &h->e[i];
        uint8_t *p = (uint8_t *)buf + i * rec;
        int32_t hd[8] = {e->len, e->dir, e->food_r, e->food_c, e->score, e->steps, e->needs_reset, e->rng.idx};
        memcpy(p, hd, 32);
        memcpy(p + 32, e->rng.mt, 624 * 4);
        uint16_t *body = (uint16_t *)(p + 32 + 624 * 4);
        for (int k = 0; k < cap; ++k) body[k] = k < e->len ? e->ring[(e->head + k) % cap] : 0xFFFF;
    }
}

void orc_snake_set_state(orc_snake *h, const void *buf) {
    size_t rec = orc_snake_state_bytes(h);
    int cap = h->G * h->G;
    for (int64_t i = 0; i < h->n; ++i) {
        snake_env *e = &h->e[i];
        const uint8_t *p = (const uint8_t *)buf + i * rec;
        int32_t hd[8];
        memcpy(hd, p, 32);
        e->len = hd[0]; e->dir = hd[1]; e->food_r = hd[2]; e->food_c = hd[3];
        e->score = hd[4]; e->steps = hd[5]; e->needs_reset = hd[6]; e->rng.idx = hd[7];
        memcpy(e->rng.mt, p + 32, 624 * 4);
        const uint16_t *body = (const uint16_t *)(p + 32 + 624 * 4);
        memset(e->occ, 0, (size_t)cap);
        e->head = 0;
        for (int k = 0; k < e->len; ++k) { e->ring[k] = body[k]; e->occ[body[k]] = 1; }
        e->board_full = 0;
    }
}


/* _render_rgb_array (snake_env.py:175-188): rgb[obs == 0] = (0,0,0), rgb[obs == 1] = (0,255,0), rgb[obs == 2] = (255,0,0) */
void orc_snake_render_rgb(const orc_snake *h, uint8_t *rgb) {
    int cells = h->G * h->G;
    int8_t obs[SNAKE_MAX_G * SNAKE_MAX_G];
    for (int64_t i = 0; i < h->n; ++i) {
        write_obs(h, &h->e[i], obs);
        uint8_t *o = rgb + i * cells * 3;
        for (int c = 0; c < cells; ++c) { o[3 * c] = obs[c] == 2 ? 255 : 0; o[3 * c + 1] = obs[c] == 1 ? 255 : 0; o[3 * c + 2] = 0; }
    }
}
