/* cge_amd.h — C ABI of the MI355X-native batched env stepper (libcge_amd.so).
 *
 * The reference (hasnainfarid/Custom_Gymnasium_Environments) has no FFI: its boundary is the
 * Gymnasium Python API of each env class.  Every entry point below therefore cites the reference
 * method it replaces for a whole batch of N independent instances:
 *
 *   <env>_create   <->  Env.__init__            e.g. snake_env_classic/snake_env.py:19-47
 *   <env>_seed     <->  random.seed()/np.random.seed()/reset(seed=) as each env uses them
 *                       (crypto_trading_env.py:305-307, traffic environment.py:145-147; snake never
 *                       seeds `random` itself, snake_env.py:50 — the per-env stream protocol is
 *                       `random.seed(seed_i)` with env i run alone)
 *   <env>_reset    <->  Env.reset()             snake_env.py:49-65, crypto:301-340, traffic:141-166
 *   <env>_step     <->  Env.step(action)        snake_env.py:67-119, crypto:342-398, traffic:168-203
 *   <env>_rollout  <->  the `while not done: env.step(a)` loops of the reference's scripts
 *                       (snake_env_classic/example.py:21-32) fused into one launch
 *   <env>_rollout_final_obs <-> the terminal observation every reference step() RETURNS (snake_env.py:88-94,113-119 and each env's
 *                       step()): step() hands it to final_obs_out in SAME_STEP mode while obs_out gets the reset observation; a fused
 *                       SAME_STEP rollout writes the reset observation to slot t of its trajectory, and the terminal rows go to a side
 *                       output registered here, so that rollout(trajectory) + this output is exactly what k step() calls return.
 *                       The rows are compacted per SEGMENT: <env>_final_obs_segment(h) consecutive envs (the envs one wavefront or
 *                       workgroup steps: 64, traffic 16) own seg_capacity consecutive rows; segment g = envs [g*S, (g+1)*S).
 *                       Caller-owned DEVICE buffers: rows_out [n_segments * seg_capacity, *obs_shape], index_out [n_segments *
 *                       seg_capacity] (int64: step-in-call * n_envs + env) and count_out [n_segments] (int32).  Every later rollout
 *                       call writes count_out[g] = terminal rows segment g produced in THAT call (no zeroing by the caller) and the
 *                       first min(count, seg_capacity) of them, in step order, to the segment's rows; the surplus is dropped (the count
 *                       still says so).  All NULL unregisters.  NEXT_STEP / DISABLED rollouts deliver nothing: slot t of their
 *                       trajectory IS the terminal observation.
 *                       A type whose observation is a key-major SLAB (bus, restaurant, world builder's Dict) has no [rows, row] array
 *                       to compact into: with R = n_segments * seg_capacity its rows_out is the type's ordinary observation slab for
 *                       R envs — bus and restaurant: int32 planes packed, plane p at p * R ints; world builder's Dict: its uint8 slab of
 *                       typed planes for R envs, each plane at a multiple of 16 bytes — and row j of segment g is "env"
 *                       g * seg_capacity + j of that slab.  A row write touches the bytes of its own row in each plane and no others.
 *                       index_out and count_out are as above.
 *   <env>_info     <->  the `info` dicts        snake_env.py:63,117
 *   <env>_episode_stats <-> the per-episode return / length that the reference's training scripts read back from their
 *                       vector-env wrapper as episode_return_mean / episode_len_mean
 *                       (smart_parking_env/examples/training.py:55, smartclimate_rl-main/training/train.py): what
 *                       gymnasium's RecordEpisodeStatistics publishes as infos["episode"] = {"r", "l"}.  Registers two
 *                       caller-owned DEVICE buffers of n_envs elements (either may be NULL; both NULL unregisters): every later
 *                       step() / rollout() writes, for each env that finishes an episode in that call and from inside the
 *                       step kernel itself, the episode's return (float64 sum of its rewards in step order; the accumulator
 *                       lives in the env's state record) and its length in env steps (a NEXT_STEP reset step is not a step
 *                       of any episode).  Entries of envs that did not finish are left untouched; the "_episode" mask of a
 *                       step is terminated | truncated.  A rollout leaves the LAST episode an env finished in it.
 *
 * Conventions
 *   - every function returns CGE_OK (0) or a negative cge_status; nothing throws across the ABI;
 *     <env>_last_error(h) gives a human-readable message for the last failure on that handle.
 *   - all *_out / actions / mask / seeds pointers are DEVICE pointers owned by the caller (e.g. a
 *     torch tensor's data_ptr()) and must stay alive until `stream` reaches the call; host_buf
 *     pointers are HOST pointers.  `stream` is a hipStream_t passed as void* (NULL = default stream).
 *   - all work is enqueued on `stream`; no call synchronises except get_state/set_state/
 *     error_count/destroy.
 *   - get_state / set_state (snake, crypto, traffic, world builder) move the batch in rounds of
 *     4,096 envs: the host memory they stage is bounded by the round, not by n_envs.  set_state
 *     validates the WHOLE buffer before it writes anything: a malformed record anywhere returns
 *     CGE_ERR_INVALID_ARG, last_error names the env ("cge_<env>_set_state: env I: reason"), and
 *     the device state of every env is as it was.
 *   - the library owns the struct-of-arrays env state inside the handle.  A handle is bound to one
 *     device and is not thread-safe; different handles are independent.
 *   - observations are written row-major as (n_envs, *single_obs_shape), exactly the layout
 *     gymnasium.vector.VectorEnv returns.
 *   - trajectory strides of the eight types whose rollout states no multiple (snake, crypto, traffic, parking, climate,
 *     fleet, manufacturing, hospital): obs_step_stride is any number of elements >= one step's n_envs * row — except that
 *     a snake grid whose G*G is a multiple of 4 takes strides that are multiples of 4 only (cge_snake_rollout refuses
 *     others).  With a 16-byte-aligned obs_out, steps 1 .. k-1 of such a trajectory then begin at addresses with the
 *     alignment of the element and no more (float rows 4 bytes, the int8 cells of a snake grid with an odd G*G 1 byte);
 *     the kernels store their 16- and 8-byte pieces there all the same (an odd n_envs already puts a wave's rows at such
 *     addresses), write the rows and nothing else, and never write the padding between steps.  Strides that are multiples
 *     of 4 floats store whole 128-byte lines and are the fast case.  An obs_out that is itself less than 16-byte aligned
 *     is not a tested configuration.  The types added later state their own multiples at their rollout.  World builder's
 *     Dict slab: the bytes between its planes are never written either.
 *   - `env_index0` is the global index of the handle's first env: per-env seeds and the synthetic
 *     action hash are functions of the GLOBAL index so results do not depend on how a batch is
 *     sharded over GPUs.
 *   - <env>_seed with seeds == NULL refuses, before it launches anything, a base_seed whose LAST env
 *     (base_seed + env_index0 + n_envs - 1) passes the limit of the type's generator: 2**32 - 1 where
 *     np.random.seed is among the calls it stands for (crypto, fleet, world builder, space station,
 *     farm), 2**64 - 1 elsewhere (the sum must not wrap uint64_t; seeds of three 32-bit limbs are not
 *     implemented).  It returns CGE_ERR_INVALID_ARG, last_error names the limit, and the streams
 *     are as they were.  A `seeds` array is device memory and is not read back: its values are the
 *     caller's duty.
 */
#ifndef CGE_AMD_H
#define CGE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    CGE_OK = 0,
    CGE_ERR_INVALID_ARG = -1,
    CGE_ERR_HIP = -2,          /* a HIP runtime call failed; see *_last_error */
    CGE_ERR_UNSUPPORTED = -3,  /* configuration not compiled into this build */
    CGE_ERR_NO_DEVICE = -4
} cge_status;

/* gymnasium.vector.AutoresetMode equivalents */
enum {
    CGE_AUTORESET_NEXT_STEP = 0, /* done env returns terminal obs; next step() resets it (action ignored) */
    CGE_AUTORESET_SAME_STEP = 1, /* done env is reset inside step(); terminal obs -> final_obs_out */
    CGE_AUTORESET_DISABLED = 2   /* never reset; stepping a finished env does what the reference does */
};

const char *cge_version(void);
/* Synthetic action source shared by device rollouts, the oracle and the tests:
 * u = mix64(mix64(a_seed + env*0x9E3779B97F4A7C15) + t*0xD1342543DE82EF95 + j); ((u>>32)*n)>>32 */
uint32_t cge_hash_action(uint64_t a_seed, uint64_t env, uint64_t t, uint32_t n, uint32_t j);

/* ------------------------------------------------------------------------------------------ */
/* Snake  (snake_env_classic/snake_env.py: SnakeEnvClassic)                                    */
/*   obs int8 (G,G): 0 empty, 1 snake, 2 food   action int32 in {0 up,1 right,2 down,3 left}    */
/* ------------------------------------------------------------------------------------------ */
typedef struct cge_snake cge_snake;

typedef struct {
    int32_t grid_size;      /* reference default 20 (snake_env.py:19); BASELINE configs use 10; any size from 4 to 30 is compiled in
                             * (other sizes: CGE_ERR_UNSUPPORTED) */
    int32_t max_steps;      /* reference: 1000 (snake_env.py:47); 0 -> 1000; <= 4095 for grid 10, <= 65535 otherwise */
    int32_t autoreset_mode; /* CGE_AUTORESET_* */
    int32_t reserved;
} cge_snake_config;

enum { /* cge_snake_info field ids (int32 per env) */
    CGE_SNAKE_INFO_SCORE = 0,
    CGE_SNAKE_INFO_LENGTH = 1,
    CGE_SNAKE_INFO_STEPS = 2,
    CGE_SNAKE_INFO_DIRECTION = 3,
    CGE_SNAKE_INFO_FOOD_R = 4,
    CGE_SNAKE_INFO_FOOD_C = 5,
    CGE_SNAKE_INFO_BOARD_FULL = 6, /* sticky: reference's _place_food would spin forever (snake_env.py:123) */
    CGE_SNAKE_INFO_EPISODES = 7,
    CGE_SNAKE_INFO_HEAD_R = 8,
    CGE_SNAKE_INFO_HEAD_C = 9,
    CGE_SNAKE_INFO_NEEDS_RESET = 10
};

int cge_snake_create(const cge_snake_config *cfg, int64_t n_envs, int device, int64_t env_index0,
                     cge_snake **out);
int cge_snake_destroy(cge_snake *h);
/* env i's private MT19937 stream := CPython random.seed(s_i); s_i = seeds[i] if seeds != NULL
 * (device pointer, n_envs uint64) else base_seed + env_index0 + i.  Does not reset the envs. */
int cge_snake_seed(cge_snake *h, const uint64_t *seeds, uint64_t base_seed, void *stream);
/* reset envs with mask[i] != 0 (all if mask == NULL); writes ALL n_envs obs rows if obs_out != NULL */
int cge_snake_reset(cge_snake *h, const uint8_t *mask, int8_t *obs_out, void *stream);
/* one step() for every env.  An action outside {0..3} raises ValueError in the reference
 * (snake_env.py:69-70); here the env is left untouched, its row reports (current obs, 0, 0, 0) and a
 * device-side counter is bumped: read it with cge_snake_error_count (which synchronises). */
int cge_snake_step(cge_snake *h, const int32_t *actions, int8_t *obs_out, float *reward_out,
                   uint8_t *terminated_out, uint8_t *truncated_out /*nullable: always 0, snake_env.py:119*/,
                   int8_t *final_obs_out /*nullable*/, void *stream);
/* k_steps fused step()s in ONE launch (env state stays in registers between steps).  actions:
 * [k_steps, n_envs] int32 or NULL -> cge_hash_action(action_seed, env_index0+i, t0+t, 4, 0).  obs_out
 * (nullable): one [n_envs,G,G] buffer rewritten every step (obs_step_stride = 0) or a trajectory buffer
 * [k_steps, n_envs, G, G] (obs_step_stride = n_envs*G*G).  reward_traj_out / terminated_traj_out
 * (nullable): per-step [k_steps, n_envs] outputs, i.e. exactly what k step() calls would return (SAME_STEP: together with
 * the terminal rows of cge_snake_rollout_final_obs);
 * reward_sum_out / done_count_out (nullable) accumulate per env over the k steps. */
int cge_snake_rollout(cge_snake *h, int32_t k_steps, const int32_t *actions, uint64_t action_seed, int64_t t0,
                      int8_t *obs_out, int64_t obs_step_stride, float *reward_traj_out,
                      uint8_t *terminated_traj_out, float *reward_sum_out, int32_t *done_count_out,
                      void *stream);
/* terminal observations of SAME_STEP rollouts, compacted per segment of 64 envs: see <env>_rollout_final_obs at the top of this file */
int cge_snake_rollout_final_obs(cge_snake *h, int8_t *rows_out, int64_t *index_out, int64_t seg_capacity, int32_t *count_out);
int64_t cge_snake_final_obs_segment(const cge_snake *h);
int cge_snake_info(cge_snake *h, int32_t field_id, int32_t *out, void *stream);
/* render_mode="rgb_array" (snake_env.py:175-188): uint8 [n_envs, G, G, 3] (4-byte aligned) — empty (0,0,0), snake (0,255,0),
 * food (255,0,0) — of the CURRENT state of every env.  The pygame window of render_mode="human" (:153-173) is out of scope. */
int cge_snake_render_rgb(cge_snake *h, uint8_t *rgb_out, void *stream);
/* canonical per-env state record (host memory), identical to the oracle's: 8 int32 {len, dir, food_r,
 * food_c, score, steps, needs_reset, mt_idx}, uint32 mt[624] (CPython layout: words >= mt_idx are
 * generated-but-unconsumed), uint16 body[G*G] head first (0xFFFF unused), zero-padded to 4 bytes
 * (get_state writes the padding too: every byte of host_buf is written). */
size_t cge_snake_state_bytes(const cge_snake *h);
int cge_snake_get_state(cge_snake *h, void *host_buf, void *stream);
int cge_snake_set_state(cge_snake *h, const void *host_buf, void *stream);
/* synchronises `stream`, returns and clears the number of invalid actions seen since the last call */
int64_t cge_snake_error_count(cge_snake *h, void *stream);
/* bytes of device memory held by the handle (SoA state + RNG streams) */
size_t cge_snake_device_bytes(const cge_snake *h);
int cge_snake_episode_stats(cge_snake *h, double *return_out, int32_t *length_out);
const char *cge_snake_last_error(const cge_snake *h);
/* the kernel(s) the last step() / rollout() call on this handle launched, by the name rocprofv3 --kernel-trace prints
 * ("" before the first call): lets a measurement attribute its time and PMC bytes to what actually ran. */
const char *cge_snake_last_kernel(const cge_snake *h);

/* ------------------------------------------------------------------------------------------ */
/* Crypto  (crypto_trading_env/crypto_trading_env.py: CryptoTradingEnv)                        */
/*   obs float32 (261,) (:505-561; the declared space says 260, :286)                          */
/*   action: int32 in {0 hold,1 buy 5%,2 buy 20%,3 sell 5%,4 sell 20%} (discrete) or float32[2] */
/*   (continuous: [buy, sell], :407-422).  All state arithmetic is float64 as in the reference; */
/*   O/H/L/V history is stored as float32 (it only feeds the float32 obs), closes as float64.   */
/* ------------------------------------------------------------------------------------------ */
typedef struct cge_crypto cge_crypto;

typedef struct {                 /* TradingConfig, crypto_trading_env.py:28-38 (history_length is fixed at 50) */
    double initial_balance;          /* 10000.0 */
    double trading_fee_rate;         /* 0.001 */
    double slippage_rate;            /* 0.0005 */
    double min_price;                /* 100.0 */
    double max_price;                /* 100000.0 */
    double volatility_base;          /* 0.02 */
    double market_psychology_factor; /* 0.1 */
    int32_t max_steps;               /* 1000 (:278); <= 65535 */
    int32_t action_type;             /* 0 discrete, 1 continuous (:247) */
    int32_t autoreset_mode;          /* CGE_AUTORESET_* */
    int32_t reserved;
} cge_crypto_config;

enum { /* cge_crypto_info field ids (float64 per env), the keys of step()'s info dict (:390-398) */
    CGE_CRYPTO_INFO_PORTFOLIO_VALUE = 0,
    CGE_CRYPTO_INFO_CASH = 1,
    CGE_CRYPTO_INFO_HOLDINGS = 2,
    CGE_CRYPTO_INFO_CURRENT_PRICE = 3,
    CGE_CRYPTO_INFO_MARKET_PSYCHOLOGY = 4,
    CGE_CRYPTO_INFO_REGIME = 5,       /* 0 bull_run 1 bear_market 2 sideways 3 crash 4 recovery (:20-25) */
    CGE_CRYPTO_INFO_STEP = 6,
    CGE_CRYPTO_INFO_TREND_STRENGTH = 7,
    CGE_CRYPTO_INFO_EPISODES = 8,
    CGE_CRYPTO_INFO_NEEDS_RESET = 9,
    CGE_CRYPTO_INFO_CASH_KIND = 10    /* dtype of self.cash under NumPy>=2: 0 Python float, 1 float32, 2 float64 */
};

void cge_crypto_default_config(cge_crypto_config *cfg);
int cge_crypto_create(const cge_crypto_config *cfg, int64_t n_envs, int device, int64_t env_index0,
                      cge_crypto **out);
int cge_crypto_destroy(cge_crypto *h);
/* reset(seed=s) seeding (:305-307): random.seed(s_i) AND np.random.seed(s_i); s_i as for snake; s_i must
 * be < 2**32 (np.random.seed raises otherwise).  Does not reset the envs; the MarketSimulator state
 * (regime, trend, psychology) is never reset, as in the reference (:257). */
int cge_crypto_seed(cge_crypto *h, const uint64_t *seeds, uint64_t base_seed, void *stream);
int cge_crypto_reset(cge_crypto *h, const uint8_t *mask, float *obs_out, void *stream);
/* actions: int32[n_envs] (discrete; any value outside 1..4 is a hold, as in the reference) or
 * float32[n_envs,2] (continuous).  reward_out is float32(reward); terminated = step>=max_steps or
 * portfolio<=0 or portfolio>=10*initial (:382-386); truncated always 0 (nullable). */
int cge_crypto_step(cge_crypto *h, const void *actions, float *obs_out, float *reward_out,
                    uint8_t *terminated_out, uint8_t *truncated_out, float *final_obs_out, void *stream);
/* k fused step()s.  actions NULL -> hash actions (discrete: cge_hash_action(seed,env,t,5,0); continuous:
 * (cge_hash(..,j) >> 40) / 2^23 - 1 for j = 0,1); else [k, n_envs(,2)].  obs_out / obs_step_stride
 * (in floats) as for snake; reward_sum_out is float64. */
int cge_crypto_rollout(cge_crypto *h, int32_t k_steps, const void *actions, uint64_t action_seed, int64_t t0,
                       float *obs_out, int64_t obs_step_stride, float *reward_traj_out,
                       uint8_t *terminated_traj_out, double *reward_sum_out, int32_t *done_count_out,
                       void *stream);
/* terminal observations of SAME_STEP rollouts, compacted per segment of 64 envs: see <env>_rollout_final_obs at the top of this file */
int cge_crypto_rollout_final_obs(cge_crypto *h, float *rows_out, int64_t *index_out, int64_t seg_capacity, int32_t *count_out);
int64_t cge_crypto_final_obs_segment(const cge_crypto *h);
int cge_crypto_info(cge_crypto *h, int32_t field_id, double *out, void *stream);
/* canonical record (host), identical to the oracle's: int32[12] {regime, step, needs_reset, cash_kind,
 * P_idx, L_idx, has_gauss, episodes, 0,0,0,0}; double[6] {cash, holdings, psych, trend_strength, gauss, episode_return_so_far (the oracle writes 0)};
 * uint32 P[624]; uint32 L[624]; double hist[50][5] (O,H,L,C,V, oldest first; O/H/L/V round-trip
 * through float32 on the device). */
size_t cge_crypto_state_bytes(const cge_crypto *h);
int cge_crypto_get_state(cge_crypto *h, void *host_buf, void *stream);
int cge_crypto_set_state(cge_crypto *h, const void *host_buf, void *stream);
size_t cge_crypto_device_bytes(const cge_crypto *h);
int cge_crypto_episode_stats(cge_crypto *h, double *return_out, int32_t *length_out);
const char *cge_crypto_last_error(const cge_crypto *h);
const char *cge_crypto_last_kernel(const cge_crypto *h);

/* ------------------------------------------------------------------------------------------ */
/* Traffic  (traffic_management_env/environment.py: TrafficManagementEnv, utils.py, config.py)  */
/*   obs float32 (14 NI + 4,) (:313-363; 130 for the default NI = 9 intersections)               */
/*   action int32[NI] in {0 maintain,1 NS_GREEN,2 EW_GREEN}                                      */
/*   State is the collapsed form of SURVEY.md 8a (queue length / waiting sum / arrivals-at-      */
/*   destination per queue, counters per intersection, vehicle count): _update_vehicles          */
/*   (:251-269) never moves a vehicle, so nothing else is observable.  Bit-exact: integer state,  */
/*   float64 reward arithmetic in the reference's order, float32 obs from float64 quotients.     */
/* ------------------------------------------------------------------------------------------ */
typedef struct cge_traffic cge_traffic;

typedef struct {                 /* TrafficManagementEnv.__init__ kwargs (:61-66) + config.py */
    int32_t grid_rows, grid_cols;    /* (5, 5); any grid of 1..64 rows / columns: the routes walk the whole grid (utils.py:196-214) */
    int32_t num_intersections;       /* 9; the env uses NI = min(num_intersections, rows*cols) (:79).  Any NI from 2 to 16: the layouts the
                                      * reference's scripts build (4, 9, 16: simple_test.py:71-76, config.py:6-7, USAGE_EXAMPLES.md:32-38)
                                      * have kernels of their own, the others share run-time-NI instances.  NI = 1 raises in the reference
                                      * at the first spawn (randint(2, 1), utils.py:181); NI = 1 or > 16: CGE_ERR_UNSUPPORTED */
    int32_t max_vehicles;            /* 50; <= 127 and max_vehicles*max_steps <= 262143 (queue word: len:7 dest:7 wait:18) */
    double spawn_rate;               /* 0.3 */
    int32_t max_steps;               /* MAX_TIMESTEPS = 1000 */
    int32_t autoreset_mode;          /* CGE_AUTORESET_* */
} cge_traffic_config;

enum { /* cge_traffic_info field ids (int32 per env; `index` selects the intersection 0..NI-1 or queue 0..4NI-1 = 4*i+dir) */
    CGE_TRAFFIC_INFO_TIMESTEP = 0,
    CGE_TRAFFIC_INFO_NUM_VEHICLES = 1,
    CGE_TRAFFIC_INFO_LIGHT_PHASE = 2,       /* 0 NS_GREEN 1 NS_YELLOW 2 EW_GREEN 3 EW_YELLOW */
    CGE_TRAFFIC_INFO_LIGHT_TIMER = 3,
    CGE_TRAFFIC_INFO_VEHICLES_PASSED = 4,
    CGE_TRAFFIC_INFO_TOTAL_WAITING_TIME = 5,
    CGE_TRAFFIC_INFO_QUEUE_LEN = 6,         /* dir order NORTH, EAST, SOUTH, WEST (utils.py:17-22) */
    CGE_TRAFFIC_INFO_QUEUE_DEST = 7,
    CGE_TRAFFIC_INFO_QUEUE_WAIT = 8,
    CGE_TRAFFIC_INFO_EPISODES = 9,
    CGE_TRAFFIC_INFO_NEEDS_RESET = 10
};

void cge_traffic_default_config(cge_traffic_config *cfg);
int cge_traffic_create(const cge_traffic_config *cfg, int64_t n_envs, int device, int64_t env_index0,
                       cge_traffic **out);
int cge_traffic_destroy(cge_traffic *h);
/* reset(seed=s) seeding (:145-147): random.seed(s_i); the NumPy generator it also seeds is never drawn from */
int cge_traffic_seed(cge_traffic *h, const uint64_t *seeds, uint64_t base_seed, void *stream);
int cge_traffic_reset(cge_traffic *h, const uint8_t *mask, float *obs_out, void *stream);
/* actions: int32 [n_envs, NI]; values other than 1/2 maintain the phase, as in the reference (:214-220) */
int cge_traffic_step(cge_traffic *h, const int32_t *actions, float *obs_out, float *reward_out,
                     uint8_t *terminated_out, uint8_t *truncated_out /*nullable*/, float *final_obs_out,
                     void *stream);
/* k fused steps; actions [k, n_envs, NI] or NULL -> cge_hash_action(seed, env, t, 3, j) for intersection j */
int cge_traffic_rollout(cge_traffic *h, int32_t k_steps, const int32_t *actions, uint64_t action_seed, int64_t t0,
                        float *obs_out, int64_t obs_step_stride, float *reward_traj_out,
                        uint8_t *terminated_traj_out, double *reward_sum_out, int32_t *done_count_out,
                        void *stream);
/* terminal observations of SAME_STEP rollouts, compacted per segment of 16 envs: see <env>_rollout_final_obs at the top of this file */
int cge_traffic_rollout_final_obs(cge_traffic *h, float *rows_out, int64_t *index_out, int64_t seg_capacity, int32_t *count_out);
int64_t cge_traffic_final_obs_segment(const cge_traffic *h);
int cge_traffic_info(cge_traffic *h, int32_t field_id, int32_t index, int32_t *out, void *stream);
/* info['total_reward'] (:372): float64 running sum of the episode's rewards */
int cge_traffic_total_reward(cge_traffic *h, double *out, void *stream);
/* canonical record (host), identical to the oracle's: int32[6] {timestep, n_vehicles, needs_reset, mt_idx,
 * episodes, 0}; double total_reward; int32 phase[NI], timer[NI], passed[NI], total_wait[NI], qlen[4 NI], qdest[4 NI],
 * qwait[4 NI]; uint32 mt[624]. */
size_t cge_traffic_state_bytes(const cge_traffic *h);
int cge_traffic_get_state(cge_traffic *h, void *host_buf, void *stream);
int cge_traffic_set_state(cge_traffic *h, const void *host_buf, void *stream);
size_t cge_traffic_device_bytes(const cge_traffic *h);
int cge_traffic_episode_stats(cge_traffic *h, double *return_out, int32_t *length_out);
const char *cge_traffic_last_error(const cge_traffic *h);
const char *cge_traffic_last_kernel(const cge_traffic *h);

/* ------------------------------------------------------------------------------------------ */
/* Smart parking  (smart_parking_env/core/parking_env.py: SmartParkingEnv + customer/parking_lot/pricing) */
/*   obs float32 (13,) in [0,1] (:306-369)   action int32 in 0..7 (:161-195)   1440 one-minute steps     */
/*   Bit-exact: integer state, float64 price/satisfaction/reward arithmetic in the reference's order.   */
/* ------------------------------------------------------------------------------------------ */
typedef struct cge_parking cge_parking;

typedef struct {
    int32_t max_steps;        /* TIMESTEPS_PER_EPISODE = 1440 (config.py:15); <= 60000 */
    int32_t autoreset_mode;   /* CGE_AUTORESET_* */
} cge_parking_config;

enum { /* cge_parking_info int32 fields (`index` = zone 0..2 where noted) — the counters behind _get_info (:371-399) */
    CGE_PARKING_INFO_TIMESTEP = 0,
    CGE_PARKING_INFO_TOTAL_CUSTOMERS = 1,
    CGE_PARKING_INFO_REJECTED = 2,
    CGE_PARKING_INFO_SATISFIED = 3,
    CGE_PARKING_INFO_TOTAL_WAIT_TIME = 4,
    CGE_PARKING_INFO_QUEUE_LENGTH = 5,
    CGE_PARKING_INFO_PRICE_CHANGES_THIS_HOUR = 6,
    CGE_PARKING_INFO_ZONE_OCCUPIED = 7,   /* index = zone */
    CGE_PARKING_INFO_PRICE_LEVEL = 8,     /* index = zone */
    CGE_PARKING_INFO_EPISODES = 9,
    CGE_PARKING_INFO_NEEDS_RESET = 10
};
enum { CGE_PARKING_INFO64_EPISODE_REVENUE = 0, CGE_PARKING_INFO64_EPISODE_SATISFACTION = 1 };

int cge_parking_create(const cge_parking_config *cfg, int64_t n_envs, int device, int64_t env_index0,
                       cge_parking **out);
int cge_parking_destroy(cge_parking *h);
/* the env never seeds `random` (parking_env.py:81): env i's private stream := random.seed(s_i), as for snake */
int cge_parking_seed(cge_parking *h, const uint64_t *seeds, uint64_t base_seed, void *stream);
int cge_parking_reset(cge_parking *h, const uint8_t *mask, float *obs_out, void *stream);
/* actions int32[n_envs]; values outside 0..7 are an idle step, as in the reference (no branch matches) */
int cge_parking_step(cge_parking *h, const int32_t *actions, float *obs_out, float *reward_out,
                     uint8_t *terminated_out, uint8_t *truncated_out /*nullable*/, float *final_obs_out,
                     void *stream);
int cge_parking_rollout(cge_parking *h, int32_t k_steps, const int32_t *actions, uint64_t action_seed, int64_t t0,
                        float *obs_out, int64_t obs_step_stride, float *reward_traj_out,
                        uint8_t *terminated_traj_out, double *reward_sum_out, int32_t *done_count_out,
                        void *stream);
/* terminal observations of SAME_STEP rollouts, compacted per segment of 64 envs: see <env>_rollout_final_obs at the top of this file */
int cge_parking_rollout_final_obs(cge_parking *h, float *rows_out, int64_t *index_out, int64_t seg_capacity, int32_t *count_out);
int64_t cge_parking_final_obs_segment(const cge_parking *h);
int cge_parking_info(cge_parking *h, int32_t field_id, int32_t index, int32_t *out, void *stream);
int cge_parking_info64(cge_parking *h, int32_t field_id, double *out, void *stream);
/* whole-handle checkpoint (host memory, opaque: 32-byte header + the device arrays in device layout); restores only
 * into a handle created with the same n_envs and config; both calls synchronise `stream` */
size_t cge_parking_snapshot_bytes(const cge_parking *h);
int cge_parking_snapshot_get(cge_parking *h, void *host_buf, void *stream);
int cge_parking_snapshot_set(cge_parking *h, const void *host_buf, void *stream);
size_t cge_parking_device_bytes(const cge_parking *h);
int cge_parking_episode_stats(cge_parking *h, double *return_out, int32_t *length_out);
const char *cge_parking_last_error(const cge_parking *h);
const char *cge_parking_last_kernel(const cge_parking *h);

/* ------------------------------------------------------------------------------------------ */
/* SmartClimate  (smartclimate_rl-main/smartclimate/env.py: SmartClimateEnv, utils.py)          */
/*   obs float32 (9,): room_temp, num_people, time_of_day, outside_temp, ac_setting, lights[4]  */
/*   action Dict{ac_temp float32[1] (clipped to 16..32), lights MultiBinary(4)} (:39-47)        */
/*   float64 dynamics; generator family D: a private default_rng(seed) (PCG64) per env —        */
/*   uniform, Lemire integers on buffered 32-bit draws, ziggurat normal, choice(p).             */
/* ------------------------------------------------------------------------------------------ */
typedef struct cge_climate cge_climate;

typedef struct {
    int32_t max_occupancy;    /* 8 (:19); <= 15 */
    int32_t episode_minutes;  /* 1440 (:21); <= 65535 */
    int32_t autoreset_mode;   /* CGE_AUTORESET_* */
    int32_t reserved;
} cge_climate_config;

enum { /* cge_climate_info float64 fields */
    CGE_CLIMATE_INFO_ROOM_TEMP = 0, CGE_CLIMATE_INFO_OUTSIDE_TEMP = 1, CGE_CLIMATE_INFO_AC_SETTING = 2,
    CGE_CLIMATE_INFO_ENERGY_USAGE = 3, CGE_CLIMATE_INFO_TOTAL_REWARD = 4, CGE_CLIMATE_INFO_NUM_PEOPLE = 5,
    CGE_CLIMATE_INFO_STEP = 6, CGE_CLIMATE_INFO_COMFORT_TIME = 7, CGE_CLIMATE_INFO_EPISODES = 8,
    CGE_CLIMATE_INFO_NEEDS_RESET = 9
};

int cge_climate_create(const cge_climate_config *cfg, int64_t n_envs, int device, int64_t env_index0,
                       cge_climate **out);
int cge_climate_destroy(cge_climate *h);
/* reset(seed=s) (:63-65): env i's generator := np.random.default_rng(s_i) (SeedSequence -> PCG64) */
int cge_climate_seed(cge_climate *h, const uint64_t *seeds, uint64_t base_seed, void *stream);
int cge_climate_reset(cge_climate *h, const uint8_t *mask, float *obs_out, void *stream);
/* ac_temp float32[n_envs] (action['ac_temp'][0]), lights int8[n_envs,4] */
int cge_climate_step(cge_climate *h, const float *ac_temp, const int8_t *lights, float *obs_out, float *reward_out,
                     uint8_t *terminated_out, uint8_t *truncated_out /*nullable*/, float *final_obs_out,
                     void *stream);
/* k fused steps; ac_temp [k,n] / lights [k,n,4] or both NULL -> hash actions:
 * ac = float32(16 + 16*(hash(seed,env,t,j=0) >> 40)/2^24), lights[j] = cge_hash_action(seed,env,t,2,1+j) */
int cge_climate_rollout(cge_climate *h, int32_t k_steps, const float *ac_temp, const int8_t *lights,
                        uint64_t action_seed, int64_t t0, float *obs_out, int64_t obs_step_stride,
                        float *reward_traj_out, uint8_t *terminated_traj_out, double *reward_sum_out,
                        int32_t *done_count_out, void *stream);
/* terminal observations of SAME_STEP rollouts, compacted per segment of 64 envs: see <env>_rollout_final_obs at the top of this file */
int cge_climate_rollout_final_obs(cge_climate *h, float *rows_out, int64_t *index_out, int64_t seg_capacity, int32_t *count_out);
int64_t cge_climate_final_obs_segment(const cge_climate *h);
int cge_climate_info(cge_climate *h, int32_t field_id, double *out, void *stream);
/* whole-handle checkpoint (host memory, opaque: 32-byte header + the device arrays in device layout); restores only
 * into a handle created with the same n_envs and config; both calls synchronise `stream` */
size_t cge_climate_snapshot_bytes(const cge_climate *h);
int cge_climate_snapshot_get(cge_climate *h, void *host_buf, void *stream);
int cge_climate_snapshot_set(cge_climate *h, const void *host_buf, void *stream);
size_t cge_climate_device_bytes(const cge_climate *h);
int cge_climate_episode_stats(cge_climate *h, double *return_out, int32_t *length_out);
const char *cge_climate_last_error(const cge_climate *h);
const char *cge_climate_last_kernel(const cge_climate *h);

/* ------------------------------------------------------------------------------------------ */
/* Fleet  (fleet_management_env/fleet_env.py: FleetManagementEnv)                               */
/*   obs float32 (76,) (:555-593; the declared space says 87)   action int32[3] in 0..7 (:157)   */
/*   terminated (:537-553) AND truncated (timestep >= 800, :265) are both reported.              */
/*   Generators: NumPy legacy np.random + CPython random, both seeded by reset(seed=) (:187-189). */
/* ------------------------------------------------------------------------------------------ */
typedef struct cge_fleet cge_fleet;

typedef struct {
    int32_t max_timesteps;    /* 800 (:123); <= 1023 */
    int32_t autoreset_mode;   /* CGE_AUTORESET_* */
} cge_fleet_config;

enum { /* cge_fleet_info float64 fields (_get_info :595-608 and per-vehicle state) */
    CGE_FLEET_INFO_TIMESTEP = 0, CGE_FLEET_INFO_MISSED_DEADLINES = 1, CGE_FLEET_INFO_COMPLETED_DELIVERIES = 2,
    CGE_FLEET_INFO_NUM_REQUESTS = 3, CGE_FLEET_INFO_WEATHER_EFFECT = 4, CGE_FLEET_INFO_TOTAL_REWARD = 5,
    CGE_FLEET_INFO_EPISODES = 6, CGE_FLEET_INFO_NEEDS_RESET = 7,
    CGE_FLEET_INFO_FUEL0 = 8, CGE_FLEET_INFO_FUEL1 = 9, CGE_FLEET_INFO_FUEL2 = 10
};

int cge_fleet_create(const cge_fleet_config *cfg, int64_t n_envs, int device, int64_t env_index0, cge_fleet **out);
int cge_fleet_destroy(cge_fleet *h);
/* reset(seed=s): np.random.seed(s_i) and random.seed(s_i); s_i < 2**32 */
int cge_fleet_seed(cge_fleet *h, const uint64_t *seeds, uint64_t base_seed, void *stream);
int cge_fleet_reset(cge_fleet *h, const uint8_t *mask, float *obs_out, void *stream);
/* actions int32 [n_envs, 3]; a value outside 0..7 costs -10 (:326-327).  truncated_out is REQUIRED here. */
int cge_fleet_step(cge_fleet *h, const int32_t *actions, float *obs_out, float *reward_out, uint8_t *terminated_out,
                   uint8_t *truncated_out, float *final_obs_out, void *stream);
/* done_count counts terminated-or-truncated steps; terminated_traj_out gets terminated | truncated << 1.
 * k_steps >= 2: the launches that finish step t (redraws, resets, their rows) run on a stream the handle owns, beside step t + 1's
 * step launch on `stream`; the call orders them with events and joins the side stream into `stream` before it returns, so to the
 * caller everything is ordered on `stream` as usual (buffers must stay valid until `stream` reaches that point). */
int cge_fleet_rollout(cge_fleet *h, int32_t k_steps, const int32_t *actions, uint64_t action_seed, int64_t t0,
                      float *obs_out, int64_t obs_step_stride, float *reward_traj_out, uint8_t *terminated_traj_out,
                      double *reward_sum_out, int32_t *done_count_out, void *stream);
/* terminal observations of SAME_STEP rollouts, compacted per segment of 64 envs: see <env>_rollout_final_obs at the top of this file */
int cge_fleet_rollout_final_obs(cge_fleet *h, float *rows_out, int64_t *index_out, int64_t seg_capacity, int32_t *count_out);
int64_t cge_fleet_final_obs_segment(const cge_fleet *h);
int cge_fleet_info(cge_fleet *h, int32_t field_id, double *out, void *stream);
/* whole-handle checkpoint (host memory, opaque: 32-byte header + the device arrays in device layout); restores only
 * into a handle created with the same n_envs and config; both calls synchronise `stream` */
size_t cge_fleet_snapshot_bytes(const cge_fleet *h);
int cge_fleet_snapshot_get(cge_fleet *h, void *host_buf, void *stream);
int cge_fleet_snapshot_set(cge_fleet *h, const void *host_buf, void *stream);
size_t cge_fleet_device_bytes(const cge_fleet *h);
int cge_fleet_episode_stats(cge_fleet *h, double *return_out, int32_t *length_out);
/* optional: cge_fleet_step also writes terminated | truncated per env into done_out (device, n_envs bytes) until it is set to NULL —
 * the mask gymnasium's SAME_STEP infos["_final_obs"] and the episode statistics want, without a second launch */
int cge_fleet_done_mask(cge_fleet *h, uint8_t *done_out);
const char *cge_fleet_last_error(const cge_fleet *h);
const char *cge_fleet_last_kernel(const cge_fleet *h);

/* ------------------------------------------------------------------------------------------ */
/* Manufacturing  (smart_manufacturing_env/manufacturing_env.py: SmartManufacturingEnv)         */
/*   obs float32 (73,) (:194-250)   action int32 in 0..24 (:85, :303-359)                        */
/*   terminated (:555-578) AND truncated (timestep >= 1500, :282) are both reported.             */
/*   Generator: gymnasium's self.np_random = Generator(PCG64(SeedSequence(seed))) (:115).        */
/* ------------------------------------------------------------------------------------------ */
typedef struct cge_manufacturing cge_manufacturing;

typedef struct {
    int32_t max_steps;        /* 1500 (:282, :569); <= 1500 (bounds the per-episode product table) */
    int32_t autoreset_mode;   /* CGE_AUTORESET_* */
} cge_manufacturing_config;

enum { /* cge_manufacturing_info float64 fields (info dict :293-299, oee_metrics :533-548, list lengths) */
    CGE_MANUFACTURING_INFO_RAW_MATERIAL = 0, CGE_MANUFACTURING_INFO_ENERGY_CONSUMPTION = 1, CGE_MANUFACTURING_INFO_TOTAL_REWARD = 2,
    CGE_MANUFACTURING_INFO_IN_SYSTEM = 3, CGE_MANUFACTURING_INFO_COMPLETED = 4, CGE_MANUFACTURING_INFO_SCRAPPED = 5,
    CGE_MANUFACTURING_INFO_PRODUCT_IDS = 6, CGE_MANUFACTURING_INFO_HISTORY_LEN = 7, CGE_MANUFACTURING_INFO_OEE_AVAILABILITY = 8,
    CGE_MANUFACTURING_INFO_OEE_PERFORMANCE = 9, CGE_MANUFACTURING_INFO_OEE_QUALITY = 10, CGE_MANUFACTURING_INFO_TIMESTEP = 11,
    CGE_MANUFACTURING_INFO_EPISODES = 12, CGE_MANUFACTURING_INFO_NEEDS_RESET = 13, CGE_MANUFACTURING_INFO_OVERFLOW = 14,
    CGE_MANUFACTURING_INFO_COMPLETED_TYPE0 = 15   /* .. + 5: products_completed['A'..'F'] (manufacturing_env.py:157,485), the dict info carries (:296) */
};

int cge_manufacturing_create(const cge_manufacturing_config *cfg, int64_t n_envs, int device, int64_t env_index0, cge_manufacturing **out);
int cge_manufacturing_destroy(cge_manufacturing *h);
/* reset(seed=s): env i gets Generator(PCG64(SeedSequence(s_i))); s_i = seeds[i] or base_seed + env_index0 + i */
int cge_manufacturing_seed(cge_manufacturing *h, const uint64_t *seeds, uint64_t base_seed, void *stream);
int cge_manufacturing_reset(cge_manufacturing *h, const uint8_t *mask, float *obs_out, void *stream);
/* actions int32 [n_envs]; a value outside 0..24 is a no-op (falls through every branch of :303-359). */
int cge_manufacturing_step(cge_manufacturing *h, const int32_t *actions, float *obs_out, float *reward_out, uint8_t *terminated_out,
                           uint8_t *truncated_out, float *final_obs_out, void *stream);
/* done_count counts terminated-or-truncated steps; terminated_traj_out gets terminated | truncated << 1 */
int cge_manufacturing_rollout(cge_manufacturing *h, int32_t k_steps, const int32_t *actions, uint64_t action_seed, int64_t t0,
                              float *obs_out, int64_t obs_step_stride, float *reward_traj_out, uint8_t *terminated_traj_out,
                              double *reward_sum_out, int32_t *done_count_out, void *stream);
/* terminal observations of SAME_STEP rollouts, compacted per segment of 64 envs: see <env>_rollout_final_obs at the top of this file */
int cge_manufacturing_rollout_final_obs(cge_manufacturing *h, float *rows_out, int64_t *index_out, int64_t seg_capacity, int32_t *count_out);
int64_t cge_manufacturing_final_obs_segment(const cge_manufacturing *h);
int cge_manufacturing_info(cge_manufacturing *h, int32_t field_id, double *out, void *stream);
/* whole-handle checkpoint (host memory, opaque: 32-byte header + the device arrays in device layout); restores only
 * into a handle created with the same n_envs and config; both calls synchronise `stream` */
size_t cge_manufacturing_snapshot_bytes(const cge_manufacturing *h);
int cge_manufacturing_snapshot_get(cge_manufacturing *h, void *host_buf, void *stream);
int cge_manufacturing_snapshot_set(cge_manufacturing *h, const void *host_buf, void *stream);
size_t cge_manufacturing_device_bytes(const cge_manufacturing *h);
int cge_manufacturing_episode_stats(cge_manufacturing *h, double *return_out, int32_t *length_out);
/* optional: cge_manufacturing_step also writes terminated | truncated per env into done_out (device, n_envs bytes) until it is set to NULL —
 * the mask gymnasium's SAME_STEP infos["_final_obs"] and the episode statistics want, without a second launch */
int cge_manufacturing_done_mask(cge_manufacturing *h, uint8_t *done_out);
const char *cge_manufacturing_last_error(const cge_manufacturing *h);
const char *cge_manufacturing_last_kernel(const cge_manufacturing *h);

/* ------------------------------------------------------------------------------------------ */
/* Hospital  (hospital_management_env/hospital_env.py: HospitalManagementEnv)                   */
/*   obs float32 (243,) (:256-321; the declared space says 295)   action int32 in 0..34 (:165)   */
/*   terminated (:726-742) AND truncated (current_time >= 1440, :357) are both reported.         */
/*   Generator: the process-global CPython `random`; the env never seeds it (:186), so           */
/*   cge_hospital_seed is the caller's random.seed(s_i) for env i.                               */
/* ------------------------------------------------------------------------------------------ */
typedef struct cge_hospital cge_hospital;

typedef struct {
    int32_t max_episode_length;   /* 1440 (:94); <= 2000 */
    int32_t autoreset_mode;       /* CGE_AUTORESET_* */
} cge_hospital_config;

enum { /* cge_hospital_info float64 fields (info dict :362-367 and internal counters) */
    CGE_HOSPITAL_INFO_DEATHS = 0, CGE_HOSPITAL_INFO_PATIENTS_TREATED = 1, CGE_HOSPITAL_INFO_TOTAL_WAIT_TIME = 2, CGE_HOSPITAL_INFO_TIME = 3,
    CGE_HOSPITAL_INFO_OUTBREAK_ACTIVE = 4, CGE_HOSPITAL_INFO_MASS_CASUALTY_EVENT = 5, CGE_HOSPITAL_INFO_NEXT_PATIENT_ID = 6,
    CGE_HOSPITAL_INFO_QUEUE0 = 7, /* .. QUEUE0 + 5: len(patient_queues[Department(d)]) */
    CGE_HOSPITAL_INFO_OCCUPIED_BEDS = 13, CGE_HOSPITAL_INFO_MEDICINE_TOTAL = 14, CGE_HOSPITAL_INFO_EPISODES = 15,
    CGE_HOSPITAL_INFO_NEEDS_RESET = 16, CGE_HOSPITAL_INFO_OVERFLOW = 17
};

int cge_hospital_create(const cge_hospital_config *cfg, int64_t n_envs, int device, int64_t env_index0, cge_hospital **out);
int cge_hospital_destroy(cge_hospital *h);
/* random.seed(s_i) for env i; s_i = seeds[i] or base_seed + env_index0 + i */
int cge_hospital_seed(cge_hospital *h, const uint64_t *seeds, uint64_t base_seed, void *stream);
int cge_hospital_reset(cge_hospital *h, const uint8_t *mask, float *obs_out, void *stream);
/* actions int32 [n_envs]; a value outside 0..34 is a no-op.  truncated_out is REQUIRED. */
int cge_hospital_step(cge_hospital *h, const int32_t *actions, float *obs_out, float *reward_out, uint8_t *terminated_out,
                      uint8_t *truncated_out, float *final_obs_out, void *stream);
/* done_count counts terminated-or-truncated steps; terminated_traj_out gets terminated | truncated << 1 */
int cge_hospital_rollout(cge_hospital *h, int32_t k_steps, const int32_t *actions, uint64_t action_seed, int64_t t0,
                         float *obs_out, int64_t obs_step_stride, float *reward_traj_out, uint8_t *terminated_traj_out,
                         double *reward_sum_out, int32_t *done_count_out, void *stream);
/* terminal observations of SAME_STEP rollouts, compacted per segment of 64 envs: see <env>_rollout_final_obs at the top of this file */
int cge_hospital_rollout_final_obs(cge_hospital *h, float *rows_out, int64_t *index_out, int64_t seg_capacity, int32_t *count_out);
int64_t cge_hospital_final_obs_segment(const cge_hospital *h);
int cge_hospital_info(cge_hospital *h, int32_t field_id, double *out, void *stream);
/* whole-handle checkpoint (host memory, opaque: 32-byte header + the device arrays in device layout); restores only
 * into a handle created with the same n_envs and config; both calls synchronise `stream` */
size_t cge_hospital_snapshot_bytes(const cge_hospital *h);
int cge_hospital_snapshot_get(cge_hospital *h, void *host_buf, void *stream);
int cge_hospital_snapshot_set(cge_hospital *h, const void *host_buf, void *stream);
size_t cge_hospital_device_bytes(const cge_hospital *h);
int cge_hospital_episode_stats(cge_hospital *h, double *return_out, int32_t *length_out);
/* optional: cge_hospital_step also writes terminated | truncated per env into done_out (device, n_envs bytes) until it is set to NULL —
 * the mask gymnasium's SAME_STEP infos["_final_obs"] and the episode statistics want, without a second launch */
int cge_hospital_done_mask(cge_hospital *h, uint8_t *done_out);
const char *cge_hospital_last_error(const cge_hospital *h);
const char *cge_hospital_last_kernel(const cge_hospital *h);

/* ------------------------------------------------------------------------------------------ */
/* Bus system  (bus_system_env/environment.py: BusSystemEnv, utils.py, config.py)                */
/*   4 buses on a 4-stop ring, 50..150 passengers per episode, 500 steps; truncated only (:176).  */
/*   action int32 [4] in 0..10: the dwell time of each bus (MultiDiscrete([11]*4), :82).          */
/*   obs: the Dict of :94-123 as KEY-MAJOR PLANES of int32 — gymnasium's batched-Dict layout.     */
/*   One observation of the whole batch is a slab of CGE_BUS_OBS_INTS * n_envs ints (16-byte      */
/*   aligned) holding, in this order, one contiguous [n_envs, ...] array per key:                 */
/*     bus_stops [n,4]  bus_states [n,4] (1 stopped)  bus_remaining_times [n,4]  bus_capacities   */
/*     [n,4]  bus_passenger_destinations [n,4,4]  stop_waiting_counts [n,4]                       */
/*     stop_destination_distributions [n,4,4]  timestep [n]  total_delivered [n]                  */
/*     total_waiting [n]  total_onboard [n]                                                       */
/*   (the reference's int8 bus_states and Python-int scalars are int32 here).                     */
/*   Bit-exact: integer state; the reward is a sum of multiples of 0.5.                           */
/*   Generator: the process-global CPython `random`, drawn only by reset() (utils.py:22-46); the  */
/*   env never seeds it (reset(seed) reaches np_random only, :127), so cge_bus_seed is the        */
/*   caller's random.seed(s_i) for env i.  A fresh handle holds empty stops until its first reset.*/
/* ------------------------------------------------------------------------------------------ */
typedef struct cge_bus cge_bus;

typedef struct {
    int32_t max_timesteps;    /* MAX_TIMESTEPS = 500 (config.py:10, __init__ :57); 0 -> 500; <= 60000 */
    int32_t autoreset_mode;   /* CGE_AUTORESET_* */
} cge_bus_config;

enum { CGE_BUS_OBS_INTS = 56 };

enum { /* cge_bus_info int32 fields (`index` = bus or stop 0..3 where noted) — the values behind _get_info (:339-350) */
    CGE_BUS_INFO_TIMESTEP = 0,
    CGE_BUS_INFO_TOTAL_DELIVERED = 1,
    CGE_BUS_INFO_TOTAL_WAITING = 2,
    CGE_BUS_INFO_TOTAL_ONBOARD = 3,
    CGE_BUS_INFO_BUS_POSITION = 4,    /* index = bus */
    CGE_BUS_INFO_BUS_STOPPED = 5,     /* index = bus; 1 = "stopped", 0 = "traveling" */
    CGE_BUS_INFO_BUS_CAPACITY = 6,    /* index = bus; free seats */
    CGE_BUS_INFO_STOP_WAITING = 7,    /* index = stop */
    CGE_BUS_INFO_NEEDS_RESET = 8
};

/* BusSystemEnv.__init__ :57-92 */
int cge_bus_create(const cge_bus_config *cfg, int64_t n_envs, int device, int64_t env_index0, cge_bus **out);
int cge_bus_destroy(cge_bus *h);
/* random.seed(s_i) for env i; s_i = seeds[i] or base_seed + env_index0 + i.  Does not reset the envs. */
int cge_bus_seed(cge_bus *h, const uint64_t *seeds, uint64_t base_seed, void *stream);
/* reset :125-151 with generate_passengers (utils.py:22-46) on env i's stream, for envs with mask[i] != 0 (all if NULL);
 * writes the whole slab if obs_out != NULL */
int cge_bus_reset(cge_bus *h, const uint8_t *mask, int32_t *obs_out, void *stream);
/* step :153-186.  actions int32 [n_envs, 4].  An action outside 0..10 raises ValueError in the reference (:160-161); here the env is
 * left untouched, its row reports (current obs, 0, 0, 0) and a device-side counter is bumped (cge_bus_error_count).
 * terminated_out is always 0; truncated_out is REQUIRED.  final_obs_out (nullable; a slab): SAME_STEP writes the pieces of the envs
 * that were truncated in this step, the others are left as they were. */
int cge_bus_step(cge_bus *h, const int32_t *actions, int32_t *obs_out, float *reward_out, uint8_t *terminated_out,
                 uint8_t *truncated_out, int32_t *final_obs_out, void *stream);
/* k fused steps.  actions int32 [k, n_envs, 4], or NULL: bus j of env i takes cge_hash_action(action_seed, env_index0 + i, t0 + t, 11, j).
 * obs_out: k slabs obs_step_stride ints apart (a multiple of 4, >= CGE_BUS_OBS_INTS * n_envs), or with stride 0 the last step's slab.
 * truncated_traj_out [k, n_envs]; done_count counts truncated steps. */
int cge_bus_rollout(cge_bus *h, int32_t k_steps, const int32_t *actions, uint64_t action_seed, int64_t t0, int32_t *obs_out,
                    int64_t obs_step_stride, float *reward_traj_out, uint8_t *truncated_traj_out, double *reward_sum_out,
                    int32_t *done_count_out, void *stream);
/* terminal observations of SAME_STEP rollouts, compacted per segment of 64 envs: see <env>_rollout_final_obs at the top of this file.
 * rows_out is a slab: CGE_BUS_OBS_INTS * R ints for R = n_segments * seg_capacity rows, plane p at p * R ints.  While rows are registered
 * a SAME_STEP rollout runs its rollout_rows_kernel instance (64-lane workgroups); rows_out must be 16-byte aligned, or cge_bus_rollout
 * refuses it.  The two are named cge_rows_bus_*: they stand beside the type's surface cge_bus_*, which is as it was */
int cge_rows_bus_rollout_final_obs(cge_bus *h, int32_t *rows_out, int64_t *index_out, int64_t seg_capacity, int32_t *count_out);
int64_t cge_rows_bus_final_obs_segment(const cge_bus *h);
/* _get_info :339-350 */
int cge_bus_info(cge_bus *h, int32_t field_id, int32_t index, int32_t *out, void *stream);
/* env-steps refused for an invalid action since the last call; synchronises */
int64_t cge_bus_error_count(cge_bus *h, void *stream);
/* whole-handle checkpoint (host memory, opaque: 32-byte header + the device arrays in device layout); restores only
 * into a handle created with the same n_envs and config; both calls synchronise `stream` */
size_t cge_bus_snapshot_bytes(const cge_bus *h);
int cge_bus_snapshot_get(cge_bus *h, void *host_buf, void *stream);
int cge_bus_snapshot_set(cge_bus *h, const void *host_buf, void *stream);
size_t cge_bus_device_bytes(const cge_bus *h);
int cge_bus_episode_stats(cge_bus *h, double *return_out, int32_t *length_out);
const char *cge_bus_last_error(const cge_bus *h);
const char *cge_bus_last_kernel(const cge_bus *h);

/* ------------------------------------------------------------------------------------------ */
/* Restaurant  (restaurant_env_updated/restaurant_env.py: RestaurantEnv, entities.py)            */
/*   10 tables, 10 waiters, a waiting line, a kitchen; one arrival draw per step; truncated only  */
/*   (:171).  action int32 [4] = (type 0..3, waiter_id 0..9, customer_id 0..49, table_id 0..9),   */
/*   the reference's Dict action (:41-46) in its key order.                                       */
/*   obs: the Dict of :47-55 as KEY-MAJOR PLANES of int32 — gymnasium's batched-Dict layout.      */
/*   One observation of the whole batch is a slab of CGE_RESTAURANT_OBS_INTS * n_envs ints        */
/*   holding, in this order, one contiguous [n_envs, ...] array per key:                          */
/*     waiting_customers [n,50,2]  waiter_status [n,10,3]  table_occupancy [n,10]                 */
/*     table_cleanliness [n,10]  kitchen_queue [n,50,3]  ready_orders [n,20,2]                    */
/*     current_timestep [n,1]                                                                     */
/*   Bit-exact (the reward is the reference's float64 sum, rounded to float32 on output) EXCEPT   */
/*   the three id columns waiting_customers[:,0], kitchen_queue[:,0], ready_orders[:,0]: the      */
/*   reference shows hash(str(uuid.uuid4())) % 100, unreproducible; here a per-env serial number  */
/*   mod 100, restarted by reset, taken by each arrival and each order in creation order.         */
/*   Generator: the process-global CPython `random`, one random.random() per step (:382); the     */
/*   env never seeds it, so cge_restaurant_seed is the caller's random.seed(s_i) for env i.       */
/*   reset() draws nothing: the stream goes on across episodes.                                   */
/* ------------------------------------------------------------------------------------------ */
typedef struct cge_restaurant cge_restaurant;

typedef struct {
    int32_t max_episode_steps;   /* :21 sets 500, the reference's inference.py:14-17 runs 1000; 1..1000, anything else is refused.
                                  * The record keeps the timestep in 16 bits and saturates it at 65,535: a CGE_AUTORESET_DISABLED batch
                                  * that is never reset stays truncated (the reference counts on; nothing else depends on it by then) */
    int32_t autoreset_mode;      /* CGE_AUTORESET_* */
} cge_restaurant_config;

enum { CGE_RESTAURANT_OBS_INTS = 341 };

enum { /* cge_restaurant_info float64 fields — the values behind _get_info (:478-494) */
    CGE_RESTAURANT_INFO_TIMESTEP = 0,
    CGE_RESTAURANT_INFO_WAITING_CUSTOMERS = 1,
    CGE_RESTAURANT_INFO_IDLE_WAITERS = 2,
    CGE_RESTAURANT_INFO_KITCHEN_QUEUE_LENGTH = 3,
    CGE_RESTAURANT_INFO_READY_ORDERS = 4,
    CGE_RESTAURANT_INFO_DIRTY_TABLES = 5,
    CGE_RESTAURANT_INFO_CUSTOMERS_SERVED = 6,
    CGE_RESTAURANT_INFO_CUSTOMERS_LEFT = 7,
    CGE_RESTAURANT_INFO_TABLES_CLEANED = 8,
    CGE_RESTAURANT_INFO_ORDERS_SERVED = 9,
    CGE_RESTAURANT_INFO_WAIT_TIME_SUM = 10,   /* over everything in the reference's self.customers: waiting, carried by a waiter, */
    CGE_RESTAURANT_INFO_NUM_CUSTOMERS = 11,   /* seated, and the ghosts a failed seating leaves behind (:312)                    */
    CGE_RESTAURANT_INFO_TOTAL_REWARD = 12,    /* self.total_reward: the returned rewards plus the completion rewards and -5 per leaver */
    CGE_RESTAURANT_INFO_NEEDS_RESET = 13
};

/* RestaurantEnv.__init__ :17-72 */
int cge_restaurant_create(const cge_restaurant_config *cfg, int64_t n_envs, int device, int64_t env_index0, cge_restaurant **out);
int cge_restaurant_destroy(cge_restaurant *h);
/* random.seed(s_i) for env i; s_i = seeds[i] or base_seed + env_index0 + i.  Does not reset the envs. */
int cge_restaurant_seed(cge_restaurant *h, const uint64_t *seeds, uint64_t base_seed, void *stream);
/* reset :74-93 for envs with mask[i] != 0 (all if NULL); writes the whole slab if obs_out != NULL */
int cge_restaurant_reset(cge_restaurant *h, const uint8_t *mask, int32_t *obs_out, void *stream);
/* step :95-175.  actions int32 [n_envs, 4], 16-byte aligned (one load per env; a misaligned pointer is CGE_ERR_INVALID_ARG, here
 * and in the rollout).  An action outside the action space — a component negative or not below its bound
 * (4, 10, 50, 10) — has no effect, like the reference's "invalid_*" results (:103-166; the reference would index from the end with a
 * negative value and ignore a customer_id >= 50 on a serve or clean action), and bumps a device-side counter
 * (cge_restaurant_error_count); the step itself always runs.
 * terminated_out is always 0; truncated_out is REQUIRED.  final_obs_out (nullable; a slab): SAME_STEP writes the pieces of every
 * wave of 64 envs that holds an env truncated in this step; valid where truncated. */
int cge_restaurant_step(cge_restaurant *h, const int32_t *actions, int32_t *obs_out, float *reward_out, uint8_t *terminated_out,
                        uint8_t *truncated_out, int32_t *final_obs_out, void *stream);
/* k fused steps.  actions int32 [k, n_envs, 4], or NULL: column c of env i takes
 * cge_hash_action(action_seed, env_index0 + i, t0 + t, (4, 10, 50, 10)[c], c).
 * obs_out: k slabs obs_step_stride ints apart (>= CGE_RESTAURANT_OBS_INTS * n_envs), or with stride 0 the last step's slab.
 * truncated_traj_out [k, n_envs]; done_count counts truncated steps. */
int cge_restaurant_rollout(cge_restaurant *h, int32_t k_steps, const int32_t *actions, uint64_t action_seed, int64_t t0, int32_t *obs_out,
                           int64_t obs_step_stride, float *reward_traj_out, uint8_t *truncated_traj_out, double *reward_sum_out,
                           int32_t *done_count_out, void *stream);
/* terminal observations of SAME_STEP rollouts, compacted per segment of 64 envs: see <env>_rollout_final_obs at the top of this file.
 * rows_out is a slab: CGE_RESTAURANT_OBS_INTS * R ints for R = n_segments * seg_capacity rows, plane p at p * R ints.  While rows are
 * registered a SAME_STEP rollout runs its rollout_rows_kernel instance; rows_out must be 4-byte aligned, or cge_restaurant_rollout
 * refuses it.  The two are named cge_rows_restaurant_*: they stand beside the type's surface cge_restaurant_*, which is as it was */
int cge_rows_restaurant_rollout_final_obs(cge_restaurant *h, int32_t *rows_out, int64_t *index_out, int64_t seg_capacity, int32_t *count_out);
int64_t cge_rows_restaurant_final_obs_segment(const cge_restaurant *h);
/* _get_info :478-494 */
int cge_restaurant_info(cge_restaurant *h, int32_t field_id, double *out, void *stream);
/* env-steps whose action had a component out of range since the last call; synchronises */
int64_t cge_restaurant_error_count(cge_restaurant *h, void *stream);
/* whole-handle checkpoint (host memory, opaque: 32-byte header + the device arrays in device layout); restores only
 * into a handle created with the same n_envs and config; both calls synchronise `stream` */
size_t cge_restaurant_snapshot_bytes(const cge_restaurant *h);
int cge_restaurant_snapshot_get(cge_restaurant *h, void *host_buf, void *stream);
int cge_restaurant_snapshot_set(cge_restaurant *h, const void *host_buf, void *stream);
size_t cge_restaurant_device_bytes(const cge_restaurant *h);
int cge_restaurant_episode_stats(cge_restaurant *h, double *return_out, int32_t *length_out);
const char *cge_restaurant_last_error(const cge_restaurant *h);
const char *cge_restaurant_last_kernel(const cge_restaurant *h);

/* ------------------------------------------------------------------------------------------ */
/* Airline operations  (airline_operations_env/airline_env.py: AirlineOperationsEnv)             */
/*   25 aircraft, 15 airports, 150 flights, 40 crew sets, up to 3 weather systems; a step is a    */
/*   quarter of an hour from 6.0; terminated only: the clock reaches 23.75 (71 steps) or          */
/*   passenger_satisfaction < 0.6.  action int32 0..44 (Discrete(45), :445-511).                  */
/*   obs float32 [n_envs, 160] row-major (:354-396), 16-byte aligned.                             */
/*   Bit-exact: observations, the integer-valued reward, flags and the float64 info values, with  */
/*   ONE stated departure: a weather system's distance is sqrt(dx*dx + dy*dy) where the reference */
/*   evaluates dx**2 through libm pow (a last-place difference in 0.07 % of its evaluations,      */
/*   seen only through the float32 weather_severity: no recorded observation differs).           */
/*   Generator: the process-global CPython `random` (randint, uniform, choice); the env never     */
/*   seeds it.  The NETWORK (aircraft bases, the flight schedule, crews) is drawn once, by the    */
/*   constructor, and survives every reset; aircraft positions carry across episodes too.         */
/*   cge_airline_seed is `random.seed(s_i); AirlineOperationsEnv()` for env i: it seeds the       */
/*   stream, draws the network and the constructor's own discarded reset (:190); the reset that   */
/*   follows draws the visible one.  cge_airline_create does the same with base seed 0.           */
/*   Device memory: 1,656 B of record + 2,560 B of generator per env (+ 8 B).                     */
/* ------------------------------------------------------------------------------------------ */
typedef struct cge_airline cge_airline;

typedef struct {
    int32_t autoreset_mode;      /* CGE_AUTORESET_* */
    int32_t reserved;            /* 0 */
} cge_airline_config;

enum { CGE_AIRLINE_OBS_FLOATS = 160, CGE_AIRLINE_RECORD_BYTES = 1656 };

enum { /* cge_airline_info float64 fields: the reference's five info values (:435-441), then what else the record knows */
    CGE_AIRLINE_INFO_ON_TIME_PERFORMANCE = 0,
    CGE_AIRLINE_INFO_PASSENGER_SATISFACTION = 1,
    CGE_AIRLINE_INFO_DAILY_REVENUE = 2,        /* 0.0 for ever: passengers_onboard is zeroed before it is paid (:562, :569) */
    CGE_AIRLINE_INFO_DAILY_COSTS = 3,
    CGE_AIRLINE_INFO_CURRENT_HOUR = 4,
    CGE_AIRLINE_INFO_TIMESTEP = 5,             /* steps since the episode's reset */
    CGE_AIRLINE_INFO_NEEDS_RESET = 6,
    CGE_AIRLINE_INFO_FLIGHTS_IN_AIR = 7,       /* aircraft with in_flight set */
    CGE_AIRLINE_INFO_DELAY_COMPENSATION = 8,
    CGE_AIRLINE_INFO_FUEL_COSTS = 9
};

/* AirlineOperationsEnv.__init__ :132-190 on the stream random.seed(env_index0 + i) */
int cge_airline_create(const cge_airline_config *cfg, int64_t n_envs, int device, int64_t env_index0, cge_airline **out);
int cge_airline_destroy(cge_airline *h);
/* random.seed(s_i); AirlineOperationsEnv() for env i; s_i = seeds[i] or base_seed + env_index0 + i.  Call reset next. */
int cge_airline_seed(cge_airline *h, const uint64_t *seeds, uint64_t base_seed, void *stream);
/* reset :274-336 for envs with mask[i] != 0 (all if NULL), continuing each env's stream; writes every row if obs_out != NULL */
int cge_airline_reset(cge_airline *h, const uint8_t *mask, float *obs_out, void *stream);
/* step :398-443.  actions int32 [n_envs].  An action outside 0..44 skips _process_action — the rest of the step runs — and bumps a
 * device-side counter (cge_airline_error_count); the reference would index its aircraft list from the back for -25..-1 and do
 * nothing for anything else.  truncated_out is nullable (always 0).  final_obs_out (nullable): SAME_STEP writes the rows of every
 * wave of 64 envs that holds an env terminated in this step; valid where terminated. */
int cge_airline_step(cge_airline *h, const int32_t *actions, float *obs_out, float *reward_out, uint8_t *terminated_out,
                     uint8_t *truncated_out, float *final_obs_out, void *stream);
/* k fused steps.  actions int32 [k, n_envs], or NULL: env i takes cge_hash_action(action_seed, env_index0 + i, t0 + t, 45, 0).
 * obs_out: k batches obs_step_stride floats apart (>= 160 * n_envs, a multiple of 4), or with stride 0 the last step's.
 * terminated_traj_out [k, n_envs]; done_count counts terminated steps.  Terminal rows of a SAME_STEP rollout are not delivered. */
int cge_airline_rollout(cge_airline *h, int32_t k_steps, const int32_t *actions, uint64_t action_seed, int64_t t0, float *obs_out,
                        int64_t obs_step_stride, float *reward_traj_out, uint8_t *terminated_traj_out, double *reward_sum_out,
                        int32_t *done_count_out, void *stream);
int cge_airline_info(cge_airline *h, int32_t field_id, double *out, void *stream);
/* env-steps whose action was outside 0..44 since the last call; synchronises */
int64_t cge_airline_error_count(cge_airline *h, void *stream);
/* whole-handle checkpoint (host memory, opaque: 32-byte header + the device arrays in device layout); restores only
 * into a handle created with the same n_envs and config; both calls synchronise `stream` */
size_t cge_airline_snapshot_bytes(const cge_airline *h);
int cge_airline_snapshot_get(cge_airline *h, void *host_buf, void *stream);
int cge_airline_snapshot_set(cge_airline *h, const void *host_buf, void *stream);
size_t cge_airline_device_bytes(const cge_airline *h);
int cge_airline_episode_stats(cge_airline *h, double *return_out, int32_t *length_out);
const char *cge_airline_last_error(const cge_airline *h);
const char *cge_airline_last_kernel(const cge_airline *h);

/* ------------------------------------------------------------------------------------------ */
/* Emergency response  (emergency_response_env/emergency_env.py: EmergencyResponseEnv)           */
/*   A 30 x 30 city, up to 20 incidents, 40 response units of which actions 0..19 dispatch the    */
/*   twelve fire trucks and eight police cars, 8 hospitals, weather, 25 traffic segments; a step  */
/*   is a minute.  terminated only (:808-827): no incident after minute 60 (success), more than   */
/*   50 casualties, a mean response time above 45, or max_timesteps reached.                      */
/*   action int32 0..49 (Discrete(50), :648-690).                                                 */
/*   obs float32 [n_envs, 276] row-major (:524-587), 16-byte aligned.                             */
/*   Bit-exact: observations, the integer-valued reward, flags and the float64 info values.       */
/*   Generator: the process-global CPython `random` (random, uniform, randint); the env never     */
/*   seeds it.  The constructor draws population densities, the stations of units 30..39 and the  */
/*   hospitals' capacities (952 randint) and does NOT reset.  cge_emergency_seed is               */
/*   `random.seed(s_i); EmergencyResponseEnv()` for env i and leaves it without an incident; the   */
/*   reset that follows draws the first episode.  cge_emergency_create does the same with base    */
/*   seed 0.  Every later reset continues the stream and keeps the network and the reward's       */
/*   _prev_ counters, as the reference does.                                                      */
/*   Device memory: 808 B of record + 2,560 B of generator per env (+ 8 B).                       */
/* ------------------------------------------------------------------------------------------ */
typedef struct cge_emergency cge_emergency;

typedef struct {
    int32_t autoreset_mode;      /* CGE_AUTORESET_* */
    int32_t max_timesteps;       /* 1..65535; the reference's attribute of the same name, 1440 */
} cge_emergency_config;

enum { CGE_EMERGENCY_OBS_FLOATS = 276, CGE_EMERGENCY_RECORD_BYTES = 808, CGE_EMERGENCY_ACTIONS = 50 };

enum { /* cge_emergency_info float64 fields: the reference's six info values (:913-920), then what else the record knows */
    CGE_EMERGENCY_INFO_ACTIVE_EMERGENCIES = 0,
    CGE_EMERGENCY_INFO_TOTAL_CASUALTIES = 1,
    CGE_EMERGENCY_INFO_LIVES_SAVED = 2,
    CGE_EMERGENCY_INFO_EMERGENCIES_RESOLVED = 3,
    CGE_EMERGENCY_INFO_AVG_RESPONSE_TIME = 4,
    CGE_EMERGENCY_INFO_TERMINATION_REASON = 5,   /* of the last step: 0 none, 1 success, 2 casualties, 3 overwhelmed, 4 timeout */
    CGE_EMERGENCY_INFO_TIMESTEP = 6,             /* steps since the episode's reset */
    CGE_EMERGENCY_INFO_NEEDS_RESET = 7,
    CGE_EMERGENCY_INFO_BUSY_UNITS = 8,
    CGE_EMERGENCY_INFO_MUTUAL_AID_REQUESTED = 9,
    CGE_EMERGENCY_INFO_NATIONAL_GUARD_ACTIVE = 10,
    CGE_EMERGENCY_INFO_STATE_OF_EMERGENCY = 11
};

/* EmergencyResponseEnv.__init__ :116-157 on the stream random.seed(env_index0 + i) */
int cge_emergency_create(const cge_emergency_config *cfg, int64_t n_envs, int device, int64_t env_index0, cge_emergency **out);
int cge_emergency_destroy(cge_emergency *h);
/* random.seed(s_i); EmergencyResponseEnv() for env i; s_i = seeds[i] or base_seed + env_index0 + i.  Call reset next. */
int cge_emergency_seed(cge_emergency *h, const uint64_t *seeds, uint64_t base_seed, void *stream);
/* reset :829-881 for envs with mask[i] != 0 (all if NULL), continuing each env's stream; writes every row if obs_out != NULL */
int cge_emergency_reset(cge_emergency *h, const uint8_t *mask, float *obs_out, void *stream);
/* step :883-922.  actions int32 [n_envs].  An action outside 0..49 falls through every branch of _execute_action, as it does in
 * the reference — the rest of the step runs — and bumps a device-side counter (cge_emergency_error_count).  truncated_out is
 * nullable (always 0).  final_obs_out (nullable): SAME_STEP writes the rows of every wave of 64 envs that holds an env terminated
 * in this step; valid where terminated. */
int cge_emergency_step(cge_emergency *h, const int32_t *actions, float *obs_out, float *reward_out, uint8_t *terminated_out,
                       uint8_t *truncated_out, float *final_obs_out, void *stream);
/* k fused steps.  actions int32 [k, n_envs], or NULL: env i takes cge_hash_action(action_seed, env_index0 + i, t0 + t, 50, 0).
 * obs_out: k batches obs_step_stride floats apart (>= 276 * n_envs, a multiple of 4), or with stride 0 the last step's.
 * terminated_traj_out [k, n_envs]; done_count counts terminated steps.  Terminal rows of a SAME_STEP rollout are not delivered. */
int cge_emergency_rollout(cge_emergency *h, int32_t k_steps, const int32_t *actions, uint64_t action_seed, int64_t t0, float *obs_out,
                          int64_t obs_step_stride, float *reward_traj_out, uint8_t *terminated_traj_out, double *reward_sum_out,
                          int32_t *done_count_out, void *stream);
/* terminal observations of SAME_STEP rollouts, compacted per segment of 64 envs: see <env>_rollout_final_obs at the top of this file.
 * While rows are registered a SAME_STEP rollout runs its rollout_rows_kernel instance; rows_out must be 16-byte aligned, or
 * cge_emergency_rollout refuses it.  The two are named cge_rows_emergency_*: they stand beside the type's surface cge_emergency_*, which is as it was */
int cge_rows_emergency_rollout_final_obs(cge_emergency *h, float *rows_out, int64_t *index_out, int64_t seg_capacity, int32_t *count_out);
int64_t cge_rows_emergency_final_obs_segment(const cge_emergency *h);
int cge_emergency_info(cge_emergency *h, int32_t field_id, double *out, void *stream);
/* env-steps whose action was outside 0..49 since the last call; synchronises */
int64_t cge_emergency_error_count(cge_emergency *h, void *stream);
/* whole-handle checkpoint (host memory, opaque: 32-byte header + the device arrays in device layout); restores only
 * into a handle created with the same n_envs and config; both calls synchronise `stream` */
size_t cge_emergency_snapshot_bytes(const cge_emergency *h);
int cge_emergency_snapshot_get(cge_emergency *h, void *host_buf, void *stream);
int cge_emergency_snapshot_set(cge_emergency *h, const void *host_buf, void *stream);
size_t cge_emergency_device_bytes(const cge_emergency *h);
int cge_emergency_episode_stats(cge_emergency *h, double *return_out, int32_t *length_out);
const char *cge_emergency_last_error(const cge_emergency *h);
const char *cge_emergency_last_kernel(const cge_emergency *h);

/* ------------------------------------------------------------------------------------------ */
/* Space station  (space_station_env/station_env.py: SpaceStationEnv)                           */
/*   Six crew members, twelve systems and eight modules in orbit; a step is five minutes.        */
/*   terminated (:714-737): all six healths <= 0, three critical systems below 10 % efficiency,  */
/*   mean oxygen < 15 or mean pressure < 80, or max_steps reached — which raises truncated too   */
/*   (:343-344) and sets mission_success.                                                         */
/*   action int32 0..39 (Discrete(40), :351-398).                                                 */
/*   obs float32 [n_envs, 120] row-major (:739-783; the reference declares 110 and returns 120),  */
/*   16-byte aligned.                                                                             */
/*   Bit-exact: observations, the integer-valued reward, flags and the float64 info values, with  */
/*   one caveat: the 32 Gaussian draws of a reset go through log(), and where the device's log    */
/*   differs from glibc's in the last place the float64 module state after that reset does too.   */
/*   Generator: the process-global NumPy legacy stream (normal, uniform, random, choice); the env */
/*   never seeds it and its constructor draws nothing.  cge_space_station_seed is                 */
/*   `np.random.seed(s_i); SpaceStationEnv()` for env i; the reset that follows draws the first   */
/*   episode.  cge_space_station_create does the same with base seed 0.  Every later reset        */
/*   continues the stream and keeps what the reference's reset() does not touch: episode_reward,  */
/*   last_emergency_time, the crew's modules, solar_angle, radiation_level and                    */
/*   total_power_consumption.                                                                     */
/*   Device memory: 752 B of record + 2,560 B of generator per env (+ 8 B).                       */
/* ------------------------------------------------------------------------------------------ */
typedef struct cge_space_station cge_space_station;

typedef struct {
    int32_t autoreset_mode;      /* CGE_AUTORESET_* */
    int32_t max_steps;           /* 1..65535; the reference's attribute of the same name, 8640 */
} cge_space_station_config;

enum { CGE_SPACE_STATION_OBS_FLOATS = 120, CGE_SPACE_STATION_RECORD_BYTES = 752, CGE_SPACE_STATION_ACTIONS = 40 };

enum { /* cge_space_station_info float64 fields: the reference's nine info values (:785-797), then what else the record knows */
    CGE_SPACE_STATION_INFO_TIME_STEP = 0,
    CGE_SPACE_STATION_INFO_DAY = 1,
    CGE_SPACE_STATION_INFO_CREW_ALIVE = 2,
    CGE_SPACE_STATION_INFO_SYSTEM_FAILURES = 3,       /* the length of the reference's list of names */
    CGE_SPACE_STATION_INFO_EMERGENCY_COUNT = 4,
    CGE_SPACE_STATION_INFO_MISSION_SUCCESS = 5,
    CGE_SPACE_STATION_INFO_EPISODE_REWARD = 6,        /* never reset by the reference: the sum over every episode since the seed */
    CGE_SPACE_STATION_INFO_BATTERY_LEVEL = 7,
    CGE_SPACE_STATION_INFO_AVG_CREW_HEALTH = 8,
    CGE_SPACE_STATION_INFO_SYSTEM_FAILURE_MASK = 9,   /* bit s: system s is named in the list */
    CGE_SPACE_STATION_INFO_NEEDS_RESET = 10,
    CGE_SPACE_STATION_INFO_CREW_CASUALTIES = 11,      /* grows by one per dead member per step, as in the reference */
    CGE_SPACE_STATION_INFO_EVACUATED = 12             /* action 38 was taken since the seed: everybody is in Docking */
};

/* SpaceStationEnv.__init__ :56-135 on the stream np.random.seed(env_index0 + i) */
int cge_space_station_create(const cge_space_station_config *cfg, int64_t n_envs, int device, int64_t env_index0, cge_space_station **out);
int cge_space_station_destroy(cge_space_station *h);
/* np.random.seed(s_i); SpaceStationEnv() for env i; s_i = seeds[i] or base_seed + env_index0 + i; s_i must be < 2**32
 * (np.random.seed raises otherwise).  Call reset next. */
int cge_space_station_seed(cge_space_station *h, const uint64_t *seeds, uint64_t base_seed, void *stream);
/* reset :247-308 for envs with mask[i] != 0 (all if NULL), continuing each env's stream; writes every row if obs_out != NULL */
int cge_space_station_reset(cge_space_station *h, const uint8_t *mask, float *obs_out, void *stream);
/* step :310-349.  actions int32 [n_envs].  An action outside 0..39 skips _process_action — 40 and above fall through every branch
 * of it in the reference, a negative one would index its list of systems from the back — the rest of the step runs, and a
 * device-side counter is bumped (cge_space_station_error_count).  truncated_out (nullable) is 1 where max_steps ended the episode,
 * which sets terminated too.  final_obs_out (nullable): SAME_STEP writes the rows of every wave of 64 envs that holds an env
 * terminated in this step; valid where terminated. */
int cge_space_station_step(cge_space_station *h, const int32_t *actions, float *obs_out, float *reward_out, uint8_t *terminated_out,
                           uint8_t *truncated_out, float *final_obs_out, void *stream);
/* k fused steps.  actions int32 [k, n_envs], or NULL: env i takes cge_hash_action(action_seed, env_index0 + i, t0 + t, 40, 0).
 * obs_out: k batches obs_step_stride floats apart (>= 120 * n_envs, a multiple of 4), or with stride 0 the last step's.
 * terminated_traj_out [k, n_envs]; done_count counts terminated steps.  Terminal rows of a SAME_STEP rollout and the per-step
 * truncated flag (terminated at time_step == max_steps) are not delivered. */
int cge_space_station_rollout(cge_space_station *h, int32_t k_steps, const int32_t *actions, uint64_t action_seed, int64_t t0, float *obs_out,
                              int64_t obs_step_stride, float *reward_traj_out, uint8_t *terminated_traj_out, double *reward_sum_out,
                              int32_t *done_count_out, void *stream);
/* terminal observations of SAME_STEP rollouts, compacted per segment of 64 envs: see <env>_rollout_final_obs at the top of this file.
 * While rows are registered a SAME_STEP rollout runs its rollout_rows_kernel instance; rows_out must be 16-byte aligned, or
 * cge_space_station_rollout refuses it.  The two are named cge_rows_space_station_*: they stand beside the type's surface cge_space_station_*, which is as it was */
int cge_rows_space_station_rollout_final_obs(cge_space_station *h, float *rows_out, int64_t *index_out, int64_t seg_capacity, int32_t *count_out);
int64_t cge_rows_space_station_final_obs_segment(const cge_space_station *h);
int cge_space_station_info(cge_space_station *h, int32_t field_id, double *out, void *stream);
/* env-steps whose action was outside 0..39 since the last call; synchronises */
int64_t cge_space_station_error_count(cge_space_station *h, void *stream);
/* whole-handle checkpoint (host memory, opaque: 32-byte header + the device arrays in device layout); restores only
 * into a handle created with the same n_envs and config; both calls synchronise `stream` */
size_t cge_space_station_snapshot_bytes(const cge_space_station *h);
int cge_space_station_snapshot_get(cge_space_station *h, void *host_buf, void *stream);
int cge_space_station_snapshot_set(cge_space_station *h, const void *host_buf, void *stream);
size_t cge_space_station_device_bytes(const cge_space_station *h);
int cge_space_station_episode_stats(cge_space_station *h, double *return_out, int32_t *length_out);
const char *cge_space_station_last_error(const cge_space_station *h);
const char *cge_space_station_last_kernel(const cge_space_station *h);

/* ------------------------------------------------------------------------------------------ */
/* Agricultural farm  (agricultural_farm_env/farm_env.py: AgriculturalFarmEnv,                  */
/*   crops/crop_data.py)                                                                          */
/*   Four fields, eight machines, a market of five crops, weather by season; a step is a day, a  */
/*   season 90 days.  terminated only (:612-621): year > max_years (in the step that makes the   */
/*   day a multiple of 360), or cash_flow < -50000 (-5000); the soil termination cannot fire.    */
/*   action int32 0..44 (Discrete(45), :629-800).                                                 */
/*   obs float32 [n_envs, 620] row-major (:435-518): 134 live values and 486 zeros, as the        */
/*   reference pads them; 16-byte aligned.  compact_obs: [n_envs, 134], 8-byte aligned.           */
/*   Bit-exact: observations, the integer-valued reward, the flag and the float64 info values,   */
/*   with one caveat: the five Gaussians of a step's prices go through log(), and where the      */
/*   device's log differs from glibc's in the last place a float64 price does too.  The number   */
/*   of draws never depends on a price.                                                           */
/*   Generators: TWO streams per env, both process-global in the reference and seeded by none of */
/*   its code: NumPy's legacy one (uniform, random, randint, normal) and CPython's `random`      */
/*   (random.choice of the crop to plant).  cge_farm_seed is `random.seed(s_i);                   */
/*   np.random.seed(s_i); AgriculturalFarmEnv()` for env i — the constructor draws the fields,   */
/*   the equipment and the market — and the reset that follows draws them again.                  */
/*   cge_farm_create does the same with base seed 0.  Every later reset continues both streams,  */
/*   the legacy Gaussian's cached second value included, and keeps what the reference's reset()  */
/*   does not touch: water_quality.                                                               */
/*   Device memory: 832 B of record + 2 x 2,560 B of generators per env (+ 8 B).                  */
/* ------------------------------------------------------------------------------------------ */
typedef struct cge_farm cge_farm;

typedef struct {
    int32_t autoreset_mode;      /* CGE_AUTORESET_* */
    int32_t max_years;           /* 1..255; the reference's attribute of the same name (:139), 1 */
    int32_t compact_obs;         /* 0: rows of 620 floats as the reference returns them; 1: their 134 leading values only */
    int32_t reserved;
} cge_farm_config;

enum { CGE_FARM_OBS_FLOATS = 620, CGE_FARM_COMPACT_OBS_FLOATS = 134, CGE_FARM_RECORD_BYTES = 832, CGE_FARM_ACTIONS = 45 };

enum { /* cge_farm_info float64 fields: the reference's eleven scalar info values (:911-924), field_status (:925-934), then what else the record knows */
    CGE_FARM_INFO_DAY = 0,
    CGE_FARM_INFO_SEASON = 1,                     /* 0 spring .. 3 winter; the reference gives the name */
    CGE_FARM_INFO_YEAR = 2,
    CGE_FARM_INFO_CASH_FLOW = 3,
    CGE_FARM_INFO_TOTAL_REVENUE = 4,
    CGE_FARM_INFO_TOTAL_EXPENSES = 5,
    CGE_FARM_INFO_PROFIT_MARGIN = 6,
    CGE_FARM_INFO_CARBON_SEQUESTERED = 7,
    CGE_FARM_INFO_WATER_CONSERVATION_SCORE = 8,
    CGE_FARM_INFO_BIODIVERSITY_INDEX = 9,
    CGE_FARM_INFO_SOIL_HEALTH_TREND = 10,
    CGE_FARM_INFO_FIELD_CROP = 11,                /* + field 0..3: the crop's index, -1 where the reference prints "None" (wheat too) */
    CGE_FARM_INFO_FIELD_STAGE = 15,               /* + field 0..3: CropStage 0..7 */
    CGE_FARM_INFO_FIELD_HEALTH = 19,              /* + field 0..3 */
    CGE_FARM_INFO_FIELD_YIELD_POTENTIAL = 23,     /* + field 0..3 */
    CGE_FARM_INFO_NEEDS_RESET = 27,
    CGE_FARM_INFO_WATER_QUALITY = 28              /* not reset by the reference */
};

/* AgriculturalFarmEnv.__init__ :127-192 on the streams random.seed / np.random.seed(env_index0 + i) */
int cge_farm_create(const cge_farm_config *cfg, int64_t n_envs, int device, int64_t env_index0, cge_farm **out);
int cge_farm_destroy(cge_farm *h);
/* random.seed(s_i); np.random.seed(s_i); AgriculturalFarmEnv() for env i; s_i = seeds[i] or base_seed + env_index0 + i; s_i must
 * be < 2**32 (np.random.seed raises otherwise).  Call reset next. */
int cge_farm_seed(cge_farm *h, const uint64_t *seeds, uint64_t base_seed, void *stream);
/* reset :520-566 for envs with mask[i] != 0 (all if NULL), continuing each env's streams; writes every row if obs_out != NULL */
int cge_farm_reset(cge_farm *h, const uint8_t *mask, float *obs_out, void *stream);
/* step :568-627.  actions int32 [n_envs].  An action outside 0..44 falls through every branch of _process_action (:629-800), as in
 * the reference; the rest of the step runs, and a device-side counter is bumped (cge_farm_error_count).  truncated_out (nullable)
 * is written 0.  final_obs_out (nullable): SAME_STEP writes the rows of every wave of 64 envs that holds an env terminated in this
 * step; valid where terminated. */
int cge_farm_step(cge_farm *h, const int32_t *actions, float *obs_out, float *reward_out, uint8_t *terminated_out, uint8_t *truncated_out,
                  float *final_obs_out, void *stream);
/* k fused steps.  actions int32 [k, n_envs], or NULL: env i takes cge_hash_action(action_seed, env_index0 + i, t0 + t, 45, 0).
 * obs_out: k batches obs_step_stride floats apart (>= the row width * n_envs; a multiple of 4, compact_obs: of 2), or with stride 0
 * the last step's.  terminated_traj_out [k, n_envs]; done_count counts terminated steps.  Terminal rows of a SAME_STEP rollout are
 * not delivered. */
int cge_farm_rollout(cge_farm *h, int32_t k_steps, const int32_t *actions, uint64_t action_seed, int64_t t0, float *obs_out, int64_t obs_step_stride,
                     float *reward_traj_out, uint8_t *terminated_traj_out, double *reward_sum_out, int32_t *done_count_out, void *stream);
/* terminal observations of SAME_STEP rollouts, compacted per segment of 64 envs: see <env>_rollout_final_obs at the top of this file.
 * While rows are registered a SAME_STEP rollout runs its rollout_rows_kernel instance; rows_out must be 16-byte aligned (compact_obs: 8-byte), or
 * cge_farm_rollout refuses it.  The two are named cge_rows_farm_*: they stand beside the type's surface cge_farm_*, which is as it was */
int cge_rows_farm_rollout_final_obs(cge_farm *h, float *rows_out, int64_t *index_out, int64_t seg_capacity, int32_t *count_out);
int64_t cge_rows_farm_final_obs_segment(const cge_farm *h);
int cge_farm_info(cge_farm *h, int32_t field_id, double *out, void *stream);
/* env-steps whose action was outside 0..44 since the last call; synchronises */
int64_t cge_farm_error_count(cge_farm *h, void *stream);
/* whole-handle checkpoint (host memory, opaque: 32-byte header + the device arrays in device layout); restores only
 * into a handle created with the same n_envs and config; both calls synchronise `stream` */
size_t cge_farm_snapshot_bytes(const cge_farm *h);
int cge_farm_snapshot_get(cge_farm *h, void *host_buf, void *stream);
int cge_farm_snapshot_set(cge_farm *h, const void *host_buf, void *stream);
size_t cge_farm_device_bytes(const cge_farm *h);
int cge_farm_episode_stats(cge_farm *h, double *return_out, int32_t *length_out);
const char *cge_farm_last_error(const cge_farm *h);
const char *cge_farm_last_kernel(const cge_farm *h);

/* ------------------------------------------------------------------------------------------ */
/* World builder  (world_builder_env/src/environment/world_builder_env.py: WorldBuilderEnv,      */
/*   game_logic.py: GameLogic)                                                                    */
/*   A G x G grid (G = 2..10, default 10, :39), food / wood / stone, a population; five actions:  */
/*   0 pass, 1 farm, 2 lumberyard, 3 quarry, 4 house (Discrete(5), :57).  terminated only (:150): */
/*   population 0 (-100) or 50 steps at population >= 20 (+100); no time limit.                    */
/*   obs, Dict layout (flatten_obs = 0; :79-86): ONE uint8 slab per observation of the whole      */
/*   batch, 16-byte aligned, key-major planes in the reference's key order, each plane starting   */
/*   at a multiple of 16 bytes (a16 = round up to 16):                                             */
/*     grid                int8    [n, G, G]  at 0                                                 */
/*     resources           float32 [n, 4]     at a16(n * G * G)       food, wood, stone, population */
/*     population_capacity float32 [n, 1]     at resources + 16 n                                  */
/*     win_steps           int32   [n, 1]     at a16(population_capacity + 4 n)                    */
/*     slab bytes = a16(win_steps + 4 n)                                                           */
/*   obs, flat layout (flatten_obs = 1; :69-77, :205-216): float32 [n, G*G + 6], row = the grid    */
/*   row-major, then food, wood, stone, population, population_capacity, win_steps.                */
/*   Bit-exact: integer state (int32 resources: the reference's unbounded ints differ only after   */
/*   millions of steps of one episode); rewards are small integers.  Box.high is not enforced by   */
/*   the reference (:73) and not here.                                                             */
/*   Generator: the process-global NumPy legacy np.random, drawn only by a successful build        */
/*   (game_logic.py:130: randint(#empty cells), no word when one cell is left); the env never      */
/*   seeds it (reset(seed) reaches np_random only, :109), so cge_world_builder_seed is the         */
/*   caller's np.random.seed(s_i) for env i.  reset() draws nothing.                               */
/*   State record (cge_world_builder_get_state / _set_state), little-endian, per env:              */
/*     int32 [16]  food, wood, stone, population, population_capacity, farm, lumberyard, quarry,   */
/*                 house, steps, win_steps, reached_win_population, needs_reset, mt_pos, 0, 0      */
/*     int8  [G*G] the grid, row-major, zero-padded to a multiple of 4 bytes                        */
/*     uint32[624] key                                                                             */
/*   (key, mt_pos) is np.random.get_state()[1:3] of env i's stream: mt_pos = 624 right after       */
/*   seeding.  The record does not hold the running episode's return (episode statistics of the    */
/*   episode in progress restart at set_state).                                                    */
/* ------------------------------------------------------------------------------------------ */
typedef struct cge_world_builder cge_world_builder;

typedef struct {
    int32_t grid_size;        /* 2..10 (__init__ :39 default 10) */
    int32_t flatten_obs;      /* 0: Dict slab, 1: float32 rows (:42) */
    int32_t autoreset_mode;   /* CGE_AUTORESET_* */
    int32_t reserved;
} cge_world_builder_config;

enum { /* cge_world_builder_info int32 fields — the values behind _get_info (:218-232) */
    CGE_WORLD_BUILDER_INFO_STEPS = 0,
    CGE_WORLD_BUILDER_INFO_WIN_STEPS = 1,
    CGE_WORLD_BUILDER_INFO_REACHED_WIN_POPULATION = 2,
    CGE_WORLD_BUILDER_INFO_FOOD = 3,
    CGE_WORLD_BUILDER_INFO_WOOD = 4,
    CGE_WORLD_BUILDER_INFO_STONE = 5,
    CGE_WORLD_BUILDER_INFO_POPULATION = 6,
    CGE_WORLD_BUILDER_INFO_POPULATION_CAPACITY = 7,
    CGE_WORLD_BUILDER_INFO_BUILDING_COUNT = 8,   /* index = 0 farm, 1 lumberyard, 2 quarry, 3 house */
    CGE_WORLD_BUILDER_INFO_NEEDS_RESET = 9
};

/* WorldBuilderEnv.__init__ :39-97; a grid_size outside 2..10 is CGE_ERR_INVALID_ARG */
int cge_world_builder_create(const cge_world_builder_config *cfg, int64_t n_envs, int device, int64_t env_index0, cge_world_builder **out);
int cge_world_builder_destroy(cge_world_builder *h);
/* np.random.seed(s_i) for env i; s_i = seeds[i] or base_seed + env_index0 + i; s_i must be < 2**32 (np.random.seed raises
 * otherwise).  Does not reset the envs. */
int cge_world_builder_seed(cge_world_builder *h, const uint64_t *seeds, uint64_t base_seed, void *stream);
/* reset :99-121 (game_logic.py:31-54) for envs with mask[i] != 0 (all if NULL); writes the whole observation if obs_out != NULL */
int cge_world_builder_reset(cge_world_builder *h, const uint8_t *mask, void *obs_out, void *stream);
/* step :123-166.  actions int32 [n_envs].  An action outside 0..4 raises ValueError in the reference (:133-134); here the env is
 * left untouched, its row reports (current obs, 0, 0) and a device-side counter is bumped (cge_world_builder_error_count).
 * truncated_out (nullable) is written 0.  final_obs_out (nullable; one observation): SAME_STEP writes the terminal observations of the
 * wavefronts (64 consecutive envs) in which an env terminated in this step; rows of envs that did not terminate are unspecified. */
int cge_world_builder_step(cge_world_builder *h, const int32_t *actions, void *obs_out, float *reward_out, uint8_t *terminated_out,
                           uint8_t *truncated_out, void *final_obs_out, void *stream);
/* k fused steps.  actions int32 [k, n_envs], or NULL: env i takes cge_hash_action(action_seed, env_index0 + i, t0 + t, 5, 0).
 * obs_out: k observations obs_step_stride elements apart (bytes of the Dict slab: a multiple of 16, >= the slab; floats of the flat
 * layout: >= n_envs * (G*G + 6)), or with stride 0 the last step's observation.  terminated_traj_out [k, n_envs]; done_count counts
 * terminated steps.  A SAME_STEP trajectory holds the reset observation at a step that ends an episode. */
int cge_world_builder_rollout(cge_world_builder *h, int32_t k_steps, const int32_t *actions, uint64_t action_seed, int64_t t0, void *obs_out,
                              int64_t obs_step_stride, float *reward_traj_out, uint8_t *terminated_traj_out, double *reward_sum_out,
                              int32_t *done_count_out, void *stream);
/* terminal observations of SAME_STEP rollouts, compacted per segment of 64 envs: see <env>_rollout_final_obs at the top of this file.
 * With R = n_segments * seg_capacity rows, rows_out is the Dict slab for R envs (grid int8 [R, G, G] at byte 0 | resources f32 [R, 4] |
 * population_capacity f32 [R, 1] | win_steps i32 [R, 1], each plane at the next multiple of 16 bytes), or with flatten_obs float32 rows
 * [R, G*G + 6].  While rows are registered a SAME_STEP rollout runs its rollout_rows_kernel instance; rows_out must be 16-byte (Dict) /
 * 4-byte (flat) aligned, or cge_world_builder_rollout refuses it.  The two are named cge_rows_world_builder_*: they stand beside the
 * type's surface cge_world_builder_*, which is as it was */
int cge_rows_world_builder_rollout_final_obs(cge_world_builder *h, void *rows_out, int64_t *index_out, int64_t seg_capacity, int32_t *count_out);
int64_t cge_rows_world_builder_final_obs_segment(const cge_world_builder *h);
/* _get_info :218-232 */
int cge_world_builder_info(cge_world_builder *h, int32_t field_id, int32_t index, int32_t *out, void *stream);
/* env-steps refused for an invalid action since the last call; synchronises */
int64_t cge_world_builder_error_count(cge_world_builder *h, void *stream);
/* canonical per-env records (host memory, n_envs * state_bytes; layout above); both calls synchronise `stream`.  set_state validates:
 * cells <= 4, counts equal to the grid's census, population_capacity = 10 + 5 * house, mt_pos <= 624, flags 0 / 1; otherwise
 * CGE_ERR_INVALID_ARG with a message and nothing is written */
size_t cge_world_builder_state_bytes(const cge_world_builder *h);
int cge_world_builder_get_state(cge_world_builder *h, void *host_buf, void *stream);
int cge_world_builder_set_state(cge_world_builder *h, const void *host_buf, void *stream);
size_t cge_world_builder_device_bytes(const cge_world_builder *h);
int cge_world_builder_episode_stats(cge_world_builder *h, double *return_out, int32_t *length_out);
const char *cge_world_builder_last_error(const cge_world_builder *h);
const char *cge_world_builder_last_kernel(const cge_world_builder *h);

/* ------------------------------------------------------------------------------------------ */
/* Canonical per-env records of airline, emergency, space station and farm: cge_records_<env>_*  */
/*   They stand beside the types' surfaces cge_<env>_*, which are as they were (snapshots        */
/*   included).  The records are packed and unpacked by kernels, so they can stay on the device: */
/*   copy the best envs over the worst, branch many envs from one, move a sub-range between       */
/*   handles of any size and env_index0.                                                          */
/*                                                                                                */
/*   One layout rule for the four.  A record is state_bytes contiguous bytes; every section is    */
/*   padded with zero bytes to a multiple of 16:                                                  */
/*     header  int32[8]: {0x4C520100 | type (1 airline, 2 emergency, 3 space station, 4 farm),    */
/*             the number of body words (CGE_<ENV>_RECORD_BYTES / 4), the number of generator     */
/*             streams, stream 0's index, stream 1's index (farm; otherwise 0), 0, 0, 0}.  An     */
/*             index is the reference's, 0..624: CPython's getstate()[1][624], NumPy's `pos`.     */
/*     body    the type's CGE_<ENV>_RECORD_BYTES / 4 32-bit words in column order, exactly as the */
/*             device holds them (DESIGN.md has each type's columns), except that the words that  */
/*             hold the device's stream cursors and ready marks read zero: airline word 243;      */
/*             emergency 199-200; space station 185-186; farm 202-205.  What a cursor means is    */
/*             in the header; a ready mark is not state.  Farm's cached legacy Gaussian and its   */
/*             flag (one bit) are body words and untouched: they belong to the stream.  The space */
/*             station keeps none (a reset's sixteen polar pairs leave the cache empty).          */
/*     streams 624 uint32 words of ONE generation each, such that with the header's index         */
/*             random.setstate((3, tuple(words) + (index,), None)) — for a NumPy legacy stream    */
/*             np.random.set_state(('MT19937', words, index, has_gauss, cached)) — continues the  */
/*             env's stream.  Airline, emergency: one CPython stream.  Space station: one NumPy   */
/*             legacy stream.  Farm: the NumPy legacy stream, then the CPython one.  Words of the */
/*             next generation that the device twisted ahead are taken back, the rest of the      */
/*             current generation is twisted.  THE LOW 31 BITS OF WORD 0 ALWAYS READ ZERO: taking */
/*             words back cannot recover them, the records keep no saved copy, and no future      */
/*             output of MT19937 depends on them once the generation is complete (word 0 enters   */
/*             the next generation through its top bit only).  unpack ignores them.               */
/*   state_bytes: airline 4192, emergency 3344, space station 3280, farm 5856.                    */
/*   Two envs in the same logical state have the same bytes, whatever launches got them there.    */
/*                                                                                                */
/*   unpack and set_state check every record before anything is written and refuse: a wrong tag,  */
/*   word count or stream count; an index above 624; a non-zero reserved header word, cursor word */
/*   or padding byte; and every field that a step, reset or info kernel uses as an index or a     */
/*   bound (the predicate is record_refusal in the type's <env>_env.hpp):                         */
/*     airline        aircraft airport / destination > 14; flight origin / destination > 14;      */
/*                    flight aircraft > 24                                                         */
/*     emergency      more than 20 incidents; an incident's unit mask with a bit above 19; a      */
/*                    unit's incident slot > 19                                                    */
/*     space station  orbit phase or angle > 17                                                    */
/*     farm           a field's stage > 7 (it selects the divisor of a modulo); a crop or last    */
/*                    crop outside -1..4.  has_gauss is one bit and cannot be out of {0, 1}.      */
/*   A record that passes cannot make a kernel of its type read or write out of range.  A refusal */
/*   is CGE_ERR_INVALID_ARG with last_error "cge_records_<env>_unpack: env I: reason" (or         */
/*   _set_state), I the lowest refused env, and every env is as it was.                            */
/*                                                                                                */
/*   pack / unpack: envs [first, first + count) <-> count records at dev_records, a DEVICE buffer */
/*   of count * state_bytes bytes, 16-byte aligned.  A range outside [0, n_envs], a null or a     */
/*   misaligned pointer is CGE_ERR_INVALID_ARG.  pack reads the handle and writes the records     */
/*   only.  Both wait for `stream` before they return (unpack reads the check's verdict): they    */
/*   are not for graph capture.  get_state / set_state: host memory, n_envs * state_bytes, moved  */
/*   in rounds of 4,096 envs through a transient device staging buffer of one round; set_state    */
/*   checks every round before it unpacks any.  The staging buffer and the status block are       */
/*   allocated and freed inside the call: device_bytes and snapshot_bytes are as they were.       */
/* ------------------------------------------------------------------------------------------ */
size_t cge_records_airline_state_bytes(const cge_airline *h);
int cge_records_airline_get_state(cge_airline *h, void *host_buf, void *stream);
int cge_records_airline_set_state(cge_airline *h, const void *host_buf, void *stream);
int cge_records_airline_pack(cge_airline *h, int64_t first, int64_t count, void *dev_records, void *stream);
int cge_records_airline_unpack(cge_airline *h, int64_t first, int64_t count, const void *dev_records, void *stream);
size_t cge_records_emergency_state_bytes(const cge_emergency *h);
int cge_records_emergency_get_state(cge_emergency *h, void *host_buf, void *stream);
int cge_records_emergency_set_state(cge_emergency *h, const void *host_buf, void *stream);
int cge_records_emergency_pack(cge_emergency *h, int64_t first, int64_t count, void *dev_records, void *stream);
int cge_records_emergency_unpack(cge_emergency *h, int64_t first, int64_t count, const void *dev_records, void *stream);
size_t cge_records_space_station_state_bytes(const cge_space_station *h);
int cge_records_space_station_get_state(cge_space_station *h, void *host_buf, void *stream);
int cge_records_space_station_set_state(cge_space_station *h, const void *host_buf, void *stream);
int cge_records_space_station_pack(cge_space_station *h, int64_t first, int64_t count, void *dev_records, void *stream);
int cge_records_space_station_unpack(cge_space_station *h, int64_t first, int64_t count, const void *dev_records, void *stream);
size_t cge_records_farm_state_bytes(const cge_farm *h);
int cge_records_farm_get_state(cge_farm *h, void *host_buf, void *stream);
int cge_records_farm_set_state(cge_farm *h, const void *host_buf, void *stream);
int cge_records_farm_pack(cge_farm *h, int64_t first, int64_t count, void *dev_records, void *stream);
int cge_records_farm_unpack(cge_farm *h, int64_t first, int64_t count, const void *dev_records, void *stream);

/* ------------------------------------------------------------------------------------------ */
/* Action-space sampler: `action_space.sample()` of a batched space on the device               */
/*   Every reference script drives its env with env.action_space.sample() (snake_env_classic/    */
/*   example.py:23, smart_parking_env/examples/test_env.py:52, traffic_management_env/demo.py:49, */
/*   crypto_trading_env/test_crypto_trading.py:151, smartclimate_rl-main/examples/demo.py:9);     */
/*   the vector form is envs.step(envs.action_space.sample()).  A sampler handle owns one NumPy   */
/*   PCG64 stream (np.random.default_rng(seed), seeded on the host) and writes, bit for bit,      */
/*   what successive sample() calls of the batched space draw from it (gymnasium 1.x):            */
/*     CGE_SAMPLE_INDEX    MultiDiscrete / batched Discrete: one random() per element, C order,   */
/*                         int(trunc(u * nvec[col])); out int32 or int64                           */
/*     CGE_SAMPLE_UNIFORM  bounded Box: one random() per element; out float32 =                    */
/*                         float32(low + (high - low) * u) (Generator.uniform), out int8 / int32 = */
/*                         floor(low + ((high + 1) - low) * u) (gymnasium's integer-Box path)      */
/*     CGE_SAMPLE_BITS     MultiBinary: Generator.integers(0, 2, dtype=int8): 32-bit words of the   */
/*                         buffered next32 path (carry kept across calls), 4 bytes per word low    */
/*                         byte first, byte b -> (b * 2) >> 8; out int8                            */
/*   params (host, copied at create): INDEX nvec[k] (integers >= 1, as doubles); UNIFORM low[k]    */
/*   then high[k] (finite, low <= high); BITS none.  Column c of every row uses params[c].         */
/*   Rows [row0, row0 + n_rows) of a world batch of world_rows rows: a shard draws its slice of    */
/*   the world's stream and every call advances the stream by the world's draw count, so shards   */
/*   of a sharding.make_sharded batch sample exactly what the unsplit batch does.                 */
/*   cge_sampler_sample writes steps successive calls, [steps, n_rows, k], advances the stream on */
/*   the device inside the same launch (no host sync; safe under graph capture and replay) and    */
/*   takes the calls in stream order: one handle is not used on two streams at once.             */
/* ------------------------------------------------------------------------------------------ */
typedef struct cge_sampler cge_sampler;

/* NumPy's bit_generator.state of a PCG64: {"state": {"state", "inc"}, "has_uint32", "uinteger"} (40 bytes) */
typedef struct {
    uint64_t state_lo, state_hi, inc_lo, inc_hi;
    uint32_t has_uint32, uinteger;
} cge_pcg64_state;

enum { CGE_SAMPLE_INDEX = 0, CGE_SAMPLE_UNIFORM = 1, CGE_SAMPLE_BITS = 2 };
enum { CGE_DTYPE_INT8 = 0, CGE_DTYPE_INT32 = 1, CGE_DTYPE_INT64 = 2, CGE_DTYPE_FLOAT32 = 3 };
enum { CGE_SAMPLER_MAX_K = 4096, CGE_SAMPLER_MAX_STEPS = 65535 };

/* host only (no device needed): bit_generator.advance(delta_hi * 2^64 + delta_lo); clears has_uint32 and uinteger as NumPy does */
int cge_pcg64_advance(cge_pcg64_state *state, uint64_t delta_lo, uint64_t delta_hi);
/* k columns per row, 1 <= k <= CGE_SAMPLER_MAX_K; 0 <= row0, n_rows >= 1, row0 + n_rows <= world_rows.  The stream starts as
 * default_rng(0) until set_state */
int cge_sampler_create(int32_t kind, int64_t k, const double *params, int64_t n_rows, int64_t row0, int64_t world_rows, int device,
                       cge_sampler **out);
int cge_sampler_destroy(cge_sampler *h);
/* host state in / out; both synchronise `stream` */
int cge_sampler_set_state(cge_sampler *h, const cge_pcg64_state *state, void *stream);
int cge_sampler_get_state(cge_sampler *h, cge_pcg64_state *state, void *stream);
/* out: DEVICE [steps, n_rows, k] of out_dtype (CGE_DTYPE_*; INDEX: int32 / int64, UNIFORM: float32 / int8 / int32, BITS: int8);
 * 1 <= steps <= CGE_SAMPLER_MAX_STEPS */
int cge_sampler_sample(cge_sampler *h, int64_t steps, void *out, int32_t out_dtype, void *stream);
size_t cge_sampler_device_bytes(const cge_sampler *h);
const char *cge_sampler_last_error(const cge_sampler *h);
const char *cge_sampler_last_kernel(const cge_sampler *h);

#ifdef __cplusplus
}
#endif
#endif /* CGE_AMD_H */
