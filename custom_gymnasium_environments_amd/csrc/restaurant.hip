// restaurant.hip — batched RestaurantEnv for MI355X (gfx950): kernels + C ABI (include/cge_amd.h).
//
// The record and the dynamics are restaurant_env.hpp (plain C++, also replayed on the host against the reference fixtures); this
// file is what is the device's own: the record's trip through HBM, the generator words, the action sources and the observation.
//
// State per env: 11 uint4 columns (SoA), in registers for a whole launch.  One lane per env, one wave per workgroup.
//
// Draws: exactly one random.random() per step() — two MT19937 words — so a lane keeps a run of READY words in registers (twisted
// ahead by mt_make_ready, fetched 16 at a time: one refill per 8 steps of a fused launch) and the step loop of a rollout holds no
// other generator access.  reset() draws nothing.
//
// Observation: 341 int32 per env in key-major planes (gymnasium's batched-Dict layout), of which at most ~140 are not padding.  A
// wave's share of a plane is ONE contiguous run (25,600 B of waiting_customers), so the wave writes it as consecutive 16-byte-per-
// lane stores, whichever env a 16-byte piece belongs to.  Each lane first parks what can be non-zero of its env as BYTES in LDS
// (136 B per env, 8,960 B per wave: restaurant_env.hpp `stage`); the store pass expands bytes to int32 and takes the zero padding
// from the piece's position alone.  A plane's run starts wherever `plane offset * n_envs` puts it: up to three single ints lead in
// to the first 16-byte boundary and up to three follow the last whole piece.
#include <cstring>
#include <string>
#include <vector>

#include "cge_lane.hpp"
#include "restaurant_env.hpp"

namespace cge {
namespace restaurant {

constexpr int OBS = CGE_RESTAURANT_OBS_INTS;
constexpr int COLS = REC_WORDS / 4;
constexpr int BLOCK = 64;        // one wave: the store pass and the staging rows are the wave's own, no cross-wave barrier
// plane offsets inside one observation slab, in units of n_envs ints (the order of cge_amd.h), and ints per env
constexpr int P_WAITING = 0, P_WAITERS = 100, P_OCC = 130, P_DIRTY = 140, P_COOKING = 150, P_READY = 300, P_TIMESTEP = 340;
constexpr int N_WAITING = 100, N_WAITERS = 30, N_TABLES = 10, N_COOKING = 150, N_READY = 40;
static_assert(P_TIMESTEP + 1 == OBS, "planes");

struct Params : LaneParams<int32_t> {
    int32_t max_t;
    static constexpr bool terminates = false;                        // truncated after max_t steps; terminated is never set (:100)
};
static_assert(std::is_trivially_copyable<Params>::value, "a kernel argument");
// rollout_rows_kernel's: the other kernels' arguments stay as they are.  fin.rows is the observation slab of R = n_segments * fin.cap
// "envs" (plane p at p * R ints); row j of segment s is env s * fin.cap + j of it.
struct RowsParams : Params {
    FinalSeg fin;
    int64_t R;
};

__device__ __forceinline__ void load_env(Env &e, const uint4 *__restrict__ s, int64_t n, int64_t i) {
    uint32_t w[REC_WORDS];
#pragma unroll
    for (int c = 0; c < COLS; ++c) {
        const uint4 v = s[(int64_t)c * n + i];
        w[4 * c] = v.x; w[4 * c + 1] = v.y; w[4 * c + 2] = v.z; w[4 * c + 3] = v.w;
    }
    e.unpack(w);
}
__device__ __forceinline__ void store_env(const Env &e, uint4 *__restrict__ s, int64_t n, int64_t i) {
    uint32_t w[REC_WORDS];
    e.pack(w);
#pragma unroll
    for (int c = 0; c < COLS; ++c) s[(int64_t)c * n + i] = make_uint4(w[4 * c], w[4 * c + 1], w[4 * c + 2], w[4 * c + 3]);
}

// One plane's run of the wave: `total` = envs of the wave * PER ints from p on.  Int f of the run belongs to env f / PER of the wave
// and is byte f % PER of that env's staged bytes at OFF when below LIM, else padding.  Writes [p, p + total) and nothing else.
template <int PER, int LIM, int OFF>
__device__ __forceinline__ void store_plane(const uint8_t *__restrict__ stg, int32_t *__restrict__ p, int total, int lane) {
    auto val = [&](int env, int elem) -> int32_t { return elem < LIM ? (int32_t)stg[env * (STG_WORDS * 4) + OFF + elem] : 0; };
    const int lead = (int)((4u - (uint32_t)((reinterpret_cast<uintptr_t>(p) >> 2) & 3u)) & 3u);
    const int head = lead < total ? lead : total;
    if (lane < head) p[lane] = val(lane / PER, lane % PER);
    const int pieces = (total - head) >> 2;
#pragma unroll 2
    for (int q = lane; q < pieces; q += BLOCK) {
        const int f = head + 4 * q;
        int env = f / PER, elem = f - env * PER;
        int32_t v[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            v[c] = val(env, elem);
            elem += 1;
            if (elem == PER) { elem = 0; env += 1; }
        }
        *reinterpret_cast<int4 *>(p + f) = make_int4(v[0], v[1], v[2], v[3]);
    }
    const int done = head + 4 * pieces, f = done + lane;
    if (f < total) p[f] = val(f / PER, f % PER);
}

// _get_observation :426-476 of the wave's envs -> their piece of every plane of one slab.  Call with every lane of the wave.
__device__ __forceinline__ void observe(const Env &e, uint32_t *__restrict__ stg, int32_t *__restrict__ o, int64_t n, int64_t i, bool live) {
    const int lane = (int)threadIdx.x;
    const int64_t first = (int64_t)blockIdx.x * BLOCK;
    const int envs = (int)(n - first < BLOCK ? n - first : BLOCK);
    if (live) e.stage([&](int k, uint32_t v) { stg[lane * STG_WORDS + k] = v; });
    __syncthreads();
    const uint8_t *b = reinterpret_cast<const uint8_t *>(stg);
    store_plane<N_WAITING, LIM_WAITING, STG_WAITING>(b, o + (int64_t)P_WAITING * n + first * N_WAITING, envs * N_WAITING, lane);
    store_plane<N_WAITERS, LIM_WAITERS, STG_WAITERS>(b, o + (int64_t)P_WAITERS * n + first * N_WAITERS, envs * N_WAITERS, lane);
    store_plane<N_TABLES, LIM_TABLES, STG_OCC>(b, o + (int64_t)P_OCC * n + first * N_TABLES, envs * N_TABLES, lane);
    store_plane<N_TABLES, LIM_TABLES, STG_DIRTY>(b, o + (int64_t)P_DIRTY * n + first * N_TABLES, envs * N_TABLES, lane);
    store_plane<N_COOKING, LIM_COOKING, STG_COOKING>(b, o + (int64_t)P_COOKING * n + first * N_COOKING, envs * N_COOKING, lane);
    store_plane<N_READY, LIM_READY, STG_READY>(b, o + (int64_t)P_READY * n + first * N_READY, envs * N_READY, lane);
    if (live) o[(int64_t)P_TIMESTEP * n + i] = (int32_t)e.t;
    __syncthreads();                                                 // the rows are free for the next observation
}

// observe() for the terminal rows of one step of rollout_rows_kernel (lane_final_rows): the lanes with `mine` park their bytes at LDS
// row `rank`, and the wave writes `keep` dense envs of every plane of the rows slab `o` (R envs) from env `row0` on: [row0, row0 + keep)
// of each plane and nothing else.  Call with every lane of the wave.
__device__ __forceinline__ void final_observe(const Env &e, uint32_t *__restrict__ stg, int32_t *__restrict__ o, int64_t R, int64_t row0, int keep, int rank,
                                              bool mine) {
    const int lane = (int)threadIdx.x;
    if (mine) e.stage([&](int k, uint32_t v) { stg[rank * STG_WORDS + k] = v; });
    __syncthreads();
    const uint8_t *b = reinterpret_cast<const uint8_t *>(stg);
    store_plane<N_WAITING, LIM_WAITING, STG_WAITING>(b, o + (int64_t)P_WAITING * R + row0 * N_WAITING, keep * N_WAITING, lane);
    store_plane<N_WAITERS, LIM_WAITERS, STG_WAITERS>(b, o + (int64_t)P_WAITERS * R + row0 * N_WAITERS, keep * N_WAITERS, lane);
    store_plane<N_TABLES, LIM_TABLES, STG_OCC>(b, o + (int64_t)P_OCC * R + row0 * N_TABLES, keep * N_TABLES, lane);
    store_plane<N_TABLES, LIM_TABLES, STG_DIRTY>(b, o + (int64_t)P_DIRTY * R + row0 * N_TABLES, keep * N_TABLES, lane);
    store_plane<N_COOKING, LIM_COOKING, STG_COOKING>(b, o + (int64_t)P_COOKING * R + row0 * N_COOKING, keep * N_COOKING, lane);
    store_plane<N_READY, LIM_READY, STG_READY>(b, o + (int64_t)P_READY * R + row0 * N_READY, keep * N_READY, lane);
    if (mine) o[(int64_t)P_TIMESTEP * R + row0 + rank] = (int32_t)e.t;
    __syncthreads();                                                 // the rows are free for the next observation
}

// k steps with the record in registers.  ROLLOUT: per-step outputs indexed [t, env], sums; GIVEN: the caller's actions, else the
// counter hash cge_hash_action(action_seed, env_index0 + i, t0 + t, (4, 10, 50, 10)[c], c).  With RowsParams (ROWS, a SAME_STEP
// rollout) the terminal observations of the truncated envs go to the wave's segment of p.fin.
template <int MODE, bool ROLLOUT, bool GIVEN, class P = Params>
__device__ __forceinline__ void run(const P &p) {
    constexpr bool ROWS = std::is_same<P, RowsParams>::value;
    static_assert(!ROWS || (ROLLOUT && MODE == CGE_AUTORESET_SAME_STEP), "terminal rows: fused SAME_STEP rollouts");
    __shared__ uint32_t stg[BLOCK * STG_WORDS];
    constexpr int RUN = ROLLOUT ? 16 : 2;                            // ready generator words a lane holds (<= MT_PAD)
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool live = i < p.n;
    const int64_t li = live ? i : p.n - 1;
    Env e;
    load_env(e, p.state, p.n, li);
    uint32_t *blk = p.mt + li * MT_STRIDE;
    uint32_t pos = e.mt_pos, pretw = mt_ready_decode(e.mt_enc), have = 0, rw[RUN];
#pragma unroll
    for (int j = 0; j < RUN; ++j) rw[j] = 0;
    const uint64_t key = GIVEN ? 0 : hash_env_key(p.a_seed, (uint64_t)(p.env0 + li));
    const int4 *acts = reinterpret_cast<const int4 *>(p.actions);
    int4 next = make_int4(0, 0, 0, 0);
    if (GIVEN) next = acts[li];
    double rsum = 0.0;
    int32_t dcount = 0;
    uint32_t fin_used = 0;                                           // ROWS: terminal rows the wave's segment has been handed
    const int ksteps = ROLLOUT ? p.k_steps : 1;
#pragma unroll 1
    for (int t = 0; t < ksteps; ++t) {
        int4 a = next;
        if (GIVEN) {
            if (t + 1 < ksteps) next = acts[(int64_t)(t + 1) * p.n + li];   // a step ahead: the load is older than this step's stores
        } else {
            a = make_int4((int)hash_action_from_key(key, (uint64_t)(p.t0 + t), 4u, 0u), (int)hash_action_from_key(key, (uint64_t)(p.t0 + t), 10u, 1u),
                          (int)hash_action_from_key(key, (uint64_t)(p.t0 + t), 50u, 2u), (int)hash_action_from_key(key, (uint64_t)(p.t0 + t), 10u, 3u));
        }
        const bool dry = live && have < 2u;
        if (__ballot(dry)) {                                         // once per RUN / 2 steps, all lanes of a wave together
            mt_make_ready(blk, pos, pretw, (uint32_t)RUN, dry);
            if (dry) { mt_load_ready<RUN>(blk, pos, rw); have = RUN; }
        }
        float reward = 0.0f;
        bool trunc = false, reset_now = false;
        if (live) {
            if (MODE == CGE_AUTORESET_NEXT_STEP && e.needs_reset) {
                reset_now = true;
            } else {
                const uint32_t ua = mt_temper(rw[0]) >> 5, ub = mt_temper(rw[1]) >> 6;   // random.random(): one per step, :382
                const double u = ((double)ua * 67108864.0 + (double)ub) / 9007199254740992.0;
#pragma unroll
                for (int j = 0; j + 2 < RUN; ++j) rw[j] = rw[j + 2];
                have -= 2u;
                mt_advance(pos, pretw, 2u);
                bool invalid;
                reward = (float)e.step(a.x, a.y, a.z, a.w, u, invalid);
                if (invalid) atomicAdd(p.err_count, 1ull);           // the action had no effect (a negative component: none at all)
                e.ret += (double)reward;
                trunc = e.t >= (uint32_t)p.max_t;                    // :171
                if (trunc) lane_episode_end<MODE>(p, i, e.ret, (int32_t)e.t, reset_now, e.needs_reset);
            }
        }
        if (MODE == CGE_AUTORESET_SAME_STEP && !ROLLOUT) {           // the terminal slab: every env of a wave with a truncated one
            if (p.final_obs && __ballot(trunc)) observe(e, stg, p.final_obs, p.n, i, live);
        }
        if constexpr (ROWS) {                                        // ... of a rollout: the truncated envs only, compacted (lane_final_rows)
            const int64_t row0 = (int64_t)blockIdx.x * p.fin.cap + (int64_t)fin_used;
            int32_t *dst;
            int keep, rank;
            if (__builtin_expect(lane_final_rows(p.fin, fin_used, trunc, t, i, 0, dst, keep, rank), false))
                final_observe(e, stg, static_cast<int32_t *>(p.fin.rows), p.R, row0, keep, rank, trunc && rank < keep);
        }
        if (MODE != CGE_AUTORESET_DISABLED && reset_now) e.clear();
        if (lane_obs_due<ROLLOUT>(p, t, ksteps)) observe(e, stg, p.obs + (int64_t)t * p.obs_step_stride, p.n, i, live);
        if (live) {
            if (ROLLOUT) {
                rsum += (double)reward;
                dcount += trunc ? 1 : 0;
                if (p.reward) p.reward[(int64_t)t * p.n + i] = reward;
                if (p.truncated) p.truncated[(int64_t)t * p.n + i] = trunc ? 1 : 0;
            } else {
                lane_step_outputs(p, i, reward, trunc);
            }
        }
    }
    if (live) {
        e.mt_pos = pos; e.mt_enc = pretw > pos ? mt_ready_encode(pretw) : 0u;
        store_env(e, p.state, p.n, i);
        if (ROLLOUT) lane_sums(p, i, rsum, dcount);
    }
    if constexpr (ROWS) {
        if (threadIdx.x == 0) p.fin.count[blockIdx.x] = (int32_t)fin_used;
    }
}

template <int MODE>
__global__ __launch_bounds__(BLOCK) void step_kernel(Params p) { run<MODE, false, true>(p); }

template <int MODE, bool ACTIONS>
__global__ __launch_bounds__(BLOCK) void rollout_kernel(Params p) { run<MODE, true, ACTIONS>(p); }

// the SAME_STEP rollout while terminal rows are registered (cge_rows_restaurant_rollout_final_obs)
template <bool ACTIONS>
__global__ __launch_bounds__(BLOCK) void rollout_rows_kernel(RowsParams p) { run<CGE_AUTORESET_SAME_STEP, true, ACTIONS>(p); }

// reset (mask) / initial state (init: an empty restaurant, cursor rewound) / rewind (after a re-seed) + obs
__global__ __launch_bounds__(BLOCK) void reset_kernel(Params p, int init, int rewind) {
    __shared__ uint32_t stg[BLOCK * STG_WORDS];
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool live = i < p.n;
    const int64_t li = live ? i : p.n - 1;
    Env e;
    load_env(e, p.state, p.n, li);
    bool dirty = false;
    if (init) { e.clear(); e.mt_pos = 0; e.mt_enc = 0; dirty = true; }
    else if (rewind) { e.mt_pos = 0; e.mt_enc = 0; dirty = true; }
    else if (live && (!p.mask || p.mask[i])) { e.clear(); dirty = true; }
    if (live && dirty) store_env(e, p.state, p.n, i);
    if (p.obs) observe(e, stg, p.obs, p.n, i, live);
}

__global__ __launch_bounds__(256) void info_kernel(const uint4 *__restrict__ state, int64_t n, int field, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    Env e;
    load_env(e, state, n, i);
    double v = 0.0;
    switch (field) {
        case CGE_RESTAURANT_INFO_TIMESTEP: v = (double)e.t; break;
        case CGE_RESTAURANT_INFO_WAITING_CUSTOMERS: v = (double)e.nw; break;
        case CGE_RESTAURANT_INFO_IDLE_WAITERS: v = (double)e.idle_waiters(); break;
        case CGE_RESTAURANT_INFO_KITCHEN_QUEUE_LENGTH: v = (double)e.cooking(); break;
        case CGE_RESTAURANT_INFO_READY_ORDERS: v = (double)e.nr; break;
        case CGE_RESTAURANT_INFO_DIRTY_TABLES: v = (double)e.bits10(e.dirty); break;
        case CGE_RESTAURANT_INFO_CUSTOMERS_SERVED: v = (double)e.served; break;
        case CGE_RESTAURANT_INFO_CUSTOMERS_LEFT: v = (double)e.left; break;
        case CGE_RESTAURANT_INFO_TABLES_CLEANED: v = (double)e.cleaned; break;
        case CGE_RESTAURANT_INFO_ORDERS_SERVED: v = (double)e.orders; break;
        case CGE_RESTAURANT_INFO_WAIT_TIME_SUM: v = (double)e.wait_sum(); break;
        case CGE_RESTAURANT_INFO_NUM_CUSTOMERS: v = (double)e.num_customers(); break;
        case CGE_RESTAURANT_INFO_TOTAL_REWARD: v = e.total; break;
        case CGE_RESTAURANT_INFO_NEEDS_RESET: v = (double)e.needs_reset; break;
    }
    out[i] = v;
}

}  // namespace restaurant
}  // namespace cge

using namespace cge;

struct cge_restaurant : LaneHandle {
    using Params = restaurant::Params;
    using RowsParams = restaurant::RowsParams;
    cge_restaurant_config cfg{};
    static constexpr uint32_t snap_tag = 7u;
    static constexpr const char *abi = "cge_restaurant", *kernel_ns = "cge::restaurant::", *rows_ns = kernel_ns;
    static constexpr int block = restaurant::BLOCK, seed_kind = 0;
    Params params() const {
        Params p{};
        fill(p);
        p.max_t = cfg.max_episode_steps;
        return p;
    }
    int64_t step_elems() const { return n * restaurant::OBS; }
    auto reset_kernel() const { return restaurant::reset_kernel; }
    template <int MODE>
    auto kernel(LaneKind kind) const {
        return kind == LANE_STEP ? restaurant::step_kernel<MODE>
               : kind == LANE_ROLLOUT_GIVEN ? restaurant::rollout_kernel<MODE, true> : restaurant::rollout_kernel<MODE, false>;
    }
    void fill_rows(RowsParams &p) const { p.R = (int64_t)lane_segments(this) * fin_cap; }
    void launch_rows(bool given, unsigned blocks, hipStream_t s, const RowsParams &p) const {
        hipLaunchKernelGGL(given ? restaurant::rollout_rows_kernel<true> : restaurant::rollout_rows_kernel<false>, dim3(blocks), dim3(block), 0, s, p);
    }
    // store_plane leads in to a 16-byte boundary with single ints: the rows slab has to hold whole ints
    const char *rows_refusal() const {
        return (reinterpret_cast<uintptr_t>(fin_rows) & 3u) != 0 ? "the registered terminal rows are not 4-byte aligned" : nullptr;
    }
    // an env's four action components are fetched as one 16-byte load
    static const char *actions_refusal(const int32_t *actions) {
        return (reinterpret_cast<uintptr_t>(actions) & 15u) != 0 ? "actions must be 16-byte aligned" : nullptr;
    }
    static int check(const cge_restaurant_config &c) {
        return bad_autoreset_mode(c.autoreset_mode) || c.max_episode_steps < 1 || c.max_episode_steps > 1000 ? CGE_ERR_INVALID_ARG : CGE_OK;
    }
    hipError_t init() {
        CGE_HIP(alloc(state, (size_t)restaurant::COLS * n * sizeof(uint4), true, true));
        CGE_HIP(alloc(mt, (size_t)n * MT_STRIDE * sizeof(uint32_t), false, true));
        CGE_HIP(alloc(err, sizeof(unsigned long long), true, false));
        CGE_HIP(launch_mt_seed(mt, MT_STRIDE, n, nullptr, 0, env0, 0, nullptr));
        lane_launch_reset(this, params(), 1, 0, nullptr);
        return hipGetLastError();
    }
};

extern "C" {

CGE_DEFINE_LIFECYCLE(restaurant)

int cge_restaurant_seed(cge_restaurant *h, const uint64_t *seeds, uint64_t base_seed, void *stream) { return lane_seed(h, seeds, base_seed, stream); }

int cge_restaurant_reset(cge_restaurant *h, const uint8_t *mask, int32_t *obs_out, void *stream) { return lane_reset(h, mask, obs_out, stream); }

int cge_restaurant_step(cge_restaurant *h, const int32_t *actions, int32_t *obs_out, float *reward_out, uint8_t *terminated_out,
                        uint8_t *truncated_out, int32_t *final_obs_out, void *stream) {
    return lane_step(h, actions && obs_out && reward_out && terminated_out && truncated_out,
                     "cge_restaurant_step: null actions/obs/reward/terminated/truncated pointer", actions, obs_out, reward_out, terminated_out,
                     truncated_out, final_obs_out, stream);
}

int cge_restaurant_rollout(cge_restaurant *h, int32_t k_steps, const int32_t *actions, uint64_t action_seed, int64_t t0, int32_t *obs_out,
                           int64_t obs_step_stride, float *reward_traj_out, uint8_t *truncated_traj_out, double *reward_sum_out,
                           int32_t *done_count_out, void *stream) {
    return lane_rollout(h, true, "cge_restaurant_rollout: bad k_steps / obs_step_stride", k_steps, actions, action_seed, t0, obs_out, obs_step_stride,
                        reward_traj_out, truncated_traj_out, reward_sum_out, done_count_out, stream);
}

int cge_restaurant_info(cge_restaurant *h, int32_t field_id, double *out, void *stream) {
    if (!h) return CGE_ERR_INVALID_ARG;
    if (!out || field_id < 0 || field_id > CGE_RESTAURANT_INFO_NEEDS_RESET) return h->fail(CGE_ERR_INVALID_ARG, "cge_restaurant_info: bad field / null out");
    DeviceGuard g(h->device);
    hipLaunchKernelGGL(restaurant::info_kernel, dim3(grid256(h->n)), dim3(256), 0, as_stream(stream), h->state, h->n, field_id, out);
    return launched(h);
}

CGE_DEFINE_ROWS_FINAL_OBS(restaurant, int32_t, 64)
CGE_DEFINE_ERROR_COUNT(restaurant)
CGE_DEFINE_SNAPSHOT(restaurant)

}  // extern "C"
