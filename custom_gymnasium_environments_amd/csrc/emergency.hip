// emergency.hip — batched EmergencyResponseEnv for MI355X (gfx950): kernels + C ABI (include/cge_amd.h).
//
// The record and the dynamics are emergency_env.hpp (plain C++, also replayed on the host against the reference fixtures); this file
// is what is the device's own: where the record lives during a launch, the generator, the action sources and the observation rows.
//
// State per env: 202 32-bit columns [word][env] (808 B).  One lane per env, one wave per workgroup.  During a launch
//   registers  what is indexed at compile time: the 25 traffic values, weather, the scalars (~100 VGPRs)
//   LDS        what a runtime index reaches, as rows [k][lane] (no bank conflict: a wave reads one row): the 3 x 20 incident words
//              (a unit's slot, the dispatch and cascade walks) and the 20 unit words with their float64 fatigue (the dispatched unit
//              is the action) — 120 words a lane, 30 KB a wave
//   HBM        nothing is read or written per step but the outputs: the whole record is loaded at the start of a launch and stored at
//              its end
// Draws: CPython's random / uniform / randint on the env's own MT19937 stream.  Every step draws at least 58 words (arrival 2,
// weather 6, traffic 50) and up to some 200 more (escalations, cascades, working units).  The words are twisted AHEAD of the cursor,
// a 32-word chunk (one 128-byte line) at a time and by the whole wave together (mt_make_ready: 160 words from the cursor at the top
// of every step), so a draw is a plain load of a ready word and nothing is written back per draw.  The step's fixed tail — weather and
// traffic, 56 words — is fetched as three runs of 16-byte loads (Rng::run) that do not depend on one another; the variable part in
// front of it (one to a few words at a time, under branches) reads its ready words singly.  A step that draws past the 160 ready
// words (it takes rejections in randint or a full house of escalations) falls back to twisting word by word (MtStream).
//
// Observation: float32 [n, 276] row-major, 69 sixteen-byte pieces a row.  Each lane stores its own row as it computes it, in four
// groups (incidents, units 0..19, units 20..39, the rest).  Parking a group in LDS and writing it with consecutive lanes on
// consecutive pieces, the other form the rows can leave in, was measured and dropped (profiles/emergency_timing.txt; that variant,
// -DCGE_EMERGENCY_LDS_ROWS, was last buildable at commit 84dc52e).
#include <cstring>
#include <string>
#include <vector>

#include "cge_lane.hpp"
#include "emergency_env.hpp"

namespace cge {
namespace emergency {

constexpr int BLOCK = 64;        // one wave: the LDS rows are the wave's own, no cross-wave barrier
constexpr uint32_t READY = 160;  // words made ready at the top of a step
static_assert(OBS == CGE_EMERGENCY_OBS_FLOATS && REC_WORDS * 4 == CGE_EMERGENCY_RECORD_BYTES && ACTIONS == CGE_EMERGENCY_ACTIONS, "cge_amd.h");

struct Params : LaneParams<float> {
    static constexpr bool terminates = true;                         // terminated only; truncated is never set (:922)
    uint32_t max_t;
};
static_assert(std::is_trivially_copyable<Params>::value, "a kernel argument");
struct RowsParams : Params {                                         // rollout_rows_kernel's: the other kernels' arguments stay as they are
    FinalSeg fin;
};

// what a runtime index reaches (emergency_env.hpp's accessor): LDS rows of this lane
struct Mem {
    uint32_t *iw, *im, *is, *uw;                                     // [k * BLOCK]
    double *fa;
    __device__ __forceinline__ uint32_t inc(uint32_t s) const { return iw[s * BLOCK]; }
    __device__ __forceinline__ void set_inc(uint32_t s, uint32_t w) { iw[s * BLOCK] = w; }
    __device__ __forceinline__ uint32_t mask(uint32_t s) const { return im[s * BLOCK]; }
    __device__ __forceinline__ void set_mask(uint32_t s, uint32_t w) { im[s * BLOCK] = w; }
    __device__ __forceinline__ uint32_t start(uint32_t s) const { return is[s * BLOCK]; }
    __device__ __forceinline__ void set_start(uint32_t s, uint32_t w) { is[s * BLOCK] = w; }
    __device__ __forceinline__ uint32_t unit(uint32_t u) const { return uw[u * BLOCK]; }
    __device__ __forceinline__ void set_unit(uint32_t u, uint32_t w) { uw[u * BLOCK] = w; }
    __device__ __forceinline__ double fatigue(uint32_t u) const { return fa[u * BLOCK]; }
    __device__ __forceinline__ void set_fatigue(uint32_t u, double v) { fa[u * BLOCK] = v; }
};

using Cols = LaneCols;
using Rng = LaneRng;

__device__ __forceinline__ void load_env(Env &e, Mem &m, const Cols &c) {
#pragma unroll
    for (int s = 0; s < NI; ++s) {
        m.set_inc(s, c.word(W_INC + 3 * s));
        m.set_mask(s, c.word(W_INC + 3 * s + 1));
        m.set_start(s, c.word(W_INC + 3 * s + 2));
    }
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        m.set_unit(u, c.word(W_UNIT + u));
        m.set_fatigue(u, c.dword(W_FAT + 2 * u));
    }
#pragma unroll
    for (int k = 0; k < NT; ++k) e.traffic[k] = c.dword(W_TRAFFIC + 2 * k);
    e.unpack_scalars([&](int k) __attribute__((always_inline)) { return c.word(W_SCAL + k); });
}
__device__ __forceinline__ void store_env(const Env &e, Mem &m, const Cols &c) {
#pragma unroll
    for (int s = 0; s < NI; ++s) {
        c.set_word(W_INC + 3 * s, m.inc(s));
        c.set_word(W_INC + 3 * s + 1, m.mask(s));
        c.set_word(W_INC + 3 * s + 2, m.start(s));
    }
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        c.set_word(W_UNIT + u, m.unit(u));
        c.set_dword(W_FAT + 2 * u, m.fatigue(u));
    }
#pragma unroll
    for (int k = 0; k < NT; ++k) c.set_dword(W_TRAFFIC + 2 * k, e.traffic[k]);
    e.pack_scalars([&](int k, uint32_t v) __attribute__((always_inline)) { c.set_word(W_SCAL + k, v); });
}

// One group of the wave's rows: floats [FIRST, FIRST + COUNT) of each, computed by gen(sink) with sink(k, value), k the element's index
// in the row.  Every lane with `live` stores its own pieces of the group to row `lane`, 64 lanes 1,104 bytes apart.
template <int FIRST, int COUNT, class G>
__device__ __forceinline__ void observe_group(float *__restrict__ rows, int lane, bool live, G gen) {
    static_assert(FIRST % 4 == 0 && COUNT % 4 == 0, "whole 16-byte pieces");
    if (live) {
        float v[COUNT];
        gen([&](int k, float x) __attribute__((always_inline)) { v[k - FIRST] = x; });
#pragma unroll
        for (int q = 0; q < COUNT; q += 4) *reinterpret_cast<float4 *>(rows + (int64_t)lane * OBS + FIRST + q) = make_float4(v[q], v[q + 1], v[q + 2], v[q + 3]);
    }
}
// _get_observation :524-587 of the wave's envs -> their rows of o [n, 276], 69 sixteen-byte pieces a row: the incidents (20 pieces),
// the units in two halves (15 pieces each), the rest (19).  Call with every lane of the wave.
__device__ __forceinline__ void observe(const Env &e, Mem &m, float *__restrict__ o, int64_t n, bool live, uint32_t max_t) {
    const int lane = (int)threadIdx.x;
    const int64_t first = (int64_t)blockIdx.x * BLOCK;
    float *rows = o + first * OBS;
    observe_group<0, 80>(rows, lane, live, [&](auto out) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < NI; ++s) observe_incident(e, m, out, s);
    });
    observe_group<80, 60>(rows, lane, live, [&](auto out) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < 20; ++u) observe_unit(e, m, out, u);
    });
    observe_group<140, 60>(rows, lane, live, [&](auto out) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 20; u < 40; ++u) observe_unit(e, m, out, u);
    });
    observe_group<200, 76>(rows, lane, live, [&](auto out) __attribute__((always_inline)) { observe_rest(e, m, out, max_t); });
}

// observe_group / observe for the terminal rows of one step of rollout_rows_kernel (lane_final_rows): the lanes with `mine` store row
// `rank` of `rows` as they store their own rows everywhere else (there is no tile: the record fills the LDS; `keep`, the number of
// dense rows, is for a store pass and unused).  final_group is a function of its own for its __restrict__: calling observe_group
// from final_observe directly compiles both rollout_rows_kernel instances to other code
// (profiles/record_lane_refactor_resources.txt).
template <int FIRST, int COUNT, class G>
__device__ __forceinline__ void final_group(float *__restrict__ rows, int rank, bool mine, G gen) {
    observe_group<FIRST, COUNT>(rows, rank, mine, gen);
}
__device__ __forceinline__ void final_observe(const Env &e, Mem &m, float *__restrict__ rows, int keep, int rank, bool mine, uint32_t max_t) {
    final_group<0, 80>(rows, rank, mine, [&](auto out) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < NI; ++s) observe_incident(e, m, out, s);
    });
    final_group<80, 60>(rows, rank, mine, [&](auto out) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < 20; ++u) observe_unit(e, m, out, u);
    });
    final_group<140, 60>(rows, rank, mine, [&](auto out) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 20; u < 40; ++u) observe_unit(e, m, out, u);
    });
    final_group<200, 76>(rows, rank, mine, [&](auto out) __attribute__((always_inline)) { observe_rest(e, m, out, max_t); });
}

#define CGE_EMERGENCY_LDS                                                               \
    __shared__ uint32_t s_iw[NI * BLOCK], s_im[NI * BLOCK], s_is[NI * BLOCK], s_uw[NU * BLOCK]; \
    __shared__ double s_fa[NU * BLOCK];

// k steps with the record in registers and LDS.  ROLLOUT: per-step outputs indexed [t, env], sums; GIVEN: the caller's actions, else
// the counter hash cge_hash_action(action_seed, env_index0 + i, t0 + t, 50, 0).  With RowsParams (ROWS, a SAME_STEP rollout) the terminal rows
// go to the wave's segment of p.fin.
template <int MODE, bool ROLLOUT, bool GIVEN, class P = Params>
__device__ __forceinline__ void run(const P &p) {
    constexpr bool ROWS = std::is_same<P, RowsParams>::value;
    static_assert(!ROWS || (ROLLOUT && MODE == CGE_AUTORESET_SAME_STEP), "terminal rows: fused SAME_STEP rollouts");
    CGE_EMERGENCY_LDS
    const int lane = (int)threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * BLOCK + lane;
    const bool live = i < p.n;
    const int64_t li = live ? i : p.n - 1;
    Mem m{s_iw + lane, s_im + lane, s_is + lane, s_uw + lane, s_fa + lane};
    Cols c{reinterpret_cast<uint32_t *>(p.state), p.n, lane_col_offset<BLOCK>(p.n)};
    Env e;
    load_env(e, m, c);
    Rng rng(p.mt + li * MT_STRIDE, e.mt_pos, e.mt_ready);
    const uint64_t key = GIVEN ? 0 : hash_env_key(p.a_seed, (uint64_t)(p.env0 + li));
    double rsum = 0.0;
    int32_t dcount = 0;
    uint32_t fin_used = 0;                                           // ROWS: terminal rows the wave's segment has been handed
    const int ksteps = ROLLOUT ? p.k_steps : 1;
#pragma unroll 1
    for (int t = 0; t < ksteps; ++t) {
        const int32_t a = GIVEN ? p.actions[(int64_t)t * p.n + li] : (int32_t)hash_action_from_key(key, (uint64_t)(p.t0 + t), (uint32_t)ACTIONS, 0u);
        mt_make_ready(rng.s.w, rng.s.pos, rng.s.pretw, READY, live);  // the whole wave: twist ahead what this step will draw
        float reward = 0.0f;
        bool term = false, reset_now = false;
        if (live) {
            if (MODE == CGE_AUTORESET_NEXT_STEP && e.needs_reset) {
                reset_now = true;
            } else {
                const bool valid = a >= 0 && a < ACTIONS;
                if (!valid) atomicAdd(p.err_count, 1ull);           // falls through every branch of _execute_action; the rest of the step runs
                const double r = env_step(e, m, rng, a, valid, p.max_t, term);
                e.ret += r;
                reward = (float)r;                                   // an integer below 2^24: exact
                if (term) lane_episode_end<MODE>(p, i, e.ret, (int32_t)e.t, reset_now, e.needs_reset);
            }
        }
        if (MODE == CGE_AUTORESET_SAME_STEP && !ROLLOUT) {           // the terminal rows: every env of a wave with a terminated one
            if (p.final_obs && __ballot(term)) observe(e, m, p.final_obs, p.n, live, p.max_t);
        }
        if constexpr (ROWS) {                                        // ... of the terminated envs only, compacted: lane_final_rows
            float *dst;
            int keep, rank;
            if (__builtin_expect(lane_final_rows(p.fin, fin_used, term, t, i, OBS, dst, keep, rank), false)) final_observe(e, m, dst, keep, rank, term && rank < keep, p.max_t);
        }
        if (live && MODE != CGE_AUTORESET_DISABLED && reset_now) reset_episode(e, m, rng);
        if (lane_obs_due<ROLLOUT>(p, t, ksteps)) observe(e, m, p.obs + (int64_t)t * p.obs_step_stride, p.n, live, p.max_t);
        if (live) {
            if (ROLLOUT) {
                rsum += (double)reward;
                dcount += term ? 1 : 0;
                if (p.reward) p.reward[(int64_t)t * p.n + i] = reward;
                if (p.terminated) p.terminated[(int64_t)t * p.n + i] = term ? 1 : 0;
            } else {
                lane_step_outputs(p, i, reward, term);
            }
        }
    }
    if (live) {
        e.mt_pos = rng.s.pos;
        e.mt_ready = rng.s.pretw;
        c.fresh();
        store_env(e, m, c);
        if (ROLLOUT) lane_sums(p, i, rsum, dcount);
    }
    if constexpr (ROWS) {
        if (lane == 0) p.fin.count[blockIdx.x] = (int32_t)fin_used;
    }
}

template <int MODE>
__global__ __launch_bounds__(BLOCK) void step_kernel(Params p) { run<MODE, false, true>(p); }

template <int MODE, bool ACTIONS_GIVEN>
__global__ __launch_bounds__(BLOCK) void rollout_kernel(Params p) { run<MODE, true, ACTIONS_GIVEN>(p); }

// the SAME_STEP rollout while terminal rows are registered (cge_rows_emergency_rollout_final_obs)
template <bool ACTIONS_GIVEN>
__global__ __launch_bounds__(BLOCK) void rollout_rows_kernel(RowsParams p) { run<CGE_AUTORESET_SAME_STEP, true, ACTIONS_GIVEN>(p); }

// reset (mask) / construction (init, or rewind after a re-seed: the constructor's draws from the start of the stream, which leave the
// env without an incident until the reset that follows) + obs
__global__ __launch_bounds__(BLOCK) void reset_kernel(Params p, int init, int rewind) {
    CGE_EMERGENCY_LDS
    const int lane = (int)threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * BLOCK + lane;
    const bool live = i < p.n;
    const int64_t li = live ? i : p.n - 1;
    Mem m{s_iw + lane, s_im + lane, s_is + lane, s_uw + lane, s_fa + lane};
    Cols c{reinterpret_cast<uint32_t *>(p.state), p.n, lane_col_offset<BLOCK>(p.n)};
    Env e;
    load_env(e, m, c);
    if (live) {
        bool dirty = false;
        if (init || rewind) {
            Rng rng(p.mt + li * MT_STRIDE, 0u, 0u);
            draw_network(e, m, rng);
            e.mt_pos = rng.s.pos; e.mt_ready = rng.s.pretw;
            dirty = true;
        } else if (!p.mask || p.mask[i]) {
            Rng rng(p.mt + li * MT_STRIDE, e.mt_pos, e.mt_ready);
            reset_episode(e, m, rng);
            e.mt_pos = rng.s.pos; e.mt_ready = rng.s.pretw;
            dirty = true;
        }
        c.fresh();
        if (dirty) store_env(e, m, c);
    }
    if (p.obs) observe(e, m, p.obs, p.n, live, p.max_t);
}

__global__ __launch_bounds__(256) void info_kernel(const uint32_t *__restrict__ state, int64_t n, int field, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    Env e;
    e.unpack_scalars([&](int k) __attribute__((always_inline)) { return state[(int64_t)(W_SCAL + k) * n + i]; });
    double v = 0.0;
    switch (field) {
        case CGE_EMERGENCY_INFO_ACTIVE_EMERGENCIES: v = (double)e.ninc; break;
        case CGE_EMERGENCY_INFO_TOTAL_CASUALTIES: v = (double)e.casualties; break;
        case CGE_EMERGENCY_INFO_LIVES_SAVED: v = (double)e.lives; break;
        case CGE_EMERGENCY_INFO_EMERGENCIES_RESOLVED: v = (double)e.resolved; break;
        case CGE_EMERGENCY_INFO_AVG_RESPONSE_TIME: v = e.avg_rt(); break;
        case CGE_EMERGENCY_INFO_TERMINATION_REASON: v = (double)e.reason; break;
        case CGE_EMERGENCY_INFO_TIMESTEP: v = (double)e.t; break;
        case CGE_EMERGENCY_INFO_NEEDS_RESET: v = (double)e.needs_reset; break;
        case CGE_EMERGENCY_INFO_BUSY_UNITS: {
            uint32_t b = 0;
            for (int u = 0; u < NU; ++u) b += state[(int64_t)(W_UNIT + u) * n + i] & U_BUSY ? 1u : 0u;
            v = (double)b;
            break;
        }
        case CGE_EMERGENCY_INFO_MUTUAL_AID_REQUESTED: v = (double)e.mutual; break;
        case CGE_EMERGENCY_INFO_NATIONAL_GUARD_ACTIVE: v = (double)e.guard; break;
        case CGE_EMERGENCY_INFO_STATE_OF_EMERGENCY: v = (double)e.soe; break;
    }
    out[i] = v;
}

}  // namespace emergency
}  // namespace cge

using namespace cge;

struct cge_emergency : LaneHandle {
    using Params = emergency::Params;
    using RowsParams = emergency::RowsParams;
    cge_emergency_config cfg{};
    static constexpr uint32_t snap_tag = 9u;
    static constexpr const char *abi = "cge_emergency", *kernel_ns = "cge::emergency::", *rows_ns = kernel_ns;
    static constexpr int block = emergency::BLOCK, seed_kind = 0;
    Params params() const {
        Params p{};
        fill(p);
        p.max_t = (uint32_t)cfg.max_timesteps;
        return p;
    }
    int64_t step_elems() const { return n * emergency::OBS; }
    CGE_LANE_KERNELS(emergency)
    CGE_LANE_LAUNCH_ROWS(emergency)
    static int check(const cge_emergency_config &c) {
        return bad_autoreset_mode(c.autoreset_mode) || c.max_timesteps < 1 || c.max_timesteps > 65535 ? CGE_ERR_INVALID_ARG : CGE_OK;
    }
    hipError_t init() { return lane_init(this, emergency::REC_WORDS); }
};

extern "C" {

CGE_DEFINE_LIFECYCLE(emergency)

int cge_emergency_seed(cge_emergency *h, const uint64_t *seeds, uint64_t base_seed, void *stream) { return lane_seed(h, seeds, base_seed, stream); }

int cge_emergency_reset(cge_emergency *h, const uint8_t *mask, float *obs_out, void *stream) {
    if (h && !rows_aligned(obs_out, nullptr)) return h->fail(CGE_ERR_INVALID_ARG, "cge_emergency_reset: obs must be 16-byte aligned");
    return lane_reset(h, mask, obs_out, stream);
}

int cge_emergency_step(cge_emergency *h, const int32_t *actions, float *obs_out, float *reward_out, uint8_t *terminated_out, uint8_t *truncated_out,
                       float *final_obs_out, void *stream) {
    return lane_step(h, actions && obs_out && reward_out && terminated_out && rows_aligned(obs_out, final_obs_out),
                     "cge_emergency_step: null actions/obs/reward/terminated pointer, or obs / final_obs not 16-byte aligned", actions, obs_out, reward_out,
                     terminated_out, truncated_out, final_obs_out, stream);
}

int cge_emergency_rollout(cge_emergency *h, int32_t k_steps, const int32_t *actions, uint64_t action_seed, int64_t t0, float *obs_out,
                          int64_t obs_step_stride, float *reward_traj_out, uint8_t *terminated_traj_out, double *reward_sum_out,
                          int32_t *done_count_out, void *stream) {
    return lane_rollout(h, h && obs_step_stride % 4 == 0 && rows_aligned(obs_out, h->fin_rows),
                        "cge_emergency_rollout: bad k_steps / obs_step_stride, or obs / the registered terminal rows not 16-byte aligned",
                        k_steps, actions, action_seed, t0, obs_out, obs_step_stride, reward_traj_out, terminated_traj_out, reward_sum_out, done_count_out,
                        stream);
}

int cge_emergency_info(cge_emergency *h, int32_t field_id, double *out, void *stream) {
    if (!h) return CGE_ERR_INVALID_ARG;
    if (!out || field_id < 0 || field_id > CGE_EMERGENCY_INFO_STATE_OF_EMERGENCY) return h->fail(CGE_ERR_INVALID_ARG, "cge_emergency_info: bad field / null out");
    DeviceGuard g(h->device);
    hipLaunchKernelGGL(emergency::info_kernel, dim3(grid256(h->n)), dim3(256), 0, as_stream(stream), reinterpret_cast<const uint32_t *>(h->state), h->n,
                       field_id, out);
    return launched(h);
}

CGE_DEFINE_ROWS_FINAL_OBS(emergency, float, 64)
CGE_DEFINE_ERROR_COUNT(emergency)
CGE_DEFINE_SNAPSHOT(emergency)
CGE_DEFINE_LANE_RECORDS(emergency, LANE_RECORDS_EMERGENCY, nullptr)

}  // extern "C"
