// space_station.hip — batched SpaceStationEnv for MI355X (gfx950): kernels + C ABI (include/cge_amd.h).
//
// The record and the dynamics are space_station_env.hpp (plain C++, also replayed on the host against the reference fixtures); this
// file is what is the device's own: where the record lives during a launch, the generator, the action sources and the observation rows.
//
// State per env: 188 32-bit columns [word][env] (752 B).  One lane per env, one wave per workgroup.  During a launch
//   registers  the whole record: 83 float64 (modules 32, crew 18, systems 24, resources 5, battery, total power, the two returns),
//              12 last_maintenance counters and the scalars.  What a runtime index reaches (a system, a module, a crew member) is
//              written with a compare and a select per element (space_station_env.hpp: set_at), so no array is indexed in memory
//   LDS        only the tile of the observation's store pass, 9,360 B a wave
//   HBM        nothing is read or written per step but the outputs: the whole record is loaded at the start of a launch and stored at
//              its end
// Draws: NumPy's legacy random_sample / uniform / normal / choice on the env's own MT19937 stream (np.random.seed(s_i)).  Every step
// draws at least 13 doubles (the emergency test and twelve failure tests, 26 words), 8 more while thermal control is down, 2 more for
// actions 30..35, and a few single words when an emergency strikes.  The words are twisted AHEAD of the cursor, a 32-word chunk (one
// 128-byte line) at a time and by the whole wave together (mt_make_ready: 192 words from the cursor at the top of every step, so that
// a reset inside the step — 32 Gaussians and 24 uniforms, about 130 words — finds ready words too).  The degradation tail (24 words),
// the thermal drift (16) and the pair of an environmental action (4) are fetched as runs of 16-byte loads (Rng::run); the emergency
// test and the draws of a reset read their ready words singly.  A draw past the ready words twists word by word (MtStream).
//
// Observation: float32 [n, 120] row-major, 30 sixteen-byte pieces a row, in four groups (crew, systems, modules, the rest).  A group is
// parked in LDS [element][env] and written with consecutive lanes on consecutive pieces of a row.  Each lane storing its own row as
// it computes it, the other form the rows can leave in, is 2-4 % slower here — the opposite of the airline and emergency types,
// whose records fill the LDS (profiles/space_station_timing.txt; that variant, -DCGE_STATION_LANE_ROWS, was last buildable at
// commit 84dc52e).
#include <cstring>
#include <string>
#include <vector>

#include "cge_lane.hpp"
#include "space_station_env.hpp"

namespace cge {
namespace station {

constexpr int BLOCK = 64;        // one wave
constexpr uint32_t READY = 192;  // words made ready at the top of a step
constexpr int STG_COUNT = 36;    // floats of a row that leave together, at the most
constexpr int STG_ROW = BLOCK + 1;   // the store pass reads down a column: an odd row length spreads it over the banks
constexpr int STG_FLOATS = STG_COUNT * STG_ROW;
static_assert(OBS == CGE_SPACE_STATION_OBS_FLOATS && REC_WORDS * 4 == CGE_SPACE_STATION_RECORD_BYTES && ACTIONS == CGE_SPACE_STATION_ACTIONS, "cge_amd.h");
static_assert(INFO_COUNT - 1 == CGE_SPACE_STATION_INFO_EVACUATED && INFO_AVG_CREW_HEALTH == CGE_SPACE_STATION_INFO_AVG_CREW_HEALTH, "cge_amd.h");

struct Params : LaneParams<float> {
    static constexpr bool terminates = true;                         // terminated; at the step limit truncated too, a second write (:343-344)
    uint32_t max_t;
};
static_assert(std::is_trivially_copyable<Params>::value, "a kernel argument");
struct RowsParams : Params {                                         // rollout_rows_kernel's: the other kernels' arguments stay as they are
    FinalSeg fin;
};

using Cols = LaneCols;
using Rng = LaneRng;

__device__ __forceinline__ void load_env(Env &e, const Cols &c) {
    Env::each_double(e, [&](int w, double &v) __attribute__((always_inline)) { v = c.dword(w); });
#pragma unroll
    for (int s = 0; s < NS; ++s) e.last_maint[s] = c.word(W_LM + s);
    e.unpack_scalars([&](int k) __attribute__((always_inline)) { return c.word(W_SCAL + k); });
}
__device__ __forceinline__ void store_env(const Env &e, const Cols &c) {
    Env::each_double(e, [&](int w, const double &v) __attribute__((always_inline)) { c.set_dword(w, v); });
#pragma unroll
    for (int s = 0; s < NS; ++s) c.set_word(W_LM + s, e.last_maint[s]);
    e.pack_scalars([&](int k, uint32_t v) __attribute__((always_inline)) { c.set_word(W_SCAL + k, v); });
}

// One group of the wave's rows: floats [FIRST, FIRST + COUNT) of each, computed by gen(sink) with sink(k, value), k the element's index
// in the row.  Call with every lane of the wave (there are barriers).
template <int FIRST, int COUNT, class G>
__device__ __forceinline__ void observe_group(float *__restrict__ stg, float *__restrict__ rows, int envs, int lane, bool live, G gen) {
    static_assert(FIRST % 4 == 0 && COUNT % 4 == 0 && COUNT <= STG_COUNT, "whole 16-byte pieces");
    if (live) gen([&](int k, float x) __attribute__((always_inline)) { stg[(k - FIRST) * STG_ROW + lane] = x; });
    __syncthreads();
    const int pieces = envs * (COUNT / 4);
#pragma unroll 2
    for (int q = lane; q < pieces; q += BLOCK) {
        const int env = q / (COUNT / 4), pc = q - env * (COUNT / 4);
        const float *s = stg + (4 * pc) * STG_ROW + env;
        *reinterpret_cast<float4 *>(rows + (int64_t)env * OBS + FIRST + 4 * pc) = make_float4(s[0], s[STG_ROW], s[2 * STG_ROW], s[3 * STG_ROW]);
    }
    __syncthreads();                                                 // the tile is free for the next group
}
// _get_observation :739-783 of the wave's envs -> their rows of o [n, 120], 30 sixteen-byte pieces a row: crew (6 pieces), systems (9),
// modules (8), the rest (7).  Call with every lane of the wave.
__device__ __forceinline__ void observe(const Env &e, float *__restrict__ stg, float *__restrict__ o, int64_t n, bool live) {
    const int lane = (int)threadIdx.x;
    const int64_t first = (int64_t)blockIdx.x * BLOCK;
    const int envs = (int)(n - first < BLOCK ? n - first : BLOCK);
    float *rows = o + first * OBS;
    observe_group<0, 24>(stg, rows, envs, lane, live, [&](auto out) __attribute__((always_inline)) { observe_crew(e, out); });
    observe_group<24, 36>(stg, rows, envs, lane, live, [&](auto out) __attribute__((always_inline)) { observe_systems(e, out); });
    observe_group<60, 32>(stg, rows, envs, lane, live, [&](auto out) __attribute__((always_inline)) { observe_modules(e, out); });
    observe_group<92, 28>(stg, rows, envs, lane, live, [&](auto out) __attribute__((always_inline)) { observe_rest(e, out); });
}

// observe_group for the terminal rows of one step of rollout_rows_kernel (lane_final_rows): the lanes with `mine` park their group in
// column `rank`, and the store pass writes `keep` dense rows at `rows`.  Call with every lane of the wave.
template <int FIRST, int COUNT, class G>
__device__ __forceinline__ void final_group(float *__restrict__ stg, float *__restrict__ rows, int keep, int rank, bool mine, G gen) {
    if (mine) gen([&](int k, float x) __attribute__((always_inline)) { stg[(k - FIRST) * STG_ROW + rank] = x; });
    __syncthreads();
    lane_store_tile<FIRST, COUNT, 4, STG_ROW>(stg, rows, OBS, keep);
    __syncthreads();                                                 // the tile is free for the next group
}
__device__ __forceinline__ void final_observe(const Env &e, float *__restrict__ stg, float *__restrict__ rows, int keep, int rank, bool mine) {
    final_group<0, 24>(stg, rows, keep, rank, mine, [&](auto out) __attribute__((always_inline)) { observe_crew(e, out); });
    final_group<24, 36>(stg, rows, keep, rank, mine, [&](auto out) __attribute__((always_inline)) { observe_systems(e, out); });
    final_group<60, 32>(stg, rows, keep, rank, mine, [&](auto out) __attribute__((always_inline)) { observe_modules(e, out); });
    final_group<92, 28>(stg, rows, keep, rank, mine, [&](auto out) __attribute__((always_inline)) { observe_rest(e, out); });
}

// k steps with the record in registers.  ROLLOUT: per-step outputs indexed [t, env], sums; GIVEN: the caller's actions, else the
// counter hash cge_hash_action(action_seed, env_index0 + i, t0 + t, 40, 0).  With RowsParams (ROWS, a SAME_STEP rollout) the terminal rows
// go to the wave's segment of p.fin.
template <int MODE, bool ROLLOUT, bool GIVEN, class P = Params>
__device__ __forceinline__ void run(const P &p) {
    constexpr bool ROWS = std::is_same<P, RowsParams>::value;
    static_assert(!ROWS || (ROLLOUT && MODE == CGE_AUTORESET_SAME_STEP), "terminal rows: fused SAME_STEP rollouts");
    __shared__ float s_stg[STG_FLOATS];
    const int lane = (int)threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * BLOCK + lane;
    const bool live = i < p.n;
    const int64_t li = live ? i : p.n - 1;
    Cols c{reinterpret_cast<uint32_t *>(p.state), p.n, lane_col_offset<BLOCK>(p.n)};
    Env e;
    load_env(e, c);
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
        bool term = false, trunc = false, reset_now = false;
        if (live) {
            if (MODE == CGE_AUTORESET_NEXT_STEP && e.needs_reset) {
                reset_now = true;
            } else {
                const bool valid = a >= 0 && a < ACTIONS;
                if (!valid) atomicAdd(p.err_count, 1ull);           // _process_action is skipped; the rest of the step runs
                reward = (float)env_step(e, rng, a, valid, p.max_t, term, trunc);   // an integer; beyond 2^24 rounded as the reference's float64 is
                if (term) lane_episode_end<MODE>(p, i, e.ep_ret, (int32_t)e.t, reset_now, e.needs_reset);
            }
        }
        if (MODE == CGE_AUTORESET_SAME_STEP && !ROLLOUT) {           // the terminal rows: every env of a wave with a terminated one
            if (p.final_obs && __ballot(term)) observe(e, s_stg, p.final_obs, p.n, live);
        }
        if constexpr (ROWS) {                                        // ... of the terminated envs only, compacted: lane_final_rows
            float *dst;
            int keep, rank;
            if (__builtin_expect(lane_final_rows(p.fin, fin_used, term, t, i, OBS, dst, keep, rank), false)) final_observe(e, s_stg, dst, keep, rank, term && rank < keep);
        }
        if (live && MODE != CGE_AUTORESET_DISABLED && reset_now) reset_episode(e, rng);
        if (lane_obs_due<ROLLOUT>(p, t, ksteps)) observe(e, s_stg, p.obs + (int64_t)t * p.obs_step_stride, p.n, live);
        if (live) {
            if (ROLLOUT) {
                rsum += (double)reward;
                dcount += term ? 1 : 0;
                if (p.reward) p.reward[(int64_t)t * p.n + i] = reward;
                if (p.terminated) p.terminated[(int64_t)t * p.n + i] = term ? 1 : 0;
            } else {
                lane_step_outputs(p, i, reward, term);
                if (p.truncated) p.truncated[i] = trunc ? 1 : 0;     // the step limit raises both flags
            }
        }
    }
    if (live) {
        e.mt_pos = rng.s.pos;
        e.mt_ready = rng.s.pretw;
        c.fresh();
        store_env(e, c);
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

// the SAME_STEP rollout while terminal rows are registered (cge_rows_space_station_rollout_final_obs)
template <bool ACTIONS_GIVEN>
__global__ __launch_bounds__(BLOCK) void rollout_rows_kernel(RowsParams p) { run<CGE_AUTORESET_SAME_STEP, true, ACTIONS_GIVEN>(p); }

// reset (mask) / construction (init, or rewind after a re-seed: a fresh SpaceStationEnv(), which draws nothing, on a stream at its
// start) + obs
__global__ __launch_bounds__(BLOCK) void reset_kernel(Params p, int init, int rewind) {
    __shared__ float s_stg[STG_FLOATS];
    const int lane = (int)threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * BLOCK + lane;
    const bool live = i < p.n;
    const int64_t li = live ? i : p.n - 1;
    Cols c{reinterpret_cast<uint32_t *>(p.state), p.n, lane_col_offset<BLOCK>(p.n)};
    Env e;
    load_env(e, c);
    const bool fresh = init || rewind, draws = !fresh && live && (!p.mask || p.mask[li]);
    if (fresh) { e.mt_pos = 0u; e.mt_ready = 0u; }
    Rng rng(p.mt + li * MT_STRIDE, e.mt_pos, e.mt_ready);
    mt_make_ready(rng.s.w, rng.s.pos, rng.s.pretw, READY, draws);     // the whole wave: a reset draws about 130 words
    if (live) {
        if (fresh) construct(e);
        else if (draws) reset_episode(e, rng);
        e.mt_pos = rng.s.pos; e.mt_ready = rng.s.pretw;
        c.fresh();
        if (fresh || draws) store_env(e, c);
    }
    if (p.obs) observe(e, s_stg, p.obs, p.n, live);
}

__global__ __launch_bounds__(BLOCK) void info_kernel(Params p, int field, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= p.n) return;
    Cols c{reinterpret_cast<uint32_t *>(p.state), p.n, lane_col_offset<BLOCK>(p.n)};
    Env e;
    load_env(e, c);
    out[i] = info_value(e, field);
}

}  // namespace station
}  // namespace cge

using namespace cge;

struct cge_space_station : LaneHandle {
    using Params = station::Params;
    using RowsParams = station::RowsParams;
    cge_space_station_config cfg{};
    static constexpr uint32_t snap_tag = 10u;
    static constexpr const char *abi = "cge_space_station", *kernel_ns = "cge::station::", *rows_ns = kernel_ns;
    static constexpr int block = station::BLOCK, seed_kind = 1;      // np.random.seed
    Params params() const {
        Params p{};
        fill(p);
        p.max_t = (uint32_t)cfg.max_steps;
        return p;
    }
    int64_t step_elems() const { return n * station::OBS; }
    CGE_LANE_KERNELS(station)
    CGE_LANE_LAUNCH_ROWS(station)
    static int check(const cge_space_station_config &c) {
        return bad_autoreset_mode(c.autoreset_mode) || c.max_steps < 1 || c.max_steps > 65535 ? CGE_ERR_INVALID_ARG : CGE_OK;
    }
    hipError_t init() {
        CGE_HIP(alloc(state, (size_t)station::REC_WORDS * n * sizeof(uint32_t), true, true));
        CGE_HIP(alloc(mt, (size_t)n * MT_STRIDE * sizeof(uint32_t), false, true));
        CGE_HIP(alloc(err, sizeof(unsigned long long), true, false));
        CGE_HIP(launch_mt_seed(mt, MT_STRIDE, n, nullptr, 0, env0, seed_kind, nullptr));
        lane_launch_reset(this, params(), 1, 0, nullptr);
        return hipGetLastError();
    }
};

extern "C" {

CGE_DEFINE_LIFECYCLE(space_station)

int cge_space_station_seed(cge_space_station *h, const uint64_t *seeds, uint64_t base_seed, void *stream) { return lane_seed(h, seeds, base_seed, stream); }

int cge_space_station_reset(cge_space_station *h, const uint8_t *mask, float *obs_out, void *stream) {
    if (h && !rows_aligned(obs_out, nullptr)) return h->fail(CGE_ERR_INVALID_ARG, "cge_space_station_reset: obs must be 16-byte aligned");
    return lane_reset(h, mask, obs_out, stream);
}

int cge_space_station_step(cge_space_station *h, const int32_t *actions, float *obs_out, float *reward_out, uint8_t *terminated_out,
                           uint8_t *truncated_out, float *final_obs_out, void *stream) {
    return lane_step(h, actions && obs_out && reward_out && terminated_out && rows_aligned(obs_out, final_obs_out),
                     "cge_space_station_step: null actions/obs/reward/terminated pointer, or obs / final_obs not 16-byte aligned", actions, obs_out,
                     reward_out, terminated_out, truncated_out, final_obs_out, stream);
}

int cge_space_station_rollout(cge_space_station *h, int32_t k_steps, const int32_t *actions, uint64_t action_seed, int64_t t0, float *obs_out,
                              int64_t obs_step_stride, float *reward_traj_out, uint8_t *terminated_traj_out, double *reward_sum_out,
                              int32_t *done_count_out, void *stream) {
    return lane_rollout(h, h && obs_step_stride % 4 == 0 && rows_aligned(obs_out, h->fin_rows),
                        "cge_space_station_rollout: bad k_steps / obs_step_stride, or obs / the registered terminal rows not 16-byte aligned",
                        k_steps, actions, action_seed, t0, obs_out, obs_step_stride, reward_traj_out, terminated_traj_out, reward_sum_out, done_count_out,
                        stream);
}

int cge_space_station_info(cge_space_station *h, int32_t field_id, double *out, void *stream) {
    return lane_info(h, out && field_id >= 0 && field_id <= CGE_SPACE_STATION_INFO_EVACUATED, "cge_space_station_info: bad field / null out", station::info_kernel,
                     field_id, out, stream);
}

CGE_DEFINE_ROWS_FINAL_OBS(space_station, float, 64)
CGE_DEFINE_ERROR_COUNT(space_station)
CGE_DEFINE_SNAPSHOT(space_station)
CGE_DEFINE_LANE_RECORDS(space_station, LANE_RECORDS_STATION, nullptr)

}  // extern "C"
