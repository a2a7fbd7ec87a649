// farm.hip — batched AgriculturalFarmEnv for MI355X (gfx950): kernels + C ABI (include/cge_amd.h).
//
// The record and the dynamics are farm_env.hpp (plain C++, also replayed on the host against the reference fixtures); this file is
// what is the device's own: where the record lives during a launch, the two generators, the action sources and the observation rows.
//
// State per env: 208 32-bit columns [word][env] (832 B).  One lane per env, one wave per workgroup.  During a launch
//   registers  the whole record: 89 float64 (fields 44, equipment 16, weather 5, market 10, the rest 14) and the integers.  What a
//              runtime index reaches (a field, a machine, a crop) is reached by a compare in an unrolled loop or a chain of selects
//              (farm_env.hpp), so no array is indexed in memory
//   LDS        only the tile of the observation's store pass, 9,360 B a wave
//   HBM        nothing is read or written per step but the outputs: the whole record is loaded at the start of a launch and stored at
//              its end
// Draws: two MT19937 blocks per env.  `mt` is NumPy's legacy stream (np.random.seed(s_i)): every step draws 15 to 25 doubles from it
// (the weather 5 or 7, a pest test per growing field and now and then its uniform, five Gaussians — 2.5 polar pairs on average, each
// with its rejections — and five uniforms for the market).  Its words are twisted AHEAD of the cursor, a 32-word chunk (one 128-byte
// line) at a time and by the whole wave together (mt_make_ready: 192 words from the cursor at the top of every step, so that a reset
// inside the step — 54 uniforms and 16 bounded integers, about 125 words — finds ready words too); the draws themselves are plain
// loads of ready words, and a draw past them twists word by word (MtStream).  `py` is CPython's global `random`
// (random.seed(s_i)): random.choice draws from it when an empty field is planted, a few words an episode, twisted as they are consumed.
//
// Observation: float32 [n, 620] row-major, 155 sixteen-byte pieces a row of which the last 121 are zero (the reference pads 134 values
// to its Box(620)).  The 134 live values leave in four groups of at most 36: a group is parked in LDS [element][env] and written with
// consecutive lanes on consecutive pieces of a row; then the wave writes the zero pieces of its rows from a register, consecutive
// lanes on consecutive pieces.  compact_obs: rows of 134 floats (536 B, so 8-byte pieces) and no zero pass.
#include <cstring>
#include <string>
#include <vector>

#include "cge_lane.hpp"
#include "farm_env.hpp"

namespace cge {
namespace farm {

constexpr int BLOCK = 64;        // one wave
constexpr uint32_t READY = 192;  // words made ready at the top of a step
constexpr int STG_COUNT = 36;    // floats of a row that leave together, at the most
constexpr int STG_ROW = BLOCK + 1;   // the store pass reads down a column: an odd row length spreads it over the banks
constexpr int STG_FLOATS = STG_COUNT * STG_ROW;
constexpr int LIVE_PIECES = (LIVE + 3) / 4, ZERO_PIECES = OBS / 4 - LIVE_PIECES;   // 34 and 121 sixteen-byte pieces of a full row
static_assert(OBS == CGE_FARM_OBS_FLOATS && LIVE == CGE_FARM_COMPACT_OBS_FLOATS && REC_WORDS * 4 == CGE_FARM_RECORD_BYTES && ACTIONS == CGE_FARM_ACTIONS, "cge_amd.h");
static_assert(INFO_COUNT - 1 == CGE_FARM_INFO_WATER_QUALITY && INFO_FIELD_YIELD_POTENTIAL == CGE_FARM_INFO_FIELD_YIELD_POTENTIAL, "cge_amd.h");
static_assert(OBS % 4 == 0 && LIVE % 2 == 0, "whole pieces");

struct Params : LaneParams<float> {
    static constexpr bool terminates = true;                         // the reference never truncates
    uint32_t *py;                                                    // the CPython streams, laid out as `mt`
    uint32_t max_years;
    int32_t row;                                                     // floats of an observation row: 620, or 134 (compact_obs)
};
static_assert(std::is_trivially_copyable<Params>::value, "a kernel argument");
struct RowsParams : Params {                                         // rollout_rows_kernel's: the other kernels' arguments stay as they are
    FinalSeg fin;
};

using Cols = LaneCols;
using Rng = LaneRng;

__device__ __forceinline__ void load_env(Env &e, const Cols &c) {
    Env::each_double(e, [&](int w, double &v) __attribute__((always_inline)) { v = c.dword(w); });
    e.unpack_ints([&](int k) __attribute__((always_inline)) { return c.word(W_INT + k); });
}
__device__ __forceinline__ void store_env(const Env &e, const Cols &c) {
    Env::each_double(e, [&](int w, const double &v) __attribute__((always_inline)) { c.set_dword(w, v); });
    e.pack_ints([&](int k, uint32_t v) __attribute__((always_inline)) { c.set_word(W_INT + k, v); });
}

// One group of the wave's rows: floats [FIRST, FIRST + COUNT) of each, of which those below LIVE come from the env and the rest are
// zero, written as pieces of PIECE floats.  Call with every lane of the wave (there are barriers).
template <int FIRST, int COUNT, int PIECE>
__device__ __forceinline__ void observe_group(const Env &e, float *__restrict__ stg, float *__restrict__ rows, int row, int envs, int lane, bool live) {
    static_assert(FIRST % PIECE == 0 && COUNT % PIECE == 0 && COUNT <= STG_COUNT, "whole pieces");
    if (live) {
        auto sink = [&](int k, float x) __attribute__((always_inline)) {
            if (k >= FIRST && k < FIRST + COUNT) stg[(k - FIRST) * STG_ROW + lane] = x;
        };
        observe(e, sink);
#pragma unroll
        for (int k = LIVE; k < FIRST + COUNT; ++k) stg[(k - FIRST) * STG_ROW + lane] = 0.0f;
    }
    __syncthreads();
    constexpr int PER = COUNT / PIECE;
    const int pieces = envs * PER;
#pragma unroll 2
    for (int q = lane; q < pieces; q += BLOCK) {
        const int env = q / PER, pc = q - env * PER;
        const float *s = stg + (PIECE * pc) * STG_ROW + env;
        float *dst = rows + (int64_t)env * row + FIRST + PIECE * pc;
        if (PIECE == 4) *reinterpret_cast<float4 *>(dst) = make_float4(s[0], s[STG_ROW], s[2 * STG_ROW], s[3 * STG_ROW]);
        else *reinterpret_cast<float2 *>(dst) = make_float2(s[0], s[STG_ROW]);
    }
    __syncthreads();                                                 // the tile is free for the next group
}
// _get_observation :435-518 of the wave's envs -> their rows of o [n, row].  Call with every lane of the wave.
__device__ __forceinline__ void observe_rows(const Env &e, float *__restrict__ stg, float *__restrict__ o, int64_t n, int row, bool live) {
    const int lane = (int)threadIdx.x;
    const int64_t first = (int64_t)blockIdx.x * BLOCK;
    const int envs = (int)(n - first < BLOCK ? n - first : BLOCK);
    float *rows = o + first * row;
    if (row == OBS) {
        observe_group<0, 36, 4>(e, stg, rows, OBS, envs, lane, live);
        observe_group<36, 36, 4>(e, stg, rows, OBS, envs, lane, live);
        observe_group<72, 36, 4>(e, stg, rows, OBS, envs, lane, live);
        observe_group<108, 4 * LIVE_PIECES - 108, 4>(e, stg, rows, OBS, envs, lane, live);
        const int pieces = envs * ZERO_PIECES;                        // the padding: 121 zero pieces a row
        const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll 4
        for (int q = lane; q < pieces; q += BLOCK) {
            const int env = q / ZERO_PIECES, pc = q - env * ZERO_PIECES;
            *reinterpret_cast<float4 *>(rows + (int64_t)env * OBS + 4 * (LIVE_PIECES + pc)) = zero;
        }
    } else {
        observe_group<0, 36, 2>(e, stg, rows, LIVE, envs, lane, live);
        observe_group<36, 36, 2>(e, stg, rows, LIVE, envs, lane, live);
        observe_group<72, 36, 2>(e, stg, rows, LIVE, envs, lane, live);
        observe_group<108, LIVE - 108, 2>(e, stg, rows, LIVE, envs, lane, live);
    }
}

// observe_group for the terminal rows of one step of rollout_rows_kernel (lane_final_rows): the lanes with `mine` park their group in
// column `rank`, and the store pass writes `keep` dense rows at `rows`.  Call with every lane of the wave.
template <int FIRST, int COUNT, int PIECE>
__device__ __forceinline__ void final_group(const Env &e, float *__restrict__ stg, float *__restrict__ rows, int row, int keep, int rank, bool mine) {
    static_assert(COUNT <= STG_COUNT, "the tile");
    if (mine) {
        auto sink = [&](int k, float x) __attribute__((always_inline)) {
            if (k >= FIRST && k < FIRST + COUNT) stg[(k - FIRST) * STG_ROW + rank] = x;
        };
        observe(e, sink);
#pragma unroll
        for (int k = LIVE; k < FIRST + COUNT; ++k) stg[(k - FIRST) * STG_ROW + rank] = 0.0f;
    }
    __syncthreads();
    lane_store_tile<FIRST, COUNT, PIECE, STG_ROW>(stg, rows, row, keep);
    __syncthreads();                                                 // the tile is free for the next group
}
// ... and observe_rows: `keep` rows of `row` floats at `rows`, the padding of a full row included
__device__ __forceinline__ void final_observe(const Env &e, float *__restrict__ stg, float *__restrict__ rows, int row, int keep, int rank, bool mine) {
    if (row == OBS) {
        final_group<0, 36, 4>(e, stg, rows, OBS, keep, rank, mine);
        final_group<36, 36, 4>(e, stg, rows, OBS, keep, rank, mine);
        final_group<72, 36, 4>(e, stg, rows, OBS, keep, rank, mine);
        final_group<108, 4 * LIVE_PIECES - 108, 4>(e, stg, rows, OBS, keep, rank, mine);
        const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (int q = (int)threadIdx.x; q < keep * ZERO_PIECES; q += BLOCK) {
            const int r = q / ZERO_PIECES, pc = q - r * ZERO_PIECES;
            *reinterpret_cast<float4 *>(rows + (int64_t)r * OBS + 4 * (LIVE_PIECES + pc)) = zero;
        }
    } else {
        final_group<0, 36, 2>(e, stg, rows, LIVE, keep, rank, mine);
        final_group<36, 36, 2>(e, stg, rows, LIVE, keep, rank, mine);
        final_group<72, 36, 2>(e, stg, rows, LIVE, keep, rank, mine);
        final_group<108, LIVE - 108, 2>(e, stg, rows, LIVE, keep, rank, mine);
    }
}

// k steps with the record in registers.  ROLLOUT: per-step outputs indexed [t, env], sums; GIVEN: the caller's actions, else the
// counter hash cge_hash_action(action_seed, env_index0 + i, t0 + t, 45, 0).  With RowsParams (ROWS, a SAME_STEP rollout) the terminal rows
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
    Rng rng(p.mt + li * MT_STRIDE, e.mt_pos, e.mt_ready), py(p.py + li * MT_STRIDE, e.py_pos, e.py_ready);
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
                if (!valid) atomicAdd(p.err_count, 1ull);           // it falls through every branch of _process_action; the rest of the step runs
                reward = (float)env_step(e, rng, py, a, valid, p.max_years, term);   // an integer below 2^24
                if (term) lane_episode_end<MODE>(p, i, e.ep_ret, (int32_t)e.day, reset_now, e.needs_reset);
            }
        }
        if (MODE == CGE_AUTORESET_SAME_STEP && !ROLLOUT) {           // the terminal rows: every env of a wave with a terminated one
            if (p.final_obs && __ballot(term)) observe_rows(e, s_stg, p.final_obs, p.n, p.row, live);
        }
        if constexpr (ROWS) {                                        // ... of the terminated envs only, compacted: lane_final_rows
            float *dst;
            int keep, rank;
            if (__builtin_expect(lane_final_rows(p.fin, fin_used, term, t, i, p.row, dst, keep, rank), false)) final_observe(e, s_stg, dst, p.row, keep, rank, term && rank < keep);
        }
        if (live && MODE != CGE_AUTORESET_DISABLED && reset_now) reset_episode(e, rng);
        if (lane_obs_due<ROLLOUT>(p, t, ksteps)) observe_rows(e, s_stg, p.obs + (int64_t)t * p.obs_step_stride, p.n, p.row, live);
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
        e.mt_pos = rng.s.pos; e.mt_ready = rng.s.pretw;
        e.py_pos = py.s.pos; e.py_ready = py.s.pretw;
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

// the SAME_STEP rollout while terminal rows are registered (cge_rows_farm_rollout_final_obs)
template <bool ACTIONS_GIVEN>
__global__ __launch_bounds__(BLOCK) void rollout_rows_kernel(RowsParams p) { run<CGE_AUTORESET_SAME_STEP, true, ACTIONS_GIVEN>(p); }

// reset (mask) / construction (init, or rewind after a re-seed: a fresh AgriculturalFarmEnv(), which draws its fields, equipment and
// market, on both streams at their start) + obs
__global__ __launch_bounds__(BLOCK) void reset_kernel(Params p, int init, int rewind) {
    __shared__ float s_stg[STG_FLOATS];
    const int lane = (int)threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * BLOCK + lane;
    const bool live = i < p.n;
    const int64_t li = live ? i : p.n - 1;
    Cols c{reinterpret_cast<uint32_t *>(p.state), p.n, lane_col_offset<BLOCK>(p.n)};
    Env e;
    load_env(e, c);
    const bool fresh = init || rewind, draws = live && (fresh || !p.mask || p.mask[li]);
    if (fresh) { e.mt_pos = 0u; e.mt_ready = 0u; e.py_pos = 0u; e.py_ready = 0u; }
    Rng rng(p.mt + li * MT_STRIDE, e.mt_pos, e.mt_ready);
    mt_make_ready(rng.s.w, rng.s.pos, rng.s.pretw, READY, draws);     // the whole wave: either draws about 125 words
    if (draws) {
        if (fresh) construct(e, rng);
        else reset_episode(e, rng);
        e.mt_pos = rng.s.pos; e.mt_ready = rng.s.pretw;
        c.fresh();
        store_env(e, c);
    }
    if (p.obs) observe_rows(e, s_stg, p.obs, p.n, p.row, live);
}

__global__ __launch_bounds__(BLOCK) void info_kernel(Params p, int field, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= p.n) return;
    Cols c{reinterpret_cast<uint32_t *>(p.state), p.n, lane_col_offset<BLOCK>(p.n)};
    Env e;
    load_env(e, c);
    out[i] = info_value(e, field);
}

}  // namespace farm
}  // namespace cge

using namespace cge;

struct cge_farm : LaneHandle {
    using Params = farm::Params;
    using RowsParams = farm::RowsParams;
    cge_farm_config cfg{};
    uint32_t *py = nullptr;
    static constexpr uint32_t snap_tag = 11u;
    static constexpr const char *abi = "cge_farm", *kernel_ns = "cge::farm::", *rows_ns = kernel_ns;
    static constexpr int block = farm::BLOCK, seed_kind = 1;         // `mt`: np.random.seed; `py` is seeded as random.seed (kind 0)
    int row() const { return cfg.compact_obs ? farm::LIVE : farm::OBS; }
    uintptr_t piece_mask() const { return cfg.compact_obs ? 7u : 15u; }   // rows leave as 16-byte pieces, compact ones as 8-byte pieces
    Params params() const {
        Params p{};
        fill(p);
        p.py = py;
        p.max_years = (uint32_t)cfg.max_years;
        p.row = row();
        return p;
    }
    int64_t step_elems() const { return n * row(); }
    CGE_LANE_KERNELS(farm)
    CGE_LANE_LAUNCH_ROWS(farm)
    static int check(const cge_farm_config &c) {
        return bad_autoreset_mode(c.autoreset_mode) || c.max_years < 1 || c.max_years > 255 || c.compact_obs < 0 || c.compact_obs > 1 ? CGE_ERR_INVALID_ARG : CGE_OK;
    }
    hipError_t seed_streams(const uint64_t *seeds, uint64_t base_seed, hipStream_t s) {
        CGE_HIP(launch_mt_seed(mt, MT_STRIDE, n, seeds, base_seed, env0, 1, s));
        return launch_mt_seed(py, MT_STRIDE, n, seeds, base_seed, env0, 0, s);
    }
    hipError_t init() {
        CGE_HIP(alloc(state, (size_t)farm::REC_WORDS * n * sizeof(uint32_t), true, true));
        CGE_HIP(alloc(mt, (size_t)n * MT_STRIDE * sizeof(uint32_t), false, true));
        CGE_HIP(alloc(py, (size_t)n * MT_STRIDE * sizeof(uint32_t), false, true));
        CGE_HIP(alloc(err, sizeof(unsigned long long), true, false));
        CGE_HIP(seed_streams(nullptr, 0, nullptr));
        lane_launch_reset(this, params(), 1, 0, nullptr);
        return hipGetLastError();
    }
};

extern "C" {

CGE_DEFINE_LIFECYCLE(farm)

int cge_farm_seed(cge_farm *h, const uint64_t *seeds, uint64_t base_seed, void *stream) {
    if (!h) return CGE_ERR_INVALID_ARG;
    if (int st = seed_base_check(h, "cge_farm_seed", seeds, base_seed, true)) return st;
    DeviceGuard g(h->device);
    CGE_TRY(h, h->seed_streams(seeds, base_seed, as_stream(stream)));
    lane_launch_reset(h, h->params(), 0, 1, as_stream(stream));
    return launched(h);
}

int cge_farm_reset(cge_farm *h, const uint8_t *mask, float *obs_out, void *stream) {
    if (h && !rows_aligned(obs_out, nullptr, h->piece_mask())) return h->fail(CGE_ERR_INVALID_ARG, "cge_farm_reset: obs must be 16-byte aligned (compact_obs: 8-byte)");
    return lane_reset(h, mask, obs_out, stream);
}

int cge_farm_step(cge_farm *h, const int32_t *actions, float *obs_out, float *reward_out, uint8_t *terminated_out, uint8_t *truncated_out,
                  float *final_obs_out, void *stream) {
    return lane_step(h, h && actions && obs_out && reward_out && terminated_out && rows_aligned(obs_out, final_obs_out, h->piece_mask()),
                     "cge_farm_step: null actions/obs/reward/terminated pointer, or obs / final_obs not 16-byte aligned (compact_obs: 8-byte)", actions,
                     obs_out, reward_out, terminated_out, truncated_out, final_obs_out, stream);
}

int cge_farm_rollout(cge_farm *h, int32_t k_steps, const int32_t *actions, uint64_t action_seed, int64_t t0, float *obs_out, int64_t obs_step_stride,
                     float *reward_traj_out, uint8_t *terminated_traj_out, double *reward_sum_out, int32_t *done_count_out, void *stream) {
    return lane_rollout(h, h && obs_step_stride % (h->cfg.compact_obs ? 2 : 4) == 0 && rows_aligned(obs_out, h->fin_rows, h->piece_mask()),
                        "cge_farm_rollout: bad k_steps / obs_step_stride, or obs / the registered terminal rows not 16-byte aligned (compact_obs: 8-byte)", k_steps, actions, action_seed, t0, obs_out, obs_step_stride,
                        reward_traj_out, terminated_traj_out, reward_sum_out, done_count_out, stream);
}

int cge_farm_info(cge_farm *h, int32_t field_id, double *out, void *stream) {
    return lane_info(h, out && field_id >= 0 && field_id <= CGE_FARM_INFO_WATER_QUALITY, "cge_farm_info: bad field / null out", farm::info_kernel, field_id, out,
                     stream);
}

CGE_DEFINE_ROWS_FINAL_OBS(farm, float, 64)
CGE_DEFINE_ERROR_COUNT(farm)
CGE_DEFINE_SNAPSHOT(farm)
CGE_DEFINE_LANE_RECORDS(farm, LANE_RECORDS_FARM, h->py)

}  // extern "C"
