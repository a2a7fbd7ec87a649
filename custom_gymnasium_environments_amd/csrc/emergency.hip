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
// groups (incidents, units 0..19, units 20..39, the rest).  -DCGE_EMERGENCY_LDS_ROWS parks a group in LDS and writes it with
// consecutive lanes on consecutive pieces instead: the other form the rows can leave in, measured in profiles/emergency_timing.txt.
#include <cstring>
#include <string>
#include <vector>

#include "cge_lane.hpp"
#include "emergency_env.hpp"

namespace cge {
namespace emergency {

constexpr int BLOCK = 64;        // one wave: the LDS rows are the wave's own, no cross-wave barrier
constexpr uint32_t READY = 160;  // words made ready at the top of a step
constexpr int STG_COUNT = 80;    // floats of a row that leave together, at the most
#ifdef CGE_EMERGENCY_LDS_ROWS
constexpr int STG_ROW = BLOCK + 1;   // the store pass reads down a column: an odd row length spreads it over the banks
constexpr int STG_FLOATS = STG_COUNT * STG_ROW;
#else
constexpr int STG_FLOATS = 1;
#endif
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

// the env's columns: word w of env i at rec[w * n + i].  A scalar base plus ONE 32-bit byte offset per lane (4 * i: n_envs < 2^30)
// addresses every column; 64-bit per-lane addresses, one pair of registers per column and kept from the loads of a launch to its
// stores, took every register there is and spilled.  After fresh() the offset is a new value to the compiler: the addresses are
// formed again where they are used (one add each).
struct Cols {
    uint32_t *rec;                                                   // uniform
    int64_t n;
    uint32_t off;
    __device__ __forceinline__ void fresh() { asm volatile("" : "+v"(off)); }
    __device__ __forceinline__ uint32_t word(int w) const { return *reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(rec + (int64_t)w * n) + off); }
    __device__ __forceinline__ void set_word(int w, uint32_t v) const { *reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(rec + (int64_t)w * n) + off) = v; }
    __device__ __forceinline__ double dword(int w) const {
        const uint64_t u = (uint64_t)word(w) | (uint64_t)word(w + 1) << 32;
        double d;
        __builtin_memcpy(&d, &u, 8);
        return d;
    }
    __device__ __forceinline__ void set_dword(int w, double d) const {
        uint64_t u;
        __builtin_memcpy(&u, &d, 8);
        set_word(w, (uint32_t)u);
        set_word(w + 1, (uint32_t)(u >> 32));
    }
};

// the generator as emergency_env.hpp draws from it: single words, and runs of W words the caller consumes in order
struct Rng {
    MtStream s;
    __device__ __forceinline__ Rng(uint32_t *block, uint32_t pos, uint32_t ready) : s(block, pos, ready) {}
    __device__ __forceinline__ uint32_t next() { return s.next(); }
    template <int W>
    __device__ __forceinline__ void run(uint32_t (&w)[W]) {
        static_assert(W % 4 == 0 && W <= MT_N, "whole 16-byte pieces");
        if (s.pos + (uint32_t)W <= s.pretw) {
            // ready: W / 4 independent loads; a piece that straddles word 623 runs into the mirror of words 0..2, which the twist of the
            // next generation's first chunk has written
#pragma unroll
            for (int q = 0; q < W; q += 4) {
                uint32_t at = s.pos + (uint32_t)q;
                at -= at >= (uint32_t)MT_N ? (uint32_t)MT_N : 0u;
                const MtQuad v = *reinterpret_cast<const MtQuad *>(s.w + at);
                w[q] = mt_temper(v.a); w[q + 1] = mt_temper(v.b); w[q + 2] = mt_temper(v.c); w[q + 3] = mt_temper(v.d);
            }
            mt_advance(s.pos, s.pretw, (uint32_t)W);
        } else {
#pragma unroll
            for (int j = 0; j < W; ++j) w[j] = 0u;
#pragma unroll 1
            for (int k = 0; k < W; ++k) {
                const uint32_t y = s.next();
#pragma unroll
                for (int j = 0; j < W; ++j) w[j] = j == k ? y : w[j];   // no indexed register array
            }
        }
    }
};

// 4 * (the env of this lane, or the last env for a lane past the end), in 32-bit arithmetic throughout
__device__ __forceinline__ uint32_t lane_offset(int64_t n) {
    const uint32_t i = blockIdx.x * (uint32_t)BLOCK + threadIdx.x, last = (uint32_t)n - 1u;
    return (i < last ? i : last) * 4u;
}

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
// in the row.  Call with every lane of the wave (the LDS variant has barriers).
template <int FIRST, int COUNT, class G>
__device__ __forceinline__ void observe_group(float *__restrict__ stg, float *__restrict__ rows, int envs, int lane, bool live, G gen) {
    static_assert(FIRST % 4 == 0 && COUNT % 4 == 0 && COUNT <= STG_COUNT, "whole 16-byte pieces");
#ifndef CGE_EMERGENCY_LDS_ROWS                                        // every lane stores its own pieces of the group, 64 lanes 1,104 bytes apart
    if (live) {
        float v[COUNT];
        gen([&](int k, float x) __attribute__((always_inline)) { v[k - FIRST] = x; });
#pragma unroll
        for (int q = 0; q < COUNT; q += 4) *reinterpret_cast<float4 *>(rows + (int64_t)lane * OBS + FIRST + q) = make_float4(v[q], v[q + 1], v[q + 2], v[q + 3]);
    }
#else                                                                 // the variant measured and dropped (profiles/emergency_timing.txt): the group
                                                                      // parked in LDS [element][env], written as consecutive pieces per env
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
#endif
}
// _get_observation :524-587 of the wave's envs -> their rows of o [n, 276], 69 sixteen-byte pieces a row: the incidents (20 pieces),
// the units in two halves (15 pieces each), the rest (19).  Call with every lane of the wave.
__device__ __forceinline__ void observe(const Env &e, Mem &m, float *__restrict__ stg, float *__restrict__ o, int64_t n, bool live, uint32_t max_t) {
    const int lane = (int)threadIdx.x;
    const int64_t first = (int64_t)blockIdx.x * BLOCK;
    const int envs = (int)(n - first < BLOCK ? n - first : BLOCK);
    float *rows = o + first * OBS;
    observe_group<0, 80>(stg, rows, envs, lane, live, [&](auto out) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < NI; ++s) observe_incident(e, m, out, s);
    });
    observe_group<80, 60>(stg, rows, envs, lane, live, [&](auto out) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < 20; ++u) observe_unit(e, m, out, u);
    });
    observe_group<140, 60>(stg, rows, envs, lane, live, [&](auto out) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 20; u < 40; ++u) observe_unit(e, m, out, u);
    });
    observe_group<200, 76>(stg, rows, envs, lane, live, [&](auto out) __attribute__((always_inline)) { observe_rest(e, m, out, max_t); });
}

// observe_group for the terminal rows of one step of rollout_rows_kernel (lane_final_rows): the lanes with `mine` store row `rank` of
// `rows` as they store their own rows everywhere else (there is no tile: the record fills the LDS); the LDS variant parks their group
// in column `rank` and writes `keep` dense rows.  Call with every lane of the wave.
template <int FIRST, int COUNT, class G>
__device__ __forceinline__ void final_group(float *__restrict__ stg, float *__restrict__ rows, int keep, int rank, bool mine, G gen) {
#ifndef CGE_EMERGENCY_LDS_ROWS
    observe_group<FIRST, COUNT>(stg, rows, keep, rank, mine, gen);
#else
    if (mine) gen([&](int k, float x) __attribute__((always_inline)) { stg[(k - FIRST) * STG_ROW + rank] = x; });
    __syncthreads();
    lane_store_tile<FIRST, COUNT, 4, STG_ROW>(stg, rows, OBS, keep);
    __syncthreads();
#endif
}
__device__ __forceinline__ void final_observe(const Env &e, Mem &m, float *__restrict__ stg, float *__restrict__ rows, int keep, int rank, bool mine, uint32_t max_t) {
    final_group<0, 80>(stg, rows, keep, rank, mine, [&](auto out) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < NI; ++s) observe_incident(e, m, out, s);
    });
    final_group<80, 60>(stg, rows, keep, rank, mine, [&](auto out) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < 20; ++u) observe_unit(e, m, out, u);
    });
    final_group<140, 60>(stg, rows, keep, rank, mine, [&](auto out) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 20; u < 40; ++u) observe_unit(e, m, out, u);
    });
    final_group<200, 76>(stg, rows, keep, rank, mine, [&](auto out) __attribute__((always_inline)) { observe_rest(e, m, out, max_t); });
}

#define CGE_EMERGENCY_LDS                                                               \
    __shared__ uint32_t s_iw[NI * BLOCK], s_im[NI * BLOCK], s_is[NI * BLOCK], s_uw[NU * BLOCK]; \
    __shared__ double s_fa[NU * BLOCK];                                                 \
    __shared__ float s_stg[STG_FLOATS];

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
    Cols c{reinterpret_cast<uint32_t *>(p.state), p.n, lane_offset(p.n)};
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
            if (p.final_obs && __ballot(term)) observe(e, m, s_stg, p.final_obs, p.n, live, p.max_t);
        }
        if constexpr (ROWS) {                                        // ... of the terminated envs only, compacted: lane_final_rows
            float *dst;
            int keep, rank;
            if (__builtin_expect(lane_final_rows(p.fin, fin_used, term, t, i, OBS, dst, keep, rank), false)) final_observe(e, m, s_stg, dst, keep, rank, term && rank < keep, p.max_t);
        }
        if (live && MODE != CGE_AUTORESET_DISABLED && reset_now) reset_episode(e, m, rng);
        if (lane_obs_due<ROLLOUT>(p, t, ksteps)) observe(e, m, s_stg, p.obs + (int64_t)t * p.obs_step_stride, p.n, live, p.max_t);
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
    Cols c{reinterpret_cast<uint32_t *>(p.state), p.n, lane_offset(p.n)};
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
    if (p.obs) observe(e, m, s_stg, p.obs, p.n, live, p.max_t);
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
    auto reset_kernel() const { return emergency::reset_kernel; }
    template <int MODE>
    auto kernel(LaneKind kind) const {
        return kind == LANE_STEP ? emergency::step_kernel<MODE>
               : kind == LANE_ROLLOUT_GIVEN ? emergency::rollout_kernel<MODE, true> : emergency::rollout_kernel<MODE, false>;
    }
    void launch_rows(bool given, unsigned blocks, hipStream_t s, const RowsParams &p) const {
        hipLaunchKernelGGL(given ? emergency::rollout_rows_kernel<true> : emergency::rollout_rows_kernel<false>, dim3(blocks), dim3(block), 0, s, p);
    }
    static int check(const cge_emergency_config &c) {
        return bad_autoreset_mode(c.autoreset_mode) || c.max_timesteps < 1 || c.max_timesteps > 65535 ? CGE_ERR_INVALID_ARG : CGE_OK;
    }
    hipError_t init() {
        CGE_HIP(alloc(state, (size_t)emergency::REC_WORDS * n * sizeof(uint32_t), true, true));
        CGE_HIP(alloc(mt, (size_t)n * MT_STRIDE * sizeof(uint32_t), false, true));
        CGE_HIP(alloc(err, sizeof(unsigned long long), true, false));
        CGE_HIP(launch_mt_seed(mt, MT_STRIDE, n, nullptr, 0, env0, 0, nullptr));
        lane_launch_reset(this, params(), 1, 0, nullptr);
        return hipGetLastError();
    }
};

// observation rows leave as 16-byte pieces
static bool rows_aligned(const void *a, const void *b) { return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15u) == 0; }

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

}  // extern "C"
