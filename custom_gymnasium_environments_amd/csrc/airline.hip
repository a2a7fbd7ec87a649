// airline.hip — batched AirlineOperationsEnv for MI355X (gfx950): kernels + C ABI (include/cge_amd.h).
//
// The record and the dynamics are airline_env.hpp (plain C++, also replayed on the host against the reference fixtures); this file is
// what is the device's own: where the record lives during a launch, the generator, the action sources and the observation rows.
//
// State per env: 414 32-bit columns [word][env] (1,656 B).  One lane per env, one wave per workgroup.  During a launch
//   registers  what is indexed at compile time and changes often: gates, weather, the scalars (~95 VGPRs)
//   LDS        what a runtime index reaches, as rows [k][lane] (no bank conflict: a wave reads one row): the 25 aircraft words, 15
//              masks "aircraft on the ground at airport p" (rebuilt at load, so the first free aircraft at a flight's origin is one
//              read and a count of trailing zeros instead of a walk over 25 words), the 15 fuel prices and weather severities
//   HBM        the 150 flight words: every step reads them as coalesced columns, thirty independent loads at a time, and writes
//              back only the word of a flight that changes state (each does so at most twice per episode); fuel level and
//              maintenance base of the 25 aircraft (float64, read by every observation, written on arrival / at a maintenance event
//              only: airline_env.hpp) and the ten float64 scheduled times the observation shows
// Draws: CPython's randint / uniform / choice on the env's own MT19937 stream, one word at a time (MtStream): a step draws at most a
// handful of words and only some lanes do; a reset draws about 270, the network about 1,100.
//
// Observation: float32 [n, 160] row-major.  Each lane computes its row in four parts of 40 floats and stores the part as ten 16-byte
// pieces (160 B, whole 32-byte sectors); the four parts complete every 128-byte line within one observation.  Parking the part in LDS
// and writing it with consecutive lanes on consecutive pieces, as the other row-major types do, was measured and is 3-23 % SLOWER
// here (profiles/airline_timing.txt): the kernel waits on dependent loads, not on stores, and the tile's 10.4 KB cost it two waves per CU.
// That variant, -DCGE_AIRLINE_LDS_ROWS, was last buildable at commit 84dc52e.
#include <cstring>
#include <string>
#include <vector>

#include "cge_lane.hpp"
#include "airline_env.hpp"

namespace cge {
namespace airline {

constexpr int BLOCK = 64;        // one wave: the LDS rows are the wave's own, no cross-wave barrier
static_assert(OBS == CGE_AIRLINE_OBS_FLOATS && REC_WORDS * 4 == CGE_AIRLINE_RECORD_BYTES, "cge_amd.h");

struct Params : LaneParams<float> {
    static constexpr bool terminates = true;                         // terminated only; truncated is never set (:430)
};
static_assert(std::is_trivially_copyable<Params>::value, "a kernel argument");

// what a runtime index reaches (airline_env.hpp's accessor): LDS rows of this lane, HBM columns of this env (LaneCols)
// The compiler forms a 64-bit per-lane address for every column it touches and keeps what it can reuse: the ~120 addresses of
// load_env for store_env, the ~70 of the observation's loads across a rollout's step loop — more registers than there are.  Hence
// fresh() at the top of every step as well as before the stores.
struct Mem : LaneCols {
    uint32_t *acw, *av;                                              // [k * BLOCK]
    float *sv;
    double *pr;
    __device__ __forceinline__ uint32_t ac(uint32_t a) const { return acw[a * BLOCK]; }
    __device__ __forceinline__ void set_ac(uint32_t a, uint32_t w) { acw[a * BLOCK] = w; }
    __device__ __forceinline__ uint32_t avail(uint32_t p) const { return av[p * BLOCK]; }
    __device__ __forceinline__ void set_avail(uint32_t p, uint32_t m) { av[p * BLOCK] = m; }
    __device__ __forceinline__ float sev(uint32_t p) const { return sv[p * BLOCK]; }
    __device__ __forceinline__ void set_sev(uint32_t p, float v) { sv[p * BLOCK] = v; }
    __device__ __forceinline__ double price(uint32_t p) const { return pr[p * BLOCK]; }
    __device__ __forceinline__ void set_price(uint32_t p, double v) { pr[p * BLOCK] = v; }
    __device__ __forceinline__ double fuel(int a) const { return dword(W_FUEL + 2 * a); }
    __device__ __forceinline__ void set_fuel(int a, double v) { set_dword(W_FUEL + 2 * a, v); }
    __device__ __forceinline__ double maint0(int a) const { return dword(W_MAINT + 2 * a); }
    __device__ __forceinline__ void set_maint0(int a, double v) { set_dword(W_MAINT + 2 * a, v); }
    __device__ __forceinline__ uint32_t flight(int f) const { return word(W_FLIGHT + f); }
    __device__ __forceinline__ void set_flight(int f, uint32_t w) { set_word(W_FLIGHT + f, w); }
    __device__ __forceinline__ double sched(int f) const { return dword(W_SCHED + 2 * f); }
    __device__ __forceinline__ void set_sched(int f, double s) { set_dword(W_SCHED + 2 * f, s); }
};

__device__ __forceinline__ void load_env(Env &e, Mem &m) {
#pragma unroll
    for (int p = 0; p < NP; ++p) m.set_avail(p, 0u);
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        const uint32_t w = m.word(W_AC + a);
        m.set_ac(a, w);
        if (!ac_flying(w)) m.set_avail(ac_airport(w), m.avail(ac_airport(w)) | 1u << a);
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        e.gate[p] = m.dword(W_GATE + 2 * p);
        m.set_price(p, m.dword(W_PRICE + 2 * p));
        m.set_sev(p, __uint_as_float(m.word(W_SEV + p)));
    }
#pragma unroll
    for (int s = 0; s < NWX; ++s) {
#pragma unroll
        for (int k = 0; k < 5; ++k) e.wx[s][k] = m.dword(W_WX + 10 * s + 2 * k);
    }
    e.unpack_scalars([&](int k) __attribute__((always_inline)) { return m.word(W_SCAL + k); });
}
// prices: only a reset changes them
__device__ __forceinline__ void store_env(const Env &e, Mem &m, bool prices) {
#pragma unroll
    for (int a = 0; a < NA; ++a) m.set_word(W_AC + a, m.ac(a));
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        m.set_dword(W_GATE + 2 * p, e.gate[p]);
        if (prices) m.set_dword(W_PRICE + 2 * p, m.price(p));
        m.set_word(W_SEV + p, __float_as_uint(m.sev(p)));
    }
#pragma unroll
    for (int s = 0; s < NWX; ++s) {
#pragma unroll
        for (int k = 0; k < 5; ++k) m.set_dword(W_WX + 10 * s + 2 * k, e.wx[s][k]);
    }
    e.pack_scalars([&](int k, uint32_t v) __attribute__((always_inline)) { m.set_word(W_SCAL + k, v); });
}

// One part of the wave's rows: floats [40 * PART, 40 * PART + 40) of row `lane` of `rows`.  Every lane stores its own 160 bytes of the
// part, 64 lanes 640 bytes apart per instruction: whole 32-byte sectors, no tile, no barrier.
template <int PART>
__device__ __forceinline__ void observe_rows(const Env &e, Mem &m, float *__restrict__ rows, int lane, bool live) {
    if (live) {
        float v4[PART_FLOATS];
        observe_part<PART>(e, m, [&](int k, float v) __attribute__((always_inline)) { v4[k] = v; });
#pragma unroll
        for (int k = 0; k < PART_FLOATS; k += 4)
            *reinterpret_cast<float4 *>(rows + (int64_t)lane * OBS + PART * PART_FLOATS + k) = make_float4(v4[k], v4[k + 1], v4[k + 2], v4[k + 3]);
    }
}
// _get_observation :354-396 of the wave's envs -> their rows of o [n, 160]
__device__ __forceinline__ void observe(const Env &e, Mem &m, float *__restrict__ o, bool live) {
    const int lane = (int)threadIdx.x;
    float *rows = o + (int64_t)blockIdx.x * BLOCK * OBS;
    observe_rows<0>(e, m, rows, lane, live);
    observe_rows<1>(e, m, rows, lane, live);
    observe_rows<2>(e, m, rows, lane, live);
    observe_rows<3>(e, m, rows, lane, live);
}

#define CGE_AIRLINE_LDS                                   \
    __shared__ uint32_t s_ac[NA * BLOCK], s_av[NP * BLOCK]; \
    __shared__ float s_sv[NP * BLOCK];                    \
    __shared__ double s_pr[NP * BLOCK];

// k steps with the record in registers and LDS.  ROLLOUT: per-step outputs indexed [t, env], sums; GIVEN: the caller's actions, else
// the counter hash cge_hash_action(action_seed, env_index0 + i, t0 + t, 45, 0).
template <int MODE, bool ROLLOUT, bool GIVEN>
__device__ __forceinline__ void run(const Params &p) {
    CGE_AIRLINE_LDS
    const int lane = (int)threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * BLOCK + lane;
    const bool live = i < p.n;
    const int64_t li = live ? i : p.n - 1;
    Mem m{{reinterpret_cast<uint32_t *>(p.state), p.n, lane_col_offset<BLOCK>(p.n)}, s_ac + lane, s_av + lane, s_sv + lane, s_pr + lane};
    Env e;
    load_env(e, m);
    MtStream rng(p.mt + li * MT_STRIDE, e.mt_pos, 0u);
    const uint64_t key = GIVEN ? 0 : hash_env_key(p.a_seed, (uint64_t)(p.env0 + li));
    double rsum = 0.0;
    int32_t dcount = 0;
    bool prices = false;
    const int ksteps = ROLLOUT ? p.k_steps : 1;
#pragma unroll 1
    for (int t = 0; t < ksteps; ++t) {
        m.fresh();
        const int32_t a = GIVEN ? p.actions[(int64_t)t * p.n + li] : (int32_t)hash_action_from_key(key, (uint64_t)(p.t0 + t), 45u, 0u);
        float reward = 0.0f;
        bool term = false, reset_now = false;
        if (live) {
            if (MODE == CGE_AUTORESET_NEXT_STEP && e.needs_reset) {
                reset_now = true;
            } else {
                const bool valid = a >= 0 && a < 45;
                if (!valid) atomicAdd(p.err_count, 1ull);           // _process_action is skipped; the rest of the step runs
                const double r = env_step(e, m, rng, a, valid, term);
                e.ret += r;
                reward = (float)r;                                   // an integer of at most five digits: exact
                if (term) lane_episode_end<MODE>(p, i, e.ret, (int32_t)e.t, reset_now, e.needs_reset);
            }
        }
        if (MODE == CGE_AUTORESET_SAME_STEP && !ROLLOUT) {           // the terminal rows: every env of a wave with a terminated one
            if (p.final_obs && __ballot(term)) observe(e, m, p.final_obs, live);
        }
        if (MODE != CGE_AUTORESET_DISABLED && reset_now) { reset_episode(e, m, rng); prices = true; }
        if (lane_obs_due<ROLLOUT>(p, t, ksteps)) observe(e, m, p.obs + (int64_t)t * p.obs_step_stride, live);
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
        e.mt_pos = rng.pos;
        m.fresh();
        store_env(e, m, prices);
        if (ROLLOUT) lane_sums(p, i, rsum, dcount);
    }
}

template <int MODE>
__global__ __launch_bounds__(BLOCK) void step_kernel(Params p) { run<MODE, false, true>(p); }

template <int MODE, bool ACTIONS>
__global__ __launch_bounds__(BLOCK) void rollout_kernel(Params p) { run<MODE, true, ACTIONS>(p); }

// reset (mask) / construction (init, or rewind after a re-seed: the network and the constructor's own reset, from the start of the
// stream) + obs
__global__ __launch_bounds__(BLOCK) void reset_kernel(Params p, int init, int rewind) {
    CGE_AIRLINE_LDS
    const int lane = (int)threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * BLOCK + lane;
    const bool live = i < p.n;
    const int64_t li = live ? i : p.n - 1;
    Mem m{{reinterpret_cast<uint32_t *>(p.state), p.n, lane_col_offset<BLOCK>(p.n)}, s_ac + lane, s_av + lane, s_sv + lane, s_pr + lane};
    Env e;
    load_env(e, m);
    bool dirty = false;
    if (live) {
        if (init || rewind) {
            MtStream rng(p.mt + li * MT_STRIDE, 0u, 0u);
            draw_network(e, m, rng);
            e.mt_pos = rng.pos;
            dirty = true;
        } else if (!p.mask || p.mask[i]) {
            MtStream rng(p.mt + li * MT_STRIDE, e.mt_pos, 0u);
            reset_episode(e, m, rng);
            e.mt_pos = rng.pos;
            dirty = true;
        }
        if (dirty) store_env(e, m, true);
    }
    if (p.obs) observe(e, m, p.obs, live);
}

__global__ __launch_bounds__(256) void info_kernel(const uint32_t *__restrict__ state, int64_t n, int field, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    Env e;
    e.unpack_scalars([&](int k) __attribute__((always_inline)) { return state[(int64_t)(W_SCAL + k) * n + i]; });
    double v = 0.0;
    switch (field) {
        case CGE_AIRLINE_INFO_ON_TIME_PERFORMANCE: v = e.otp(); break;
        case CGE_AIRLINE_INFO_PASSENGER_SATISFACTION: v = e.sat; break;
        case CGE_AIRLINE_INFO_DAILY_REVENUE: v = 0.0; break;
        case CGE_AIRLINE_INFO_DAILY_COSTS: v = e.costs; break;
        case CGE_AIRLINE_INFO_CURRENT_HOUR: v = (double)e.h4 * 0.25; break;
        case CGE_AIRLINE_INFO_TIMESTEP: v = (double)e.t; break;
        case CGE_AIRLINE_INFO_NEEDS_RESET: v = (double)e.needs_reset; break;
        case CGE_AIRLINE_INFO_FLIGHTS_IN_AIR: {
            uint32_t c = 0;
            for (int a = 0; a < NA; ++a) c += ac_flying(state[(int64_t)(W_AC + a) * n + i]) ? 1u : 0u;
            v = (double)c;
            break;
        }
        case CGE_AIRLINE_INFO_DELAY_COMPENSATION: v = e.comp; break;
        case CGE_AIRLINE_INFO_FUEL_COSTS: v = e.fuel_costs; break;
    }
    out[i] = v;
}

}  // namespace airline
}  // namespace cge

using namespace cge;

struct cge_airline : LaneHandle {
    using Params = airline::Params;
    cge_airline_config cfg{};
    static constexpr uint32_t snap_tag = 8u;
    static constexpr const char *abi = "cge_airline", *kernel_ns = "cge::airline::";
    static constexpr int block = airline::BLOCK, seed_kind = 0;
    Params params() const {
        Params p{};
        fill(p);
        return p;
    }
    int64_t step_elems() const { return n * airline::OBS; }
    CGE_LANE_KERNELS(airline)
    static int check(const cge_airline_config &c) { return bad_autoreset_mode(c.autoreset_mode) || c.reserved != 0 ? CGE_ERR_INVALID_ARG : CGE_OK; }
    hipError_t init() { return lane_init(this, airline::REC_WORDS); }
};

extern "C" {

CGE_DEFINE_LIFECYCLE(airline)

int cge_airline_seed(cge_airline *h, const uint64_t *seeds, uint64_t base_seed, void *stream) { return lane_seed(h, seeds, base_seed, stream); }

int cge_airline_reset(cge_airline *h, const uint8_t *mask, float *obs_out, void *stream) {
    if (h && !rows_aligned(obs_out, nullptr)) return h->fail(CGE_ERR_INVALID_ARG, "cge_airline_reset: obs must be 16-byte aligned");
    return lane_reset(h, mask, obs_out, stream);
}

int cge_airline_step(cge_airline *h, const int32_t *actions, float *obs_out, float *reward_out, uint8_t *terminated_out, uint8_t *truncated_out,
                     float *final_obs_out, void *stream) {
    return lane_step(h, actions && obs_out && reward_out && terminated_out && rows_aligned(obs_out, final_obs_out),
                     "cge_airline_step: null actions/obs/reward/terminated pointer, or obs / final_obs not 16-byte aligned", actions, obs_out, reward_out,
                     terminated_out, truncated_out, final_obs_out, stream);
}

int cge_airline_rollout(cge_airline *h, int32_t k_steps, const int32_t *actions, uint64_t action_seed, int64_t t0, float *obs_out,
                        int64_t obs_step_stride, float *reward_traj_out, uint8_t *terminated_traj_out, double *reward_sum_out,
                        int32_t *done_count_out, void *stream) {
    return lane_rollout(h, obs_step_stride % 4 == 0 && rows_aligned(obs_out, nullptr), "cge_airline_rollout: bad k_steps / obs_step_stride / obs alignment",
                        k_steps, actions, action_seed, t0, obs_out, obs_step_stride, reward_traj_out, terminated_traj_out, reward_sum_out, done_count_out,
                        stream);
}

int cge_airline_info(cge_airline *h, int32_t field_id, double *out, void *stream) {
    if (!h) return CGE_ERR_INVALID_ARG;
    if (!out || field_id < 0 || field_id > CGE_AIRLINE_INFO_FUEL_COSTS) return h->fail(CGE_ERR_INVALID_ARG, "cge_airline_info: bad field / null out");
    DeviceGuard g(h->device);
    hipLaunchKernelGGL(airline::info_kernel, dim3(grid256(h->n)), dim3(256), 0, as_stream(stream), reinterpret_cast<const uint32_t *>(h->state), h->n,
                       field_id, out);
    return launched(h);
}

CGE_DEFINE_ERROR_COUNT(airline)
CGE_DEFINE_SNAPSHOT(airline)
CGE_DEFINE_LANE_RECORDS(airline, LANE_RECORDS_AIRLINE, nullptr)

}  // extern "C"
