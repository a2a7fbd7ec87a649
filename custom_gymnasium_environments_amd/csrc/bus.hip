// bus.hip — batched BusSystemEnv for MI355X (gfx950): kernels + C ABI (include/cge_amd.h).
//
// Re-expresses the reference's bus_system_env/ for N independent instances, one lane per env:
//   environment.py  reset :125-151, step :153-186, _update_buses :188-237, _process_passenger_movements :239-276,
//                   _calculate_boarding_priority :278-294, _update_passenger_counts :296-299, _get_observation :301-337
//   utils.py        generate_passengers :22-46, get_destination_distribution :49-62, get_next_stop :83-93
//   config.py       :6-19
// A passenger is only its destination and waits at its source, so the reference's passenger LISTS reduce exactly to COUNTS:
// 16 waiting counts [stop][destination] and 16 onboard counts [bus][destination].  The boarding priority (:278-294) depends only
// on (destination - stop) mod 4 — next stop 0, previous stop 1, opposite stop 2 — so the stable sort + pop(0) until full is
// "board min(free seats, count)" for destinations c+1, then c+3, then c+2.  bus.dwell_time is written on arrival and read only in
// the same iteration (:208-211): it is not state.
//
// State per env: 3 uint4 columns (SoA) — the waiting counts as bytes (one word per stop), the onboard counts as bytes (one word
// per bus), and one column of scalars: the four buses (stop:2 stopped:1 remaining:4), timestep, delivered, the episode return
// in half units (every reward is a multiple of 0.5), the MT19937 cursor and its ready mark.  The record lives in VGPRs.
//
// Draws: only reset() draws (CPython `random.randint` through _randbelow_with_getrandbits) — about 470 generator words per
// episode, and every env of a batch hits the time limit in the same step, so the reset is wave-convergent: the lanes twist
// their 32-word chunks ahead together (mt_make_ready), fetch 16 ready words per round and feed them to a three-state machine
// (passenger count / source / destination), one word per transition.
//
// Observations are key-major planes of int32 (gymnasium's batched-Dict layout): per key one contiguous [N, ...] array, each
// lane stores its own 16 / 64 / 4 bytes, a wave writes one contiguous run per key straight from registers.
#include <cstring>
#include <string>
#include <vector>

#include "cge_lane.hpp"

namespace cge {
namespace bus {

constexpr int NBUS = 4;          // config.py:7
constexpr int NSTOP = 4;         // config.py:6
constexpr uint32_t CAP = 20;     // config.py:8
constexpr uint32_t TRAVEL = 5;   // environment.py:202, :227
constexpr int MAX_DWELL = 10;    // config.py:11
constexpr int OBS = CGE_BUS_OBS_INTS;
constexpr int COLS = 3;
constexpr int BLOCK = 256;
constexpr int DRAW_RUN = 16;     // ready words fetched per round of the reset's draw loop (<= MT_PAD)

// plane offsets inside one observation slab, in units of n_envs ints (the order of cge_amd.h)
constexpr int P_STOPS = 0, P_STATES = 4, P_REMAINING = 8, P_CAPACITIES = 12, P_BUS_DEST = 16, P_WAITING = 32, P_STOP_DEST = 36,
              P_TIMESTEP = 52, P_DELIVERED = 53, P_TOTAL_WAITING = 54, P_TOTAL_ONBOARD = 55;

struct Params : LaneParams<int32_t> {
    int32_t max_t;
    static constexpr bool terminates = false;                       // truncated after max_t steps; terminated is never set (:156)
};
static_assert(std::is_trivially_copyable<Params>::value, "a kernel argument");
// rollout_rows_kernel's: the other kernels' arguments stay as they are.  fin.rows is the observation slab of R = n_segments * fin.cap
// "envs" (plane p at p * R ints); row j of segment s is env s * fin.cap + j of it.
struct RowsParams : Params {
    FinalSeg fin;
    int64_t R;
};

__device__ __forceinline__ uint32_t bsum(uint32_t x) { return (x & 255u) + ((x >> 8) & 255u) + ((x >> 16) & 255u) + (x >> 24); }
// a[i] for a runtime i in 0..3, mask form (a ternary over array elements becomes "select the address, then load": scratch)
__device__ __forceinline__ uint32_t sel4(const uint32_t (&a)[4], uint32_t i) {
    return (a[0] & (0u - (uint32_t)(i == 0u))) | (a[1] & (0u - (uint32_t)(i == 1u))) | (a[2] & (0u - (uint32_t)(i == 2u))) | (a[3] & (0u - (uint32_t)(i == 3u)));
}

struct Env {
    uint32_t wait[NSTOP];    // wait[s]: byte d = passengers waiting at stop s for destination d (at most 150 in all)
    uint32_t onb[NBUS];      // onb[b]: byte d = passengers on bus b for destination d (at most 20 per bus)
    uint32_t stop[NBUS], stopped[NBUS], rem[NBUS];
    uint32_t t, delivered, needs_reset, mt_pos, mt_pretw;
    int32_t ret2;            // twice the running episode's return: exact, |reward| <= 750 per step and <= 60000 steps

    __device__ __forceinline__ void load(const uint4 *__restrict__ s, int64_t n, int64_t i) {
        const uint4 a = s[i], b = s[n + i], c = s[2 * n + i];
        wait[0] = a.x; wait[1] = a.y; wait[2] = a.z; wait[3] = a.w;
        onb[0] = b.x; onb[1] = b.y; onb[2] = b.z; onb[3] = b.w;
#pragma unroll
        for (int k = 0; k < NBUS; ++k) {
            const uint32_t v = (c.x >> (7 * k)) & 127u;
            stop[k] = v & 3u; stopped[k] = (v >> 2) & 1u; rem[k] = v >> 3;
        }
        needs_reset = (c.x >> 28) & 1u;
        t = c.y & 0xFFFFFFu; delivered = c.y >> 24;
        mt_pos = c.z & 1023u; mt_pretw = mt_ready_decode((c.z >> 10) & 31u);
        ret2 = (int32_t)c.w;
    }
    __device__ __forceinline__ void store(uint4 *__restrict__ s, int64_t n, int64_t i) const {
        uint32_t bw = needs_reset << 28;
#pragma unroll
        for (int k = 0; k < NBUS; ++k) bw |= (stop[k] | (stopped[k] << 2) | (rem[k] << 3)) << (7 * k);
        s[i] = make_uint4(wait[0], wait[1], wait[2], wait[3]);
        s[n + i] = make_uint4(onb[0], onb[1], onb[2], onb[3]);
        s[2 * n + i] = make_uint4(bw, (t & 0xFFFFFFu) | (delivered << 24), mt_pos | ((mt_pretw > mt_pos ? mt_ready_encode(mt_pretw) : 0u) << 10), (uint32_t)ret2);
    }
    __device__ __forceinline__ void clear() {                       // environment.py:129-141
#pragma unroll
        for (int k = 0; k < NBUS; ++k) { wait[k] = 0; onb[k] = 0; stop[k] = (uint32_t)k % NSTOP; stopped[k] = 1; rem[k] = 0; }
        t = 0; delivered = 0; needs_reset = 0; ret2 = 0;
    }
};

// generate_passengers, utils.py:22-46, on the env's own stream, for the lanes with `go` (call with all lanes of the wave).
//   randint(50, 150) = 50 + _randbelow(101): 7 bits per try;  randint(0, 3) = _randbelow(4): (4).bit_length() = 3 bits per try,
//   values >= 4 rejected;  a destination equal to the source is drawn again.
// Every generator word drives exactly one transition of {0 count, 1 source, 2 destination, 3 done}.
__device__ __forceinline__ void env_reset(Env &e, uint32_t *__restrict__ blk, bool go) {
    if (go) e.clear();
    uint32_t phase = go ? 0u : 3u, left = 0, src = 0;
    uint32_t pos = e.mt_pos, pretw = e.mt_pretw;
#pragma unroll 1
    while (__ballot(phase != 3u)) {
        const bool act = phase != 3u;
        mt_make_ready(blk, pos, pretw, (uint32_t)DRAW_RUN, act);
        uint32_t w[DRAW_RUN];
#pragma unroll
        for (int j = 0; j < DRAW_RUN; ++j) w[j] = 0;
        if (act) mt_load_ready<DRAW_RUN>(blk, pos, w);
        uint32_t used = 0;
#pragma unroll
        for (int j = 0; j < DRAW_RUN; ++j) {
            if (phase != 3u) {
                const uint32_t y = mt_temper(w[j]);
                used += 1;
                if (phase == 0u) {
                    const uint32_t r = y >> 25;
                    if (r < 101u) { left = 50u + r; phase = 1u; }
                } else {
                    const uint32_t r = y >> 29;
                    if (r < 4u) {
                        if (phase == 1u) { src = r; phase = 2u; }
                        else if (r != src) {
                            const uint32_t inc = 1u << (8u * r);
#pragma unroll
                            for (int s = 0; s < NSTOP; ++s) e.wait[s] += src == (uint32_t)s ? inc : 0u;
                            left -= 1;
                            phase = left ? 1u : 3u;
                        }
                    }
                }
            }
        }
        if (act) mt_advance(pos, pretw, used);
    }
    e.mt_pos = pos; e.mt_pretw = pretw;
}

// step :153-186 without the action check; returns truncated, r2 = twice the reward
__device__ __forceinline__ bool env_step(Env &e, int32_t max_t, const int32_t (&a)[NBUS], int32_t &r2) {
    int32_t r = 0;
    const bool every3 = e.t % 3u == 0u;                             // current_timestep BEFORE the increment (:223)
#pragma unroll
    for (int b = 0; b < NBUS; ++b) {                                // _update_buses :188-237
        uint32_t rem = e.rem[b], st = e.stop[b], sp = e.stopped[b];
        const uint32_t load = bsum(e.onb[b]);
        if (rem > 0) {
            rem -= 1;
            if (rem == 0) {
                if (sp) { sp = 0; st = (st + 1u) & 3u; rem = TRAVEL; }
                else { sp = 1; if (a[b] > 0) rem = (uint32_t)a[b]; }   // arrived: dwell as the agent says; 0 may leave at once
            }
        }
        if (sp && rem == 0) {
            if (load >= CAP || bsum(sel4(e.wait, st)) == 0u || every3) { sp = 0; st = (st + 1u) & 3u; rem = TRAVEL; }
        }
        r -= (int32_t)load;                                         // -0.5 per onboard passenger, stopped or not (:230-235)
        e.rem[b] = rem; e.stop[b] = st; e.stopped[b] = sp;
    }
#pragma unroll
    for (int b = 0; b < NBUS; ++b) {                                // _process_passenger_movements :239-276, bus order
        if (e.stopped[b]) {
            const uint32_t c = e.stop[b];
            uint32_t ob = e.onb[b];
            const uint32_t al = (ob >> (8u * c)) & 255u;            // alighting :251-260
            r += 10 * (int32_t)al;
            e.delivered += al;
            ob &= ~(255u << (8u * c));
            uint32_t w = sel4(e.wait, c);
            uint32_t load = bsum(ob);
#pragma unroll
            for (int pr = 0; pr < 3; ++pr) {                        // boarding :263-274 in priority order: c+1, c+3, c+2
                const uint32_t d = (c + (pr == 0 ? 1u : pr == 1 ? 3u : 2u)) & 3u, sh = 8u * d;
                const uint32_t cnt = (w >> sh) & 255u, room = CAP - load;
                const uint32_t m = cnt < room ? cnt : room;
                w -= m << sh; ob += m << sh; load += m;
            }
            e.onb[b] = ob;
#pragma unroll
            for (int s = 0; s < NSTOP; ++s) e.wait[s] = c == (uint32_t)s ? w : e.wait[s];
        }
    }
    e.t += 1;
    r2 = r;
    return e.t >= (uint32_t)max_t;
}

__device__ __forceinline__ int4 bytes4(uint32_t x) { return make_int4((int)(x & 255u), (int)((x >> 8) & 255u), (int)((x >> 16) & 255u), (int)(x >> 24)); }

// _get_observation :301-337 -> env i's piece of every plane of one slab
__device__ __forceinline__ void observe(const Env &e, int32_t *__restrict__ o, int64_t n, int64_t i) {
    int4 *o4 = reinterpret_cast<int4 *>(o);                         // plane p starts at int p * n = int4 p * n / 4; P_* up to 36 are multiples of 4
    uint32_t load[NBUS], wc[NSTOP];
#pragma unroll
    for (int k = 0; k < NBUS; ++k) { load[k] = bsum(e.onb[k]); wc[k] = bsum(e.wait[k]); }
    o4[(P_STOPS / 4) * n + i] = make_int4((int)e.stop[0], (int)e.stop[1], (int)e.stop[2], (int)e.stop[3]);
    o4[(P_STATES / 4) * n + i] = make_int4((int)e.stopped[0], (int)e.stopped[1], (int)e.stopped[2], (int)e.stopped[3]);
    o4[(P_REMAINING / 4) * n + i] = make_int4((int)e.rem[0], (int)e.rem[1], (int)e.rem[2], (int)e.rem[3]);
    o4[(P_CAPACITIES / 4) * n + i] = make_int4((int)(CAP - load[0]), (int)(CAP - load[1]), (int)(CAP - load[2]), (int)(CAP - load[3]));
#pragma unroll
    for (int k = 0; k < NBUS; ++k) o4[(P_BUS_DEST / 4) * n + 4 * i + k] = bytes4(e.onb[k]);
    o4[(P_WAITING / 4) * n + i] = make_int4((int)wc[0], (int)wc[1], (int)wc[2], (int)wc[3]);
#pragma unroll
    for (int k = 0; k < NSTOP; ++k) o4[(P_STOP_DEST / 4) * n + 4 * i + k] = bytes4(e.wait[k]);
    o[(int64_t)P_TIMESTEP * n + i] = (int32_t)e.t;
    o[(int64_t)P_DELIVERED * n + i] = (int32_t)e.delivered;
    o[(int64_t)P_TOTAL_WAITING * n + i] = (int32_t)(wc[0] + wc[1] + wc[2] + wc[3]);
    o[(int64_t)P_TOTAL_ONBOARD * n + i] = (int32_t)(load[0] + load[1] + load[2] + load[3]);
}

// k steps with the record in registers.  ROLLOUT: per-step outputs indexed [t, env], sums; GIVEN: the caller's actions, else the
// counter hash cge_hash_action(action_seed, env_index0 + i, t0 + t, 11, bus).  With RowsParams (ROWS, a SAME_STEP rollout) a
// truncated env's terminal observation goes to the wave's segment of p.fin, each lane storing its own pieces.
template <int MODE, bool ROLLOUT, bool GIVEN, class P = Params>
__device__ __forceinline__ void run(const P &p) {
    constexpr bool ROWS = std::is_same<P, RowsParams>::value;
    static_assert(!ROWS || (ROLLOUT && MODE == CGE_AUTORESET_SAME_STEP), "terminal rows: fused SAME_STEP rollouts");
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool live = i < p.n;
    const int64_t li = live ? i : p.n - 1;
    Env e;
    e.load(p.state, p.n, li);
    uint32_t *blk = p.mt + li * MT_STRIDE;
    const uint64_t key = GIVEN ? 0 : hash_env_key(p.a_seed, (uint64_t)(p.env0 + li));
    double rsum = 0.0;
    int32_t dcount = 0;
    uint32_t fin_used = 0;                                          // ROWS: terminal rows the wave's segment has been handed
    // the segment is the wave, not the workgroup: wave-uniform, so a scalar
    const int64_t seg = ROWS ? (int64_t)blockIdx.x * (BLOCK / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : 0;
    const int ksteps = ROLLOUT ? p.k_steps : 1;
#pragma unroll 1
    for (int t = 0; t < ksteps; ++t) {
        int32_t r2 = 0;
        bool trunc = false, reset_now = false;
        if (live) {
            if (MODE == CGE_AUTORESET_NEXT_STEP && e.needs_reset) {
                reset_now = true;
            } else {
                int32_t a[NBUS];
                if (GIVEN) {
                    const int4 v = reinterpret_cast<const int4 *>(p.actions)[(int64_t)t * p.n + i];
                    a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w;
                } else {
#pragma unroll
                    for (int b = 0; b < NBUS; ++b) a[b] = (int32_t)hash_action_from_key(key, (uint64_t)(p.t0 + t), (uint32_t)(MAX_DWELL + 1), (uint32_t)b);
                }
                bool valid = true;
#pragma unroll
                for (int b = 0; b < NBUS; ++b) valid = valid && a[b] >= 0 && a[b] <= MAX_DWELL;
                if (!valid) {
                    atomicAdd(p.err_count, 1ull);                   // reference: ValueError (:160-161); the env is left as it was
                } else {
                    trunc = env_step(e, p.max_t, a, r2);
                    e.ret2 += r2;
                    if (trunc) lane_episode_end<MODE>(p, i, 0.5 * (double)e.ret2, (int32_t)e.t, reset_now, e.needs_reset);
                }
            }
        }
        if (MODE == CGE_AUTORESET_SAME_STEP && !ROLLOUT) {
            if (p.final_obs && trunc && reset_now) observe(e, p.final_obs, p.n, i);   // the terminal rows; the others are not written
        }
        if constexpr (ROWS) {                                       // ... of a rollout, compacted: row `rank` after the segment's `first` used ones
            const int64_t first = seg * p.fin.cap + (int64_t)fin_used;
            int32_t *dst;
            int keep, rank;
            if (lane_final_rows(p.fin, seg, fin_used, trunc, t, i, 0, dst, keep, rank)) {
                if (trunc && rank < keep) observe(e, static_cast<int32_t *>(p.fin.rows), p.R, first + rank);
            }
        }
        if (MODE != CGE_AUTORESET_DISABLED) {
            if (__ballot(reset_now)) env_reset(e, blk, reset_now);
        }
        if (live) {
            if (lane_obs_due<ROLLOUT>(p, t, ksteps)) observe(e, p.obs + (int64_t)t * p.obs_step_stride, p.n, i);
            const float reward = 0.5f * (float)r2;                  // multiples of 0.5 below 2^24: exact
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
        e.store(p.state, p.n, i);
        if (ROLLOUT) lane_sums(p, i, rsum, dcount);
    }
    if constexpr (ROWS) {
        if ((threadIdx.x & 63u) == 0 && live) p.fin.count[seg] = (int32_t)fin_used;   // a wave past the last env has no segment
    }
}

template <int MODE>
__global__ __launch_bounds__(BLOCK) void step_kernel(Params p) { run<MODE, false, true>(p); }

template <int MODE, bool ACTIONS>
__global__ __launch_bounds__(BLOCK) void rollout_kernel(Params p) { run<MODE, true, ACTIONS>(p); }

// the SAME_STEP rollout while terminal rows are registered (cge_rows_bus_rollout_final_obs)
template <bool ACTIONS>
__global__ __launch_bounds__(BLOCK) void rollout_rows_kernel(RowsParams p) { run<CGE_AUTORESET_SAME_STEP, true, ACTIONS>(p); }

// reset (mask) / initial state (init: cleared buses, no passengers, cursor rewound) / rewind (after a re-seed) + obs
__global__ __launch_bounds__(BLOCK) void reset_kernel(Params p, int init, int rewind) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    const bool live = i < p.n;
    const int64_t li = live ? i : p.n - 1;
    Env e;
    e.load(p.state, p.n, li);
    bool dirty = false;
    if (init) { e.clear(); e.mt_pos = 0; e.mt_pretw = 0; dirty = true; }
    else if (rewind) { e.mt_pos = 0; e.mt_pretw = 0; dirty = true; }
    else {
        const bool go = live && (!p.mask || p.mask[i]);
        if (__ballot(go)) env_reset(e, p.mt + li * MT_STRIDE, go);
        dirty = go;
    }
    if (live) {
        if (dirty) e.store(p.state, p.n, i);
        if (p.obs) observe(e, p.obs, p.n, i);
    }
}

__global__ __launch_bounds__(256) void info_kernel(const uint4 *__restrict__ state, int64_t n, int field, int idx, int32_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    Env e;
    e.load(state, n, i);
    const uint32_t k = (uint32_t)idx;
    int32_t v = 0;
    switch (field) {
        case CGE_BUS_INFO_TIMESTEP: v = (int32_t)e.t; break;
        case CGE_BUS_INFO_TOTAL_DELIVERED: v = (int32_t)e.delivered; break;
        case CGE_BUS_INFO_TOTAL_WAITING: v = (int32_t)(bsum(e.wait[0]) + bsum(e.wait[1]) + bsum(e.wait[2]) + bsum(e.wait[3])); break;
        case CGE_BUS_INFO_TOTAL_ONBOARD: v = (int32_t)(bsum(e.onb[0]) + bsum(e.onb[1]) + bsum(e.onb[2]) + bsum(e.onb[3])); break;
        case CGE_BUS_INFO_BUS_POSITION: v = (int32_t)sel4(e.stop, k); break;
        case CGE_BUS_INFO_BUS_STOPPED: v = (int32_t)sel4(e.stopped, k); break;
        case CGE_BUS_INFO_BUS_CAPACITY: v = (int32_t)(CAP - bsum(sel4(e.onb, k))); break;
        case CGE_BUS_INFO_STOP_WAITING: v = (int32_t)bsum(sel4(e.wait, k)); break;
        case CGE_BUS_INFO_NEEDS_RESET: v = (int32_t)e.needs_reset; break;
    }
    out[i] = v;
}

}  // namespace bus
}  // namespace cge

using namespace cge;

struct cge_bus : LaneHandle {
    using Params = bus::Params;
    using RowsParams = bus::RowsParams;
    cge_bus_config cfg{};
    static constexpr uint32_t snap_tag = 6u;
    static constexpr const char *abi = "cge_bus", *kernel_ns = "cge::bus::", *rows_ns = kernel_ns;
    static constexpr int block = bus::BLOCK, seed_kind = 0;
    Params params() const {
        Params p{};
        fill(p);
        p.max_t = cfg.max_timesteps;
        return p;
    }
    int64_t step_elems() const { return n * bus::OBS; }
    auto reset_kernel() const { return bus::reset_kernel; }
    template <int MODE>
    auto kernel(LaneKind kind) const {
        return kind == LANE_STEP ? bus::step_kernel<MODE> : kind == LANE_ROLLOUT_GIVEN ? bus::rollout_kernel<MODE, true> : bus::rollout_kernel<MODE, false>;
    }
    void fill_rows(RowsParams &p) const { p.R = (int64_t)lane_segments(this) * fin_cap; }
    // a finishing lane stores 16-byte pieces of every plane of the rows slab
    const char *rows_refusal() const {
        return (reinterpret_cast<uintptr_t>(fin_rows) & 15u) != 0 ? "the registered terminal rows are not 16-byte aligned" : nullptr;
    }
    void launch_rows(bool given, unsigned blocks, hipStream_t s, const RowsParams &p) const {
        hipLaunchKernelGGL(given ? bus::rollout_rows_kernel<true> : bus::rollout_rows_kernel<false>, dim3(blocks), dim3(block), 0, s, p);
    }
    static int check(const cge_bus_config &c) {
        return bad_autoreset_mode(c.autoreset_mode) || c.max_timesteps < 0 || c.max_timesteps > 60000 ? CGE_ERR_INVALID_ARG : CGE_OK;
    }
    hipError_t init() {
        if (cfg.max_timesteps == 0) cfg.max_timesteps = 500;      // config.py:10
        CGE_HIP(alloc(state, (size_t)bus::COLS * n * sizeof(uint4), true, true));
        CGE_HIP(alloc(mt, (size_t)n * MT_STRIDE * sizeof(uint32_t), false, true));
        CGE_HIP(alloc(err, sizeof(unsigned long long), true, false));
        CGE_HIP(launch_mt_seed(mt, MT_STRIDE, n, nullptr, 0, env0, 0, nullptr));
        lane_launch_reset(this, params(), 1, 0, nullptr);
        return hipGetLastError();
    }
};

extern "C" {

CGE_DEFINE_LIFECYCLE(bus)

int cge_bus_seed(cge_bus *h, const uint64_t *seeds, uint64_t base_seed, void *stream) { return lane_seed(h, seeds, base_seed, stream); }

int cge_bus_reset(cge_bus *h, const uint8_t *mask, int32_t *obs_out, void *stream) { return lane_reset(h, mask, obs_out, stream); }

int cge_bus_step(cge_bus *h, const int32_t *actions, int32_t *obs_out, float *reward_out, uint8_t *terminated_out, uint8_t *truncated_out,
                 int32_t *final_obs_out, void *stream) {
    return lane_step(h, actions && obs_out && reward_out && terminated_out && truncated_out,
                     "cge_bus_step: null actions/obs/reward/terminated/truncated pointer", actions, obs_out, reward_out, terminated_out, truncated_out,
                     final_obs_out, stream);
}

int cge_bus_rollout(cge_bus *h, int32_t k_steps, const int32_t *actions, uint64_t action_seed, int64_t t0, int32_t *obs_out,
                    int64_t obs_step_stride, float *reward_traj_out, uint8_t *truncated_traj_out, double *reward_sum_out,
                    int32_t *done_count_out, void *stream) {
    // observations are stored as 16-byte pieces: a trajectory step starts at a multiple of four ints
    return lane_rollout(h, obs_step_stride % 4 == 0, "cge_bus_rollout: bad k_steps / obs_step_stride", k_steps, actions, action_seed, t0, obs_out,
                        obs_step_stride, reward_traj_out, truncated_traj_out, reward_sum_out, done_count_out, stream);
}

int cge_bus_info(cge_bus *h, int32_t field_id, int32_t index, int32_t *out, void *stream) {
    if (!h) return CGE_ERR_INVALID_ARG;
    if (!out || field_id < 0 || field_id > CGE_BUS_INFO_NEEDS_RESET || index < 0 || index > 3)
        return h->fail(CGE_ERR_INVALID_ARG, "cge_bus_info: bad field / index / null out");
    DeviceGuard g(h->device);
    hipLaunchKernelGGL(bus::info_kernel, dim3(grid256(h->n)), dim3(256), 0, as_stream(stream), h->state, h->n, field_id, index, out);
    return launched(h);
}

CGE_DEFINE_ROWS_FINAL_OBS(bus, int32_t, 64)
CGE_DEFINE_ERROR_COUNT(bus)
CGE_DEFINE_SNAPSHOT(bus)

}  // extern "C"
