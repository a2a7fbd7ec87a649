// cge_lane.hpp — what the lane-per-env types (bus, world builder, restaurant, airline, emergency, space station, farm) share that is not dynamics.
//
// Such a type steps one env per lane with the record in registers for the whole launch, and has step_kernel<MODE...>,
// rollout_kernel<MODE..., ACTIONS> and reset_kernel(p, init, rewind), an error counter and a key-major observation slab.  Here are
// the fields its Params shares, the parts of its step loop that read the same in every type, and the host side of its
// seed / reset / step / rollout entry points.  The step loops themselves stay with their types: they differ in where the wave
// acts together (bus resets by drawing under a ballot, world builder's env_step is called by every lane with a `go` flag,
// restaurant prefetches actions and keeps a run of generator words in registers), and a shared loop would branch on its caller.
// Airline, emergency, space station and farm (the record-lane types: hundreds of columns a record) share LaneCols, lane_col_offset,
// LaneRng and the host helpers below, and keep their loops too.  Emergency's, station's and farm's read alike, and one loop over a
// per-type Lane struct owning Cols, Env and Rng was tried: station's kernels kept registers and instruction counts, farm's did not
// in any of three forms (members in either order, or references to run()'s locals), by spills and some tens of instructions of
// 28,000 — nothing that was measured, so nothing that was merged (profiles/record_lane_refactor_resources.txt).  Airline differs in
// its text as well: fresh() at the top of every step, a `prices` flag into store_env, no ready-ahead and no rows instance.
//
// A new lane-per-env type supplies
//   device  struct Params : LaneParams<Obs> with its own fields and `static constexpr bool terminates` (the flag it raises:
//           terminated, or truncated), its run() loop calling the lane_* helpers below, and the three __global__ kernels; a type
//           whose record is columns of 32-bit words takes LaneCols, lane_col_offset<BLOCK> and LaneRng (`using Cols = LaneCols;`)
//           and writes load_env / store_env over them;
//   host    a handle derived from LaneHandle with Params, abi, kernel_ns, block, seed_kind, params(), step_elems(), reset_kernel(),
//           kernel<MODE>(kind) (CGE_LANE_KERNELS(ns) where the kernels have no layout argument), and whichever of layout_arg() /
//           actions_refusal() differ from the defaults; for the terminal rows of fused rollouts (all but airline) RowsParams, rows_ns
//           and launch_rows() (CGE_LANE_LAUNCH_ROWS(ns)) as well, and fill_rows() where RowsParams holds more than `fin` (the Dict
//           types' slab of compacted rows), see LaneHandle; init() is lane_init(this, REC_WORDS) where the arrays are state, mt, err
//           and no test reads the allocation from the source;
//   C ABI   entry points that are one lane_seed / lane_reset / lane_step / lane_rollout (/ lane_info) call each, with the type's own
//           pointer and stride predicates (rows_aligned) and error texts as arguments.
// Parking's seed / reset have the same shape and use lane_seed / lane_reset (and lane_blocks for its grid); the rest of parking is its own.
#pragma once
#include <string>
#include <type_traits>

#include "cge_device.hpp"
#include "cge_host.hpp"

namespace cge {

// The kernel arguments every lane-per-env type has (passed by value: a type's Params must stay trivially copyable).
template <class Obs>
struct LaneParams {
    uint4 *state;                  // the record's SoA columns; first, with mt / n / env0 behind it, as every type's kernels load them
    uint32_t *mt;
    int64_t n, env0;
    const int32_t *actions;
    const uint8_t *mask;
    Obs *obs, *final_obs;
    float *reward;
    uint8_t *terminated, *truncated;
    int32_t k_steps;
    uint64_t a_seed;
    int64_t t0, obs_step_stride;   // stride in elements of the observation layout
    double *reward_sum;
    int32_t *done_count;
    double *ep_ret;                // episode statistics (cge_<env>_episode_stats), nullable
    int32_t *ep_len;
    unsigned long long *err_count;
};

// ---------------------------------------------------------------------------------------------------------------- device
// Env i's episode has just ended with return `ret` after `len` steps: the registered statistics, then what the autoreset mode asks.
template <int MODE, class P, class F>
__device__ __forceinline__ void lane_episode_end(const P &p, int64_t i, double ret, int32_t len, bool &reset_now, F &needs_reset) {
    if (p.ep_ret) p.ep_ret[i] = ret;
    if (p.ep_len) p.ep_len[i] = len;
    if (MODE == CGE_AUTORESET_SAME_STEP) reset_now = true;
    else if (MODE == CGE_AUTORESET_NEXT_STEP) needs_reset = 1;
}

// Is an observation due at step t?  Always for step(); a rollout without a trajectory (stride 0) writes its last step only.
template <bool ROLLOUT, class P>
__device__ __forceinline__ bool lane_obs_due(const P &p, int t, int ksteps) {
    return p.obs && (!ROLLOUT || p.obs_step_stride != 0 || t == ksteps - 1);
}

// step()'s outputs of env i; `done` is the flag the type raises (P::terminates), the one the reference never sets is written 0 (for a
// type that only terminates `truncated` is nullable).  A rollout's per-step outputs — the sums and the nullable trajectories — are
// four lines in each run() loop and stay there: written as a function, in any of the forms tried (accumulators by reference or at the
// call site, the [t, env] index computed inside or passed in), they cost bus's fused rollout 3-4 % at 131,072 envs with the same
// registers (profiles/lane_refactor_ab.txt).
template <class P>
__device__ __forceinline__ void lane_step_outputs(const P &p, int64_t i, float reward, bool done) {
    p.reward[i] = reward;
    if (P::terminates) {
        p.terminated[i] = done ? 1 : 0;
        if (p.truncated) p.truncated[i] = 0;
    } else {
        p.terminated[i] = 0;
        p.truncated[i] = done ? 1 : 0;
    }
}

// a rollout's per-env sums, after the last step
template <class P>
__device__ __forceinline__ void lane_sums(const P &p, int64_t i, double rsum, int32_t dcount) {
    if (p.reward_sum) p.reward_sum[i] = rsum;
    if (p.done_count) p.done_count[i] = dcount;
}

// One step's terminal rows in a rows rollout (rollout_rows_kernel<ACTIONS>: SAME_STEP, launched only while rows are registered; every
// lane-per-env type but airline).  The segment `seg` is the wave's 64 envs and `used` its fill count, wave-uniform and in a
// register for the whole launch; it counts past the capacity, and the wave's first lane writes it to count[seg] after the step loop.  The lanes
// with `fin` take the segment's next rows in lane order and record (t, env) for them (final_slot).  Returns whether a row is to be
// stored — the same for every lane, so the caller's store pass may have barriers: `dst` is then the segment's first free row, `keep`
// how many of this step's rows fit and `rank` this lane's place among the finishing ones; its row is kept if fin && rank < keep.  A
// type with a tile parks the kept lanes' groups in columns 0..keep-1 and writes `keep` dense rows at `dst` (lane_store_tile); a type
// whose lanes store their own rows has the kept lanes store row `rank` of `dst`.  The types whose rows are a slab (bus, restaurant, world
// builder) pass row_elems 0 and take the row's number, seg * f.cap + used (before the call) + rank, to the planes of the slab themselves.
template <class T>
__device__ __forceinline__ bool lane_final_rows(const FinalSeg &f, int64_t seg, uint32_t &used, bool fin, int64_t t, int64_t i, int64_t row_elems, T *&dst,
                                                int &keep, int &rank) {
    const unsigned long long m = __ballot(fin);
    if (!m) return false;
    (void)final_slot(f, seg, used, fin, t, i);
    const int64_t room = f.cap - (int64_t)used;
    const int ends = __popcll(m);
    keep = room <= 0 ? 0 : room < ends ? (int)room : ends;
    rank = __popcll(m & ((1ull << (threadIdx.x & 63u)) - 1ull));
    dst = static_cast<T *>(f.rows) + (seg * f.cap + (int64_t)used) * row_elems;
    used += (uint32_t)ends;
    return keep > 0;
}
// ... in a workgroup of one wave: the segment is the workgroup
template <class T>
__device__ __forceinline__ bool lane_final_rows(const FinalSeg &f, uint32_t &used, bool fin, int64_t t, int64_t i, int64_t row_elems, T *&dst, int &keep,
                                                int &rank) {
    return lane_final_rows(f, (int64_t)blockIdx.x, used, fin, t, i, row_elems, dst, keep, rank);
}
// The store pass of a tile parked [element][column] with STRIDE floats a row: floats [FIRST, FIRST + COUNT) of the dense rows
// 0..nrows-1 at `rows` (`row` floats each) from columns 0..nrows-1, as pieces of PIECE floats with consecutive lanes on consecutive
// pieces of a row.  Call with every lane of a one-wave workgroup, between the barriers that hand the tile over.
template <int FIRST, int COUNT, int PIECE, int STRIDE>
__device__ __forceinline__ void lane_store_tile(const float *__restrict__ stg, float *__restrict__ rows, int row, int nrows) {
    static_assert((PIECE == 4 || PIECE == 2) && FIRST % PIECE == 0 && COUNT % PIECE == 0, "whole pieces");
    constexpr int PER = COUNT / PIECE;
    const int pieces = nrows * PER;
    for (int q = (int)threadIdx.x; q < pieces; q += 64) {
        const int r = q / PER, pc = q - r * PER;
        const float *s = stg + (PIECE * pc) * STRIDE + r;
        float *dst = rows + (int64_t)r * row + FIRST + PIECE * pc;
        if (PIECE == 4) *reinterpret_cast<float4 *>(dst) = make_float4(s[0], s[STRIDE], s[2 * STRIDE], s[3 * STRIDE]);
        else *reinterpret_cast<float2 *>(dst) = make_float2(s[0], s[STRIDE]);
    }
}

// ------------------------------------------------------------------------------------------- device: the record-lane kit
// Airline, emergency, space station and farm keep a record of hundreds of 32-bit columns, word w of env i at rec[w * n + i], in
// registers (and LDS) from the start of a launch to its end.  A scalar base plus ONE 32-bit byte offset per lane (4 * i: n_envs < 2^30)
// addresses every column; 64-bit per-lane addresses, one pair of registers per column and kept from the loads of a launch to its
// stores, took every register there is and spilled.  After fresh() the offset is a new value to the compiler: the addresses are
// formed again where they are used (one add each).
struct LaneCols {
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
// LaneCols::off: 4 * (the env of this lane, or the last env for a lane past the end), in 32-bit arithmetic throughout
template <int BLOCK>
__device__ __forceinline__ uint32_t lane_col_offset(int64_t n) {
    const uint32_t i = blockIdx.x * (uint32_t)BLOCK + threadIdx.x, last = (uint32_t)n - 1u;
    return (i < last ? i : last) * 4u;
}
// the generator as the dynamics headers draw from it: single words, and runs of W words the caller consumes in order
struct LaneRng {
    MtStream s;
    __device__ __forceinline__ LaneRng(uint32_t *block, uint32_t pos, uint32_t ready) : s(block, pos, ready) {}
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

// ------------------------------------------------------------------------------------------------------------------ host
enum LaneKind { LANE_STEP, LANE_ROLLOUT_GIVEN, LANE_ROLLOUT_HASHED };   // the kernel of a launch: step(), rollout() with / without actions

// f(std::integral_constant<int, mode>): the one place an autoreset mode becomes the MODE template argument
template <class F>
void for_mode(int mode, F &&f) {
    if (mode == CGE_AUTORESET_NEXT_STEP) f(std::integral_constant<int, CGE_AUTORESET_NEXT_STEP>{});
    else if (mode == CGE_AUTORESET_SAME_STEP) f(std::integral_constant<int, CGE_AUTORESET_SAME_STEP>{});
    else f(std::integral_constant<int, CGE_AUTORESET_DISABLED>{});
}

struct LaneHandle : HandleBase {
    uint4 *state = nullptr;
    uint32_t *mt = nullptr;
    unsigned long long *err = nullptr;
    // the shared fields a handle knows; the per-call ones are filled in by the drivers below
    template <class P>
    void fill(P &p) const { p.state = state; p.mt = mt; p.n = n; p.env0 = env0; p.err_count = err; p.ep_ret = ep_ret; p.ep_len = ep_len; }
    // A type with terminal rows adds RowsParams (its Params and `FinalSeg fin`), launch_rows(given, blocks, stream, params) and this,
    // the namespace of its rollout_rows_kernel
    static constexpr const char *rows_ns = nullptr;
    template <class RP>
    void fill_rows(RP &) const {}                                                   // what RowsParams holds beside Params and `fin`
    const char *rows_refusal() const { return nullptr; }                            // why the store pass cannot take the registered rows, or nullptr
    const char *layout_arg() const { return ""; }                                   // template arguments between MODE and ACTIONS, as text
    static const char *actions_refusal(const int32_t *) { return nullptr; }         // why the type cannot read these actions, or nullptr
};

template <class H>
unsigned lane_blocks(const H *h) { return (unsigned)((h->n + H::block - 1) / H::block); }
// segments of the terminal-row output: one per wave of 64 envs, whatever H::block is
template <class H>
unsigned lane_segments(const H *h) { return (unsigned)((h->n + 63) / 64); }

template <class H, class P>
void lane_launch_reset(const H *h, const P &p, int init, int rewind, hipStream_t s) {
    hipLaunchKernelGGL(h->reset_kernel(), dim3(lane_blocks(h)), dim3(H::block), 0, s, p, init, rewind);
}

// The init() of a handle whose device arrays are the record's columns, one generator block per env and the error counter: allocate,
// seed the streams as a fresh handle has them, construct the envs.  Airline and emergency; station and farm spell theirs out, as
// tests/test_farm_cpu.py reads from their sources that the record is the first array of a snapshot.
template <class H>
hipError_t lane_init(H *h, int rec_words) {
    CGE_HIP(h->alloc(h->state, (size_t)rec_words * h->n * sizeof(uint32_t), true, true));
    CGE_HIP(h->alloc(h->mt, (size_t)h->n * MT_STRIDE * sizeof(uint32_t), false, true));
    CGE_HIP(h->alloc(h->err, sizeof(unsigned long long), true, false));
    CGE_HIP(launch_mt_seed(h->mt, MT_STRIDE, h->n, nullptr, 0, h->env0, H::seed_kind, nullptr));
    lane_launch_reset(h, h->params(), 1, 0, nullptr);
    return hipGetLastError();
}

// a handle's reset_kernel() and kernel<MODE>(kind) where namespace NS has reset_kernel, step_kernel<MODE> and rollout_kernel<MODE, GIVEN>
#define CGE_LANE_KERNELS(NS)                                                                                              \
    auto reset_kernel() const { return NS::reset_kernel; }                                                                \
    template <int MODE>                                                                                                   \
    auto kernel(cge::LaneKind kind) const {                                                                               \
        return kind == cge::LANE_STEP ? NS::step_kernel<MODE>                                                             \
               : kind == cge::LANE_ROLLOUT_GIVEN ? NS::rollout_kernel<MODE, true> : NS::rollout_kernel<MODE, false>;      \
    }
// ... and its launch_rows() where NS has rollout_rows_kernel<GIVEN>
#define CGE_LANE_LAUNCH_ROWS(NS)                                                                                          \
    void launch_rows(bool given, unsigned blocks, hipStream_t s, const RowsParams &p) const {                             \
        hipLaunchKernelGGL(given ? NS::rollout_rows_kernel<true> : NS::rollout_rows_kernel<false>, dim3(blocks), dim3(block), 0, s, p); \
    }

// are observation rows that leave as 16-byte (mask 15) or 8-byte (7) pieces aligned at both addresses?  A null one is.
inline bool rows_aligned(const void *a, const void *b, uintptr_t mask = 15u) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & mask) == 0;
}

// cge_<env>_info where an info_kernel(Params, field, out) computes the field from the whole record.  `ok` / `what`: the field and
// pointer check and its error text.
template <class H, class K>
int lane_info(H *h, bool ok, const char *what, K info_kernel, int32_t field_id, double *out, void *stream) {
    if (!h) return CGE_ERR_INVALID_ARG;
    if (!ok) return h->fail(CGE_ERR_INVALID_ARG, what);
    DeviceGuard g(h->device);
    hipLaunchKernelGGL(info_kernel, dim3(lane_blocks(h)), dim3(H::block), 0, as_stream(stream), h->params(), (int)field_id, out);
    return launched(h);
}

template <class H>
void lane_launch(H *h, LaneKind kind, const typename H::Params &p, const char *which, const char *tail, hipStream_t s) {
    for_mode(h->cfg.autoreset_mode, [&](auto mode) {
        hipLaunchKernelGGL(h->template kernel<decltype(mode)::value>(kind), dim3(lane_blocks(h)), dim3(H::block), 0, s, p);
    });
    h->last_kernel = std::string(H::kernel_ns) + which + "<" + std::to_string(h->cfg.autoreset_mode) + h->layout_arg() + tail + ">";
}

template <class H>
int lane_refuse_actions(H *h, const char *fn, const char *why) {
    return h->fail(CGE_ERR_INVALID_ARG, (std::string(H::abi) + "_" + fn + ": " + why).c_str());
}

// cge_<env>_seed: re-seed the streams (H::seed_kind: 0 CPython, 1 NumPy legacy), then rewind the cursors
template <class H>
int lane_seed(H *h, const uint64_t *seeds, uint64_t base_seed, void *stream) {
    if (!h) return CGE_ERR_INVALID_ARG;
    if (int st = seed_base_check(h, (std::string(H::abi) + "_seed").c_str(), seeds, base_seed, H::seed_kind == 1)) return st;
    DeviceGuard g(h->device);
    CGE_TRY(h, launch_mt_seed(h->mt, MT_STRIDE, h->n, seeds, base_seed, h->env0, H::seed_kind, as_stream(stream)));
    lane_launch_reset(h, h->params(), 0, 1, as_stream(stream));
    return launched(h);
}

// cge_<env>_reset
template <class H, class O>
int lane_reset(H *h, const uint8_t *mask, O *obs, void *stream) {
    if (!h) return CGE_ERR_INVALID_ARG;
    DeviceGuard g(h->device);
    auto p = h->params();
    p.mask = mask; p.obs = obs;
    lane_launch_reset(h, p, 0, 0, as_stream(stream));
    return launched(h);
}

// cge_<env>_step.  `have` / `what`: as step_params (cge_host.hpp).
template <class H, class O>
int lane_step(H *h, bool have, const char *what, const int32_t *actions, O *obs, float *reward, uint8_t *terminated, uint8_t *truncated,
              O *final_obs, void *stream) {
    typename H::Params p;
    if (int st = step_params(h, p, have, what, obs, reward, terminated, truncated, final_obs)) return st;
    if (const char *why = H::actions_refusal(actions)) return lane_refuse_actions(h, "step", why);
    DeviceGuard g(h->device);
    p.actions = actions;
    lane_launch(h, LANE_STEP, p, "step_kernel", "", as_stream(stream));
    return launched(h);
}

// cge_<env>_rollout.  `env_ok` / `what`: as rollout_params_nofin (cge_host.hpp); `flags`: the per-step trajectory of the flag the
// type raises.  k_steps == 0 launches nothing.  With terminal rows registered (cge_rows_<env>_rollout_final_obs, a type with rows_ns) a
// SAME_STEP rollout runs rollout_rows_kernel; in the other modes no episode ends with a reset inside the step, so the usual instance
// runs and the segments' counts are cleared on the call's stream.
template <class H, class O>
int lane_rollout(H *h, bool env_ok, const char *what, int32_t k_steps, const int32_t *actions, uint64_t action_seed, int64_t t0, O *obs,
                 int64_t obs_step_stride, float *reward, uint8_t *flags, double *reward_sum, int32_t *done_count, void *stream) {
    if (!h) return CGE_ERR_INVALID_ARG;
    typename H::Params p;
    const int st = rollout_params_nofin(h, p, env_ok, h->step_elems(), what, k_steps, action_seed, t0, obs, obs_step_stride, reward, reward_sum,
                                        done_count);
    if (st != CGE_OK || k_steps == 0) return st;
    if (const char *why = H::actions_refusal(actions)) return lane_refuse_actions(h, "rollout", why);
    DeviceGuard g(h->device);
    p.actions = actions;
    (H::Params::terminates ? p.terminated : p.truncated) = flags;
    if constexpr (H::rows_ns != nullptr) {
        if (const char *why = h->fin_rows ? h->rows_refusal() : nullptr) return lane_refuse_actions(h, "rollout", why);
        if (h->fin_rows && h->cfg.autoreset_mode == CGE_AUTORESET_SAME_STEP) {
            typename H::RowsParams rp;
            static_cast<typename H::Params &>(rp) = p;
            rp.fin = FinalSeg{h->fin_rows, h->fin_index, h->fin_count, h->fin_cap, h->n};
            h->fill_rows(rp);
            h->launch_rows(actions != nullptr, lane_blocks(h), as_stream(stream), rp);
            std::string layout = h->layout_arg();                                   // ", true" -> "true, ": the arguments before ACTIONS
            if (!layout.empty()) layout = layout.substr(2) + ", ";
            h->last_kernel = std::string(H::rows_ns) + "rollout_rows_kernel<" + layout + (actions ? "true>" : "false>");
            return launched(h);
        }
        if (h->fin_rows) CGE_TRY(h, hipMemsetAsync(h->fin_count, 0, lane_segments(h) * sizeof(int32_t), as_stream(stream)));
    }
    lane_launch(h, actions ? LANE_ROLLOUT_GIVEN : LANE_ROLLOUT_HASHED, p, "rollout_kernel", actions ? ", true" : ", false", as_stream(stream));
    return launched(h);
}

// ----------------------------------------------------------------------------------- host: canonical records (lane_records.hip)
// cge_records_<env>_* of the four record-lane types: per-env records packed and unpacked on the device (include/cge_amd.h has the
// layout, lane_records.hip the kernels and the drivers).  A handle shows the drivers what they need of it as a LaneRecords: its
// type's number, the columns, and the generator blocks of its streams in the record's order.  The staging buffer of the host forms
// and the status block of a check are transient, allocated and freed inside the call: device_bytes and the snapshot do not move.
enum { LANE_RECORDS_AIRLINE = 1, LANE_RECORDS_EMERGENCY = 2, LANE_RECORDS_STATION = 3, LANE_RECORDS_FARM = 4 };
struct LaneRecords {
    HandleBase *h;
    const char *abi;               // "cge_records_<env>", the prefix of the error texts
    int type;
    uint32_t *state, *mt[2];
};
size_t lane_records_bytes(int type);
int lane_records_pack(const LaneRecords &v, int64_t first, int64_t count, void *dev_records, hipStream_t s);
int lane_records_unpack(const LaneRecords &v, int64_t first, int64_t count, const void *dev_records, hipStream_t s);
int lane_records_get(const LaneRecords &v, void *host_buf, hipStream_t s);
int lane_records_set(const LaneRecords &v, const void *host_buf, hipStream_t s);

// the five entry points (inside extern "C"); SECOND: the handle's second stream (farm's `py`), or nullptr
#define CGE_DEFINE_LANE_RECORDS(ENV, TYPE, SECOND)                                                                                          \
    static cge::LaneRecords records_of(cge_##ENV *h) {                                                                                      \
        return cge::LaneRecords{h, "cge_records_" #ENV, TYPE, reinterpret_cast<uint32_t *>(h->state), {h->mt, SECOND}};                     \
    }                                                                                                                                       \
    size_t cge_records_##ENV##_state_bytes(const cge_##ENV *h) { return h ? cge::lane_records_bytes(TYPE) : 0; }                            \
    int cge_records_##ENV##_get_state(cge_##ENV *h, void *host_buf, void *stream) {                                                         \
        return h ? cge::lane_records_get(records_of(h), host_buf, cge::as_stream(stream)) : CGE_ERR_INVALID_ARG;                            \
    }                                                                                                                                       \
    int cge_records_##ENV##_set_state(cge_##ENV *h, const void *host_buf, void *stream) {                                                   \
        return h ? cge::lane_records_set(records_of(h), host_buf, cge::as_stream(stream)) : CGE_ERR_INVALID_ARG;                            \
    }                                                                                                                                       \
    int cge_records_##ENV##_pack(cge_##ENV *h, int64_t first, int64_t count, void *dev_records, void *stream) {                             \
        return h ? cge::lane_records_pack(records_of(h), first, count, dev_records, cge::as_stream(stream)) : CGE_ERR_INVALID_ARG;          \
    }                                                                                                                                       \
    int cge_records_##ENV##_unpack(cge_##ENV *h, int64_t first, int64_t count, const void *dev_records, void *stream) {                     \
        return h ? cge::lane_records_unpack(records_of(h), first, count, dev_records, cge::as_stream(stream)) : CGE_ERR_INVALID_ARG;        \
    }

}  // namespace cge
