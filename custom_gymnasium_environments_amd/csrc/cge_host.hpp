// cge_host.hpp — host-side plumbing shared by the per-env C-ABI translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdio>
#include <string>
#include <utility>
#include <vector>
#include <cstring>

#include "../../include/cge_amd.h"

namespace cge {

struct HandleBase {
    int device = 0;
    int64_t n = 0;
    int64_t env0 = 0;
    std::string last_error;
    std::string last_kernel;       // the kernel(s) the last step() / rollout() call launched, as rocprofv3 prints them (<env>_last_kernel)
    size_t device_bytes = 0;
    double *ep_ret = nullptr;      // episode-statistics outputs registered by <env>_episode_stats (caller-owned device buffers)
    int32_t *ep_len = nullptr;
    uint8_t *done_out = nullptr;   // step(): terminated | truncated per env, registered by <env>_done_mask (caller-owned device buffer, nullable)
    // <env>_rollout_final_obs: terminal observations of SAME_STEP rollouts, compacted per SEGMENT of consecutive envs (one wave's envs)
    void *fin_rows = nullptr;      // [n_segments * fin_cap, *obs_shape]
    int64_t *fin_index = nullptr;  // [n_segments * fin_cap]: step-in-call * n_envs + env
    int64_t fin_cap = 0;           // rows per segment
    int32_t *fin_count = nullptr;  // [n_segments]: rows the last rollout delivered for the segment (may exceed fin_cap: the surplus was dropped)

    // The handle's device arrays.  alloc() is the only place one is created; free_all(), device_bytes and the snapshot's blobs()
    // all follow from what it recorded, in registration order.  snap: the array is part of a whole-handle snapshot, and is zeroed
    // here whatever `zero` says: a snapshot copies the array whole, entries no kernel has written yet included, and must not carry
    // what hipMalloc happened to hand out (two snapshots of the same state are the same bytes).
    struct Array { void *ptr; size_t bytes; bool snap; };
    std::vector<Array> arrays;
    template <class T>
    hipError_t alloc(T *&slot, size_t bytes, bool zero, bool snap) {
        hipError_t e = hipMalloc(&slot, bytes);
        if (e != hipSuccess) return e;
        arrays.push_back({slot, bytes, snap});
        device_bytes += bytes;
        return zero || snap ? hipMemset(slot, 0, bytes) : hipSuccess;
    }
    void free_all() {
        for (const Array &a : arrays) (void)hipFree(a.ptr);
        arrays.clear();
    }
    std::vector<std::pair<void *, size_t>> blobs() const {
        std::vector<std::pair<void *, size_t>> b;
        for (const Array &a : arrays)
            if (a.snap) b.emplace_back(a.ptr, a.bytes);
        return b;
    }
    uint32_t snap_extra() const { return 0u; }       // host-side state a snapshot carries in its header (fleet has its own pair)
    void set_snap_extra(uint32_t v) { (void)v; }
    int record_prologue(const char *who) { (void)who; return CGE_OK; }   // get_records / set_records: nothing to read per call (crypto has its own)

    int fail(int status, const char *what, hipError_t e = hipSuccess) {
        char buf[512];
        if (e != hipSuccess)
            snprintf(buf, sizeof buf, "%s: %s (%s)", what, hipGetErrorName(e), hipGetErrorString(e));
        else
            snprintf(buf, sizeof buf, "%s", what);
        last_error = buf;
        return status;
    }
};

// Makes `device` current for the scope of one ABI call (torch may have another one selected).
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(int device) {
        if (hipGetDevice(&prev) == hipSuccess && prev != device) {
            switched = hipSetDevice(device) == hipSuccess;
        }
    }
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
};

// shared body of cge_<env>_rollout_final_obs
template <class H>
int register_final_obs(H *h, void *rows, int64_t *index, int64_t seg_capacity, int32_t *count, const char *who) {
    if (!h) return CGE_ERR_INVALID_ARG;
    if ((rows || index || count) && (!rows || !index || !count || seg_capacity <= 0)) return h->fail(CGE_ERR_INVALID_ARG, who);
    h->fin_rows = rows; h->fin_index = index; h->fin_cap = rows ? seg_capacity : 0; h->fin_count = count;
    return CGE_OK;
}

// the two entry points every env type exports for it (inside extern "C"); SEG = envs per segment = envs one wave steps
#define CGE_DEFINE_FINAL_OBS(ENV, ROWTYPE, SEG)                                                                                          \
    int cge_##ENV##_rollout_final_obs(cge_##ENV *h, ROWTYPE *rows_out, int64_t *index_out, int64_t seg_capacity, int32_t *count_out) {   \
        return cge::register_final_obs(h, rows_out, index_out, seg_capacity, count_out,                                                  \
                                       "cge_" #ENV "_rollout_final_obs: rows, index and count go together (all NULL unregisters)");      \
    }                                                                                                                                    \
    int64_t cge_##ENV##_final_obs_segment(const cge_##ENV *h) { return h ? (SEG) : 0; }
// ... under the names cge_rows_<env>_*: the six types that got the output after their surface cge_<env>_* was fixed at fifteen entry points
#define CGE_DEFINE_ROWS_FINAL_OBS(ENV, ROWTYPE, SEG)                                                                                          \
    int cge_rows_##ENV##_rollout_final_obs(cge_##ENV *h, ROWTYPE *rows_out, int64_t *index_out, int64_t seg_capacity, int32_t *count_out) {   \
        return cge::register_final_obs(h, rows_out, index_out, seg_capacity, count_out,                                                       \
                                       "cge_rows_" #ENV "_rollout_final_obs: rows, index and count go together (all NULL unregisters)");      \
    }                                                                                                                                         \
    int64_t cge_rows_##ENV##_final_obs_segment(const cge_##ENV *h) { return h ? (SEG) : 0; }

#define CGE_TRY(h, expr)                                                   \
    do {                                                                   \
        hipError_t _e = (expr);                                            \
        if (_e != hipSuccess) return (h)->fail(CGE_ERR_HIP, #expr, _e);    \
    } while (0)

// inside a function that returns hipError_t (a handle's init()): pass the first failure on
#define CGE_HIP(expr)                          \
    do {                                       \
        hipError_t _e = (expr);                \
        if (_e != hipSuccess) return _e;       \
    } while (0)

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

inline unsigned grid256(int64_t n) { return (unsigned)((n + 255) / 256); }   // blocks of 256 threads, one thread per env

// the tail of every entry point that launched kernels
template <class H>
int launched(H *h) {
    CGE_TRY(h, hipGetLastError());
    return CGE_OK;
}

// Head of cge_<env>_seed on the base path (seeds == NULL): the last env's seed is base_seed + env0 + n - 1, which must not pass the
// limit of the type's generator — 2**32 - 1 where a NumPy legacy stream is seeded (np.random.seed raises above it), 2**64 - 1
// elsewhere (the kernels form the sum in uint64_t; a third 32-bit limb is not implemented).  Host arithmetic, before any launch: a
// refused call seeds nothing.  A `seeds` array lives on the device and stays the caller's duty.  Returns CGE_OK or the failure.
template <class H>
int seed_base_check(H *h, const char *fn, const uint64_t *seeds, uint64_t base_seed, bool numpy_legacy) {
    if (seeds) return CGE_OK;
    const uint64_t limit = numpy_legacy ? 0xFFFFFFFFull : ~0ull;
    const uint64_t last = (uint64_t)h->env0 + (uint64_t)h->n - 1;      // create_handle: env0 >= 0, n >= 1
    if (last < (uint64_t)h->env0 || last > limit || base_seed > limit - last) {
        char buf[256];
        snprintf(buf, sizeof buf, numpy_legacy ? "%s: base_seed + env_index0 + n_envs - 1 must be between 0 and 2**32 - 1 (np.random.seed raises above it)"
                                               : "%s: base_seed + env_index0 + n_envs - 1 must be between 0 and 2**64 - 1", fn);
        return h->fail(CGE_ERR_INVALID_ARG, buf);
    }
    return CGE_OK;
}

// cge_<env>_create / _destroy.  An env type's handle H supplies what is its own:
//   static int check(const config &)   the status of a config it cannot run (CGE_OK: fine); runs before the device is looked at
//   hipError_t init()                  defaults, derived fields, alloc() of every device array, initial seed and reset launches
// The order of the checks decides the status code: arguments, config, device.  *out is null on every failure.
template <class H, class C>
int create_handle(const C *cfg, int64_t n_envs, int device, int64_t env_index0, H **out) {
    if (!cfg || !out || n_envs <= 0 || env_index0 < 0) return CGE_ERR_INVALID_ARG;
    *out = nullptr;
    if (int st = H::check(*cfg)) return st;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return CGE_ERR_NO_DEVICE;
    H *h = new H();
    h->cfg = *cfg; h->n = n_envs; h->env0 = env_index0; h->device = device;
    DeviceGuard g(device);
    hipError_t e = h->init();
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) {
        h->free_all();
        delete h;
        return CGE_ERR_HIP;
    }
    *out = h;
    return CGE_OK;
}
template <class H>
int destroy_handle(H *h) {
    if (!h) return CGE_ERR_INVALID_ARG;
    DeviceGuard g(h->device);
    (void)hipDeviceSynchronize();
    h->free_all();
    delete h;
    return CGE_OK;
}
inline bool bad_autoreset_mode(int mode) { return mode < 0 || mode > 2; }

// Head of cge_<env>_step: null checks (`have`: every pointer this env type requires is there; `what`: the error text if not), then
// p = h->params() with one step's outputs filled in.  The action pointers stay with the caller.
template <class H, class P, class O>
int step_params(H *h, P &p, bool have, const char *what, O *obs, float *reward, uint8_t *terminated, uint8_t *truncated, O *final_obs) {
    if (!h) return CGE_ERR_INVALID_ARG;
    if (!have) return h->fail(CGE_ERR_INVALID_ARG, what);
    p = h->params();
    p.obs = obs; p.reward = reward; p.terminated = terminated; p.truncated = truncated; p.final_obs = final_obs; p.k_steps = 1;
    return CGE_OK;
}

// Head of cge_<env>_rollout, h not null: k_steps and obs_step_stride (0, or at least one step's `step_elems` = n * obs row) are
// checked together with what the env type adds (`env_ok`), then p = h->params() with the rollout's arguments filled in.
// Returns CGE_OK for k_steps == 0 too: the caller returns then, there is nothing to launch.
template <class H, class P, class O, class S>
int rollout_params_nofin(H *h, P &p, bool env_ok, int64_t step_elems, const char *what, int32_t k_steps, uint64_t a_seed, int64_t t0, O *obs,
                         int64_t obs_step_stride, float *reward, S *reward_sum, int32_t *done_count) {
    if (!env_ok || k_steps < 0 || obs_step_stride < 0 || (obs_step_stride != 0 && obs_step_stride < step_elems))
        return h->fail(CGE_ERR_INVALID_ARG, what);
    p = h->params();
    p.k_steps = k_steps; p.a_seed = a_seed; p.t0 = t0; p.obs = obs; p.obs_step_stride = obs_step_stride;
    p.reward = reward; p.reward_sum = reward_sum; p.done_count = done_count;
    return CGE_OK;
}
// ... and, for the env types whose rollout reports terminated and compacts terminal observations (all but the bus system), those two
template <class H, class P, class O, class S>
int rollout_params(H *h, P &p, bool env_ok, int64_t step_elems, const char *what, int32_t k_steps, uint64_t a_seed, int64_t t0, O *obs,
                   int64_t obs_step_stride, float *reward, uint8_t *terminated, S *reward_sum, int32_t *done_count) {
    const int st = rollout_params_nofin(h, p, env_ok, step_elems, what, k_steps, a_seed, t0, obs, obs_step_stride, reward, reward_sum, done_count);
    if (st != CGE_OK) return st;
    p.terminated = terminated;
    p.fin = decltype(p.fin){h->fin_rows, h->fin_index, h->fin_count, h->fin_cap, h->n};
    return CGE_OK;
}

// The entry points that read the same in every env type (inside extern "C")
#define CGE_DEFINE_LIFECYCLE(ENV)                                                                                                        \
    int cge_##ENV##_create(const cge_##ENV##_config *cfg, int64_t n_envs, int device, int64_t env_index0, cge_##ENV **out) {             \
        return cge::create_handle(cfg, n_envs, device, env_index0, out);                                                                 \
    }                                                                                                                                    \
    int cge_##ENV##_destroy(cge_##ENV *h) { return cge::destroy_handle(h); }                                                             \
    size_t cge_##ENV##_device_bytes(const cge_##ENV *h) { return h ? h->device_bytes : 0; }                                              \
    int cge_##ENV##_episode_stats(cge_##ENV *h, double *return_out, int32_t *length_out) {                                               \
        if (!h) return CGE_ERR_INVALID_ARG;                                                                                              \
        h->ep_ret = return_out; h->ep_len = length_out;                                                                                  \
        return CGE_OK;                                                                                                                   \
    }                                                                                                                                    \
    const char *cge_##ENV##_last_error(const cge_##ENV *h) { return h ? h->last_error.c_str() : "null handle"; }                         \
    const char *cge_##ENV##_last_kernel(const cge_##ENV *h) { return h ? h->last_kernel.c_str() : ""; }

#define CGE_DEFINE_DONE_MASK(ENV)                                    \
    int cge_##ENV##_done_mask(cge_##ENV *h, uint8_t *done_out) {     \
        if (!h) return CGE_ERR_INVALID_ARG;                          \
        h->done_out = done_out;                                      \
        return CGE_OK;                                               \
    }

// the handle's `err`: one counter of the conditions a kernel reports instead of acting on; reading it clears it
#define CGE_DEFINE_ERROR_COUNT(ENV)                                                                              \
    int64_t cge_##ENV##_error_count(cge_##ENV *h, void *stream) {                                                \
        if (!h) return CGE_ERR_INVALID_ARG;                                                                      \
        cge::DeviceGuard g(h->device);                                                                           \
        unsigned long long v = 0;                                                                                \
        if (hipStreamSynchronize(cge::as_stream(stream)) != hipSuccess) return CGE_ERR_HIP;                      \
        if (hipMemcpy(&v, h->err, sizeof v, hipMemcpyDeviceToHost) != hipSuccess) return CGE_ERR_HIP;            \
        if (v && hipMemset(h->err, 0, sizeof v) != hipSuccess) return CGE_ERR_HIP;                               \
        return (int64_t)v;                                                                                       \
    }

// Whole-handle snapshots (checkpoint / resume) for the env types without a canonical per-env record: a 32-byte header
// {magic, n_envs, env tag, extra} followed by the handle's device arrays in their device layout.  Only valid for a handle
// created with the same n_envs and config.  The blobs are the arrays H registered with alloc(..., snap = true); H adds snap_tag.
struct SnapHeader { uint64_t magic; int64_t n; uint32_t tag, extra; uint64_t reserved; };
// "CGESNAP3": 1 = round 1; 2 = round 2 (MT blocks grew mirror words 624..639, ep_return fields in the records) — blobs of an older
// layout are refused instead of being read with the wrong meaning
constexpr uint64_t SNAP_MAGIC = 0x3350414e53454743ull;
template <class H>
size_t snapshot_bytes(const H *h) {
    size_t t = sizeof(SnapHeader);
    for (const auto &b : h->blobs()) t += b.second;
    return t;
}
template <class H>
int snapshot_get(H *h, void *host, hipStream_t s) {
    if (!h || !host) return CGE_ERR_INVALID_ARG;
    DeviceGuard g(h->device);
    CGE_TRY(h, hipStreamSynchronize(s));
    SnapHeader hd{SNAP_MAGIC, h->n, H::snap_tag, h->snap_extra(), 0};
    memcpy(host, &hd, sizeof hd);
    char *dst = static_cast<char *>(host) + sizeof hd;
    for (const auto &b : h->blobs()) { CGE_TRY(h, hipMemcpy(dst, b.first, b.second, hipMemcpyDeviceToHost)); dst += b.second; }
    return CGE_OK;
}
template <class H>
int snapshot_set(H *h, const void *host, hipStream_t s) {
    if (!h || !host) return CGE_ERR_INVALID_ARG;
    DeviceGuard g(h->device);
    SnapHeader hd;
    memcpy(&hd, host, sizeof hd);
    if (hd.magic != SNAP_MAGIC || hd.n != h->n || hd.tag != H::snap_tag) return h->fail(CGE_ERR_INVALID_ARG, "snapshot_set: not a snapshot of this env type / batch size");
    CGE_TRY(h, hipStreamSynchronize(s));
    const char *src = static_cast<const char *>(host) + sizeof hd;
    for (const auto &b : h->blobs()) { CGE_TRY(h, hipMemcpy(b.first, src, b.second, hipMemcpyHostToDevice)); src += b.second; }
    h->set_snap_extra(hd.extra);
    return CGE_OK;
}
#define CGE_DEFINE_SNAPSHOT(ENV)                                                                                                                            \
    size_t cge_##ENV##_snapshot_bytes(const cge_##ENV *h) { return h ? cge::snapshot_bytes(h) : 0; }                                                       \
    int cge_##ENV##_snapshot_get(cge_##ENV *h, void *host_buf, void *stream) { return cge::snapshot_get(h, host_buf, cge::as_stream(stream)); }            \
    int cge_##ENV##_snapshot_set(cge_##ENV *h, const void *host_buf, void *stream) { return cge::snapshot_set(h, host_buf, cge::as_stream(stream)); }

// device stream (block, cursor, ready mark) -> CPython layout (624 words of ONE generation + index of the next unconsumed word).
// Words [pos, pretw) are twisted already; the rest of the generation is twisted here.  A ready mark beyond 624 means the first
// chunk of the NEXT generation has been twisted in place as well (cge_device.hpp: mt_make_ready): those words are taken back
// to the current generation first — the twist is invertible word by word: new[k] ^ cur[k+397] = g(y) with y = (cur[k] & 0x80000000)
// | (cur[k+1] & 0x7fffffff), and g(y) = (y >> 1) ^ (y & 1 ? 0x9908b0df : 0) gives y back (bit 31 of g(y) is y's bit 0).  What cannot
// be recovered, the low 31 bits of cur[0], no future output depends on.
// old0: the saved word 0 of the current generation (its dead low bits), or nullptr: then they read as zero.
// The un-twist of word k reads word k + 397 of the current generation, so it can take back at most MT_EXPORT_MAX_AHEAD words
// of the next generation (224 in whole 32-word chunks).  The kernels stay far below it (crypto: at most 64 words, traffic: at most
// 96; tests/test_mt_export_cpu.py derives both); a longer run is refused (returns false, *idx = -1) instead of read past the record.
constexpr uint32_t MT_EXPORT_MAX_AHEAD = 624u - 397u;
inline bool mt_export_cpython(const uint32_t *w, uint32_t pos, uint32_t pretw, uint32_t *omt, int32_t *idx, const uint32_t *old0 = nullptr) {
    memcpy(omt, w, 624 * 4);
    // a cursor that has just wrapped (pos 0) with chunks of the new generation already twisted: CPython regenerates lazily, its
    // state at this point is index 624 over the OLD generation — the same un-twist, seen from the end of that generation
    if (pos == 0u && pretw > 0u && pretw < 624u) { pos = 624u; pretw += 624u; }
    if (pretw > 624u) {
        const uint32_t ahead = pretw - 624u;         // words [0, ahead) belong to the next generation
        if (ahead > MT_EXPORT_MAX_AHEAD) { *idx = -1; return false; }
        std::vector<uint32_t> y(ahead);
        for (uint32_t k = 0; k < ahead; ++k) {
            const uint32_t g = omt[k] ^ omt[k + 397];          // k + 397 < 624: a word of the current generation
            const uint32_t odd = g >> 31;
            y[k] = (((g ^ (odd ? 0x9908b0dfu : 0u)) << 1) | odd);
        }
        for (uint32_t k = 0; k < ahead; ++k) {
            const uint32_t upper = y[k] & 0x80000000u, lower = k ? (y[k - 1] & 0x7fffffffu) : (old0 ? *old0 & 0x7fffffffu : 0u);
            omt[k] = upper | lower;
        }
        omt[ahead] = (omt[ahead] & 0x80000000u) | (y[ahead - 1] & 0x7fffffffu);   // (its low bits were never changed: a consistency no-op)
        pretw = 624;
    }
    if (pretw >= 624u) { *idx = (int32_t)pos; return true; }
    if (pos == 0 && pretw == 0) { *idx = 624; return true; }
    for (uint32_t k = pretw > pos ? pretw : pos; k < 624u; ++k) {
        const uint32_t k1 = k + 1 == 624u ? 0 : k + 1, km = k + 397 >= 624u ? k + 397 - 624 : k + 397;
        const uint32_t t = (omt[k] & 0x80000000u) | (omt[k1] & 0x7fffffffu);
        omt[k] = omt[km] ^ (t >> 1) ^ ((t & 1u) ? 0x9908b0dfu : 0u);
    }
    *idx = (int32_t)pos;
    return true;
}

// CPython layout (624 words, index) -> device stream: the block with its 16 mirror words (624..639 repeat 0..15, cge_device.hpp) and
// the cursor.  Every word from the index on is generated but unconsumed, so the whole generation is ready (mark 624); index 624
// means "regenerate at the next draw": cursor 0 with nothing ready.
inline void mt_import_cpython(const uint32_t *words624, int32_t index, uint32_t *block640, uint32_t *pos, uint32_t *pretw) {
    memcpy(block640, words624, 624 * 4);
    memcpy(block640 + 624, block640, 16 * 4);
    const bool regenerate = index >= 624;
    *pos = regenerate ? 0u : (uint32_t)index;
    *pretw = regenerate ? 0u : 624u;
}

// Canonical per-env records (get_state / set_state), for the env types that have them.  The driver below owns the null checks, the
// device guard, the stream synchronisation, the rounds of STATE_CHUNK envs, the host staging (sized by the chunk, never by n), the
// copies and the error return.  A handle H supplies what is its own:
//   static constexpr const char *abi         "cge_<env>", the prefix of the error texts
//   size_t record_bytes() const
//   std::vector<RecordArray> record_arrays() const     the device arrays a record is made from, in the order stage.at() names them
//   int record_prologue(const char *who)     handle-level values read once per call, after the synchronisation (default: none)
//   const char *check_record(const uint8_t *rec)       nullptr, or why set_state refuses the record; reads the record only
//   int to_record(const RecordStage &, int64_t j, uint8_t *rec, const char **why) const     env j of the staged round -> record;
//                                            CGE_OK, or a status and *why
//   void from_record(const uint8_t *rec, RecordStage &, int64_t j) const                    a checked record -> env j of the round
constexpr int64_t STATE_CHUNK = 4096;      // envs per host staging round: bounds the host memory of a large batch's export
struct RecordArray {
    void *dev;
    size_t elem;          // bytes per element
    int64_t rows;         // elements per env
    bool env_major;       // true: env i owns `rows` consecutive elements; false (column-major): element (row r, env i) at r * n + i
    bool get;             // false: get_state does not read it; set_state uploads it as zeros unless from_record writes it
};
struct RecordStage {
    std::vector<RecordArray> arrays;
    int64_t n, cap;       // envs of the handle, envs per round
    std::vector<std::vector<uint8_t>> buf;
    RecordStage(std::vector<RecordArray> a, int64_t n_) : arrays(std::move(a)), n(n_), cap(n_ < STATE_CHUNK ? n_ : STATE_CHUNK) {
        for (const RecordArray &d : arrays) buf.emplace_back(d.elem * (size_t)d.rows * (size_t)cap, (uint8_t)0);
    }
    // element `row` of env j of the round in array a
    template <class T>
    T *at(int a, int64_t j, int64_t row = 0) const {
        const RecordArray &d = arrays[a];
        return reinterpret_cast<T *>(const_cast<uint8_t *>(buf[a].data())) + (d.env_major ? j * d.rows + row : row * cap + j);
    }
    // envs [c0, c0 + m) of array a between the device and the stage: one contiguous piece (env-major), or one piece per row
    hipError_t copy(int a, int64_t c0, int64_t m, bool to_device) {
        const RecordArray &d = arrays[a];
        const int64_t pieces = d.env_major ? 1 : d.rows;
        const size_t bytes = (size_t)m * d.elem * (d.env_major ? (size_t)d.rows : 1u);
        for (int64_t r = 0; r < pieces; ++r) {
            char *dev = static_cast<char *>(d.dev) + (d.env_major ? (size_t)c0 * d.rows : (size_t)r * n + c0) * d.elem;
            uint8_t *host = buf[a].data() + (size_t)r * cap * d.elem;
            const hipError_t e = to_device ? hipMemcpy(dev, host, bytes, hipMemcpyHostToDevice) : hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
};
template <class H>
int record_fail(H *h, int status, const char *fn, int64_t env, const char *why) {
    char msg[256];
    snprintf(msg, sizeof msg, "%s_%s: env %lld: %s", H::abi, fn, (long long)env, why);
    return h->fail(status, msg);
}
template <class H>
int get_records(H *h, void *host_buf, hipStream_t s) {
    if (!h || !host_buf) return CGE_ERR_INVALID_ARG;
    DeviceGuard g(h->device);
    CGE_TRY(h, hipStreamSynchronize(s));
    if (int st = h->record_prologue("get_state")) return st;
    const size_t rec = h->record_bytes();
    RecordStage stage(h->record_arrays(), h->n);
    for (int64_t c0 = 0; c0 < h->n; c0 += stage.cap) {
        const int64_t m = h->n - c0 < stage.cap ? h->n - c0 : stage.cap;
        for (int a = 0; a < (int)stage.arrays.size(); ++a)
            if (stage.arrays[a].get) CGE_TRY(h, stage.copy(a, c0, m, false));
        for (int64_t j = 0; j < m; ++j) {
            const char *why = "";
            if (int st = h->to_record(stage, j, static_cast<uint8_t *>(host_buf) + (size_t)(c0 + j) * rec, &why)) return record_fail(h, st, "get_state", c0 + j, why);
        }
    }
    return CGE_OK;
}
// Every record is checked before the stream is waited for and before anything is written: a malformed record anywhere leaves the
// device state of every env as it was.
template <class H>
int set_records(H *h, const void *host_buf, hipStream_t s) {
    if (!h || !host_buf) return CGE_ERR_INVALID_ARG;
    DeviceGuard g(h->device);
    const size_t rec = h->record_bytes();
    const uint8_t *in = static_cast<const uint8_t *>(host_buf);
    for (int64_t i = 0; i < h->n; ++i)
        if (const char *bad = h->check_record(in + (size_t)i * rec)) return record_fail(h, CGE_ERR_INVALID_ARG, "set_state", i, bad);
    CGE_TRY(h, hipStreamSynchronize(s));
    if (int st = h->record_prologue("set_state")) return st;
    RecordStage stage(h->record_arrays(), h->n);
    for (int64_t c0 = 0; c0 < h->n; c0 += stage.cap) {
        const int64_t m = h->n - c0 < stage.cap ? h->n - c0 : stage.cap;
        for (int64_t j = 0; j < m; ++j) h->from_record(in + (size_t)(c0 + j) * rec, stage, j);
        for (int a = 0; a < (int)stage.arrays.size(); ++a) CGE_TRY(h, stage.copy(a, c0, m, true));
    }
    return CGE_OK;
}
#define CGE_DEFINE_RECORDS(ENV)                                                                                                                \
    size_t cge_##ENV##_state_bytes(const cge_##ENV *h) { return h ? h->record_bytes() : 0; }                                                   \
    int cge_##ENV##_get_state(cge_##ENV *h, void *host_buf, void *stream) { return cge::get_records(h, host_buf, cge::as_stream(stream)); }    \
    int cge_##ENV##_set_state(cge_##ENV *h, const void *host_buf, void *stream) { return cge::set_records(h, host_buf, cge::as_stream(stream)); }


// Seeds n MT19937 stream blocks (cge_device.hpp layout, `stride_words` apart starting at `mt`).
//   kind 0: CPython random.seed(s)  = init_by_array(32-bit limbs of s)
//   kind 1: NumPy legacy np.random.seed(s) = init_genrand((uint32)s)
// s = seeds[i] if seeds != nullptr (device pointer) else base_seed + env0 + i.
hipError_t launch_mt_seed(uint32_t *mt, int64_t stride_words, int64_t n, const uint64_t *seeds, uint64_t base_seed,
                          int64_t env0, int kind, hipStream_t stream);

}  // namespace cge
