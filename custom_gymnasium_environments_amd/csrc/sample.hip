// sample.hip — `action_space.sample()` of the batched action spaces on the device, bit for bit what a space seeded with
// np.random.default_rng(seed) returns from successive sample() calls (gymnasium 1.x; include/cge_amd.h, sampler section).
//
// One handle = one NumPy PCG64 stream, 40 bytes of state in device memory.  The draws of one call are numbered in stream order;
// draw g of the world batch is the output the stream gives after g steps, so a thread that owns a contiguous run of draws jumps
// once (cge_pcg.hpp: Pcg64::jump, a seed-independent table of 64 (A, S) pairs) and then steps sequentially.  Every block reads the
// stream's state, does its draws, then takes a ticket from a per-handle counter; the block that takes the last ticket — every other
// block has read the state by then — writes the advanced state and resets the counter.  So one launch both samples and advances, with no host
// synchronisation, and a captured graph replays it as it is.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "cge_host.hpp"
#include "cge_pcg.hpp"

namespace cge {
namespace smp {

constexpr int BLOCK = 256;
constexpr int RUN = 8;          // draws per thread (index / uniform): one 64-bit output each
constexpr int RUN_BYTES = 32;   // bytes per thread (bits): 8 words, 4 outputs

// the device record: cge_pcg64_state (40 bytes), the block counter, then the per-column parameters (k doubles, k more for UNIFORM's high)
constexpr size_t OFF_COUNTER = 40, OFF_PARAMS = 64;

struct Shared {
    uint64_t w[5];   // state lo / hi, inc lo / hi, has_uint32 | uinteger << 32
    int last;
};

// every block: thread 0 reads the stream's state into LDS; returns the stream as it was at the call's start
__device__ __forceinline__ Pcg64 load_stream(const uint64_t *gst, Shared &sh) {
    if (threadIdx.x == 0) {
        const uint64_t w0 = gst[0], w1 = gst[1], w2 = gst[2], w3 = gst[3], w4 = gst[4];
        sh.w[0] = w0; sh.w[1] = w1; sh.w[2] = w2; sh.w[3] = w3; sh.w[4] = w4;
    }
    __syncthreads();
    Pcg64 p;
    p.state = ((u128)sh.w[1] << 64) | sh.w[0];
    p.inc = ((u128)sh.w[3] << 64) | sh.w[2];
    p.has_uint32 = (uint32_t)sh.w[4];
    p.uinteger = (uint32_t)(sh.w[4] >> 32);
    return p;
}

// every block, after its work: thread 0 takes a ticket; true for the block that takes the last one.  The block's read of the state
// has completed long before (its value went through LDS into every draw), so a relaxed atomic suffices: no fence, which at agent
// scope would write back the block's dirty L2 lines; taking the ticket at the end keeps the atomic's round trip off the draws' path.
__device__ __forceinline__ bool take_ticket(uint32_t *counter) {
    return __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x * gridDim.y - 1u;
}

// the last block's thread 0: the stream after the call
__device__ __forceinline__ void store_stream(uint64_t *gst, uint32_t *counter, const Pcg64 &p) {
    gst[0] = (uint64_t)p.state;
    gst[1] = (uint64_t)(p.state >> 64);
    gst[4] = (uint64_t)p.has_uint32 | ((uint64_t)p.uinteger << 32);
    *counter = 0u;
}

// jump by m << J0 steps, m < 2^NB, with the table entries as compile-time constants (the per-lane part of a thread's offset)
template <int J0, int NB>
__device__ __forceinline__ void jump_lane(Pcg64 &q, uint32_t m) {
#pragma unroll
    for (int b = 0; b < NB; ++b)
        if ((m >> b) & 1u) q.state = pcg64_jump_table.a[J0 + b] * q.state + pcg64_jump_table.s[J0 + b] * q.inc;
}

// a full run of N values of T: 16-byte stores when the run is aligned, element stores otherwise
template <class T, int N>
__device__ __forceinline__ void store_run(T *o, const T (&v)[N]) {
    constexpr int BYTES = (int)sizeof(T) * N;
    if (BYTES % 16 == 0 && ((uintptr_t)o & 15u) == 0) {
        const uint4 *src = reinterpret_cast<const uint4 *>(v);
#pragma unroll
        for (int i = 0; i < BYTES / 16; ++i) reinterpret_cast<uint4 *>(o)[i] = src[i];
    } else if (BYTES == 8 && ((uintptr_t)o & 7u) == 0) {
        *reinterpret_cast<uint2 *>(o) = *reinterpret_cast<const uint2 *>(v);
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) o[i] = v[i];
    }
}

// thread t of block (x, s) owns draws [i0, i0 + RUN) of step s, i0 = (x * BLOCK + t) * RUN; its first draw is output number
// s * world_draws + first + i0 of the call: the block-uniform part of that offset goes through Pcg64::jump (uniform loop, scalar
// table loads), the lane part t * RUN through jump_lane
__device__ __forceinline__ Pcg64 run_start(const Pcg64 &p, int64_t s, int64_t world_draws, int64_t first) {
    Pcg64 q = p;
    q.jump((uint64_t)(s * world_draws + first + (int64_t)blockIdx.x * BLOCK * RUN));
    jump_lane<3, 8>(q, threadIdx.x);                               // RUN = 8 = 2^3, BLOCK = 256 = 2^8
    return q;
}
static_assert(RUN == 8 && BLOCK == 256, "run_start's lane jump assumes RUN = 8 and BLOCK = 256");

// MultiDiscrete: out = trunc(random() * nvec[col]); draws of step s, local element i: s * world_draws + first + i
template <class T>
__global__ __launch_bounds__(BLOCK) void cge_sample_index_kernel(uint64_t *gst, uint32_t *counter, const double *__restrict__ nvec, int64_t k,
                                                                 int64_t row_draws, int64_t first, int64_t world_draws, T *__restrict__ out) {
    __shared__ Shared sh;
    const Pcg64 p = load_stream(gst, sh);
    const int64_t s = blockIdx.y, i0 = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) * RUN;
    if (i0 < row_draws) {
        Pcg64 q = run_start(p, s, world_draws, first);
        int64_t col = i0 % k;                                      // first is a whole number of rows
        T *o = out + s * row_draws + i0;
        if (i0 + RUN <= row_draws) {
            T v[RUN];
            if (k == 1) {
                const double nv = nvec[0];
#pragma unroll
                for (int r = 0; r < RUN; ++r) v[r] = (T)(int64_t)(q.random() * nv);
            } else {
#pragma unroll
                for (int r = 0; r < RUN; ++r) {
                    v[r] = (T)(int64_t)(q.random() * nvec[col]);
                    if (++col == k) col = 0;
                }
            }
            store_run(o, v);
        } else {
            for (int r = 0; r < (int)(row_draws - i0); ++r) {
                o[r] = (T)(int64_t)(q.random() * nvec[col]);
                if (++col == k) col = 0;
            }
        }
    }
    if (threadIdx.x == 0) sh.last = take_ticket(counter);
    __syncthreads();
    if (sh.last && threadIdx.x == 0) {
        Pcg64 q = p;
        q.jump((uint64_t)(gridDim.y * world_draws));
        store_stream(gst, counter, q);
    }
}

// bounded Box: float out = float(low + (high - low) * u) (Generator.uniform, no FMA: -ffp-contract=off); integer out =
// floor(low + ((high + 1) - low) * u) (gymnasium's integer-Box path)
template <class T, bool INTEGER>
__device__ __forceinline__ T uniform_value(double l, double h, double u) {
    if (INTEGER) return (T)(int64_t)floor(l + ((h + 1.0) - l) * u);
    return (T)(l + (h - l) * u);
}

template <class T, bool INTEGER>
__global__ __launch_bounds__(BLOCK) void cge_sample_uniform_kernel(uint64_t *gst, uint32_t *counter, const double *__restrict__ lo,
                                                                   const double *__restrict__ hi, int64_t k, int64_t row_draws, int64_t first,
                                                                   int64_t world_draws, T *__restrict__ out) {
    __shared__ Shared sh;
    const Pcg64 p = load_stream(gst, sh);
    const int64_t s = blockIdx.y, i0 = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) * RUN;
    if (i0 < row_draws) {
        Pcg64 q = run_start(p, s, world_draws, first);
        int64_t col = i0 % k;
        T *o = out + s * row_draws + i0;
        if (i0 + RUN <= row_draws) {
            T v[RUN];
#pragma unroll
            for (int r = 0; r < RUN; ++r) {
                v[r] = uniform_value<T, INTEGER>(lo[col], hi[col], q.random());
                if (++col == k) col = 0;
            }
            store_run(o, v);
        } else {
            for (int r = 0; r < (int)(row_draws - i0); ++r) {
                o[r] = uniform_value<T, INTEGER>(lo[col], hi[col], q.random());
                if (++col == k) col = 0;
            }
        }
    }
    if (threadIdx.x == 0) sh.last = take_ticket(counter);
    __syncthreads();
    if (sh.last && threadIdx.x == 0) {
        Pcg64 q = p;
        q.jump((uint64_t)(gridDim.y * world_draws));
        store_stream(gst, counter, q);
    }
}

// MultiBinary: Generator.integers(0, 2, dtype=int8).  Each call takes words_per_step 32-bit words from next32 (its byte buffer
// is local to the call); word w of the launch (w = s * words_per_step + byte / 4) is the carried upper half when the stream starts
// with has_uint32 = 1 and w = 0, else half (w - c) & 1 of output (w - c) >> 1, c = has_uint32 at the start.  Byte b -> (b * 2) >> 8,
// i.e. bit 7 of the byte: a whole word gives its four results as (word >> 7) & 0x01010101.
__global__ __launch_bounds__(BLOCK) void cge_sample_bits_kernel(uint64_t *gst, uint32_t *counter, int64_t row_bytes, int64_t first,
                                                                int64_t words_per_step, int8_t *__restrict__ out) {
    __shared__ Shared sh;
    const Pcg64 p = load_stream(gst, sh);
    const int64_t c = p.has_uint32 ? 1 : 0;
    const int64_t s = blockIdx.y, b0 = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) * RUN_BYTES;
    if (b0 < row_bytes) {
        // word of the thread's first byte: wu + 8 t (b0 is a multiple of 4, so (first + b0) / 4 = first / 4 + b0 / 4)
        const int64_t wu = s * words_per_step + first / 4 - c + (int64_t)blockIdx.x * BLOCK * (RUN_BYTES / 4);
        const int64_t w0 = wu + (int64_t)threadIdx.x * (RUN_BYTES / 4);
        Pcg64 q = p;
        if (wu >= 0) {                                             // q's next output: number w0 >> 1 = (wu >> 1) + 4 t
            q.jump((uint64_t)(wu >> 1));
            jump_lane<2, 8>(q, threadIdx.x);                       // RUN_BYTES / 8 = 4 = 2^2 outputs per thread
        } else if (w0 > 0) {                                       // (wu = -1: the carried half opens the call)
            q.jump((uint64_t)(w0 >> 1));
        }
        int8_t *o = out + s * row_bytes + b0;
        if (b0 + RUN_BYTES <= row_bytes && ((first & 3) == 0) && ((uintptr_t)o & 15u) == 0) {
            uint32_t v[RUN_BYTES / 4];
            uint64_t cur = 0;
#pragma unroll
            for (int m = 0; m < RUN_BYTES / 4; ++m) {
                const int64_t w = w0 + m;
                uint32_t word;
                if (w < 0) {
                    word = p.uinteger;
                } else {
                    if (m == 0 || (w & 1) == 0) cur = q.next64();
                    word = (w & 1) ? (uint32_t)(cur >> 32) : (uint32_t)cur;
                }
                v[m] = (word >> 7) & 0x01010101u;
            }
            uint32_t *o32 = reinterpret_cast<uint32_t *>(o);
            store_run(o32, v);
        } else {
            const int n = (int)(row_bytes - b0 < RUN_BYTES ? row_bytes - b0 : RUN_BYTES);
            int64_t cur_o = -1;
            uint64_t cur = 0;
            for (int r = 0; r < n; ++r) {
                const int64_t g = first + b0 + r, w = s * words_per_step + g / 4 - c;
                uint32_t word;
                if (w < 0) {
                    word = p.uinteger;
                } else {
                    if ((w >> 1) != cur_o) { cur = q.next64(); cur_o = w >> 1; }
                    word = (w & 1) ? (uint32_t)(cur >> 32) : (uint32_t)cur;
                }
                const uint32_t b = (word >> (8 * (g & 3))) & 0xffu;
                o[r] = (int8_t)((b * 2u) >> 8);
            }
        }
    }
    if (threadIdx.x == 0) sh.last = take_ticket(counter);
    __syncthreads();
    if (sh.last && threadIdx.x == 0) {
        Pcg64 q = p;
        const int64_t d = (int64_t)gridDim.y * words_per_step - c;   // words taken from fresh outputs (>= 0)
        if (d > 0) {
            const int64_t u = (d + 1) / 2;
            q.jump((uint64_t)(u - 1));
            q.uinteger = (uint32_t)(q.next64() >> 32);             // NumPy keeps the upper half of every fresh output, used or not
        }
        q.has_uint32 = (uint32_t)(d & 1);
        store_stream(gst, counter, q);
    }
}

}  // namespace smp
}  // namespace cge

using namespace cge;

struct cge_sampler : cge::HandleBase {
    int32_t kind = 0;
    int64_t k = 0, row0 = 0, world = 0;
    double pmin = 0, pmax = 0;      // smallest / largest parameter (UNIFORM: low / high over the columns; INDEX: nvec)
    bool integral = true;           // every parameter is a whole number (UNIFORM integer outputs need that)
    char *dev = nullptr;
    uint64_t *st() const { return reinterpret_cast<uint64_t *>(dev); }
    uint32_t *counter() const { return reinterpret_cast<uint32_t *>(dev + smp::OFF_COUNTER); }
    double *params() const { return reinterpret_cast<double *>(dev + smp::OFF_PARAMS); }
};

namespace {

void to_host(const Pcg64 &p, cge_pcg64_state *s) {
    s->state_lo = (uint64_t)p.state; s->state_hi = (uint64_t)(p.state >> 64);
    s->inc_lo = (uint64_t)p.inc; s->inc_hi = (uint64_t)(p.inc >> 64);
    s->has_uint32 = p.has_uint32; s->uinteger = p.uinteger;
}

Pcg64 from_host(const cge_pcg64_state *s) {
    Pcg64 p;
    p.state = ((u128)s->state_hi << 64) | s->state_lo;
    p.inc = ((u128)s->inc_hi << 64) | s->inc_lo;
    p.has_uint32 = s->has_uint32; p.uinteger = s->uinteger;
    return p;
}

constexpr int64_t MAX_DRAWS = (int64_t)1 << 62;

}  // namespace

extern "C" {

int cge_pcg64_advance(cge_pcg64_state *state, uint64_t delta_lo, uint64_t delta_hi) {
    if (!state) return CGE_ERR_INVALID_ARG;
    Pcg64 p = from_host(state);
    p.advance(((u128)delta_hi << 64) | delta_lo);
    to_host(p, state);
    return CGE_OK;
}

int cge_sampler_create(int32_t kind, int64_t k, const double *params, int64_t n_rows, int64_t row0, int64_t world_rows, int device,
                       cge_sampler **out) {
    if (!out) return CGE_ERR_INVALID_ARG;
    *out = nullptr;
    if (kind < CGE_SAMPLE_INDEX || kind > CGE_SAMPLE_BITS || k < 1 || k > CGE_SAMPLER_MAX_K || n_rows < 1 || row0 < 0 ||
        world_rows < 1 || row0 > world_rows - n_rows || world_rows > MAX_DRAWS / k)
        return CGE_ERR_INVALID_ARG;
    const int64_t np = kind == CGE_SAMPLE_INDEX ? k : kind == CGE_SAMPLE_UNIFORM ? 2 * k : 0;
    if (np && !params) return CGE_ERR_INVALID_ARG;
    double pmin = 0, pmax = 0;
    bool integral = true;
    for (int64_t i = 0; i < np; ++i) {
        const double v = params[i];
        if (!std::isfinite(v)) return CGE_ERR_INVALID_ARG;
        if (kind == CGE_SAMPLE_INDEX && (v < 1.0 || v != std::floor(v) || v > 9007199254740992.0)) return CGE_ERR_INVALID_ARG;
        if (kind == CGE_SAMPLE_UNIFORM && i < k && !(v <= params[k + i])) return CGE_ERR_INVALID_ARG;
        integral = integral && v == std::floor(v);
        pmin = i ? std::fmin(pmin, v) : v;
        pmax = i ? std::fmax(pmax, v) : v;
    }
    if (device < 0) return CGE_ERR_INVALID_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) return CGE_ERR_NO_DEVICE;
    cge_sampler *h = new cge_sampler();
    h->kind = kind; h->k = k; h->n = n_rows; h->row0 = row0; h->env0 = row0; h->world = world_rows; h->device = device;
    h->pmin = pmin; h->pmax = pmax; h->integral = integral;
    DeviceGuard g(device);
    const size_t bytes = smp::OFF_PARAMS + (size_t)np * sizeof(double);
    cge_pcg64_state s0;
    Pcg64 p;
    p.seed(0);                                                      // np.random.default_rng(0) until set_state
    to_host(p, &s0);
    char hostbuf[smp::OFF_PARAMS] = {};
    memcpy(hostbuf, &s0, sizeof s0);
    hipError_t e;
    if ((e = hipMalloc(&h->dev, bytes)) != hipSuccess || (e = hipMemcpy(h->dev, hostbuf, sizeof hostbuf, hipMemcpyHostToDevice)) != hipSuccess ||
        (np && (e = hipMemcpy(h->params(), params, (size_t)np * sizeof(double), hipMemcpyHostToDevice)) != hipSuccess)) {
        if (h->dev) (void)hipFree(h->dev);
        delete h;
        return CGE_ERR_HIP;
    }
    h->device_bytes = bytes;
    *out = h;
    return CGE_OK;
}

int cge_sampler_destroy(cge_sampler *h) {
    if (!h) return CGE_ERR_INVALID_ARG;
    DeviceGuard g(h->device);
    (void)hipDeviceSynchronize();
    if (h->dev) (void)hipFree(h->dev);
    delete h;
    return CGE_OK;
}

int cge_sampler_set_state(cge_sampler *h, const cge_pcg64_state *state, void *stream) {
    if (!h) return CGE_ERR_INVALID_ARG;
    if (!state || !(state->inc_lo & 1)) return h->fail(CGE_ERR_INVALID_ARG, "cge_sampler_set_state: null state or an even PCG64 increment");
    if (state->has_uint32 > 1) return h->fail(CGE_ERR_INVALID_ARG, "cge_sampler_set_state: has_uint32 must be 0 or 1");
    DeviceGuard g(h->device);
    CGE_TRY(h, hipStreamSynchronize(as_stream(stream)));
    CGE_TRY(h, hipMemcpy(h->st(), state, sizeof *state, hipMemcpyHostToDevice));
    return CGE_OK;
}

int cge_sampler_get_state(cge_sampler *h, cge_pcg64_state *state, void *stream) {
    if (!h) return CGE_ERR_INVALID_ARG;
    if (!state) return h->fail(CGE_ERR_INVALID_ARG, "cge_sampler_get_state: null state");
    DeviceGuard g(h->device);
    CGE_TRY(h, hipStreamSynchronize(as_stream(stream)));
    CGE_TRY(h, hipMemcpy(state, h->st(), sizeof *state, hipMemcpyDeviceToHost));
    return CGE_OK;
}

int cge_sampler_sample(cge_sampler *h, int64_t steps, void *out, int32_t out_dtype, void *stream) {
    if (!h) return CGE_ERR_INVALID_ARG;
    if (!out) return h->fail(CGE_ERR_INVALID_ARG, "cge_sampler_sample: null out");
    if (steps < 1 || steps > CGE_SAMPLER_MAX_STEPS) return h->fail(CGE_ERR_INVALID_ARG, "cge_sampler_sample: steps out of range");
    const int64_t row_draws = h->n * h->k, world_draws = h->world * h->k, first = h->row0 * h->k;
    if (world_draws > MAX_DRAWS / steps) return h->fail(CGE_ERR_INVALID_ARG, "cge_sampler_sample: too many draws in one call");
    const hipStream_t s = as_stream(stream);
    DeviceGuard g(h->device);
    if (h->kind == CGE_SAMPLE_BITS) {
        if (out_dtype != CGE_DTYPE_INT8) return h->fail(CGE_ERR_INVALID_ARG, "cge_sampler_sample: BITS writes int8");
        const dim3 grid((unsigned)((row_draws + (int64_t)smp::BLOCK * smp::RUN_BYTES - 1) / ((int64_t)smp::BLOCK * smp::RUN_BYTES)), (unsigned)steps);
        hipLaunchKernelGGL(smp::cge_sample_bits_kernel, grid, dim3(smp::BLOCK), 0, s, h->st(), h->counter(), row_draws, first,
                           (world_draws + 3) / 4, static_cast<int8_t *>(out));
        h->last_kernel = "cge::smp::cge_sample_bits_kernel";
        CGE_TRY(h, hipGetLastError());
        return CGE_OK;
    }
    const dim3 grid((unsigned)((row_draws + (int64_t)smp::BLOCK * smp::RUN - 1) / ((int64_t)smp::BLOCK * smp::RUN)), (unsigned)steps);
    const double *p = h->params();
    if (h->kind == CGE_SAMPLE_INDEX) {
        if (out_dtype == CGE_DTYPE_INT32) {
            if (h->pmax > 2147483648.0) return h->fail(CGE_ERR_INVALID_ARG, "cge_sampler_sample: nvec too large for int32");
            hipLaunchKernelGGL(smp::cge_sample_index_kernel<int32_t>, grid, dim3(smp::BLOCK), 0, s, h->st(), h->counter(), p, h->k, row_draws,
                               first, world_draws, static_cast<int32_t *>(out));
            h->last_kernel = "cge::smp::cge_sample_index_kernel<int>";
        } else if (out_dtype == CGE_DTYPE_INT64) {
            hipLaunchKernelGGL(smp::cge_sample_index_kernel<int64_t>, grid, dim3(smp::BLOCK), 0, s, h->st(), h->counter(), p, h->k, row_draws,
                               first, world_draws, static_cast<int64_t *>(out));
            h->last_kernel = "cge::smp::cge_sample_index_kernel<long>";
        } else {
            return h->fail(CGE_ERR_INVALID_ARG, "cge_sampler_sample: INDEX writes int32 or int64");
        }
        CGE_TRY(h, hipGetLastError());
        return CGE_OK;
    }
    const double *lo = p, *hi = p + h->k;
    if (out_dtype == CGE_DTYPE_FLOAT32) {
        hipLaunchKernelGGL((smp::cge_sample_uniform_kernel<float, false>), grid, dim3(smp::BLOCK), 0, s, h->st(), h->counter(), lo, hi, h->k,
                           row_draws, first, world_draws, static_cast<float *>(out));
        h->last_kernel = "cge::smp::cge_sample_uniform_kernel<float, false>";
    } else if (out_dtype == CGE_DTYPE_INT8 || out_dtype == CGE_DTYPE_INT32) {
        const double lim = out_dtype == CGE_DTYPE_INT8 ? 128.0 : 2147483648.0;
        if (!h->integral || h->pmin < -lim || h->pmax > lim - 1.0)
            return h->fail(CGE_ERR_INVALID_ARG, "cge_sampler_sample: integer Box bounds must be whole numbers within the output type");
        if (out_dtype == CGE_DTYPE_INT8) {
            hipLaunchKernelGGL((smp::cge_sample_uniform_kernel<int8_t, true>), grid, dim3(smp::BLOCK), 0, s, h->st(), h->counter(), lo, hi, h->k,
                               row_draws, first, world_draws, static_cast<int8_t *>(out));
            h->last_kernel = "cge::smp::cge_sample_uniform_kernel<signed char, true>";
        } else {
            hipLaunchKernelGGL((smp::cge_sample_uniform_kernel<int32_t, true>), grid, dim3(smp::BLOCK), 0, s, h->st(), h->counter(), lo, hi, h->k,
                               row_draws, first, world_draws, static_cast<int32_t *>(out));
            h->last_kernel = "cge::smp::cge_sample_uniform_kernel<int, true>";
        }
    } else {
        return h->fail(CGE_ERR_INVALID_ARG, "cge_sampler_sample: UNIFORM writes float32, int8 or int32");
    }
    CGE_TRY(h, hipGetLastError());
    return CGE_OK;
}

size_t cge_sampler_device_bytes(const cge_sampler *h) { return h ? h->device_bytes : 0; }

const char *cge_sampler_last_error(const cge_sampler *h) { return h ? h->last_error.c_str() : "null handle"; }

const char *cge_sampler_last_kernel(const cge_sampler *h) { return h ? h->last_kernel.c_str() : ""; }

}  // extern "C"
