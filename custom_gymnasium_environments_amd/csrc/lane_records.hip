// lane_records.hip — canonical per-env state records of the four record-lane types (airline, emergency, space station, farm) for
// MI355X (gfx950): the kernels that pack the handle's columns and generator blocks into records and unpack them again, the check
// that stands between a caller's bytes and the step kernels, and the host side of cge_records_<env>_* (include/cge_amd.h has the
// layout; cge_lane.hpp the view a handle gives of itself).
//
// A record is int32[8] header | REC_WORDS body words (padded to 16 bytes) | 624 words per stream.  The handle holds the same data as
// columns [word][env] and as one 640-word block per env and stream whose words are twisted in place: some of the next generation
// ahead of the cursor (mt_make_ready), the rest of the current one not yet (MtStream).
//
// Mapping: one wave per workgroup; a tile of 64 consecutive envs has one workgroup for its bodies and eight for its generator blocks
// (eight envs each: with all sixty-four behind one another in one wave, pack took five times a copy of the same bytes at 131,072 envs).
//   body       columns -> records through an LDS tile of 64 envs x 64 words: a lane loads its env's words, consecutive lanes on
//              consecutive envs (a 256-byte run per instruction), and parks them four at a time as its row of the tile; the store pass
//              takes 16-byte pieces with consecutive lanes on consecutive pieces of a record, sixteen lanes (256 bytes) a record and
//              chunk.  unpack is the same walk backwards.
//   generator  one env at a time by the whole wave, lane l on word l mod 64 of each 64-word run: the block comes into LDS, words of
//              the next generation are taken back and the rest of the current one is twisted there, as mt_export_cpython does on the
//              host, and the 624 words leave as 156 pieces.  Nothing is written back to the handle.
// Airline keeps no ready mark: its kernels twist every word as it is drawn, so a block must hold the words from the cursor on in the
// PREVIOUS generation's form.  unpack un-twists them (the inverse of mt_twist, word by word, in two parallel phases: words 227..623
// depend on twisted words only, words below on what the first phase restored) and takes the low 31 bits of word 0, which a record
// does not carry and the twist of word 623 needs, from the un-twist of word 623.
#include <cstring>
#include <string>

#include "cge_lane.hpp"
#include "airline_env.hpp"
#include "emergency_env.hpp"
#include "space_station_env.hpp"
#include "farm_env.hpp"

namespace cge {
namespace records {

constexpr int HEADER_WORDS = 8, STREAM_WORDS = MT_N;
constexpr uint32_t TAG = 0x4c520100u;                               // 'L' 'R', version 1, type in the low byte

// what the kernels know of a type: T is its LANE_RECORDS_* number (never its name: the types' namespaces stay their kernels' own)
template <int T> struct Type;
template <> struct Type<LANE_RECORDS_AIRLINE> {
    static constexpr int words = airline::REC_WORDS, streams = 1, cursor = airline::RECORD_CURSOR_FIRST;
    static constexpr bool ready_mark = false;
    template <class G> static __host__ __device__ int refusal(G get) { return airline::record_refusal(get); }
    static const char *text(int c) { return airline::record_refusal_text(c); }
};
template <> struct Type<LANE_RECORDS_EMERGENCY> {
    static constexpr int words = emergency::REC_WORDS, streams = 1, cursor = emergency::RECORD_CURSOR_FIRST;
    static constexpr bool ready_mark = true;
    template <class G> static __host__ __device__ int refusal(G get) { return emergency::record_refusal(get); }
    static const char *text(int c) { return emergency::record_refusal_text(c); }
};
template <> struct Type<LANE_RECORDS_STATION> {
    static constexpr int words = station::REC_WORDS, streams = 1, cursor = station::RECORD_CURSOR_FIRST;
    static constexpr bool ready_mark = true;
    template <class G> static __host__ __device__ int refusal(G get) { return station::record_refusal(get); }
    static const char *text(int c) { return station::record_refusal_text(c); }
};
template <> struct Type<LANE_RECORDS_FARM> {                          // streams: NumPy legacy (`mt`), CPython (`py`)
    static constexpr int words = farm::REC_WORDS, streams = 2, cursor = farm::RECORD_CURSOR_FIRST;
    static constexpr bool ready_mark = true;
    template <class G> static __host__ __device__ int refusal(G get) { return farm::record_refusal(get); }
    static const char *text(int c) { return farm::record_refusal_text(c); }
};
static_assert(airline::RECORD_CURSOR_WORDS == 1 && emergency::RECORD_CURSOR_WORDS == 2 && station::RECORD_CURSOR_WORDS == 2 && farm::RECORD_CURSOR_WORDS == 4,
              "one cursor word a stream, and a ready mark behind it where the type keeps one");

template <class Y>
struct Layout {
    static constexpr int cursor_words = Y::streams * (Y::ready_mark ? 2 : 1);
    static constexpr int body_words = (Y::words + 3) / 4 * 4;       // padded to 16 bytes
    static constexpr int front_words = HEADER_WORDS + body_words;   // header and body: what the tile carries
    static constexpr int record_words = front_words + Y::streams * STREAM_WORDS;
    static_assert(record_words % 4 == 0 && STREAM_WORDS % 4 == 0, "every section is whole 16-byte pieces");
    // the cursor (and ready mark) of stream s sit at body words pos(s) (and pos(s) + 1)
    static __host__ __device__ constexpr int pos(int s) { return Y::cursor + s * (Y::ready_mark ? 2 : 1); }
    static __host__ __device__ constexpr bool is_cursor(int w) { return w >= Y::cursor && w < Y::cursor + cursor_words; }
};
static_assert(Layout<Type<LANE_RECORDS_AIRLINE>>::record_words * 4 == 4192 && Layout<Type<LANE_RECORDS_EMERGENCY>>::record_words * 4 == 3344 &&
              Layout<Type<LANE_RECORDS_STATION>>::record_words * 4 == 3280 && Layout<Type<LANE_RECORDS_FARM>>::record_words * 4 == 5856, "cge_amd.h");

enum { REASON_TAG = 1, REASON_WORDS, REASON_STREAMS, REASON_INDEX, REASON_CURSOR, REASON_PADDING, REASON_HEADER };   // 16 and above: the type's own
static const char *reason_text(int c) {
    switch (c) {
        case REASON_TAG: return "not a record of this env type (format tag)";
        case REASON_WORDS: return "wrong number of record words";
        case REASON_STREAMS: return "wrong number of generator streams";
        case REASON_INDEX: return "a stream index outside 0..624";
        case REASON_CURSOR: return "a cursor word of the body is not zero";
        case REASON_PADDING: return "a padding byte is not zero";
        case REASON_HEADER: return "a reserved header word is not zero";
    }
    return nullptr;
}

struct Args {
    uint32_t *state;              // columns [word][n]
    uint32_t *mt[2];              // blocks of MT_STRIDE words per env
    int64_t n, first, count;      // envs of the handle; the range [first, first + count) <-> records 0..count-1
    uint32_t *rec;
};

constexpr int BLOCK = 64, TILE_WORDS = 64, TILE_STRIDE = TILE_WORDS + 4;   // rows stay 16-byte aligned; +4 words spreads the rows over the banks
constexpr uint32_t MAGIC = 0x9908b0dfu, UPPER = 0x80000000u, LOWER = 0x7fffffffu;
constexpr int PASS = 192;                                          // words twisted together: below 227, so none reads another's result
static_assert(PASS <= MT_N - MT_M && PASS % BLOCK == 0, "a pass of the twist is mutually independent words, whole runs");
static_assert(MT_EXPORT_MAX_AHEAD == (uint32_t)(MT_N - MT_M), "the un-twist of word k reads word k + 397 of the current generation");

// the reference's index of a device cursor (mt_export_cpython): a cursor at 0 without a whole generation ready stands at the end of
// the generation the block holds
__device__ __forceinline__ uint32_t index_of(uint32_t pos, uint32_t ready) { return pos == 0u && ready < (uint32_t)MT_N ? (uint32_t)MT_N : pos; }
// y of mt_twist from g = new ^ word 397 ahead: bit 31 of g is y's bit 0
__device__ __forceinline__ uint32_t untwist(uint32_t g) {
    const uint32_t odd = g >> 31;
    return ((g ^ (odd ? MAGIC : 0u)) << 1) | odd;
}

// One env's block -> 624 words of one generation at `out` (16-byte aligned), by the whole wave.  b: 640 words, y: 256 words of LDS.
__device__ __forceinline__ void export_stream(const uint32_t *__restrict__ blk, uint32_t pos, uint32_t ready, uint32_t *b, uint32_t *y,
                                              uint32_t *__restrict__ out) {
    const uint32_t lane = threadIdx.x;
    for (uint32_t k = lane; k < (uint32_t)MT_N; k += BLOCK) b[k] = blk[k];
    pos = pos < (uint32_t)MT_N ? pos : (uint32_t)MT_N - 1u;         // a handle's cursors are in range; an index into LDS is made to be
    if (pos == 0u && ready > 0u && ready < (uint32_t)MT_N) { pos = MT_N; ready += MT_N; }   // just wrapped: seen from the old generation's end
    __syncthreads();
    if (ready > (uint32_t)MT_N) {                                   // words [0, ahead) are the next generation's: take them back
        uint32_t ahead = ready - (uint32_t)MT_N;
        ahead = ahead < MT_EXPORT_MAX_AHEAD ? ahead : MT_EXPORT_MAX_AHEAD;
        for (uint32_t k = lane; k < ahead; k += BLOCK) y[k] = untwist(b[k] ^ b[k + MT_M]);
        __syncthreads();
        for (uint32_t k = lane; k <= ahead; k += BLOCK) {
            const uint32_t upper = k < ahead ? y[k] & UPPER : b[k] & UPPER, lower = k ? y[k - 1u] & LOWER : 0u;
            b[k] = upper | lower;
        }
        ready = MT_N;
        __syncthreads();
    }
    if (ready < (uint32_t)MT_N && !(pos == 0u && ready == 0u)) {    // twist what is left of the generation, PASS words at a time
        for (uint32_t s = ready > pos ? ready : pos; s < (uint32_t)MT_N; s += PASS) {
            uint32_t v[PASS / BLOCK];
#pragma unroll
            for (int j = 0; j < PASS / BLOCK; ++j) {
                const uint32_t k = s + lane + (uint32_t)(BLOCK * j);
                if (k < (uint32_t)MT_N) {
                    const uint32_t k1 = k + 1u == (uint32_t)MT_N ? 0u : k + 1u, km = k + MT_M >= (uint32_t)MT_N ? k + MT_M - MT_N : k + MT_M;
                    v[j] = mt_twist(b[k], b[k1], b[km]);
                }
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < PASS / BLOCK; ++j) {
                const uint32_t k = s + lane + (uint32_t)(BLOCK * j);
                if (k < (uint32_t)MT_N) b[k] = v[j];
            }
            __syncthreads();
        }
    }
    for (uint32_t q = lane; q < (uint32_t)MT_N / 4u; q += BLOCK) {
        uint4 v = *reinterpret_cast<const uint4 *>(b + 4u * q);
        if (q == 0u) v.x &= UPPER;                                  // no future output depends on the low 31 bits of word 0: a record never carries them
        *reinterpret_cast<uint4 *>(out + 4u * q) = v;
    }
    __syncthreads();
}

// 624 words and an index -> one env's block with its mirror words, by the whole wave.  UNTWIST (airline): the words from the index on
// go back to the previous generation's form.
template <bool UNTWIST>
__device__ __forceinline__ void import_stream(const uint32_t *__restrict__ in, uint32_t index, uint32_t *b, uint32_t *y, uint32_t *__restrict__ blk) {
    const uint32_t lane = threadIdx.x;
    for (uint32_t q = lane; q < (uint32_t)MT_N / 4u; q += BLOCK) *reinterpret_cast<uint4 *>(b + 4u * q) = *reinterpret_cast<const uint4 *>(in + 4u * q);
    __syncthreads();
    if (UNTWIST && index < (uint32_t)MT_N) {
        constexpr uint32_t SPLIT = MT_N - MT_M;                     // 227: word k >= 227 was twisted from twisted word k - 227
        const uint32_t lo = index ? index - 1u : 0u;                // y[index - 1] holds the low bits of word `index`
        // the low 31 bits of twisted word 0, which the record does not carry: word 623 was twisted with them, and the un-twists of
        // words 0 and 227 below read them
        if (lane == 0u) b[0] = (b[0] & UPPER) | (untwist(b[MT_N - 1] ^ b[MT_M - 1]) & LOWER);
        __syncthreads();
        for (uint32_t k = (lo > SPLIT ? lo : SPLIT) + lane; k < (uint32_t)MT_N; k += BLOCK) y[k] = untwist(b[k] ^ b[k - SPLIT]);
        __syncthreads();
        for (uint32_t k = (index > SPLIT + 1u ? index : SPLIT + 1u) + lane; k < (uint32_t)MT_N; k += BLOCK) b[k] = (y[k] & UPPER) | (y[k - 1u] & LOWER);
        __syncthreads();
        for (uint32_t k = lo + lane; k < SPLIT; k += BLOCK) y[k] = untwist(b[k] ^ b[k + MT_M]);   // b[k + 397]: restored above
        __syncthreads();
        for (uint32_t k = index + lane; k <= SPLIT; k += BLOCK) b[k] = (y[k] & UPPER) | (k ? y[k - 1u] & LOWER : 0u);
        __syncthreads();
    }
    for (uint32_t k = lane; k < (uint32_t)MT_N; k += BLOCK) blk[k] = b[k];
    if (lane < (uint32_t)MT_PAD) blk[MT_N + lane] = b[lane];
    __syncthreads();
}

// A workgroup is either the body's (blockIdx.y == 0: the tile) or one of STREAM_PARTS that share the tile's generator blocks among them
// (b and y, in the same LDS): eight envs each, so that the serial walk over a tile's envs is eight long and not sixty-four.
constexpr int STREAM_PARTS = 8, PART_ENVS = BLOCK / STREAM_PARTS;
static_assert(2 * MT_STRIDE <= BLOCK * TILE_STRIDE, "b and y fit where the tile is");
#define CGE_RECORDS_LDS                                                   \
    __shared__ __attribute__((aligned(16))) uint32_t s_tile[BLOCK * TILE_STRIDE]; \
    uint32_t *const s_b = s_tile, *const s_y = s_tile + MT_STRIDE;

template <int T>
__global__ __launch_bounds__(BLOCK) void pack_kernel(Args a) {
    using Y = Type<T>;
    using L = Layout<Y>;
    CGE_RECORDS_LDS
    const int lane = (int)threadIdx.x;
    const int64_t j0 = (int64_t)blockIdx.x * BLOCK, left = a.count - j0;
    const int live_n = left < BLOCK ? (int)left : BLOCK;            // records of this tile
    const bool live = lane < live_n;
    const int64_t env = a.first + j0 + (live ? lane : 0);
    const uint32_t *col = a.state + env;                            // word w of this lane's env: col[w * n]
    uint32_t index[2] = {0u, 0u};
#pragma unroll
    for (int s = 0; s < Y::streams; ++s) index[s] = index_of(col[(int64_t)L::pos(s) * a.n], Y::ready_mark ? col[(int64_t)(L::pos(s) + 1) * a.n] : 0u);
    uint32_t *out = a.rec + j0 * L::record_words;
    for (int c0 = 0; blockIdx.y == 0 && c0 < L::front_words; c0 += TILE_WORDS) {
        const int nw = L::front_words - c0 < TILE_WORDS ? L::front_words - c0 : TILE_WORDS;   // a multiple of 4
        for (int q = 0; q < nw; q += 4) {
            uint32_t v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int r = c0 + q + k, w = r - HEADER_WORDS;     // uniform over the wave
                v[k] = r == 0 ? TAG | (uint32_t)T : r == 1 ? (uint32_t)Y::words : r == 2 ? (uint32_t)Y::streams : r == 3 ? index[0]
                       : r == 4 && Y::streams > 1 ? index[1] : w < 0 || w >= Y::words || L::is_cursor(w) ? 0u : col[(int64_t)w * a.n];
            }
            *reinterpret_cast<uint4 *>(s_tile + lane * TILE_STRIDE + q) = make_uint4(v[0], v[1], v[2], v[3]);
        }
        __syncthreads();
        const int per = nw / 4;                                     // pieces a record in this chunk
        for (int p = lane; p < live_n * per; p += BLOCK) {
            const int r = p / per, pc = p - r * per;
            *reinterpret_cast<uint4 *>(out + (int64_t)r * L::record_words + c0 + 4 * pc) = *reinterpret_cast<const uint4 *>(s_tile + r * TILE_STRIDE + 4 * pc);
        }
        __syncthreads();
    }
    if (blockIdx.y == 0) return;
    const int r0 = ((int)blockIdx.y - 1) * PART_ENVS, r1 = r0 + PART_ENVS < live_n ? r0 + PART_ENVS : live_n;
    for (int r = r0; r < r1; ++r) {
        const int64_t e = a.first + j0 + r;
#pragma unroll
        for (int s = 0; s < Y::streams; ++s) {
            const uint32_t pos = a.state[(int64_t)L::pos(s) * a.n + e], ready = Y::ready_mark ? a.state[(int64_t)(L::pos(s) + 1) * a.n + e] : 0u;
            export_stream(a.mt[s] + e * MT_STRIDE, pos, ready, s_b, s_y, out + (int64_t)r * L::record_words + L::front_words + s * STREAM_WORDS);
        }
    }
}

// status: {(lowest refused record << 8 | reason) as uint64, initialised to all ones; unused}
template <int T>
__global__ __launch_bounds__(256) void check_kernel(Args a, unsigned long long *status) {
    using Y = Type<T>;
    using L = Layout<Y>;
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= a.count) return;
    const uint32_t *r = a.rec + j * L::record_words;
    int why = 0;
    if (r[0] != (TAG | (uint32_t)T)) why = REASON_TAG;
    else if (r[1] != (uint32_t)Y::words) why = REASON_WORDS;
    else if (r[2] != (uint32_t)Y::streams) why = REASON_STREAMS;
    else if (r[3] > (uint32_t)MT_N || (Y::streams > 1 && r[4] > (uint32_t)MT_N)) why = REASON_INDEX;
    else if ((Y::streams > 1 ? 0u : r[4]) | r[5] | r[6] | r[7]) why = REASON_HEADER;
    if (!why) {
        for (int w = Y::cursor; w < Y::cursor + L::cursor_words; ++w)
            if (r[HEADER_WORDS + w]) why = REASON_CURSOR;
    }
    if (!why) {
        for (int w = Y::words; w < L::body_words; ++w)
            if (r[HEADER_WORDS + w]) why = REASON_PADDING;
    }
    if (!why) why = Y::refusal([&](int w) { return r[HEADER_WORDS + w]; });
    if (why) atomicMin(status, (unsigned long long)j << 8 | (unsigned long long)why);
}

template <int T>
__global__ __launch_bounds__(BLOCK) void unpack_kernel(Args a) {
    using Y = Type<T>;
    using L = Layout<Y>;
    CGE_RECORDS_LDS
    const int lane = (int)threadIdx.x;
    const int64_t j0 = (int64_t)blockIdx.x * BLOCK, left = a.count - j0;
    const int live_n = left < BLOCK ? (int)left : BLOCK;
    const bool live = lane < live_n;
    const int64_t env = a.first + j0 + (live ? lane : 0);
    uint32_t *col = a.state + env;
    const uint32_t *in = a.rec + j0 * L::record_words;
    uint32_t index[2] = {0u, 0u};
    for (int c0 = 0; blockIdx.y == 0 && c0 < L::front_words; c0 += TILE_WORDS) {
        const int nw = L::front_words - c0 < TILE_WORDS ? L::front_words - c0 : TILE_WORDS;
        const int per = nw / 4;
        for (int p = lane; p < live_n * per; p += BLOCK) {
            const int r = p / per, pc = p - r * per;
            *reinterpret_cast<uint4 *>(s_tile + r * TILE_STRIDE + 4 * pc) = *reinterpret_cast<const uint4 *>(in + (int64_t)r * L::record_words + c0 + 4 * pc);
        }
        __syncthreads();
        if (live) {
            const uint32_t *row = s_tile + lane * TILE_STRIDE;
            if (c0 == 0) { index[0] = row[3]; index[1] = row[4]; }   // the header is in the first chunk, every cursor word behind it
            for (int q = 0; q < nw; ++q) {
                const int w = c0 + q - HEADER_WORDS;
                if (w < 0 || w >= Y::words) continue;
                uint32_t v = row[q];
                if (L::is_cursor(w)) {                              // mt_import_cpython: the whole generation is ready; index 624 regenerates
                    const int k = w - Y::cursor, s = Y::ready_mark ? k / 2 : k;
                    const bool fresh = index[s] >= (uint32_t)MT_N;
                    v = Y::ready_mark && (k & 1) ? (fresh ? 0u : (uint32_t)MT_N) : (fresh ? 0u : index[s]);
                }
                col[(int64_t)w * a.n] = v;
            }
        }
        __syncthreads();
    }
    static_assert(HEADER_WORDS + Y::cursor >= 5, "the cursor words come after the header's indices");
    if (blockIdx.y == 0) return;
    const int r0 = ((int)blockIdx.y - 1) * PART_ENVS, r1 = r0 + PART_ENVS < live_n ? r0 + PART_ENVS : live_n;
    for (int r = r0; r < r1; ++r) {
        const int64_t e = a.first + j0 + r;
        const uint32_t *rec = in + (int64_t)r * L::record_words;
#pragma unroll
        for (int s = 0; s < Y::streams; ++s) import_stream<!Y::ready_mark>(rec + L::front_words + s * STREAM_WORDS, rec[3 + s], s_b, s_y, a.mt[s] + e * MT_STRIDE);
    }
}

// ------------------------------------------------------------------------------------------------------------------ host
template <class F>
static auto for_type(int type, F &&f) {
    switch (type) {
        case LANE_RECORDS_AIRLINE: return f(std::integral_constant<int, LANE_RECORDS_AIRLINE>{});
        case LANE_RECORDS_EMERGENCY: return f(std::integral_constant<int, LANE_RECORDS_EMERGENCY>{});
        case LANE_RECORDS_STATION: return f(std::integral_constant<int, LANE_RECORDS_STATION>{});
        default: return f(std::integral_constant<int, LANE_RECORDS_FARM>{});
    }
}

static int fail(const LaneRecords &v, int status, const char *fn, const char *what, hipError_t e = hipSuccess) {
    return v.h->fail(status, (std::string(v.abi) + "_" + fn + ": " + what).c_str(), e);
}
#define CGE_RECORDS_TRY(v, fn, expr)                                        \
    do {                                                                    \
        hipError_t _e = (expr);                                             \
        if (_e != hipSuccess) return fail(v, CGE_ERR_HIP, fn, #expr, _e);   \
    } while (0)

static Args args_of(const LaneRecords &v, int64_t first, int64_t count, const void *rec) {
    return Args{v.state, {v.mt[0], v.mt[1]}, v.h->n, first, count, static_cast<uint32_t *>(const_cast<void *>(rec))};
}
static int range_check(const LaneRecords &v, const char *fn, int64_t first, int64_t count, const void *dev) {
    if (first < 0 || count < 0 || first > v.h->n || count > v.h->n - first) return fail(v, CGE_ERR_INVALID_ARG, fn, "the range [first, first + count) must lie within [0, n_envs]");
    if (!dev) return fail(v, CGE_ERR_INVALID_ARG, fn, "null records pointer");
    if (reinterpret_cast<uintptr_t>(dev) & 15u) return fail(v, CGE_ERR_INVALID_ARG, fn, "the records must be 16-byte aligned");
    return CGE_OK;
}
static unsigned tiles(int64_t count) { return (unsigned)((count + BLOCK - 1) / BLOCK); }

static void launch_pack(const LaneRecords &v, const Args &a, hipStream_t s) {
    for_type(v.type, [&](auto t) { hipLaunchKernelGGL(pack_kernel<decltype(t)::value>, dim3(tiles(a.count), 1 + STREAM_PARTS), dim3(BLOCK), 0, s, a); return 0; });
}
static void launch_unpack(const LaneRecords &v, const Args &a, hipStream_t s) {
    for_type(v.type, [&](auto t) { hipLaunchKernelGGL(unpack_kernel<decltype(t)::value>, dim3(tiles(a.count), 1 + STREAM_PARTS), dim3(BLOCK), 0, s, a); return 0; });
}
// the transient status block of a check: allocated and freed inside the call
struct Status {
    unsigned long long *dev = nullptr;
    ~Status() { if (dev) (void)hipFree(dev); }
    hipError_t init() { return hipMalloc(&dev, 16); }
};
// runs the check over `count` records at a.rec, waits for the stream; CGE_OK, or the refusal of record `base` + j as the call's error
static int checked(const LaneRecords &v, const char *fn, const Args &a, Status &st, int64_t base, hipStream_t s) {
    CGE_RECORDS_TRY(v, fn, hipMemsetAsync(st.dev, 0xff, 16, s));
    for_type(v.type, [&](auto t) { hipLaunchKernelGGL(check_kernel<decltype(t)::value>, dim3(grid256(a.count)), dim3(256), 0, s, a, st.dev); return 0; });
    CGE_RECORDS_TRY(v, fn, hipGetLastError());
    unsigned long long word = 0;
    CGE_RECORDS_TRY(v, fn, hipMemcpyAsync(&word, st.dev, sizeof word, hipMemcpyDeviceToHost, s));
    CGE_RECORDS_TRY(v, fn, hipStreamSynchronize(s));
    if (word == ~0ull) return CGE_OK;
    const int why = (int)(word & 255u);
    const char *text = reason_text(why);
    if (!text) text = for_type(v.type, [&](auto t) { return Type<decltype(t)::value>::text(why); });
    char msg[256];
    snprintf(msg, sizeof msg, "env %lld: %s", (long long)(base + (int64_t)(word >> 8)), text);
    return fail(v, CGE_ERR_INVALID_ARG, fn, msg);
}

}  // namespace records

using namespace records;

size_t lane_records_bytes(int type) {
    return for_type(type, [](auto t) { return (size_t)Layout<Type<decltype(t)::value>>::record_words * 4u; });
}

int lane_records_pack(const LaneRecords &v, int64_t first, int64_t count, void *dev_records, hipStream_t s) {
    if (int st = range_check(v, "pack", first, count, dev_records)) return st;
    if (count == 0) return CGE_OK;
    DeviceGuard g(v.h->device);
    launch_pack(v, args_of(v, first, count, dev_records), s);
    CGE_RECORDS_TRY(v, "pack", hipGetLastError());
    CGE_RECORDS_TRY(v, "pack", hipStreamSynchronize(s));
    return CGE_OK;
}

int lane_records_unpack(const LaneRecords &v, int64_t first, int64_t count, const void *dev_records, hipStream_t s) {
    if (int st = range_check(v, "unpack", first, count, dev_records)) return st;
    if (count == 0) return CGE_OK;
    DeviceGuard g(v.h->device);
    Status status;
    CGE_RECORDS_TRY(v, "unpack", status.init());
    const Args a = args_of(v, first, count, dev_records);
    if (int st = checked(v, "unpack", a, status, first, s)) return st;   // before anything is written
    launch_unpack(v, a, s);
    CGE_RECORDS_TRY(v, "unpack", hipGetLastError());
    CGE_RECORDS_TRY(v, "unpack", hipStreamSynchronize(s));
    return CGE_OK;
}

// the host forms: rounds of STATE_CHUNK envs through a device staging buffer of one round, one copy a round
namespace records {
struct Staging {
    void *dev = nullptr;
    ~Staging() { if (dev) (void)hipFree(dev); }
    hipError_t init(size_t bytes) { return hipMalloc(&dev, bytes); }
};
}  // namespace records

int lane_records_get(const LaneRecords &v, void *host_buf, hipStream_t s) {
    if (!host_buf) return fail(v, CGE_ERR_INVALID_ARG, "get_state", "null buffer");
    DeviceGuard g(v.h->device);
    const size_t rec = lane_records_bytes(v.type);
    const int64_t n = v.h->n, cap = n < STATE_CHUNK ? n : STATE_CHUNK;
    Staging stage;
    CGE_RECORDS_TRY(v, "get_state", stage.init((size_t)cap * rec));
    for (int64_t c0 = 0; c0 < n; c0 += cap) {
        const int64_t m = n - c0 < cap ? n - c0 : cap;
        launch_pack(v, args_of(v, c0, m, stage.dev), s);
        CGE_RECORDS_TRY(v, "get_state", hipGetLastError());
        CGE_RECORDS_TRY(v, "get_state", hipMemcpyAsync(static_cast<char *>(host_buf) + (size_t)c0 * rec, stage.dev, (size_t)m * rec, hipMemcpyDeviceToHost, s));
        CGE_RECORDS_TRY(v, "get_state", hipStreamSynchronize(s));     // the staging buffer is the next round's
    }
    return CGE_OK;
}

// every round is checked before any is unpacked: a refused buffer leaves every env as it was
int lane_records_set(const LaneRecords &v, const void *host_buf, hipStream_t s) {
    if (!host_buf) return fail(v, CGE_ERR_INVALID_ARG, "set_state", "null buffer");
    DeviceGuard g(v.h->device);
    const size_t rec = lane_records_bytes(v.type);
    const int64_t n = v.h->n, cap = n < STATE_CHUNK ? n : STATE_CHUNK;
    Staging stage;
    Status status;
    CGE_RECORDS_TRY(v, "set_state", stage.init((size_t)cap * rec));
    CGE_RECORDS_TRY(v, "set_state", status.init());
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1 && n <= cap) {                                 // one round: it is checked and still staged
            launch_unpack(v, args_of(v, 0, n, stage.dev), s);
            CGE_RECORDS_TRY(v, "set_state", hipGetLastError());
            break;
        }
        for (int64_t c0 = 0; c0 < n; c0 += cap) {
            const int64_t m = n - c0 < cap ? n - c0 : cap;
            CGE_RECORDS_TRY(v, "set_state", hipMemcpyAsync(stage.dev, static_cast<const char *>(host_buf) + (size_t)c0 * rec, (size_t)m * rec, hipMemcpyHostToDevice, s));
            const Args a = args_of(v, c0, m, stage.dev);
            if (pass == 0) {
                if (int st = checked(v, "set_state", a, status, c0, s)) return st;
            } else {
                launch_unpack(v, a, s);
                CGE_RECORDS_TRY(v, "set_state", hipGetLastError());
                CGE_RECORDS_TRY(v, "set_state", hipStreamSynchronize(s));
            }
        }
    }
    CGE_RECORDS_TRY(v, "set_state", hipStreamSynchronize(s));
    return CGE_OK;
}

}  // namespace cge
