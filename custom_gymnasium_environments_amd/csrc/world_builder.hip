// world_builder.hip — batched WorldBuilderEnv for MI355X (gfx950): kernels + C ABI (include/cge_amd.h).
//
// Re-expresses the reference's world_builder_env/src/environment/ for N independent instances, one lane per env:
//   world_builder_env.py  __init__ :39-97, reset :99-121, step :123-166, _get_observation :186-216, _get_info :218-232,
//                         _check_termination :234-248
//   game_logic.py         reset :31-54, execute_action :56-116, _try_build :118-150, costs :15-20, production :164-174,
//                         consumption :176-183, growth :185-194
//
// State per env: five uint4 columns (SoA) + one int32 — the grid as 100 nibbles (13 words), food / wood / stone as int32, one word
// of counts and flags, one of population + the MT19937 cursor and its ready mark, steps, win_steps; and the running episode's
// return.  The record lives in VGPRs for a whole launch; the occupancy mask (2 x 64 bits) is derived from the nibbles on load and
// kept current, so "the idx-th empty cell in row-major order" is two popcounts and a six-step halving, no scan.
//
// Draws: only a successful build draws — NumPy-legacy randint(n) over the n empty cells: n == 1 takes no word, otherwise words are
// masked to the smallest 2^b - 1 >= n - 1 and rejected above n - 1 (no bound on the rejections).  The lanes of a wave that draw
// twist their 32-word chunks ahead together (mt_make_ready), take DRAW_WINDOW ready words and go round again while any of them has
// rejected its whole window; a wave in which no lane builds skips all of it by ballot.  A window never reaches past word 623, so
// the ready mark never enters the next generation and the state export (mt_export_cpython) is exact at every cursor with no
// saved word.
//
// Observations, one wave = one workgroup = 64 consecutive envs whose rows are ONE contiguous run in HBM in both layouts:
//   Dict  a uint8 slab of key-major planes (grid int8 [N, G, G] | resources f32 [N, 4] | population_capacity f32 [N, 1] |
//         win_steps i32 [N, 1], each plane starting at a multiple of 16 bytes).  The grid rows are staged as bytes in the wave's LDS tile
//         and streamed out as 16-byte pieces; the three small planes are coalesced stores straight from registers.
//   FLAT  float32 [N, G*G + 6] rows (the reference's flatten_obs=True): the same byte tile plus six staged floats per env, streamed
//         as consecutive dwords (256 contiguous bytes per store instruction).  Dword stores on purpose: with an odd N the rows of a
//         trajectory step start at 4-byte-aligned addresses only, which the 16-byte form of stream_image does not take.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "cge_lane.hpp"

namespace cge {
namespace wb {

constexpr int BLOCK = 64;              // one wave per workgroup: the LDS tile is the wave's own
constexpr int DRAW_WINDOW = 4;         // ready words a drawing lane takes per round of the rejection loop
constexpr int GW = 13;                 // grid words: 8 nibbles each, 100 cells at most
constexpr int COLS = 5;
constexpr int MAX_RS = 25;             // dwords per env in the LDS byte tile (100 cells)
constexpr int NEXTRA = 6;              // food, wood, stone, population, population_capacity, win_steps
constexpr uint32_t MAX_POPULATION = 20, WIN_STEPS = 50;   // world_builder_env.py:45-46

struct Params : LaneParams<void> {     // obs_step_stride in elements of the layout: bytes (Dict) or floats (FLAT)
    int32_t *ret;
    int32_t G, GG, W, RS;              // grid size, cells, floats per flat row, dwords per env in the LDS tile
    uint32_t magic_gg, magic_w;        // ceil(2^32 / GG), ceil(2^32 / W): x / d == umulhi(x, magic) for the x < 2^16 used here
    int64_t off_res, off_cap, off_win; // byte offsets of the Dict slab's planes after the grid
    static constexpr bool terminates = true;   // terminated only: the reference never truncates (world_builder_env.py:150)
};
static_assert(std::is_trivially_copyable<Params>::value, "a kernel argument");
// rollout_rows_kernel's: the other kernels' arguments stay as they are.  Dict: fin.rows is the observation slab of R = n_segments *
// fin.cap "envs", its planes at the byte offsets below; row j of segment s is env s * fin.cap + j of it.  FLAT: plain rows [R, W].
struct RowsParams : Params {
    FinalSeg fin;
    int64_t rows_off_res, rows_off_cap, rows_off_win;
};

// bit j = nibble j of w is non-zero
__device__ __forceinline__ uint32_t nonzero_nibbles(uint32_t w) {
    uint32_t x = (w | (w >> 1) | (w >> 2) | (w >> 3)) & 0x11111111u;
    x = (x | (x >> 3)) & 0x03030303u;
    x = (x | (x >> 6)) & 0x000F000Fu;
    return (x | (x >> 12)) & 0xFFu;
}
// four nibbles -> four bytes
__device__ __forceinline__ uint32_t spread4(uint32_t x) { return (x & 0xFu) | ((x & 0xF0u) << 4) | ((x & 0xF00u) << 8) | ((x & 0xF000u) << 12); }

struct Env {
    uint32_t g[GW];                    // cell c (row-major) is nibble c & 7 of g[c >> 3]: 0 empty, 1 farm, 2 lumberyard, 3 quarry, 4 house
    int32_t food, wood, stone, ret;
    uint32_t pop, farm, lumber, quarry, house, steps, win, latch, needs_reset, mt_pos, mt_pretw;
    unsigned long long occ0, occ1;     // occupied cells 0..63 / 64..99 (derived)

    __device__ __forceinline__ uint32_t capacity() const { return 10u + 5u * house; }   // game_logic.py:47, :147-148
    __device__ __forceinline__ void derive() {
        occ0 = 0; occ1 = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) occ0 |= (unsigned long long)nonzero_nibbles(g[k]) << (8 * k);
#pragma unroll
        for (int k = 8; k < GW; ++k) occ1 |= (unsigned long long)nonzero_nibbles(g[k]) << (8 * (k - 8));
    }
    __device__ __forceinline__ void load(const uint4 *__restrict__ s, const int32_t *__restrict__ r, int64_t n, int64_t i) {
        const uint4 a = s[i], b = s[n + i], c = s[2 * n + i], d = s[3 * n + i], f = s[4 * n + i];
        g[0] = a.x; g[1] = a.y; g[2] = a.z; g[3] = a.w; g[4] = b.x; g[5] = b.y; g[6] = b.z; g[7] = b.w;
        g[8] = c.x; g[9] = c.y; g[10] = c.z; g[11] = c.w; g[12] = d.x;
        food = (int32_t)d.y; wood = (int32_t)d.z; stone = (int32_t)d.w;
        farm = f.x & 127u; lumber = (f.x >> 7) & 127u; quarry = (f.x >> 14) & 127u; house = (f.x >> 21) & 127u;
        latch = (f.x >> 28) & 1u; needs_reset = (f.x >> 29) & 1u;
        pop = f.y & 1023u; mt_pos = (f.y >> 10) & 1023u; mt_pretw = mt_ready_decode((f.y >> 20) & 31u);
        steps = f.z; win = f.w;
        ret = r[i];
        derive();
    }
    __device__ __forceinline__ void store(uint4 *__restrict__ s, int32_t *__restrict__ r, int64_t n, int64_t i) const {
        s[i] = make_uint4(g[0], g[1], g[2], g[3]);
        s[n + i] = make_uint4(g[4], g[5], g[6], g[7]);
        s[2 * n + i] = make_uint4(g[8], g[9], g[10], g[11]);
        s[3 * n + i] = make_uint4(g[12], (uint32_t)food, (uint32_t)wood, (uint32_t)stone);
        s[4 * n + i] = make_uint4(farm | (lumber << 7) | (quarry << 14) | (house << 21) | (latch << 28) | (needs_reset << 29),
                                  pop | (mt_pos << 10) | ((mt_pretw > mt_pos ? mt_ready_encode(mt_pretw) : 0u) << 20), steps, win);
        r[i] = ret;
    }
    __device__ __forceinline__ void clear() {                       // game_logic.py:31-54, world_builder_env.py:111-117; draws nothing
#pragma unroll
        for (int k = 0; k < GW; ++k) g[k] = 0;
        occ0 = 0; occ1 = 0;
        food = 25; wood = 20; stone = 10; pop = 3;
        farm = 0; lumber = 0; quarry = 0; house = 0; steps = 0; win = 0; latch = 0; needs_reset = 0; ret = 0;
    }
};

// One step (world_builder_env.py:123-166) for the lanes with `go` (a valid action 0..4); call with all lanes of the wave.
// Returns terminated; r = the step's reward.
__device__ __forceinline__ bool env_step(Env &e, uint32_t *__restrict__ blk, int32_t a, bool go, int32_t GG, int32_t &r) {
    r = 0;
    const uint32_t prev_pop = e.pop, prev_cap = e.capacity();
    const bool build = go && a > 0;
    const int32_t cost_w = (a == 1 || a == 3) ? 5 : a == 4 ? 10 : 0, cost_s = a == 2 ? 3 : a == 4 ? 5 : 0;   // game_logic.py:15-20
    const bool afford = build && e.wood >= cost_w && e.stone >= cost_s;                                        // the check comes first (:121)
    const unsigned long long valid0 = GG >= 64 ? ~0ull : (1ull << GG) - 1ull, valid1 = GG > 64 ? (1ull << (GG - 64)) - 1ull : 0ull;
    const unsigned long long e0 = ~e.occ0 & valid0, e1 = ~e.occ1 & valid1;
    const uint32_t c0 = (uint32_t)__popcll(e0), n = c0 + (uint32_t)__popcll(e1);
    const bool ok = afford && n > 0u;                               // no empty cell: the build fails, no draw (:126-127)
    uint32_t idx = 0;
    bool need = ok && n > 1u;                                       // legacy randint(1) returns 0 and consumes no word
    if (__ballot(need)) {
        uint32_t m = n - 1u;
        m |= m >> 1; m |= m >> 2; m |= m >> 4;                      // smallest 2^b - 1 >= n - 1 (n <= 100)
        uint32_t pos = e.mt_pos, pretw = e.mt_pretw;
#pragma unroll 1
        while (__ballot(need)) {
            const bool act = need;
            const uint32_t room = (uint32_t)MT_N - pos, avail = room < (uint32_t)DRAW_WINDOW ? room : (uint32_t)DRAW_WINDOW;
            mt_make_ready(blk, pos, pretw, avail, act);             // never past word 623: the ready mark stays inside the generation
            uint32_t w[DRAW_WINDOW];
#pragma unroll
            for (int j = 0; j < DRAW_WINDOW; ++j) w[j] = 0;
            if (act) mt_load_ready<DRAW_WINDOW>(blk, pos, w);
            uint32_t used = 0;
#pragma unroll
            for (int j = 0; j < DRAW_WINDOW; ++j) {
                if (need && (uint32_t)j < avail) {
                    const uint32_t v = mt_temper(w[j]) & m;
                    used += 1;
                    if (v <= n - 1u) { idx = v; need = false; }
                }
            }
            if (act) mt_advance(pos, pretw, used);
        }
        e.mt_pos = pos; e.mt_pretw = pretw;
    }
    if (ok) {                                                       // the idx-th zero of the grid in row-major order (:130-131)
        unsigned long long word = e0;
        uint32_t cell = 0;
        if (idx >= c0) { idx -= c0; word = e1; cell = 64; }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            const uint32_t c = (uint32_t)__popcll(word & ((1ull << s) - 1ull));
            if (idx >= c) { idx -= c; word >>= s; cell += (uint32_t)s; }
        }
        const uint32_t nib = (uint32_t)a << (4u * (cell & 7u));
#pragma unroll
        for (int k = 0; k < GW; ++k) e.g[k] |= (cell >> 3) == (uint32_t)k ? nib : 0u;
        if (cell < 64u) e.occ0 |= 1ull << cell; else e.occ1 |= 1ull << (cell - 64u);
        e.wood -= cost_w; e.stone -= cost_s;                        // :134
        e.farm += a == 1; e.lumber += a == 2; e.quarry += a == 3; e.house += a == 4;
        r += a == 1 ? 3 : a == 4 ? 4 : 2;                           // :73-81
        if (a == 4 && prev_pop + 1u >= prev_cap) r += 10;           // :83-84, both values from before the build
    } else if (build) {
        r -= 3;                                                     // :86
    }
    bool term = false;
    if (go) {
        e.steps += 1;
        e.food += 2 * (int32_t)e.farm; e.wood += 3 * (int32_t)e.lumber; e.stone += 2 * (int32_t)e.quarry;   // :164-174
        if (e.food < (int32_t)e.pop) e.pop = 0; else e.food -= (int32_t)e.pop;                            // :176-183
        if (e.pop > 0u && e.food > 2 && e.pop < e.capacity()) { e.pop += 1; e.food -= 1; }                  // :185-194
        const int32_t pop = (int32_t)e.pop;
        if (e.pop > prev_pop) r += 5;                               // :95-114
        if (e.pop < prev_pop) r -= 50;
        if (e.food > 2 * pop) r += 1;
        if (e.food < pop) r -= 2;
        if (e.food < (pop > 2 ? pop : 2)) r -= 5;
        const int32_t diff = e.wood - e.stone;
        if ((diff < 0 ? -diff : diff) < 5) r += 1;
        if (a == 1 && e.food > 3 * pop) r -= 1;
        if (e.pop >= MAX_POPULATION) e.latch = 1;                   // world_builder_env.py:141-146
        e.win += e.latch;
        const bool won = e.latch && e.win >= WIN_STEPS;
        term = e.pop == 0u || won;                                  // :234-248
        if (term) r = e.pop == 0u ? -100 : won ? 100 : -50;         // :153-159
    }
    return term;
}

// the lane's grid row as bytes + its six numbers -> the wave's LDS tile (FLAT: all six as floats)
__device__ __forceinline__ void stage(const Env &e, uint32_t *__restrict__ tile, float *__restrict__ ex, uint32_t lane, int32_t RS, bool flat) {
#pragma unroll
    for (int k = 0; k < MAX_RS; ++k)
        if (k < RS) tile[lane * (uint32_t)RS + (uint32_t)k] = spread4(e.g[k >> 1] >> (16 * (k & 1)));
    if (flat) {
        float *x = ex + lane * NEXTRA;
        x[0] = (float)e.food; x[1] = (float)e.wood; x[2] = (float)e.stone; x[3] = (float)e.pop; x[4] = (float)e.capacity(); x[5] = (float)e.win;
    }
}

// One observation of the wave's `nrows` envs (the first nrows lanes; `row0` = the wave's first env) -> `base`, the observation's
// first byte (16-byte aligned for the Dict slab, 4-byte aligned for FLAT rows).  Call with all lanes of the wave.
template <bool FLAT>
__device__ __forceinline__ void write_obs(const Env &e, const Params &p, void *base, int64_t row0, uint32_t nrows, uint32_t lane, bool live,
                                          uint32_t *__restrict__ tile, float *__restrict__ ex) {
    if (live) stage(e, tile, ex, lane, p.RS, FLAT);
    lds_barrier();
    const uint8_t *tb = reinterpret_cast<const uint8_t *>(tile);
    const uint32_t GG = (uint32_t)p.GG, RSB = 4u * (uint32_t)p.RS;
    if (FLAT) {
        const uint32_t W = (uint32_t)p.W, total = nrows * W;
        float *dst = static_cast<float *>(base) + row0 * (int64_t)W;
#pragma unroll 2
        for (uint32_t q = lane; q < total; q += 64u) {
            const uint32_t r = __umulhi(q, p.magic_w), c = q - r * W;
            dst[q] = c < GG ? (float)tb[r * RSB + c] : ex[r * NEXTRA + (c - GG)];
        }
    } else {
        uint8_t *slab = static_cast<uint8_t *>(base);
        uint32_t *dst = reinterpret_cast<uint32_t *>(slab + row0 * (int64_t)GG);      // row0 is a multiple of 64: 16-byte aligned
        const uint32_t nbytes = nrows * GG, ndw = (nbytes + 3u) >> 2;
        if ((GG & 3u) == 0u) {                                                         // rows are whole dwords: the tile is the image
            const uint32_t n16 = ndw >> 2;
#pragma unroll 2
            for (uint32_t q = lane; q < n16; q += 64u) reinterpret_cast<uint4 *>(dst)[q] = reinterpret_cast<const uint4 *>(tile)[q];
            const uint32_t q = 4u * n16 + lane;
            if (q < ndw) dst[q] = tile[q];
        } else {
            const uint32_t nfull = nbytes >> 2;                                        // whole dwords; the plane's padding is never written
#pragma unroll 1
            for (uint32_t q = lane; q < nfull; q += 64u) {
                uint32_t v = 0;
#pragma unroll
                for (uint32_t j = 0; j < 4u; ++j) {
                    const uint32_t b = 4u * q + j, r = __umulhi(b, p.magic_gg), c = b - r * GG;
                    v |= (uint32_t)tb[r * RSB + c] << (8u * j);
                }
                dst[q] = v;
            }
            const uint32_t b = 4u * nfull + lane;                                      // the ragged wave's last one to three bytes
            if (b < nbytes) slab[row0 * (int64_t)GG + b] = tb[__umulhi(b, p.magic_gg) * RSB + (b - __umulhi(b, p.magic_gg) * GG)];
        }
        if (live) {
            const int64_t i = row0 + lane;
            reinterpret_cast<float4 *>(slab + p.off_res)[i] = make_float4((float)e.food, (float)e.wood, (float)e.stone, (float)e.pop);
            reinterpret_cast<float *>(slab + p.off_cap)[i] = (float)e.capacity();
            reinterpret_cast<int32_t *>(slab + p.off_win)[i] = (int32_t)e.win;
        }
    }
    lds_barrier();                                                   // the tile is free again
}

// write_obs for the terminal rows of one step of rollout_rows_kernel (lane_final_rows): the lanes with `mine` stage at column `rank`,
// and the wave writes `keep` dense rows from row `row0` of the rows output on.  FLAT: the dword path of write_obs.  Dict: the grid run
// is bytes [row0 * GG, (row0 + keep) * GG) of the slab, which starts and ends wherever that puts it — its whole dwords are composed from
// the tile, the up-to-three bytes before the first and after the last are byte stores, so nothing outside the run is written; the
// three small planes are stored by the kept lanes.  Call with all lanes of the wave.
template <bool FLAT>
__device__ __forceinline__ void write_final_rows(const Env &e, const RowsParams &p, int64_t row0, uint32_t keep, uint32_t rank, bool mine, uint32_t lane,
                                                 uint32_t *__restrict__ tile, float *__restrict__ ex) {
    if (mine) stage(e, tile, ex, rank, p.RS, FLAT);
    lds_barrier();
    const uint8_t *tb = reinterpret_cast<const uint8_t *>(tile);
    const uint32_t GG = (uint32_t)p.GG, RSB = 4u * (uint32_t)p.RS;
    if (FLAT) {
        const uint32_t W = (uint32_t)p.W, total = keep * W;
        float *dst = static_cast<float *>(p.fin.rows) + row0 * (int64_t)W;
#pragma unroll 2
        for (uint32_t q = lane; q < total; q += 64u) {
            const uint32_t r = __umulhi(q, p.magic_w), c = q - r * W;
            dst[q] = c < GG ? (float)tb[r * RSB + c] : ex[r * NEXTRA + (c - GG)];
        }
    } else {
        uint8_t *slab = static_cast<uint8_t *>(p.fin.rows);
        uint8_t *run = slab + row0 * (int64_t)GG;                                      // the slab is 16-byte aligned; the run is not
        const uint32_t nbytes = keep * GG;
        auto byte_at = [&](uint32_t b) -> uint32_t {                                   // byte b of the run: cell b % GG of tile column b / GG
            const uint32_t r = __umulhi(b, p.magic_gg), c = b - r * GG;
            return (uint32_t)tb[r * RSB + c];
        };
        const uint32_t lead = (4u - (uint32_t)(reinterpret_cast<uintptr_t>(run) & 3u)) & 3u, head = lead < nbytes ? lead : nbytes;
        if (lane < head) run[lane] = (uint8_t)byte_at(lane);
        const uint32_t ndw = (nbytes - head) >> 2;
        uint32_t *dst = reinterpret_cast<uint32_t *>(run + head);
#pragma unroll 1
        for (uint32_t q = lane; q < ndw; q += 64u) {
            const uint32_t b = head + 4u * q;
            dst[q] = byte_at(b) | (byte_at(b + 1u) << 8) | (byte_at(b + 2u) << 16) | (byte_at(b + 3u) << 24);
        }
        const uint32_t b = head + 4u * ndw + lane;
        if (b < nbytes) run[b] = (uint8_t)byte_at(b);
        if (mine) {
            const int64_t i = row0 + rank;
            reinterpret_cast<float4 *>(slab + p.rows_off_res)[i] = make_float4((float)e.food, (float)e.wood, (float)e.stone, (float)e.pop);
            reinterpret_cast<float *>(slab + p.rows_off_cap)[i] = (float)e.capacity();
            reinterpret_cast<int32_t *>(slab + p.rows_off_win)[i] = (int32_t)e.win;
        }
    }
    lds_barrier();                                                   // the tile is free again
}

// k steps with the record in registers.  ROLLOUT: per-step outputs indexed [t, env], sums; GIVEN: the caller's actions, else the
// counter hash cge_hash_action(action_seed, env_index0 + i, t0 + t, 5, 0).  With RowsParams (ROWS, a SAME_STEP rollout) the terminal
// observations of the terminated envs go to the wave's segment of p.fin.
template <int MODE, bool FLAT, bool ROLLOUT, bool GIVEN, class P = Params>
__device__ __forceinline__ void run(const P &p) {
    constexpr bool ROWS = std::is_same<P, RowsParams>::value;
    static_assert(!ROWS || (ROLLOUT && MODE == CGE_AUTORESET_SAME_STEP), "terminal rows: fused SAME_STEP rollouts");
    __shared__ __attribute__((aligned(16))) uint32_t tile[BLOCK * MAX_RS];
    __shared__ float ex[BLOCK * NEXTRA];
    const uint32_t lane = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * BLOCK, i = row0 + lane;
    const bool live = i < p.n;
    const int64_t li = live ? i : p.n - 1;
    const uint32_t nrows = (uint32_t)(p.n - row0 < BLOCK ? p.n - row0 : BLOCK);
    const int64_t step_bytes = p.obs_step_stride * (FLAT ? 4 : 1);
    Env e;
    e.load(p.state, p.ret, p.n, li);
    uint32_t *blk = p.mt + li * MT_STRIDE;
    const uint64_t key = GIVEN ? 0 : hash_env_key(p.a_seed, (uint64_t)(p.env0 + li));
    double rsum = 0.0;
    int32_t dcount = 0;
    uint32_t fin_used = 0;                                           // ROWS: terminal rows the wave's segment has been handed
    const int ksteps = ROLLOUT ? p.k_steps : 1;
#pragma unroll 1
    for (int t = 0; t < ksteps; ++t) {
        int32_t r = 0;
        bool go = false, reset_now = false;
        int32_t a = 0;
        if (live) {
            if (MODE == CGE_AUTORESET_NEXT_STEP && e.needs_reset) {
                reset_now = true;
            } else {
                a = GIVEN ? p.actions[(int64_t)t * p.n + i] : (int32_t)hash_action_from_key(key, (uint64_t)(p.t0 + t), 5u, 0u);
                go = a >= 0 && a <= 4;
                if (!go) atomicAdd(p.err_count, 1ull);              // reference: ValueError (:133-134); the env is left as it was
            }
        }
        const bool term = env_step(e, blk, a, go, p.GG, r);
        if (go) {
            e.ret += r;
            if (term) lane_episode_end<MODE>(p, i, (double)e.ret, (int32_t)e.steps, reset_now, e.needs_reset);
        }
        if (MODE == CGE_AUTORESET_SAME_STEP && !ROLLOUT) {          // the terminal rows; a wave with none writes nothing
            if (p.final_obs && __ballot(term)) write_obs<FLAT>(e, p, p.final_obs, row0, nrows, lane, live, tile, ex);
        }
        if constexpr (ROWS) {                                       // ... of a rollout: the terminated envs only, compacted (lane_final_rows)
            const int64_t first = (int64_t)blockIdx.x * p.fin.cap + (int64_t)fin_used;
            uint8_t *dst;
            int keep, rank;
            if (__builtin_expect(lane_final_rows(p.fin, fin_used, term, t, i, 0, dst, keep, rank), false))
                write_final_rows<FLAT>(e, p, first, (uint32_t)keep, (uint32_t)rank, term && rank < keep, lane, tile, ex);
        }
        if (MODE != CGE_AUTORESET_DISABLED && reset_now) e.clear();
        if (lane_obs_due<ROLLOUT>(p, t, ksteps))
            write_obs<FLAT>(e, p, static_cast<char *>(p.obs) + (int64_t)t * step_bytes, row0, nrows, lane, live, tile, ex);
        if (live) {
            const float reward = (float)r;                          // small integers: exact
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
        e.store(p.state, p.ret, p.n, i);
        if (ROLLOUT) lane_sums(p, i, rsum, dcount);
    }
    if constexpr (ROWS) {
        if (lane == 0) p.fin.count[blockIdx.x] = (int32_t)fin_used;
    }
}

template <int MODE, bool FLAT>
__global__ __launch_bounds__(BLOCK) void step_kernel(Params p) { run<MODE, FLAT, false, true>(p); }

template <int MODE, bool FLAT, bool ACTIONS>
__global__ __launch_bounds__(BLOCK) void rollout_kernel(Params p) { run<MODE, FLAT, true, ACTIONS>(p); }

// the SAME_STEP rollout while terminal rows are registered (cge_rows_world_builder_rollout_final_obs).  The register budget is the
// sibling rollout_kernel's waves per SIMD, stated: left alone the hashed FLAT instance takes 170 registers, two over the 168 of three
// waves (the sibling: 161); held to them it needs no scratch.
template <bool FLAT, bool ACTIONS>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(FLAT ? 3 : 2))) void rollout_rows_kernel(RowsParams p) { run<CGE_AUTORESET_SAME_STEP, FLAT, true, ACTIONS>(p); }

// reset (mask, or all) / initial state (init: the reset state, cursor rewound) / rewind (after a re-seed) + obs.  Draws nothing.
template <bool FLAT>
__global__ __launch_bounds__(BLOCK) void reset_kernel(Params p, int init, int rewind) {
    __shared__ __attribute__((aligned(16))) uint32_t tile[BLOCK * MAX_RS];
    __shared__ float ex[BLOCK * NEXTRA];
    const uint32_t lane = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * BLOCK, i = row0 + lane;
    const bool live = i < p.n;
    const int64_t li = live ? i : p.n - 1;
    const uint32_t nrows = (uint32_t)(p.n - row0 < BLOCK ? p.n - row0 : BLOCK);
    Env e;
    e.load(p.state, p.ret, p.n, li);
    bool dirty = false;
    if (init) { e.clear(); e.mt_pos = 0; e.mt_pretw = 0; dirty = true; }
    else if (rewind) { e.mt_pos = 0; e.mt_pretw = 0; dirty = true; }
    else if (live && (!p.mask || p.mask[i])) { e.clear(); dirty = true; }
    if (live && dirty) e.store(p.state, p.ret, p.n, i);
    if (p.obs) write_obs<FLAT>(e, p, p.obs, row0, nrows, lane, live, tile, ex);
}

__global__ __launch_bounds__(256) void info_kernel(const uint4 *__restrict__ state, const int32_t *__restrict__ ret, int64_t n, int field, int idx,
                                                   int32_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    Env e;
    e.load(state, ret, n, i);
    int32_t v = 0;
    switch (field) {
        case CGE_WORLD_BUILDER_INFO_STEPS: v = (int32_t)e.steps; break;
        case CGE_WORLD_BUILDER_INFO_WIN_STEPS: v = (int32_t)e.win; break;
        case CGE_WORLD_BUILDER_INFO_REACHED_WIN_POPULATION: v = (int32_t)e.latch; break;
        case CGE_WORLD_BUILDER_INFO_FOOD: v = e.food; break;
        case CGE_WORLD_BUILDER_INFO_WOOD: v = e.wood; break;
        case CGE_WORLD_BUILDER_INFO_STONE: v = e.stone; break;
        case CGE_WORLD_BUILDER_INFO_POPULATION: v = (int32_t)e.pop; break;
        case CGE_WORLD_BUILDER_INFO_POPULATION_CAPACITY: v = (int32_t)e.capacity(); break;
        case CGE_WORLD_BUILDER_INFO_BUILDING_COUNT: v = (int32_t)(idx == 0 ? e.farm : idx == 1 ? e.lumber : idx == 2 ? e.quarry : e.house); break;
        case CGE_WORLD_BUILDER_INFO_NEEDS_RESET: v = (int32_t)e.needs_reset; break;
    }
    out[i] = v;
}

}  // namespace wb
}  // namespace cge

using namespace cge;

static inline int64_t align16(int64_t x) { return (x + 15) & ~(int64_t)15; }

struct cge_world_builder : LaneHandle {
    using Params = wb::Params;
    using RowsParams = wb::RowsParams;
    cge_world_builder_config cfg{};
    int32_t *ret = nullptr;
    static constexpr const char *kernel_ns = "cge::wb::", *rows_ns = kernel_ns;
    static constexpr int block = wb::BLOCK, seed_kind = 1;
    int64_t cells() const { return (int64_t)cfg.grid_size * cfg.grid_size; }
    int64_t off_res() const { return align16(n * cells()); }
    int64_t off_cap() const { return off_res() + 16 * n; }
    int64_t off_win() const { return align16(off_cap() + 4 * n); }
    int64_t slab_bytes() const { return align16(off_win() + 4 * n); }
    int64_t step_elems() const { return cfg.flatten_obs ? n * (cells() + wb::NEXTRA) : slab_bytes(); }
    size_t record_bytes() const { return 64 + (size_t)((cells() + 3) / 4 * 4) + 4 * MT_N; }
    Params params() const {
        Params p{};
        fill(p);
        p.ret = ret;
        p.G = cfg.grid_size; p.GG = (int32_t)cells(); p.W = p.GG + wb::NEXTRA; p.RS = (p.GG + 3) / 4;
        p.magic_gg = (uint32_t)(((1ull << 32) + (uint64_t)p.GG - 1) / (uint64_t)p.GG);
        p.magic_w = (uint32_t)(((1ull << 32) + (uint64_t)p.W - 1) / (uint64_t)p.W);
        p.off_res = off_res(); p.off_cap = off_cap(); p.off_win = off_win();
        return p;
    }
    // Dict slabs are written in 16-byte pieces, FLAT rows in dwords
    bool aligned(const void *ptr) const { return (reinterpret_cast<uintptr_t>(ptr) & (cfg.flatten_obs ? 3u : 15u)) == 0; }
    static int check(const cge_world_builder_config &c) {
        return bad_autoreset_mode(c.autoreset_mode) || c.grid_size < 2 || c.grid_size > 10 || c.flatten_obs < 0 || c.flatten_obs > 1 ? CGE_ERR_INVALID_ARG : CGE_OK;
    }
    // the FLAT axis sits on top of the mode: kernels and their names
    auto reset_kernel() const { return cfg.flatten_obs ? wb::reset_kernel<true> : wb::reset_kernel<false>; }
    template <int MODE, bool FLAT>
    static auto kernel_of(LaneKind kind) {
        return kind == LANE_STEP ? wb::step_kernel<MODE, FLAT>
               : kind == LANE_ROLLOUT_GIVEN ? wb::rollout_kernel<MODE, FLAT, true> : wb::rollout_kernel<MODE, FLAT, false>;
    }
    template <int MODE>
    auto kernel(LaneKind kind) const { return cfg.flatten_obs ? kernel_of<MODE, true>(kind) : kernel_of<MODE, false>(kind); }
    const char *layout_arg() const { return cfg.flatten_obs ? ", true" : ", false"; }
    // the Dict slab of compacted rows: this type's slab layout for R = segments * capacity envs
    void fill_rows(RowsParams &p) const {
        const int64_t R = (int64_t)lane_segments(this) * fin_cap;
        p.rows_off_res = align16(R * cells());
        p.rows_off_cap = p.rows_off_res + 16 * R;
        p.rows_off_win = align16(p.rows_off_cap + 4 * R);
    }
    void launch_rows(bool given, unsigned blocks, hipStream_t s, const RowsParams &p) const {
        auto k = cfg.flatten_obs ? (given ? wb::rollout_rows_kernel<true, true> : wb::rollout_rows_kernel<true, false>)
                                 : (given ? wb::rollout_rows_kernel<false, true> : wb::rollout_rows_kernel<false, false>);
        hipLaunchKernelGGL(k, dim3(blocks), dim3(block), 0, s, p);
    }
    const char *rows_refusal() const {
        if (aligned(fin_rows)) return nullptr;
        return cfg.flatten_obs ? "the registered terminal rows are not 4-byte aligned" : "the registered terminal rows are not 16-byte aligned";
    }
    hipError_t init() {
        CGE_HIP(alloc(state, (size_t)wb::COLS * n * sizeof(uint4), true, true));
        CGE_HIP(alloc(ret, (size_t)n * sizeof(int32_t), true, true));
        CGE_HIP(alloc(mt, (size_t)n * MT_STRIDE * sizeof(uint32_t), false, true));
        CGE_HIP(alloc(err, sizeof(unsigned long long), true, false));
        CGE_HIP(launch_mt_seed(mt, MT_STRIDE, n, nullptr, 0, env0, 1, nullptr));
        lane_launch_reset(this, params(), 1, 0, nullptr);
        return hipGetLastError();
    }

    // canonical records (cge_host.hpp: get_records / set_records; layout: include/cge_amd.h): the int32[16] header below, the grid
    // one byte per cell padded to whole dwords, NumPy's 624 key words
    static constexpr const char *abi = "cge_world_builder";
    enum { H_FOOD, H_WOOD, H_STONE, H_POP, H_CAP, H_FARM, H_LUMBER, H_QUARRY, H_HOUSE, H_STEPS, H_WIN, H_LATCH, H_NEEDS_RESET, H_MT_POS, H_INTS = 16 };
    enum { A_STATE, A_MT, A_RET };
    size_t grid_bytes() const { return (size_t)((cells() + 3) / 4 * 4); }
    std::vector<RecordArray> record_arrays() const {            // ret: the record holds no running return, set_state zeroes it
        return {{state, sizeof(uint4), wb::COLS, false, true}, {mt, sizeof(uint32_t), MT_STRIDE, true, true}, {ret, sizeof(int32_t), 1, false, false}};
    }
    const char *check_record(const uint8_t *in) const {
        int32_t hd[H_INTS];
        memcpy(hd, in, 64);
        int32_t census[5] = {0, 0, 0, 0, 0};
        for (int64_t c = 0; c < cells(); ++c) {
            if (in[64 + c] > 4) return "a grid cell above 4";
            census[in[64 + c]] += 1;
        }
        if (hd[H_FARM] != census[1] || hd[H_LUMBER] != census[2] || hd[H_QUARRY] != census[3] || hd[H_HOUSE] != census[4])
            return "building counts that differ from the grid's census";
        if (hd[H_CAP] != 10 + 5 * hd[H_HOUSE]) return "population_capacity != 10 + 5 * houses";
        if (hd[H_POP] < 0 || hd[H_POP] > 1023) return "population outside 0..1023";
        if (hd[H_STEPS] < 0 || hd[H_WIN] < 0 || hd[H_WIN] > hd[H_STEPS]) return "steps / win_steps out of range";
        if ((hd[H_LATCH] | hd[H_NEEDS_RESET]) & ~1) return "a flag that is not 0 or 1";
        if (hd[H_MT_POS] < 0 || hd[H_MT_POS] > MT_N) return "mt_pos outside 0..624";
        return nullptr;
    }
    int to_record(const RecordStage &st, int64_t j, uint8_t *out, const char **why) const {
        uint32_t gw[wb::GW + 3];
        for (int c = 0; c < 4; ++c) memcpy(gw + 4 * c, st.at<uint4>(A_STATE, j, c), 16);
        const uint4 f = *st.at<uint4>(A_STATE, j, 4);
        int32_t hd[H_INTS] = {0};
        hd[H_FOOD] = (int32_t)gw[13]; hd[H_WOOD] = (int32_t)gw[14]; hd[H_STONE] = (int32_t)gw[15];
        hd[H_FARM] = f.x & 127; hd[H_LUMBER] = (f.x >> 7) & 127; hd[H_QUARRY] = (f.x >> 14) & 127; hd[H_HOUSE] = (f.x >> 21) & 127;
        hd[H_LATCH] = (f.x >> 28) & 1; hd[H_NEEDS_RESET] = (f.x >> 29) & 1;
        hd[H_POP] = f.y & 1023; hd[H_CAP] = 10 + 5 * hd[H_HOUSE]; hd[H_STEPS] = (int32_t)f.z; hd[H_WIN] = (int32_t)f.w;
        if (!mt_export_cpython(st.at<uint32_t>(A_MT, j), (f.y >> 10) & 1023u, mt_ready_decode((f.y >> 20) & 31u), (uint32_t *)(out + 64 + grid_bytes()), &hd[H_MT_POS])) {
            *why = "generator block twisted too far ahead";
            return CGE_ERR_UNSUPPORTED;
        }
        memcpy(out, hd, 64);
        memset(out + 64, 0, grid_bytes());
        for (int64_t c = 0; c < cells(); ++c) out[64 + c] = (uint8_t)((gw[c >> 3] >> (4 * (c & 7))) & 15u);
        return CGE_OK;
    }
    void from_record(const uint8_t *in, RecordStage &st, int64_t j) const {
        int32_t hd[H_INTS];
        memcpy(hd, in, 64);
        uint32_t gw[wb::GW + 3] = {0}, pos, ready;
        for (int64_t c = 0; c < cells(); ++c) gw[c >> 3] |= (uint32_t)in[64 + c] << (4 * (c & 7));
        gw[13] = (uint32_t)hd[H_FOOD]; gw[14] = (uint32_t)hd[H_WOOD]; gw[15] = (uint32_t)hd[H_STONE];
        for (int c = 0; c < 4; ++c) memcpy(st.at<uint4>(A_STATE, j, c), gw + 4 * c, 16);
        mt_import_cpython((const uint32_t *)(in + 64 + grid_bytes()), hd[H_MT_POS], st.at<uint32_t>(A_MT, j), &pos, &ready);
        *st.at<uint4>(A_STATE, j, 4) = make_uint4(
            (uint32_t)hd[H_FARM] | ((uint32_t)hd[H_LUMBER] << 7) | ((uint32_t)hd[H_QUARRY] << 14) | ((uint32_t)hd[H_HOUSE] << 21) |
                ((uint32_t)hd[H_LATCH] << 28) | ((uint32_t)hd[H_NEEDS_RESET] << 29),
            (uint32_t)hd[H_POP] | (pos << 10) | ((ready > pos ? mt_ready_encode(ready) : 0u) << 20), (uint32_t)hd[H_STEPS], (uint32_t)hd[H_WIN]);
    }
};

extern "C" {

CGE_DEFINE_LIFECYCLE(world_builder)

int cge_world_builder_seed(cge_world_builder *h, const uint64_t *seeds, uint64_t base_seed, void *stream) { return lane_seed(h, seeds, base_seed, stream); }

int cge_world_builder_reset(cge_world_builder *h, const uint8_t *mask, void *obs_out, void *stream) {
    if (!h) return CGE_ERR_INVALID_ARG;
    if (obs_out && !h->aligned(obs_out)) return h->fail(CGE_ERR_INVALID_ARG, "cge_world_builder_reset: obs_out must be 16-byte (Dict) / 4-byte (flat) aligned");
    return lane_reset(h, mask, obs_out, stream);
}

int cge_world_builder_step(cge_world_builder *h, const int32_t *actions, void *obs_out, float *reward_out, uint8_t *terminated_out,
                           uint8_t *truncated_out, void *final_obs_out, void *stream) {
    return lane_step(h, h && actions && obs_out && reward_out && terminated_out && h->aligned(obs_out) && h->aligned(final_obs_out),
                     "cge_world_builder_step: null actions/obs/reward/terminated pointer, or a misaligned observation buffer", actions, obs_out,
                     reward_out, terminated_out, truncated_out, final_obs_out, stream);
}

int cge_world_builder_rollout(cge_world_builder *h, int32_t k_steps, const int32_t *actions, uint64_t action_seed, int64_t t0, void *obs_out,
                              int64_t obs_step_stride, float *reward_traj_out, uint8_t *terminated_traj_out, double *reward_sum_out,
                              int32_t *done_count_out, void *stream) {
    const bool ok = h && h->aligned(obs_out) && (h->cfg.flatten_obs || obs_step_stride % 16 == 0);
    return lane_rollout(h, ok, "cge_world_builder_rollout: bad k_steps / obs_step_stride / observation alignment", k_steps, actions, action_seed, t0,
                        obs_out, obs_step_stride, reward_traj_out, terminated_traj_out, reward_sum_out, done_count_out, stream);
}

int cge_world_builder_info(cge_world_builder *h, int32_t field_id, int32_t index, int32_t *out, void *stream) {
    if (!h) return CGE_ERR_INVALID_ARG;
    if (!out || field_id < 0 || field_id > CGE_WORLD_BUILDER_INFO_NEEDS_RESET || index < 0 || index > 3)
        return h->fail(CGE_ERR_INVALID_ARG, "cge_world_builder_info: bad field / index / null out");
    DeviceGuard g(h->device);
    hipLaunchKernelGGL(wb::info_kernel, dim3(grid256(h->n)), dim3(256), 0, as_stream(stream), h->state, h->ret, h->n, field_id, index, out);
    return launched(h);
}

CGE_DEFINE_ROWS_FINAL_OBS(world_builder, void, 64)
CGE_DEFINE_ERROR_COUNT(world_builder)

CGE_DEFINE_RECORDS(world_builder)

}  // extern "C"
