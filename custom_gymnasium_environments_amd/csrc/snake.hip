// snake.hip — batched SnakeEnvClassic for MI355X (gfx950): kernels + C ABI (include/cge_amd.h).
//
// Re-expresses /root/reference/snake_env_classic/snake_env.py  reset :49-65, step :67-119,
// _place_food :121-129, _get_observation :131-143 for N independent instances, one lane per env.
//
// Device representation (per env, all integer, bit-exact with the reference's Python objects):
//   sr    2 bits per move  the snake's move history, newest first (replaces the Python list's order: walking from the head
//                          against it visits the body head to tail; list.insert(0,..)/pop() become a shift and a truncate)
//   occ   CELLS bits       occupancy of the body (`new_head in self.snake`, obs value 1)
//   head, tail, len, food, dir, steps, score, flags, episodes, and the env's MT19937 cursor (pos, pretw)
// stored struct-of-arrays as columns of uint4 (column c of env i at state[c*N+i]) so a wavefront's loads/stores are 16 B per
// lane, fully coalesced.  For the benchmark grid (G=10) the HOT column holds every scalar plus the 28 newest moves — 16 B per
// env is all a step() reads and writes for snakes up to 29 cells — older moves live in two cold columns, and the occupancy
// bits are not stored: they are rebuilt in registers by the head-to-tail walk when the record is loaded.
// The whole record lives in VGPRs during a step (static-index mask/select chains, cge_device.hpp).
// Food placement (the only RNG use) never opens the env's 2560-byte MT19937 block on the common path: every env owns a RING of
// 64 pre-drawn digits (the top KBITS bits of the next generator words, tempered) in two uint4 columns next to the state, with
// the number of digits left in the hot record; a placement reads two dwords of it, and the ring is refilled wave-cooperatively
// (64 lanes twist 64 consecutive words of ONE env) when it runs dry — once per ~256 env-steps per env (DigitQ below).
// The (N,G,G) int8 observation is built in LDS (one row per lane, dword stride G*G/4 — odd for
// G=10, so conflict-free) and streamed out as 16-byte-per-lane stores.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cge_device.hpp"
#include "cge_host.hpp"
#include "snake_place.hpp"

#ifndef CGE_SNAKE_FINCOPY
#define CGE_SNAKE_FINCOPY 1     // A/B knob: 0 every finishing lane builds and stores its own terminal row, 1 via the LDS rows, one coalesced store per env
#endif
namespace cge {
namespace snake {

constexpr int bitlen(int n) {
    int k = 0;
    while (n) { ++k; n >>= 1; }
    return k;
}

enum : uint32_t { F_NEEDS_RESET = 1u, F_BOARD_FULL = 2u, F_FOOD_VALID = 4u };

template <int G>
struct Lay {
    static constexpr int CELLS = G * G;
    static constexpr int OCCW = (CELLS + 31) / 32;
    static constexpr int SRW = (2 * (CELLS - 1) + 31) / 32;   // move history: 2 bits per body segment behind the head
    // G=10 (the benchmark grid): a 16-byte HOT record holds every scalar and the 24 most recent moves; older moves spill into two
    // cold columns that only snakes longer than 25 / 89 cells ever touch.  Occupancy is not stored at all there (see Env).
    static constexpr bool TIGHT = (G == 10);
    static constexpr int HOT_SH = 15;                          // bit of hot word 2 at which the move history starts
    static constexpr int HOT_DIRS = (2 * 32 - HOT_SH) / 2, COLD0_DIRS = 64;   // 24 moves in the hot record
    static constexpr int NW = TIGHT ? 12 : OCCW + SRW + 4;
    static constexpr int COLS = (NW + 3) / 4;
    static constexpr bool PACKED = CELLS % 4 == 0;             // even G: a lane's LDS row is exactly its G*G bytes; odd G: padded to whole dwords
    static constexpr int OBS_DW = (CELLS + 3) / 4;             // dwords per LDS obs row
    static constexpr int KBITS = bitlen(G);  // CPython: k = n.bit_length() for _randbelow(G)
    static constexpr int BLOCK = (CELLS <= 144) ? 256 : 64;
    static_assert(G >= 4 && G <= 30, "center start needs G >= 4 (and a 10x10-style 3 cell margin is not assumed); 64 rows of G*G bytes + the digit rings fit 64 KB of LDS up to 30");
    static constexpr int MAX_STEPS_LIMIT = TIGHT ? 4095 : 65535;
    static constexpr uint32_t MAX_EPISODES = TIGHT ? 0xFFFFu : 0xFFFFFFFFu;   // the counter saturates
    static_assert(CELLS <= 1023, "cell index is packed in 10 bits");
    static_assert(!TIGHT || (SRW == 7 && OCCW == 4), "hot / cold split below is written for 10x10");
};

__host__ __device__ __forceinline__ int dir_delta(uint32_t d, int g) { return d == 0 ? -g : d == 1 ? 1 : d == 2 ? g : -1; }

// Body representation: `sr` is the snake's move history, most recent move in bits 1:0 — move k (k = 0 newest) is the direction in
// which the head entered the cell it occupied k moves ago, so walking from the head AGAINST sr[0], sr[1], ... visits the body
// head to tail (the Python list's order).  list.insert(0, new_head) = shift left by 2 and OR the direction in; list.pop() =
// drop entry len-1 and advance `tail` along it.  O(1) per step, no per-env byte-granular memory traffic.
// `occ` (occupancy bits: `new_head in self.snake`, obs value 1) lives in registers only for G=10: it is rebuilt at load time by
// that walk (len-1 iterations: 0-3 under random play), which is what lets the stored record shrink from 48 to 16 bytes.
template <int G>
struct Env {
    using L = Lay<G>;
    uint32_t occ[L::OCCW];
    uint32_t sr[L::SRW];
    uint32_t head, tail, len, food, dir, steps, score, flags, episodes, mt_pos, mt_pretw, dq_left;

    __device__ __forceinline__ void load(const uint4 *__restrict__ state, int64_t n, int64_t i) {
        uint32_t raw[L::COLS * 4];
        if constexpr (L::TIGHT) {
            const uint4 h = state[i];
            raw[0] = h.x; raw[1] = h.y; raw[2] = h.z; raw[3] = h.w;
            const uint32_t moves = ((h.x >> 7) & 127u) - 1u;
            uint4 c0 = make_uint4(0, 0, 0, 0), c1 = make_uint4(0, 0, 0, 0);
            if (moves > (uint32_t)L::HOT_DIRS) c0 = state[n + i];                              // rare: long snakes only
            if (moves > (uint32_t)(L::HOT_DIRS + L::COLD0_DIRS)) c1 = state[2 * n + i];
            raw[4] = c0.x; raw[5] = c0.y; raw[6] = c0.z; raw[7] = c0.w;
            raw[8] = c1.x; raw[9] = c1.y; raw[10] = c1.z; raw[11] = c1.w;
        } else {
#pragma unroll
            for (int c = 0; c < L::COLS; ++c) {
                uint4 v = state[(int64_t)c * n + i];
                raw[4 * c] = v.x; raw[4 * c + 1] = v.y; raw[4 * c + 2] = v.z; raw[4 * c + 3] = v.w;
            }
        }
        unpack(raw);
    }
    __device__ __forceinline__ void store(uint4 *__restrict__ state, int64_t n, int64_t i) const {
        uint32_t raw[L::COLS * 4];
        pack(raw);
        if constexpr (L::TIGHT) {
            state[i] = make_uint4(raw[0], raw[1], raw[2], raw[3]);
            if (len - 1u > (uint32_t)L::HOT_DIRS) state[n + i] = make_uint4(raw[4], raw[5], raw[6], raw[7]);
            if (len - 1u > (uint32_t)(L::HOT_DIRS + L::COLD0_DIRS)) state[2 * n + i] = make_uint4(raw[8], raw[9], raw[10], raw[11]);
        } else {
#pragma unroll
            for (int c = 0; c < L::COLS; ++c)
                state[(int64_t)c * n + i] = make_uint4(raw[4 * c], raw[4 * c + 1], raw[4 * c + 2], raw[4 * c + 3]);
        }
    }
    // G=10 hot record  w0: head:7 | len:7 @7 | food:7 @14 | dir:2 @21 | flags:3 @23 | score[5:0] @26
    //                  w1: steps:12 | mt_pos:10 @12 | mt_pretw!=0 @22 | score[6] @23 | episodes[7:0] @24
    //                  w2: episodes[15:8] | dq_left:7 @8 | sr bits 0..16 @15      w3: sr bits 17..48
    //       cold words 4..11: sr bits 49..  (read / written only when len-1 > 24, words 8.. only when len-1 > 88)
    // mt_pos (0..624) is the first generator word that has NOT been turned into a digit yet; the dq_left digits in the env's
    // ring are those of words [mt_pos - dq_left, mt_pos), so the CPython cursor of the stream is mt_pos - dq_left.
    __host__ __device__ __forceinline__ void unpack(const uint32_t *raw) {
        if constexpr (L::TIGHT) {
            const uint32_t w0 = raw[0], w1 = raw[1], w2 = raw[2];
            head = w0 & 127u; len = (w0 >> 7) & 127u; food = (w0 >> 14) & 127u; dir = (w0 >> 21) & 3u; flags = (w0 >> 23) & 7u;
            score = (w0 >> 26) | (((w1 >> 23) & 1u) << 6);
            steps = w1 & 0xFFFu; mt_pos = (w1 >> 12) & 1023u; mt_pretw = (w1 & (1u << 22)) ? (uint32_t)MT_N : 0u;
            episodes = (w1 >> 24) | ((w2 & 0xFFu) << 8);
            dq_left = (w2 >> 8) & 127u;
#pragma unroll
            for (int k = 0; k < L::SRW; ++k) sr[k] = (raw[2 + k] >> L::HOT_SH) | (raw[3 + k] << (32 - L::HOT_SH));
            mask_history();
            rebuild_occupancy();
        } else {
#pragma unroll
            for (int k = 0; k < L::OCCW; ++k) occ[k] = raw[k];
#pragma unroll
            for (int k = 0; k < L::SRW; ++k) sr[k] = raw[L::OCCW + k];
            const uint32_t m0 = raw[L::OCCW + L::SRW], m1 = raw[L::OCCW + L::SRW + 1], m3 = raw[L::OCCW + L::SRW + 3];
            head = m0 & 1023u; tail = (m0 >> 10) & 1023u; food = (m0 >> 20) & 1023u; dir = m0 >> 30;
            steps = m1 & 0xffffu; score = (m1 >> 16) & 1023u; flags = m1 >> 26;
            episodes = raw[L::OCCW + L::SRW + 2];
            mt_pos = m3 & 1023u; mt_pretw = (m3 & 1024u) ? (uint32_t)MT_N : 0u; len = (m3 >> 11) & 1023u; dq_left = (m3 >> 24) & 127u;
        }
    }
    __host__ __device__ __forceinline__ void pack(uint32_t *raw) const {
        if constexpr (L::TIGHT) {
            const uint32_t ep = episodes < L::MAX_EPISODES ? episodes : L::MAX_EPISODES;
            raw[0] = head | (len << 7) | (food << 14) | (dir << 21) | (flags << 23) | ((score & 63u) << 26);
            raw[1] = steps | (mt_pos << 12) | (mt_pretw ? (1u << 22) : 0u) | (((score >> 6) & 1u) << 23) | ((ep & 0xFFu) << 24);
            raw[2] = (ep >> 8) | (dq_left << 8) | (sr[0] << L::HOT_SH);
#pragma unroll
            for (int k = 1; k < L::SRW; ++k) raw[2 + k] = (sr[k - 1] >> (32 - L::HOT_SH)) | (sr[k] << L::HOT_SH);
            raw[2 + L::SRW] = sr[L::SRW - 1] >> (32 - L::HOT_SH);
#pragma unroll
            for (int k = 3 + L::SRW; k < 12; ++k) raw[k] = 0;
        } else {
#pragma unroll
            for (int k = 0; k < L::OCCW; ++k) raw[k] = occ[k];
#pragma unroll
            for (int k = 0; k < L::SRW; ++k) raw[L::OCCW + k] = sr[k];
            raw[L::OCCW + L::SRW] = head | (tail << 10) | (food << 20) | (dir << 30);
            raw[L::OCCW + L::SRW + 1] = steps | (score << 16) | (flags << 26);
            raw[L::OCCW + L::SRW + 2] = episodes;
            raw[L::OCCW + L::SRW + 3] = mt_pos | (mt_pretw ? 1024u : 0u) | (len << 11) | (dq_left << 24);
#pragma unroll
            for (int k = L::NW; k < L::COLS * 4; ++k) raw[k] = 0;
        }
    }
    // entries at and beyond len-1 are not part of the body: keep them zero (canonical records; stale cold columns are ignored)
    __host__ __device__ __forceinline__ void mask_history() {
        const uint32_t bits = len == 0u ? 0u : 2u * (len - 1u);
#pragma unroll
        for (int k = 0; k < L::SRW; ++k) {
            const uint32_t lo = 32u * k;
            sr[k] = bits >= lo + 32u ? sr[k] : (bits > lo ? (sr[k] & ((1u << (bits - lo)) - 1u)) : 0u);
        }
    }
    // head -> tail walk against the move history: occupancy bits and the tail cell.  The first 32 moves come out of a 64-bit
    // shift register (all that random play ever needs); longer bodies continue with indexed extraction.
    __host__ __device__ __forceinline__ void rebuild_occupancy() {
#pragma unroll
        for (int k = 0; k < L::OCCW; ++k) occ[k] = 0;
        uint32_t cell = head;
        or_word(occ, cell >> 5, 1u << (cell & 31u));
        // len is 0 in never-initialised (zeroed) records and arbitrary in a corrupted one: bound the walk, whatever the bits say
        const uint32_t moves = len == 0u ? 0u : (len <= (uint32_t)L::CELLS ? len - 1u : (uint32_t)L::CELLS - 1u);
        uint64_t q = (uint64_t)sr[0] | ((uint64_t)sr[1] << 32);
        const uint32_t n1 = moves < 32u ? moves : 32u;
        for (uint32_t k = 0; k < n1; ++k) {
            cell = (uint32_t)((int)cell - dir_delta((uint32_t)q & 3u, G));
            q >>= 2;
            or_word(occ, cell >> 5, 1u << (cell & 31u));
        }
        for (uint32_t k = 32u; k < moves; ++k) {
            const uint32_t d = (sel(sr, k >> 4) >> ((k & 15u) * 2u)) & 3u;
            cell = (uint32_t)((int)cell - dir_delta(d, G));
            or_word(occ, cell >> 5, 1u << (cell & 31u));
        }
        tail = cell;
    }

    __host__ __device__ __forceinline__ uint32_t occupied(uint32_t cell) const {
        if constexpr (L::OCCW == 4) {                          // two 64-bit halves: 2 selects + one 64-bit shift instead of a 4-way select chain
            const uint64_t lo = (uint64_t)occ[0] | ((uint64_t)occ[1] << 32), hi = (uint64_t)occ[2] | ((uint64_t)occ[3] << 32);
            return (uint32_t)(((cell < 64u ? lo : hi) >> (cell & 63u)) & 1ull);
        } else {
            return (sel(occ, cell >> 5) >> (cell & 31u)) & 1u;
        }
    }
    __host__ __device__ __forceinline__ uint32_t length() const { return len; }

    // snake_env.py:123 would spin forever on a full board: reported via info (sticky), never silent
    __device__ __forceinline__ bool can_place_food() {
        if (len >= (uint32_t)L::CELLS) {
            flags = (flags | F_BOARD_FULL) & ~F_FOOD_VALID;
            return false;
        }
        return true;
    }

    // snake_env.py:49-65 without the trailing _place_food()
    __device__ __forceinline__ void reset_body() {
#pragma unroll
        for (int k = 0; k < L::OCCW; ++k) occ[k] = 0;
#pragma unroll
        for (int k = 0; k < L::SRW; ++k) sr[k] = 0;
        constexpr uint32_t center = (G / 2) * G + (G / 2);
        head = tail = center;
        len = 1;
        occ[center >> 5] |= 1u << (center & 31u);
        dir = 1;
        score = 0;
        steps = 0;
        flags &= ~F_NEEDS_RESET;
    }

    // snake_env.py:67-119 without _place_food(); returns terminated, sets `ate`
    __device__ __forceinline__ bool move(uint32_t action, uint32_t max_steps, float &reward, bool &ate, bool short_wave) {
        ate = false;
        const int d = (int)action - (int)dir;
        if (d != 2 && d != -2) dir = action;                                      // :73-74
        const uint32_t hr = head / G, hc = head - hr * G;
        int nr = (int)hr, nc = (int)hc;
        if (dir == 0) nr -= 1; else if (dir == 1) nc += 1; else if (dir == 2) nr += 1; else nc -= 1;   // :77-85
        const bool wall = (unsigned)nr >= (unsigned)G || (unsigned)nc >= (unsigned)G;             // :88-89
        const uint32_t ncell = wall ? head : (uint32_t)(nr * G + nc);
        if (wall || occupied(ncell)) {                                            // :90, :93-94 (tail cell counts)
            reward = -10.0f;
            return true;
        }
        // :97 insert(0, new_head): the move joins the history at position 0.  short_wave (wave-uniform: no lane of the wave has more
        // than 15 cells, i.e. all of random play): the whole history sits in sr[0] and stays there after this move
        if (!short_wave) {
#pragma unroll
            for (int k = L::SRW - 1; k > 0; --k) sr[k] = (sr[k] << 2) | (sr[k - 1] >> 30);
        }
        sr[0] = (sr[0] << 2) | dir;
        or_word(occ, ncell >> 5, 1u << (ncell & 31u));
        head = ncell;
        reward = 0.0f;
        if ((flags & F_FOOD_VALID) && ncell == food) {                            // :101-104
            score += 1;
            len += 1;
            reward = 10.0f;
            ate = true;
        } else {                                                                  // :107 pop(): the oldest move (entry len-1) leaves
            const uint32_t p = 2u * (len - 1u);
            uint32_t td;
            if (short_wave) {
                td = (sr[0] >> p) & 3u;
                sr[0] &= ~(3u << p);
            } else {
                td = (sel(sr, p >> 5) >> (p & 31u)) & 3u;
                andnot_word(sr, p >> 5, 3u << (p & 31u));
            }
            andnot_word(occ, tail >> 5, 1u << (tail & 31u));
            tail = (uint32_t)((int)tail + dir_delta(td, G));
        }
        steps += 1;                                                               // :109
        return steps >= max_steps;                                                // :113-114
    }

    // snake_env.py:131-143 — one int8 row of G*G cells as OBS_DW dwords; `row` may be LDS or global
    __device__ __forceinline__ void write_obs_body(uint32_t *row) const {
#pragma unroll
        for (int j = 0; j < L::OBS_DW; ++j) {
            const uint32_t b = (occ[(4 * j) >> 5] >> ((4 * j) & 31)) & 0xFu;
            row[j] = (b * 0x00204081u) & 0x01010101u;   // 4 occupancy bits -> 4 bytes of 0/1
        }
    }
    __device__ __forceinline__ void write_obs_food(uint32_t *row) const {
        if (flags & F_FOOD_VALID) reinterpret_cast<int8_t *>(row)[food] = 2;
    }
};

struct Params {
    uint4 *state;
    uint4 *dq;            // digit rings (DigitQ), COLS columns of uint4
    uint32_t *mt;
    int64_t n, env0;
    const int32_t *actions;
    const uint8_t *mask;
    int8_t *obs;
    float *reward;
    uint8_t *terminated, *truncated;
    int8_t *final_obs;
    FinalSeg fin;             // fused rollouts (SAME_STEP): terminal rows compacted per wave (cge_snake_rollout_final_obs); rows nullable
    int32_t mode, max_steps, k_steps;
    uint32_t dq_topup;    // rollout: rings with fewer digits than this are topped up when the launch starts (host: by k_steps)
    uint64_t a_seed;
    int64_t t0, obs_step_stride;
    float *reward_sum;
    int32_t *done_count;
    double *ep_ret;       // episode statistics (cge_snake_episode_stats), nullable
    int32_t *ep_len;
    unsigned long long *err_count;
};

__device__ __forceinline__ uint32_t shfl_u32(uint32_t v, uint32_t src) { return (uint32_t)__shfl((int)v, (int)src, 64); }

// ------------------------------------------------------------------ the env's digit ring (DigitQ)
// _place_food (snake_env.py:121-129) only ever looks at the top KBITS bits of a generator word (`getrandbits(k)` inside
// `random.randint`), ~0.25 words per env-step under random play.  Opening the env's 2560-byte MT19937 block for that — three
// scattered lines read, one written back, per placement — was a quarter of step()'s HBM traffic (round 2: 33 of 176 bytes per
// env-step), and inside a fused rollout the block loads queued behind the CU's backlog of observation stores.  So the digits
// are drawn ahead of time and kept NEXT TO THE STATE:
//   * ring: SLOTS = 64 digits of DB bits (4 for G <= 15, else 8) per env in COLS uint4 columns, struct-of-arrays like the state
//     (column c of env i at dq[c*N + i]); the digit of generator word w sits in slot w mod 64.
//   * cursor: Env::mt_pos = first word that has not been turned into a digit yet (0..624), Env::dq_left = digits not consumed
//     yet — those of words [mt_pos - dq_left, mt_pos), so the ring's head slot is (mt_pos - dq_left) mod 64 and the stream's
//     CPython cursor is mt_pos - dq_left.  Both live in the hot record: a placement costs no dependent "load the cursor" trip.
//   * refill (dq_refill): wave-cooperative and per env — lane l serves slot l: it loads the three state words its word needs
//     (64 CONSECUTIVE words per load instruction: coalesced, unlike a lane walking its own block), twists the word in place
//     (the block is advanced exactly as CPython's batch regeneration would, one word at a time), tempers it and ORs the digit
//     into the ring.  A refill tops the ring up to 64 digits but never crosses word 623: every parked digit belongs to the
//     generation of mt_pos, which keeps cge_snake_get_state's canonical (CPython) form a plain "twist the rest" away; the
//     generation wraps when the ring is empty at word 624.
//   * use: step() loads the ring columns of just the lanes that place food (~8 %), the fused rollout parks every lane's ring in
//     LDS for the launch and tops up the lanes that are likely to run dry (threshold by k_steps) before the first observation
//     store is in flight; both write a ring back only if it was refilled.  There is ONE rollout kernel for every k_steps
//     (round 2 had a per-launch queue for k >= 24 and per-step window loads below: the driver's 20-step launch ran the slow one).
template <int G>
struct DigitQ {
    static constexpr int DB = Lay<G>::KBITS <= 4 ? 4 : 8;      // stored bits per digit
    static constexpr int PER = 32 / DB;                        // digits per dword = digits examined per placement round
    static constexpr int SLOTS = 64;
    static constexpr int QDW = SLOTS / PER;                    // dwords per ring (8 or 16)
    static constexpr int COLS = QDW / 4;                       // uint4 columns per env
    static constexpr int QROW = QDW + 1;                       // LDS row stride in dwords (odd: the 64 rows start in different banks)
    static constexpr uint32_t DMASK = (1u << DB) - 1u;
    static constexpr uint32_t ALL_COLS = (1u << COLS) - 1u;
};

// per-lane view of the ring while a kernel runs: the lane's row of the wave's LDS rows, which columns of it are loaded, whether
// it has to go back to HBM
template <int G>
struct DqCtx {
    uint32_t *wave_q;      // LDS: `stride` dwords per lane of this wave, the first QDW of them the ring
    uint32_t stride;       // >= QDW, odd where it can be (QROW in a dedicated array; the step kernel borrows its obs tile rows: OBS_DW)
    uint32_t *blk;         // this lane's generator block
    uint4 *dq;             // global ring columns
    int64_t n, i;          // batch size, this lane's env (a valid env for every lane, see the callers)
    uint32_t loaded;       // bit c: column c of this lane's row is in LDS
    bool dirty;

    __device__ __forceinline__ uint32_t *my_row() const { return wave_q + (threadIdx.x & 63u) * stride; }
    // every column of this lane's ring (fused rollout, launch start), in two halves so that the caller can put its own loads
    // (the env record) into the same round trip
    __device__ __forceinline__ void issue_all(uint4 (&v)[DigitQ<G>::COLS]) const {
#pragma unroll
        for (int c = 0; c < DigitQ<G>::COLS; ++c) v[c] = dq[(int64_t)c * n + i];
    }
    __device__ __forceinline__ void park_all(const uint4 (&v)[DigitQ<G>::COLS]) {
        uint32_t *row = my_row();
#pragma unroll
        for (int c = 0; c < DigitQ<G>::COLS; ++c) { row[4 * c] = v[c].x; row[4 * c + 1] = v[c].y; row[4 * c + 2] = v[c].z; row[4 * c + 3] = v[c].w; }
        loaded = DigitQ<G>::ALL_COLS;
    }
    // the (at most two) columns a placement round reads, c0 and c1, for the lanes with `want`: both loads are issued inside ONE
    // predicated region, so a wave whose lanes need different columns still pays one memory round trip (a load per `if` would
    // be closed by its own s_waitcnt); c1 == c0 re-reads the same 16 bytes
    __device__ __forceinline__ void load_pair(bool want, uint32_t c0, uint32_t c1) {
        if (want && ((~loaded >> c0) & 1u || (~loaded >> c1) & 1u)) {
            uint32_t *row = my_row();
            const uint4 v0 = dq[(int64_t)c0 * n + i], v1 = dq[(int64_t)c1 * n + i];
            row[4 * c0] = v0.x; row[4 * c0 + 1] = v0.y; row[4 * c0 + 2] = v0.z; row[4 * c0 + 3] = v0.w;
            row[4 * c1] = v1.x; row[4 * c1 + 1] = v1.y; row[4 * c1 + 2] = v1.z; row[4 * c1 + 3] = v1.w;
            loaded |= (1u << c0) | (1u << c1);
        }
    }
    __device__ __forceinline__ void write_back() {
        using Q = DigitQ<G>;
        if (!dirty) return;
        const uint32_t *row = my_row();
#pragma unroll
        for (int c = 0; c < Q::COLS; ++c) dq[(int64_t)c * n + i] = make_uint4(row[4 * c], row[4 * c + 1], row[4 * c + 2], row[4 * c + 3]);
        dirty = false;
    }
};

// Top the rings of the lanes in `want` (a ballot) up to 64 digits, RG envs per memory round trip.  Must be called by all 64
// lanes of the wave.  Every load of a round precedes its stores (program order); lanes whose slot is not being filled re-read
// the first word of the run.
template <int G, int RG = 2>
__device__ __forceinline__ void dq_refill(Env<G> &e, DqCtx<G> &q, unsigned long long want) {
    using L = Lay<G>;
    using Q = DigitQ<G>;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t plo = (uint32_t)reinterpret_cast<uintptr_t>(q.blk), phi = (uint32_t)(reinterpret_cast<uintptr_t>(q.blk) >> 32);
#pragma unroll 1
    while (want) {
        int r[RG];
        bool has[RG];
        uint32_t pos[RG], pretw[RG], left[RG], fill[RG], k[RG], a[RG], b[RG], c[RG];
        uint32_t *ob[RG];
#pragma unroll
        for (int g = 0; g < RG; ++g) {
            has[g] = want != 0ull;
            r[g] = has[g] ? (int)__builtin_ctzll(want) : r[0];
            want = has[g] ? (want & (want - 1ull)) : 0ull;
            uint32_t p = lane_u32(e.mt_pos, r[g]) & 1023u, lf = lane_u32(e.dq_left, r[g]) & 127u, pt = lane_u32(e.mt_pretw, r[g]);
            p = p < (uint32_t)MT_N ? p : (uint32_t)MT_N;       // a valid cursor is <= 624: keeps every index inside the 640-word block
            lf = lf < (uint32_t)Q::SLOTS ? lf : (uint32_t)Q::SLOTS;
            if (p == (uint32_t)MT_N && lf == 0u) { p = 0u; pt = 0u; }          // the generation wraps on an empty ring
            const uint32_t room = (uint32_t)Q::SLOTS - lf, rest = (uint32_t)MT_N - p;
            pos[g] = p; pretw[g] = pt; left[g] = lf; fill[g] = room < rest ? room : rest;
            const uint32_t j = (lane - p) & 63u;               // slot `lane` holds word p + j
            const uint32_t kk = j < fill[g] ? p + j : (p < (uint32_t)MT_N ? p : 0u);
            const uint32_t km = kk + MT_M >= (uint32_t)MT_N ? kk + MT_M - MT_N : kk + MT_M;
            k[g] = kk;
            ob[g] = lane_ptr(plo, phi, r[g]);
            a[g] = ob[g][kk]; b[g] = ob[g][kk + 1]; c[g] = ob[g][km];          // kk + 1 <= 624: word 624 mirrors word 0 (cge_device.hpp)
        }
#pragma unroll
        for (int g = 0; g < RG; ++g) {
            if (!has[g]) continue;                             // wave-uniform
            const bool active = ((lane - pos[g]) & 63u) < fill[g];
            const bool ready = k[g] < pretw[g];                // an imported CPython state: this generation's words are already twisted
            const uint32_t y = ready ? a[g] : mt_twist(a[g], b[g], c[g]);
            if (active && !ready) mt_store(ob[g], k[g], y);
            const uint32_t sh = (lane % Q::PER) * Q::DB;
            uint32_t x = active ? (mt_temper(y) >> (32 - L::KBITS)) << sh : 0u;
            uint32_t m = active ? Q::DMASK << sh : 0u;
            x |= shfl_u32(x, lane ^ 1u); m |= shfl_u32(m, lane ^ 1u);           // OR over each aligned group of PER lanes -> one ring dword
            x |= shfl_u32(x, lane ^ 2u); m |= shfl_u32(m, lane ^ 2u);
            if (Q::PER == 8) { x |= shfl_u32(x, lane ^ 4u); m |= shfl_u32(m, lane ^ 4u); }
            uint32_t *row = q.wave_q + (uint32_t)r[g] * q.stride;
            if (lane % Q::PER == 0u && m) row[lane / Q::PER] = (row[lane / Q::PER] & ~m) | x;
            if (lane == (uint32_t)r[g]) {
                e.mt_pos = pos[g] + fill[g];
                e.mt_pretw = pretw[g];
                e.dq_left = left[g] + fill[g];
                q.dirty = true;
                q.loaded = Q::ALL_COLS;                        // every slot that means anything is in the row now
            }
        }
    }
}

// a ring can take more digits: it is not full, and it is not sitting at the end of a generation with digits of it still unused
template <int G>
__device__ __forceinline__ bool dq_can_fill(const Env<G> &e) {
    return e.dq_left < (uint32_t)DigitQ<G>::SLOTS && !(e.mt_pos >= (uint32_t)MT_N && e.dq_left > 0u);
}

// _place_food (snake_env.py:121-129) out of the lane's digit ring: `random.randint(0,G-1)` twice (row first, then column), each
// _randbelow(G): r = getrandbits(k), redrawn while r >= G; the pair is redrawn while it lies on the snake.  Must be called by all
// 64 lanes of the wave.  FETCH: the ring columns a round needs are loaded on demand (step() / reset()); the rollout has them all.
template <int G, bool FETCH>
__device__ __forceinline__ void dq_place_food(Env<G> &e, DqCtx<G> &q, bool need) {
    using L = Lay<G>;
    using Q = DigitQ<G>;
    const uint32_t *myq = q.my_row();
    bool pending = need;
    uint32_t phase = 0, row = 0;
#pragma unroll 1
    while (__ballot(pending)) {
        if (FETCH) {
            const uint32_t head = (e.mt_pos - e.dq_left) & 63u, d0 = head / Q::PER, d1 = (d0 + 1u) & (uint32_t)(Q::QDW - 1);
            q.load_pair(pending && e.dq_left != 0u, d0 >> 2, d1 >> 2);
        }
        const unsigned long long dry = __ballot(pending && e.dq_left < (uint32_t)Q::PER && dq_can_fill<G>(e));
        if (dry) dq_refill<G>(e, q, dry);                      // wave-convergent; once per ~256 env-steps per env
        const uint32_t head = (e.mt_pos - e.dq_left) & 63u;
        const uint32_t idx = head / Q::PER, off = (head % Q::PER) * Q::DB;
        uint32_t bits = (uint32_t)((((uint64_t)myq[(idx + 1u) & (uint32_t)(Q::QDW - 1)] << 32) | (uint64_t)myq[idx]) >> off);
        const uint32_t avail = e.dq_left < (uint32_t)Q::PER ? e.dq_left : (uint32_t)Q::PER;
        if (avail < (uint32_t)Q::PER) bits |= 0xFFFFFFFFu << (avail * Q::DB);   // slots past the ring's end read as digits >= G: skipped
        uint32_t used = 0;
        bool done = !pending;
        if constexpr (L::TIGHT) {                              // 10x10: bit-parallel scan of the 8 digits (snake_place.hpp)
            const uint64_t lo = (uint64_t)e.occ[0] | ((uint64_t)e.occ[1] << 32), hi = (uint64_t)e.occ[2] | ((uint64_t)e.occ[3] << 32);
            const PlaceScan r = place_scan8<G>(bits, phase, row, lo, hi);
            if (pending) { used = r.used; phase = r.phase; row = r.row; done = r.done; if (r.done) e.food = r.food; }
        } else {
#pragma unroll
            for (int j = 0; j < Q::PER; ++j) {
                if (!done) {
                    const uint32_t r = (bits >> (Q::DB * j)) & Q::DMASK;
                    used = j + 1;
                    if (r < (uint32_t)G) {
                        if (phase == 0) {
                            row = r;
                            phase = 1;
                        } else {
                            phase = 0;
                            const uint32_t cell = row * G + r;
                            if (!e.occupied(cell)) { e.food = cell; done = true; }
                        }
                    }
                }
            }
        }
        if (pending) {
            e.dq_left -= used < avail ? used : avail;
            if (done) { pending = false; e.flags |= F_FOOD_VALID; }
        }
    }
}

enum : uint32_t { T_NEED_FOOD = 1u, T_WAS_RESET = 2u, T_DEFERRED = 4u, T_FIN_ROW = 8u };   // T_FIN_ROW: the lane's LDS row now holds its terminal observation

// SameStep: the terminal observation of a lane whose episode just ended (rare lanes only: direct row store).  step(): row i of
// final_obs_out; fused rollout: the next slots of the wave's segment of the compacted side output (FinalSeg, cge_device.hpp) — the
// lanes that are in here together rank themselves by a ballot; fin_base = rows the segment holds before them
// FIN: the kernel instance serves the rollouts' compacted side output (p.fin); the instances without it carry none of its code
template <int G, bool FIN = false>
__device__ __forceinline__ void write_final_obs(const Env<G> &e, const Params &p, int64_t i, int64_t t = 0, uint32_t fin_base = 0) {
    using L = Lay<G>;
    int8_t *dst;
    if (FIN && p.fin.rows) {
        const int64_t gs = final_slot(p.fin, i >> 6, fin_base, true, t, i);
        if (gs < 0) return;
        dst = static_cast<int8_t *>(p.fin.rows) + gs * L::CELLS;
    } else if (p.final_obs) {
        dst = p.final_obs + i * L::CELLS;
    } else {
        return;
    }
    if constexpr (L::PACKED) {
        uint32_t *frow = reinterpret_cast<uint32_t *>(dst);
        e.write_obs_body(frow);
        e.write_obs_food(frow);
    } else {                                                   // odd G: rows are not dword aligned and end inside a dword (rare lanes: byte stores)
        int8_t *frow = dst;
        const bool fv = e.flags & F_FOOD_VALID;
#pragma unroll 1
        for (uint32_t c = 0; c < (uint32_t)L::CELLS; ++c) frow[c] = (fv && c == e.food) ? 2 : (int8_t)e.occupied(c);
    }
}

// One env transition with fused auto-reset.  Everything except the food draw happens first; the RNG
// window load is issued, the obs body is staged while it is in flight, then the food is placed.
template <int G, int MODE, bool FIN = false>
__device__ __forceinline__ uint32_t transition(Env<G> &e, const Params &p, int64_t i, uint32_t action, bool valid_action,
                                               uint32_t *__restrict__ obs_row, float &reward, bool &term, bool short_wave, int64_t t = 0,
                                               uint32_t fin_base = 0, int8_t *__restrict__ fin_rowb = nullptr, uint32_t old_tail = 0) {
    bool need_food = false, was_reset = false, deferred = false, fin_row = false;
    reward = 0.0f;
    term = false;
    if (MODE == CGE_AUTORESET_NEXT_STEP && (e.flags & F_NEEDS_RESET)) {
        e.reset_body();
        need_food = true; was_reset = true;
    } else if (!valid_action) {
        atomicAdd(p.err_count, 1ull);   // reference: ValueError (snake_env.py:69-70)
    } else {
        term = e.move(action, (uint32_t)p.max_steps, reward, need_food, short_wave);
        if (term) {
            e.episodes += 1;
            // episode statistics need no accumulator here: every reward is +10 per point of `score`, -10 for the collision that
            // ends the episode (which is not counted in `steps`, snake_env.py:88-94), 0 otherwise
            const bool crashed = reward < 0.0f;
            if (p.ep_ret) p.ep_ret[i] = 10.0 * (double)e.score - (crashed ? 10.0 : 0.0);
            if (p.ep_len) p.ep_len[i] = (int32_t)e.steps + (crashed ? 1 : 0);
            if (MODE == CGE_AUTORESET_SAME_STEP) {
                if (need_food) {
                    // time limit on a step that also ate: the reference places the new food (snake_env.py:104) BEFORE it tests
                    // steps >= max_steps (:113), so the terminal obs shows it and the reset draws a second one.  Both draws go
                    // through the caller's wave-cooperative placement: this round places the post-eat food, finish_deferred()
                    // then writes the terminal obs, resets, and the caller runs a second round.
                    deferred = true;
                } else {
                    if (FIN && fin_rowb) {
                        // fused rollout: the lane's LDS row — the previous step's observation, kept incrementally — BECOMES the terminal one:
                        // a crash returns the unchanged board (snake_env.py:88-94), a time limit the board after the move (head on, vacated
                        // tail off; the food stays: this branch did not eat).  The caller copies the row to the lane's slot of the side
                        // output with one coalesced store per finishing env, then clears it for the reset.  (Built from the record and
                        // stored dword by dword by every finishing lane — SOME lane of a 64-env wave in 99 % of the steps — the terminal
                        // rows cost the 1M-env rollout 7 us of its 23 per step.)
                        if (!crashed) { fin_rowb[e.head] = 1; if (e.tail != old_tail) fin_rowb[old_tail] = 0; }
                        fin_row = true;                          // slot, index entry and the copy: by the caller, on wave-uniform values
                    } else {
                        write_final_obs<G, FIN>(e, p, i, t, fin_base);
                    }
                    e.reset_body();
                    need_food = true; was_reset = true;
                }
            } else if (MODE == CGE_AUTORESET_NEXT_STEP) {
                e.flags |= F_NEEDS_RESET;
            }
        }
    }
    if (need_food) need_food = e.can_place_food();
    if (obs_row) e.write_obs_body(obs_row);
    // the caller runs dq_place_food with the whole wave, then (T_DEFERRED, rare) finish_deferred + a second round, then write_obs_food
    return (need_food ? T_NEED_FOOD : 0u) | (was_reset ? T_WAS_RESET : 0u) | (deferred ? T_DEFERRED : 0u) | (fin_row ? T_FIN_ROW : 0u);
}

// second half of a SameStep episode end whose last step also ate (see transition): terminal obs with the post-eat food, reset.
// Returns whether the fresh episode needs its food placed (always, unless the board were full).
template <int G, bool FIN = false>
__device__ __forceinline__ bool finish_deferred(Env<G> &e, const Params &p, int64_t i, uint32_t *__restrict__ obs_row, int64_t t = 0,
                                                uint32_t fin_base = 0) {
    write_final_obs<G, FIN>(e, p, i, t, fin_base);
    e.reset_body();
    if (obs_row) e.write_obs_body(obs_row);
    return e.can_place_food();
}

// Odd G: the LDS rows are padded to whole dwords (ROW_DW each) while the destination is G*G bytes per row, back to back.  `nthreads`
// threads numbered tid stream `nrows` rows as whole dwords of the DESTINATION, gathering each dword's four bytes from the padded
// rows (byte-granular LDS reads: a generic path for the odd grids — the reference's scripts use 15 — not a tuned one).
template <int CELLS, int ROW_DW>
__device__ __forceinline__ void store_rows_realign(const uint32_t *rows, int8_t *dst, uint32_t nrows, uint32_t tid, uint32_t nthreads) {
    const uint8_t *rb = reinterpret_cast<const uint8_t *>(rows);
    auto src = [&](uint32_t b) { const uint32_t r = b / (uint32_t)CELLS; return rb[r * (uint32_t)(ROW_DW * 4) + (b - r * (uint32_t)CELLS)]; };
    const uint32_t total = nrows * (uint32_t)CELLS;
    // the destination need not be dword aligned (a [k, N, G, G] trajectory with N*G*G odd): `head` bytes up to the first aligned
    // dword and the bytes behind the last whole one are written one by one
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 3u), head0 = mis ? 4u - mis : 0u, head = head0 < total ? head0 : total;
    const uint32_t ndw = (total - head) >> 2;
    uint32_t *d1 = reinterpret_cast<uint32_t *>(dst + head);
    for (uint32_t q = tid; q < ndw; q += nthreads) {
        const uint32_t b0 = head + 4u * q;
        uint32_t r = b0 / (uint32_t)CELLS, c = b0 - r * (uint32_t)CELLS, w = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            w |= (uint32_t)rb[r * (uint32_t)(ROW_DW * 4) + c] << (8 * k);
            if (++c == (uint32_t)CELLS) { c = 0; ++r; }
        }
        d1[q] = w;
    }
    if (tid == 0) {
        for (uint32_t b = 0; b < head; ++b) dst[b] = (int8_t)src(b);
        for (uint32_t b = head + (ndw << 2); b < total; ++b) dst[b] = (int8_t)src(b);
    }
}

// One wave streams its own 64 obs rows (FULL contiguous bytes) from LDS to HBM: (ds_read_b128, global_store_dwordx4) pairs at
// constant offsets, two pairs in flight at a time — the fully unrolled copy kept 28 VGPRs of tile data live across the step and
// cost a wave per SIMD of occupancy.  Partial last wave / unaligned destination: the generic store_tile paths.
template <int FULL>
__device__ __forceinline__ void store_wave_rows(const uint32_t *rows, int8_t *dst, uint32_t bytes_valid, uint32_t lane) {
    if (bytes_valid == (uint32_t)FULL && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
        constexpr int NVEC = FULL / 16, ITERS = NVEC / 64, TAIL = NVEC % 64;
        static_assert(FULL % 16 == 0, "whole tiles are a multiple of 16 bytes");
        const uint4 *t4 = reinterpret_cast<const uint4 *>(rows) + lane;
        uint4 *d4 = reinterpret_cast<uint4 *>(dst) + lane;
#pragma unroll 2
        for (int it = 0; it < ITERS; ++it) d4[it * 64] = t4[it * 64];
        if (TAIL && lane < (uint32_t)TAIL) d4[ITERS * 64] = t4[ITERS * 64];
        return;
    }
    store_tile<64, 0>(rows, dst, bytes_valid, lane);
}

template <int G, int BLOCK, int MINW, int MODE>
__global__ __launch_bounds__(BLOCK, MINW) void step_kernel(Params p) {
    using L = Lay<G>;
    using Q = DigitQ<G>;
    constexpr bool OVERLAY = L::OBS_DW >= Q::QDW;               // a ring row fits a lane's obs row (not for G < 6)
    __shared__ uint4 tile4[(BLOCK * L::OBS_DW + 3) / 4];
    __shared__ uint32_t qown[OVERLAY ? 1 : BLOCK * Q::QROW];
    uint32_t *tile = reinterpret_cast<uint32_t *>(tile4);
    const int64_t first = (int64_t)blockIdx.x * BLOCK;
    const int64_t i = first + threadIdx.x;
    const bool live_lane = i < p.n;
    const int64_t li = live_lane ? i : first;
    Env<G> e;
    e.load(p.state, p.n, li);
    float r = 0.0f;
    bool term = false;
    uint32_t tf = 0;
    uint32_t *row = tile + threadIdx.x * L::OBS_DW;
    const bool short_wave = __ballot(e.len > 15u) == 0ull;     // every history of this wave fits one word (see Env::move)
    if (live_lane) {
        const int32_t a = p.actions[i];
        tf = transition<G, MODE>(e, p, i, (uint32_t)a, (uint32_t)a <= 3u, nullptr, r, term, short_wave);
    }
    // Only the lanes that place food (~8 %) touch their digit ring: two dwords of it, fetched on demand (dq_place_food<.., true>).
    // The ring rows borrow the lanes' own obs tile rows (the observation is staged after the placement): a separate 9 KB array
    // took the kernel from 6 to 4 workgroups per CU.  Measured on one box and dropped (round 3, gpurun_out/r3_ab_step1.txt):
    // prefetching every lane's ring next to the hot record (no dependent round trip, +32 B per env-step) 35.0 vs 34.8-35.1 us;
    // every wave streaming its own 64 rows without the workgroup barrier 35.0-35.5 us — the kernel runs at the box's copy
    // bandwidth on the 157 B per env-step it moves, the second round trip is hidden by the other 23 waves of the CU.
    DqCtx<G> q{OVERLAY ? tile + (threadIdx.x & ~63u) * L::OBS_DW : qown + (threadIdx.x & ~63u) * Q::QROW,
               (uint32_t)(OVERLAY ? L::OBS_DW : Q::QROW), p.mt + li * MT_STRIDE, p.dq, p.n, li, 0u, false};
    dq_place_food<G, true>(e, q, tf & T_NEED_FOOD);
    bool again = false;
    if (__ballot(tf & T_DEFERRED)) {                           // rare, wave-uniform: see transition()
        again = (tf & T_DEFERRED) && finish_deferred<G>(e, p, i, nullptr);
        dq_place_food<G, true>(e, q, again);
    }
    if (live_lane) q.write_back();                             // before the row is reused for the observation
    e.write_obs_body(row);
    if (live_lane) {
        e.write_obs_food(row);
        e.store(p.state, p.n, i);
        p.reward[i] = r;
        p.terminated[i] = term ? 1 : 0;
        if (p.truncated) p.truncated[i] = 0;   // reference never truncates (snake_env.py:119)
    }
    lds_barrier();
    const int64_t live = p.n - first < BLOCK ? p.n - first : BLOCK;
    if constexpr (L::PACKED) store_tile<BLOCK, BLOCK * L::CELLS>(tile, p.obs + first * L::CELLS, (uint32_t)(live * L::CELLS));
    else store_rows_realign<L::CELLS, L::OBS_DW>(tile, p.obs + first * L::CELLS, (uint32_t)live, threadIdx.x, BLOCK);
}

// k fused steps per launch: state stays in VGPRs, only the obs rows (+ optional per-step reward / flag / explicit actions) touch
// HBM per step.  Every WAVE is on its own here — no workgroup barrier anywhere in the kernel: a wave keeps the 64 observation
// rows of its envs in LDS (updated incrementally), streams them out itself after each step (6400 contiguous bytes for 10x10:
// six full 1-KiB store instructions and a 256-byte tail) and goes straight on to the next transition while the stores drain.
// History: round 1 gave the stores to a dedicated writer wave behind two LDS-only barriers per step, because on gfx950 loads
// and stores retire through one in-order counter and a compute wave's next food-placement LOADS had to wait for its own obs
// STORES.  Pre-drawn digits (round 2: a per-launch queue; now the env's persistent ring, DigitQ) removed the global loads from
// the step loop, and with them the reason for the writer: measured on 1M envs with every step's obs written to a [K, N, 100]
// trajectory, writer-wave kernel 28.5-38 us per step (74 % of wave time parked at the barriers), this kernel see DESIGN.md 6.
// FIN: launched when the caller registered the terminal-observation side output.  Two instances on purpose: with the side output's code
// compiled in, the SAME_STEP instance needs 157 registers instead of 116 and 410 more instructions, and runs 7-10 % slower even with the
// side output idle (same box, 22.3-23.0 vs 24.1-25.6 us per 1M-env step: profiles/r04_snake_final_rows_ab.txt).
template <int G, int BLOCK, int MINW, int MODE, bool ACTIONS, bool FIN>
__global__ __launch_bounds__(BLOCK, MINW) void rollout_kernel(Params p) {
    using L = Lay<G>;
    using Q = DigitQ<G>;
#ifndef CGE_SNAKE_TOPUP_RG
#define CGE_SNAKE_TOPUP_RG 8
#endif
    constexpr int TOPUP_RG = CGE_SNAKE_TOPUP_RG;
    __shared__ uint4 tile4[(BLOCK * L::OBS_DW + 3) / 4];
    __shared__ uint32_t qmem[BLOCK * Q::QROW];
    uint32_t *tile = reinterpret_cast<uint32_t *>(tile4);
    const int64_t first = (int64_t)blockIdx.x * BLOCK;
    const int64_t wfirst = first + (threadIdx.x & ~63u);       // first env of this wave
    if (wfirst >= p.n) return;                                 // a wholly dead wave of the last workgroup (no barriers to miss)
    const int64_t wlive = p.n - wfirst < 64 ? p.n - wfirst : 64;
    const int64_t i = first + threadIdx.x;
    const bool live_lane = i < p.n;
    const int64_t li = live_lane ? i : wfirst;                 // dead lanes of the last wave mirror a valid env: the cooperative
    Env<G> e;                                                  // refill reads every lane's cursor (and never serves a dead lane)
    uint64_t key = 0;
    float rsum = 0.0f;
    int32_t dcount = 0;
    uint32_t fin_used = 0;                                     // terminal rows this wave has delivered to its segment of the side output
    // the digit rings of the wave's envs are parked in LDS for the launch; their loads share the env record's round trip
    DqCtx<G> q{qmem + (threadIdx.x & ~63u) * Q::QROW, (uint32_t)Q::QROW, p.mt + li * MT_STRIDE, p.dq, p.n, li, 0u, false};
    uint4 ring[Q::COLS];
    q.issue_all(ring);
    e.load(p.state, p.n, li);
    q.park_all(ring);
    if (live_lane) key = hash_env_key(p.a_seed, (uint64_t)(p.env0 + i));
    // The lane's obs row lives in LDS for the whole rollout and is kept up to date INCREMENTALLY: a move sets the new head
    // byte and clears the vacated tail byte, a new food sets one byte; only an episode reset rewrites the row, and that is
    // done by the wave together (25 lanes clear the row of each resetting env) — rebuilding 25 dwords per lane per step
    // cost every wave ~175 VALU for the ~7 % of lanes that had actually changed more than two cells.
    uint32_t *row = p.obs ? tile + threadIdx.x * L::OBS_DW : nullptr;
    int8_t *rowb = reinterpret_cast<int8_t *>(row);
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t *wave_rows = tile + (threadIdx.x & ~63u) * L::OBS_DW;
    // SAME_STEP terminal rows through the LDS rows (dword-aligned 4 G^2-byte rows only; else every finishing lane stores its own)
    int8_t *const fin_rowb = (FIN && CGE_SNAKE_FINCOPY != 0 && MODE == CGE_AUTORESET_SAME_STEP && L::PACKED && row && p.fin.rows) ? rowb : nullptr;
    uint32_t *const fin_rows_seg = static_cast<uint32_t *>(p.fin.rows) + (wfirst >> 6) * p.fin.cap * L::OBS_DW;    // this wave's segment (wave-uniform)
    int64_t *const fin_index_seg = p.fin.index + (wfirst >> 6) * p.fin.cap;
    if (row && live_lane) { e.write_obs_body(row); e.write_obs_food(row); }
    // ACTIONS (compile time): explicit [k, n] actions, fetched one step ahead so the load's latency hides behind the previous step.
    // The hash-action instance has NO global load in its step loop on the common path — on purpose: gfx950 counts loads and
    // stores in one in-order counter, and a load that is merely POSSIBLE on some path makes the compiler put `s_waitcnt vmcnt(0)`
    // at the join, which also drains the wave's observation stores (round 2, found in the ISA).  The ring refill below is the one
    // exception: wave-uniform, behind a scalar branch that is taken once per ~4 wave-steps in long launches and (with the top-up
    // before the loop) practically never in short ones.
    uint32_t a_next = (ACTIONS && live_lane && p.k_steps > 0) ? (uint32_t)p.actions[i] : 0u;
    // rings that could run dry during the launch are topped up now, before the first observation store is in flight
    {
        const unsigned long long low = __ballot(live_lane && e.dq_left < p.dq_topup && dq_can_fill<G>(e));
        if (low) dq_refill<G, TOPUP_RG>(e, q, low);            // several envs per round trip: nothing else is live yet
    }
    for (int t = 0; t < p.k_steps; ++t) {
        float r = 0.0f;
        bool term = false, need_food = false, was_reset = false;
        uint32_t tf = 0;
        const uint32_t old_head = e.head, old_tail = e.tail;
        const bool short_wave = __ballot(e.len > 15u) == 0ull;  // every history of this wave fits one word (see Env::move)
        if (live_lane) {
            uint32_t a;
            if constexpr (ACTIONS) {
                a = a_next;
                if (t + 1 < p.k_steps) a_next = (uint32_t)p.actions[(int64_t)(t + 1) * p.n + i];
            } else {
                a = hash_action_from_key(key, (uint64_t)(p.t0 + t), 4u, 0u);
            }
            tf = transition<G, MODE, FIN>(e, p, i, a, a <= 3u, nullptr, r, term, short_wave, t, fin_used, fin_rowb, old_tail);
            need_food = tf & T_NEED_FOOD; was_reset = tf & T_WAS_RESET;
        }
        if (FIN && fin_rowb) {
            // terminal rows staged in the lanes' LDS rows -> the segment's next slots, in lane order; everything but the lane's own index
            // entry is wave-uniform (the segment's pointers and fill count live in scalar registers)
            unsigned long long fm = __ballot((tf & T_FIN_ROW) != 0u);
            if (fm) {
                if (tf & T_FIN_ROW) {
                    const uint32_t slot = fin_used + (uint32_t)__popcll(fm & ((1ull << lane) - 1ull));
                    if ((int64_t)slot < p.fin.cap) fin_index_seg[slot] = (int64_t)t * p.fin.n + i;
                }
                uint32_t k = fin_used;
                while (fm) {                                   // per finishing env, its OBS_DW-dword row in coalesced passes of 64 dwords
                    const uint32_t rl = (uint32_t)__builtin_ctzll(fm);
                    fm &= fm - 1ull;
                    if ((int64_t)k < p.fin.cap && lane < (uint32_t)L::OBS_DW) fin_rows_seg[k * (uint32_t)L::OBS_DW + lane] = wave_rows[rl * L::OBS_DW + lane];
                    if constexpr (L::OBS_DW > 64) {            // even G >= 18: 81..225 dwords, the rest of the row
                        if ((int64_t)k < p.fin.cap)
                            for (uint32_t q2 = lane + 64u; q2 < (uint32_t)L::OBS_DW; q2 += 64u) fin_rows_seg[k * (uint32_t)L::OBS_DW + q2] = wave_rows[rl * L::OBS_DW + q2];
                    }
                    ++k;
                }
            }
        }
        // terminal rows: the lanes that finished without eating wrote theirs inside transition(); those that also ate follow below
        const uint32_t fin_deferred = (FIN && MODE == CGE_AUTORESET_SAME_STEP) ? fin_used + (uint32_t)__popcll(__ballot(term && !(tf & T_DEFERRED))) : 0u;
        // one inlined copy of the placement code, run a second time only when some lane ate on the very step its time limit fired
        // (SameStep: post-eat food, then reset, then the fresh episode's food — rare, wave-uniform)
        bool want = need_food;
#pragma unroll 1
        for (int round = 0; round < 2; ++round) {
            dq_place_food<G, false>(e, q, want);
            if (round == 1 || __ballot(tf & T_DEFERRED) == 0ull) break;
            want = (tf & T_DEFERRED) && finish_deferred<G, FIN>(e, p, i, nullptr, t, fin_deferred);
            if (tf & T_DEFERRED) { was_reset = true; need_food = want; }
        }
        if (FIN && MODE == CGE_AUTORESET_SAME_STEP) fin_used += (uint32_t)__popcll(__ballot(term));
        if (row) {
            unsigned long long rm = __ballot(was_reset);
            while (rm) {                                       // wave-uniform: clear the rows of the envs that were reset
                const uint32_t rl = (uint32_t)__ffsll((long long)rm) - 1u;
                rm &= rm - 1ull;
                if (lane < (uint32_t)L::OBS_DW) wave_rows[rl * L::OBS_DW + lane] = 0u;
                if (L::OBS_DW > 64) for (uint32_t q2 = lane + 64u; q2 < (uint32_t)L::OBS_DW; q2 += 64u) wave_rows[rl * L::OBS_DW + q2] = 0u;
            }
            if (live_lane) {
                if (was_reset) rowb[e.head] = 1;
                else if (e.head != old_head) { rowb[e.head] = 1; if (e.tail != old_tail) rowb[old_tail] = 0; }
                if (need_food) e.write_obs_food(row);
            }
            // the wave's own LDS traffic is ordered (one in-order queue per wave): the tile reads below see the row writes above,
            // and the next step's row writes cannot overtake these reads
            int8_t *dst_t = p.obs + (int64_t)t * p.obs_step_stride + wfirst * L::CELLS;
            if constexpr (L::PACKED) store_wave_rows<64 * L::CELLS>(wave_rows, dst_t, (uint32_t)(wlive * L::CELLS), lane);
            else store_rows_realign<L::CELLS, L::OBS_DW>(wave_rows, dst_t, (uint32_t)wlive, lane, 64u);
        }
        if (live_lane) {
            rsum += r;
            dcount += term ? 1 : 0;
            if (p.reward) p.reward[(int64_t)t * p.n + i] = r;                   // optional [k, n] trajectories
            if (p.terminated) p.terminated[(int64_t)t * p.n + i] = term ? 1 : 0;
        }
    }
    if (live_lane) {
        e.store(p.state, p.n, i);
        q.write_back();
        if (p.reward_sum) p.reward_sum[i] = rsum;
        if (p.done_count) p.done_count[i] = dcount;
        if (FIN && p.fin.count && (threadIdx.x & 63u) == 0u) p.fin.count[wfirst >> 6] = (int32_t)fin_used;
    }
}

template <int G>
__global__ __launch_bounds__(Lay<G>::BLOCK) void reset_kernel(Params p) {
    using L = Lay<G>;
    using Q = DigitQ<G>;
    __shared__ uint4 tile4[(L::BLOCK * L::OBS_DW + 3) / 4];
    __shared__ uint32_t qmem[L::BLOCK * Q::QROW];
    uint32_t *tile = reinterpret_cast<uint32_t *>(tile4);
    const int64_t first = (int64_t)blockIdx.x * L::BLOCK;
    const int64_t i = first + threadIdx.x;
    const bool live_lane = i < p.n;
    const int64_t li = live_lane ? i : first;                  // dead lanes mirror a valid env (they take part in the cooperative refill)
    Env<G> e;
    e.load(p.state, p.n, li);
    uint32_t *row = p.obs ? tile + threadIdx.x * L::OBS_DW : nullptr;
    const bool doit = live_lane && (!p.mask || p.mask[i]);
    bool need_food = false;
    if (doit) {
        e.reset_body();
        need_food = e.can_place_food();
    }
    if (row) e.write_obs_body(row);
    DqCtx<G> q{qmem + (threadIdx.x & ~63u) * Q::QROW, (uint32_t)Q::QROW, p.mt + li * MT_STRIDE, p.dq, p.n, li, 0u, false};
    dq_place_food<G, true>(e, q, need_food);
    if (row) e.write_obs_food(row);
    if (doit) { e.store(p.state, p.n, i); q.write_back(); }
    if (p.obs) {
        lds_barrier();
        const int64_t live = p.n - first < L::BLOCK ? p.n - first : L::BLOCK;
        if constexpr (L::PACKED) store_tile<L::BLOCK>(tile, p.obs + first * L::CELLS, (uint32_t)(live * L::CELLS));
        else store_rows_realign<L::CELLS, L::OBS_DW>(tile, p.obs + first * L::CELLS, (uint32_t)live, threadIdx.x, L::BLOCK);
    }
}

// after (re)seeding: the streams restart at word 0 with nothing pre-twisted
template <int G>
__global__ __launch_bounds__(256) void rewind_kernel(uint4 *__restrict__ state, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    Env<G> e;
    e.load(state, n, i);
    e.mt_pos = 0;
    e.mt_pretw = 0;
    e.dq_left = 0;                                             // digits drawn from the old stream are dropped with it
    e.store(state, n, i);
}

template <int G>
__global__ __launch_bounds__(256) void info_kernel(const uint4 *__restrict__ state, int64_t n, int field, int32_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    Env<G> e;
    e.load(state, n, i);
    int32_t v = 0;
    const bool fv = e.flags & F_FOOD_VALID;
    switch (field) {
        case CGE_SNAKE_INFO_SCORE: v = (int32_t)e.score; break;
        case CGE_SNAKE_INFO_LENGTH: v = (int32_t)e.length(); break;
        case CGE_SNAKE_INFO_STEPS: v = (int32_t)e.steps; break;
        case CGE_SNAKE_INFO_DIRECTION: v = (int32_t)e.dir; break;
        case CGE_SNAKE_INFO_FOOD_R: v = fv ? (int32_t)(e.food / G) : -1; break;
        case CGE_SNAKE_INFO_FOOD_C: v = fv ? (int32_t)(e.food % G) : -1; break;
        case CGE_SNAKE_INFO_BOARD_FULL: v = (e.flags & F_BOARD_FULL) ? 1 : 0; break;
        case CGE_SNAKE_INFO_EPISODES: v = (int32_t)e.episodes; break;
        case CGE_SNAKE_INFO_HEAD_R: v = (int32_t)(e.head / G); break;
        case CGE_SNAKE_INFO_HEAD_C: v = (int32_t)(e.head % G); break;
        case CGE_SNAKE_INFO_NEEDS_RESET: v = (e.flags & F_NEEDS_RESET) ? 1 : 0; break;
    }
    out[i] = v;
}

// _render_rgb_array (snake_env.py:175-188): a 3-colour look-up over the observation — empty black, snake (0,255,0), food (255,0,0) —
// as uint8 [n, G, G, 3].  One thread per output DWORD (4 of the 3*G*G bytes of an env: coalesced 4-byte stores); the env record
// it decodes is shared by the 3*G*G/4 threads of that env and comes from cache.  Not a hot path.
template <int G>
__global__ __launch_bounds__(256) void render_kernel(const uint4 *__restrict__ state, int64_t n, uint32_t *__restrict__ out) {
    using L = Lay<G>;
    constexpr int64_t ROWB = (int64_t)L::CELLS * 3;             // bytes of one env's frame; odd G: not a multiple of 4, so a dword may
    const int64_t total = n * ROWB, ndw = (total + 3) / 4;       // straddle two envs and the output may end inside one
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= ndw) return;
    int64_t i = (4 * gid) / ROWB;
    uint32_t within = (uint32_t)(4 * gid - i * ROWB);
    Env<G> e;
    e.load(state, n, i < n ? i : n - 1);
    uint32_t w = 0, nb = 0;
#pragma unroll
    for (uint32_t b = 0; b < 4; ++b) {
        if (4 * gid + b >= total) break;
        if (within == (uint32_t)ROWB) { within = 0; ++i; e.load(state, n, i); }   // (odd G only)
        const uint32_t cell = within / 3u, ch = within - 3u * cell;
        const bool fv = e.flags & F_FOOD_VALID;
        uint32_t v = 0;
        if (fv && cell == e.food) v = ch == 0u ? 255u : 0u;          // obs == 2 (written last in _get_observation)
        else if (e.occupied(cell)) v = ch == 1u ? 255u : 0u;         // obs == 1
        w |= v << (8u * b);
        ++within; ++nb;
    }
    if (nb == 4) out[gid] = w;
    else for (uint32_t b = 0; b < nb; ++b) reinterpret_cast<uint8_t *>(out)[4 * gid + b] = (uint8_t)(w >> (8u * b));
}

// ------------------------------------------------------------------ host side
struct Ops {
    int cells, cols, block, nw, max_steps_limit;
    void (*rewind)(uint4 *, int64_t, hipStream_t);
    int dq_cols;
    void (*step)(const Params &, hipStream_t, std::string *);
    void (*rollout)(const Params &, hipStream_t, std::string *);
    void (*reset)(const Params &, hipStream_t);
    void (*info)(const uint4 *, int64_t, int, int32_t *, hipStream_t);
    void (*render)(const uint4 *, int64_t, uint32_t *, hipStream_t);
    void (*decode)(const uint32_t *raw, int32_t *hdr, uint16_t *body, uint32_t *mt_pos, uint32_t *mt_pretw, uint32_t *dq_left);
    bool (*encode)(const int32_t *hdr, const uint16_t *body, uint32_t mt_pos, uint32_t mt_pretw, uint32_t *raw);
};

template <int G>
void decode_env(const uint32_t *raw, int32_t *hdr, uint16_t *body, uint32_t *mt_pos, uint32_t *mt_pretw, uint32_t *dq_left) {
    using L = Lay<G>;
    Env<G> e;
    e.unpack(raw);
    *mt_pos = e.mt_pos;
    *mt_pretw = e.mt_pretw;
    *dq_left = e.dq_left;
    const int len = (int)e.length();
    const bool fv = e.flags & F_FOOD_VALID;
    hdr[0] = len; hdr[1] = (int32_t)e.dir;
    hdr[2] = fv ? (int32_t)(e.food / G) : -1; hdr[3] = fv ? (int32_t)(e.food % G) : -1;
    hdr[4] = (int32_t)e.score; hdr[5] = (int32_t)e.steps; hdr[6] = (e.flags & F_NEEDS_RESET) ? 1 : 0;
    // walk head -> tail against the move history (the Python list's order)
    uint32_t c = e.head;
    for (int k = 0; k < L::CELLS; ++k) {
        body[k] = k < len ? (uint16_t)c : 0xFFFF;
        if (k + 1 < len) c = (uint32_t)((int)c - dir_delta((e.sr[k >> 4] >> ((k & 15) * 2)) & 3u, G));
    }
}

// false: the body is not a path of unit moves inside the board (no such list can arise from the reference's step())
template <int G>
bool encode_env(const int32_t *hdr, const uint16_t *body, uint32_t mt_pos, uint32_t mt_pretw, uint32_t *raw) {
    Env<G> e;
    memset(&e, 0, sizeof e);
    const int len = hdr[0];
    for (int k = 0; k < len; ++k) {
        if (e.occ[body[k] >> 5] & (1u << (body[k] & 31u))) return false;               // a cell twice
        e.occ[body[k] >> 5] |= 1u << (body[k] & 31u);
    }
    for (int k = 0; k + 1 < len; ++k) {   // move k took the snake from body[k+1] to body[k]
        const int from = body[k + 1], to = body[k];
        uint32_t d;
        if (to == from - G) d = 0u;
        else if (to == from + 1 && from % G != G - 1) d = 1u;
        else if (to == from + G) d = 2u;
        else if (to == from - 1 && from % G != 0) d = 3u;
        else return false;
        e.sr[k >> 4] |= d << ((k & 15) * 2);
    }
    e.head = body[0];
    e.tail = body[len - 1];
    e.len = (uint32_t)len;
    e.dir = (uint32_t)hdr[1];
    const bool fv = hdr[2] >= 0;
    e.food = fv ? (uint32_t)(hdr[2] * G + hdr[3]) : 0u;
    e.score = (uint32_t)hdr[4];
    e.steps = (uint32_t)hdr[5];
    e.flags = (hdr[6] ? F_NEEDS_RESET : 0u) | (fv ? F_FOOD_VALID : 0u);
    e.episodes = 0;                        // not part of the canonical record: a restored env starts counting again
    e.mt_pos = mt_pos; e.mt_pretw = mt_pretw;      // the incremental cursor of the canonical index hdr[7] (mt_import_cpython)
    e.pack(raw);
    return true;
}

// the autoreset mode and the action source are compile-time properties of the kernels (no mode tests in the step loop).
// `name` receives the launched kernel as rocprofv3 prints it (cge_snake_last_kernel: bench.py keys its roofline block on it).
template <int G, int BLOCK, int MINW, int MODE>
void launch_mode(const Params &p, bool rollout, hipStream_t s, std::string *name) {
    const dim3 grid((unsigned)((p.n + BLOCK - 1) / BLOCK)), block(BLOCK);
    char buf[96];
    if (!rollout) {
        hipLaunchKernelGGL((step_kernel<G, BLOCK, MINW, MODE>), grid, block, 0, s, p);
        snprintf(buf, sizeof buf, "cge::snake::step_kernel<%d, %d, %d, %d>", G, BLOCK, MINW, MODE);
    } else {
        const bool fin = p.fin.rows != nullptr;
        if (p.actions) { if (fin) hipLaunchKernelGGL((rollout_kernel<G, BLOCK, MINW, MODE, true, true>), grid, block, 0, s, p);
                         else hipLaunchKernelGGL((rollout_kernel<G, BLOCK, MINW, MODE, true, false>), grid, block, 0, s, p); }
        else { if (fin) hipLaunchKernelGGL((rollout_kernel<G, BLOCK, MINW, MODE, false, true>), grid, block, 0, s, p);
               else hipLaunchKernelGGL((rollout_kernel<G, BLOCK, MINW, MODE, false, false>), grid, block, 0, s, p); }
        snprintf(buf, sizeof buf, "cge::snake::rollout_kernel<%d, %d, %d, %d, %s, %s>", G, BLOCK, MINW, MODE, p.actions ? "true" : "false", fin ? "true" : "false");
    }
    if (name) *name = buf;
}
template <int G, int BLOCK, int MINW>
void launch_any(const Params &p, bool rollout, hipStream_t s, std::string *name) {
    if (p.mode == CGE_AUTORESET_SAME_STEP) launch_mode<G, BLOCK, MINW, CGE_AUTORESET_SAME_STEP>(p, rollout, s, name);
    else if (p.mode == CGE_AUTORESET_NEXT_STEP) launch_mode<G, BLOCK, MINW, CGE_AUTORESET_NEXT_STEP>(p, rollout, s, name);
    else launch_mode<G, BLOCK, MINW, CGE_AUTORESET_DISABLED>(p, rollout, s, name);
}

constexpr int MAX_RAW = 4 * Lay<30>::COLS;      // words of the largest grid's device record

template <int G>
Ops make_ops() {
    using L = Lay<G>;
    Ops o;
    o.cells = L::CELLS; o.cols = L::COLS; o.block = L::BLOCK; o.nw = L::NW; o.max_steps_limit = L::MAX_STEPS_LIMIT;
    o.dq_cols = DigitQ<G>::COLS;
    o.rewind = [](uint4 *st, int64_t n, hipStream_t s) {
        hipLaunchKernelGGL(rewind_kernel<G>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, st, n);
    };
    o.step = [](const Params &p, hipStream_t s, std::string *name) { launch_any<G, L::BLOCK, 1>(p, false, s, name); };
    o.rollout = [](const Params &p, hipStream_t s, std::string *name) { launch_any<G, L::BLOCK, 1>(p, true, s, name); };
    o.reset = [](const Params &p, hipStream_t s) {
        hipLaunchKernelGGL(reset_kernel<G>, dim3((unsigned)((p.n + L::BLOCK - 1) / L::BLOCK)), dim3(L::BLOCK), 0, s, p);
    };
    o.info = [](const uint4 *st, int64_t n, int field, int32_t *out, hipStream_t s) {
        hipLaunchKernelGGL(info_kernel<G>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, st, n, field, out);
    };
    o.render = [](const uint4 *st, int64_t n, uint32_t *out, hipStream_t s) {
        const int64_t total = (n * (int64_t)L::CELLS * 3 + 3) / 4;
        hipLaunchKernelGGL(render_kernel<G>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, st, n, out);
    };
    o.decode = decode_env<G>;
    o.encode = encode_env<G>;
    return o;
}

static bool ops_for(int grid, Ops &o) {
    // every grid_size from 4 to 30 (snake_env.py:19 takes any; the reference's scripts use 10, 15 (test_visualization.py:17) and 20);
    // 10 is the tuned benchmark instance (16-byte hot record), the others share the generic record layout
    switch (grid) {
#define CGE_GRID(G_) case G_: o = make_ops<G_>(); return true;
        CGE_GRID(4) CGE_GRID(5) CGE_GRID(6) CGE_GRID(7) CGE_GRID(8) CGE_GRID(9) CGE_GRID(10) CGE_GRID(11) CGE_GRID(12) CGE_GRID(13)
        CGE_GRID(14) CGE_GRID(15) CGE_GRID(16) CGE_GRID(17) CGE_GRID(18) CGE_GRID(19) CGE_GRID(20) CGE_GRID(21) CGE_GRID(22)
        CGE_GRID(23) CGE_GRID(24) CGE_GRID(25) CGE_GRID(26) CGE_GRID(27) CGE_GRID(28) CGE_GRID(29) CGE_GRID(30)
#undef CGE_GRID
    }
    return false;
}

}  // namespace snake
}  // namespace cge

using namespace cge;

struct cge_snake : HandleBase {
    cge_snake_config cfg{};
    snake::Ops ops{};
    uint4 *state = nullptr;
    uint4 *dq = nullptr;           // digit rings (snake::DigitQ)
    uint32_t *mt = nullptr;
    unsigned long long *err = nullptr;

    snake::Params params() const {
        snake::Params p{};
        p.state = state; p.dq = dq; p.mt = mt; p.n = n; p.env0 = env0;
        p.mode = cfg.autoreset_mode; p.max_steps = cfg.max_steps; p.err_count = err;
        p.ep_ret = ep_ret; p.ep_len = ep_len;
        return p;
    }
    // cfg.max_steps == 0: the reference's default (snake_env.py:47)
    static int check(const cge_snake_config &c) {
        if (bad_autoreset_mode(c.autoreset_mode) || c.max_steps < 0 || c.max_steps > 65535) return CGE_ERR_INVALID_ARG;
        snake::Ops o;
        return snake::ops_for(c.grid_size, o) && (c.max_steps ? c.max_steps : 1000) <= o.max_steps_limit ? CGE_OK : CGE_ERR_UNSUPPORTED;
    }
    hipError_t init() {
        if (cfg.max_steps == 0) cfg.max_steps = 1000;
        snake::ops_for(cfg.grid_size, ops);
        CGE_HIP(alloc(state, (size_t)ops.cols * n * sizeof(uint4), true, false));
        CGE_HIP(alloc(mt, (size_t)n * MT_STRIDE * sizeof(uint32_t), false, false));
        CGE_HIP(alloc(dq, (size_t)ops.dq_cols * n * sizeof(uint4), true, false));
        CGE_HIP(alloc(err, sizeof(unsigned long long), true, false));
        // default streams: random.seed(env_index0 + i); default state: reset() so a handle is always steppable
        CGE_HIP(launch_mt_seed(mt, MT_STRIDE, n, nullptr, 0, env0, 0, nullptr));
        ops.reset(params(), nullptr);
        return hipGetLastError();
    }

    // canonical records (cge_host.hpp: get_records / set_records): header int32[8] = {length, direction, food row, food col, score,
    // steps, needs_reset, CPython index}, the 624 generator words, the body head -> tail as uint16 cells (0xFFFF beyond the length)
    static constexpr const char *abi = "cge_snake";
    enum { A_STATE, A_MT };
    size_t record_bytes() const { return (8 * 4 + (size_t)MT_N * 4 + (size_t)ops.cells * 2 + 3) & ~(size_t)3; }
    std::vector<RecordArray> record_arrays() const {
        return {{state, sizeof(uint4), ops.cols, false, true}, {mt, sizeof(uint32_t), MT_STRIDE, true, true}};
    }
    const char *check_record(const uint8_t *p) const {
        const int32_t *hdr = (const int32_t *)p;
        const uint16_t *body = (const uint16_t *)(p + 32 + MT_N * 4);
        const int cells = ops.cells, G = cfg.grid_size;
        if (hdr[0] < 1 || hdr[0] > cells || hdr[1] < 0 || hdr[1] > 3 || hdr[7] < 0 || hdr[7] > MT_N) return "malformed record";
        const bool no_food = hdr[2] == -1 && hdr[3] == -1;
        if ((!no_food && (hdr[2] < 0 || hdr[2] >= G || hdr[3] < 0 || hdr[3] >= G)) || hdr[4] < 0 || hdr[4] > cells || hdr[5] < 0 ||
            hdr[5] > ops.max_steps_limit || (hdr[6] != 0 && hdr[6] != 1))
            return "food / score / steps / needs_reset out of range";
        for (int k = 0; k < hdr[0]; ++k)
            if (body[k] >= cells) return "body cell out of range";
        uint32_t raw[snake::MAX_RAW];                              // encoded and discarded: the path check is the encoder's
        return ops.encode(hdr, body, 0u, 0u, raw) ? nullptr : "the body is not a path of unit moves";
    }
    int to_record(const RecordStage &st, int64_t j, uint8_t *p, const char **why) const {
        uint32_t raw[snake::MAX_RAW];
        for (int c = 0; c < ops.cols; ++c) memcpy(raw + 4 * c, st.at<uint4>(A_STATE, j, c), 16);
        int32_t *hdr = (int32_t *)p;
        uint32_t pos = 0, pretw = 0, left = 0;
        ops.decode(raw, hdr, (uint16_t *)(p + 32 + MT_N * 4), &pos, &pretw, &left);
        if (left > pos) { *why = "corrupted digit-ring cursor"; return CGE_ERR_INVALID_ARG; }
        // Words [pos - left, pos) are twisted already and wait in the env's digit ring (snake::DigitQ): the CPython index is the
        // exported one minus `left`, and since a ring never holds digits of two generations, the export's "twist the rest" completes
        // the generation.  The record keeps the ready mark as one bit (0 or 624), so the export never has a next generation to take
        // back and cannot refuse; with cursor 0 and nothing ready (index 624) left is 0.
        int32_t idx = 0;
        mt_export_cpython(st.at<uint32_t>(A_MT, j), pos, pretw, (uint32_t *)(p + 32), &idx);
        hdr[7] = idx - (int32_t)left;
        const size_t used = 32 + (size_t)MT_N * 4 + (size_t)ops.cells * 2;     // odd G: the record's last two bytes are padding, written as zero
        memset(p + used, 0, record_bytes() - used);
        return CGE_OK;
    }
    void from_record(const uint8_t *p, RecordStage &st, int64_t j) const {
        const int32_t *hdr = (const int32_t *)p;
        uint32_t raw[snake::MAX_RAW], pos, pretw;
        mt_import_cpython((const uint32_t *)(p + 32), hdr[7], st.at<uint32_t>(A_MT, j), &pos, &pretw);
        ops.encode(hdr, (const uint16_t *)(p + 32 + MT_N * 4), pos, pretw, raw);
        for (int c = 0; c < ops.cols; ++c) memcpy(st.at<uint4>(A_STATE, j, c), raw + 4 * c, 16);
    }
};

extern "C" {

const char *cge_version(void) { return "cge_amd 0.1 (gfx950)"; }

uint32_t cge_hash_action(uint64_t a_seed, uint64_t env, uint64_t t, uint32_t n, uint32_t j) {
    return hash_action_from_key(hash_env_key(a_seed, env), t, n, j);
}

CGE_DEFINE_LIFECYCLE(snake)

int cge_snake_seed(cge_snake *h, const uint64_t *seeds, uint64_t base_seed, void *stream) {
    if (!h) return CGE_ERR_INVALID_ARG;
    if (int st = seed_base_check(h, "cge_snake_seed", seeds, base_seed, false)) return st;
    DeviceGuard g(h->device);
    CGE_TRY(h, launch_mt_seed(h->mt, MT_STRIDE, h->n, seeds, base_seed, h->env0, 0, as_stream(stream)));
    h->ops.rewind(h->state, h->n, as_stream(stream));   // stream cursors back to word 0
    return launched(h);
}

int cge_snake_reset(cge_snake *h, const uint8_t *mask, int8_t *obs_out, void *stream) {
    if (!h) return CGE_ERR_INVALID_ARG;
    DeviceGuard g(h->device);
    snake::Params p = h->params();
    p.mask = mask;
    p.obs = obs_out;
    h->ops.reset(p, as_stream(stream));
    return launched(h);
}

int cge_snake_step(cge_snake *h, const int32_t *actions, int8_t *obs_out, float *reward_out, uint8_t *terminated_out,
                   uint8_t *truncated_out, int8_t *final_obs_out, void *stream) {
    snake::Params p;
    if (int st = step_params(h, p, actions && obs_out && reward_out && terminated_out, "cge_snake_step: null actions/obs/reward/terminated pointer",
                             obs_out, reward_out, terminated_out, truncated_out, final_obs_out)) return st;
    DeviceGuard g(h->device);
    p.actions = actions;
    h->ops.step(p, as_stream(stream), &h->last_kernel);
    return launched(h);
}

int cge_snake_rollout(cge_snake *h, int32_t k_steps, const int32_t *actions, uint64_t action_seed, int64_t t0,
                      int8_t *obs_out, int64_t obs_step_stride, float *reward_traj_out, uint8_t *terminated_traj_out,
                      float *reward_sum_out, int32_t *done_count_out, void *stream) {
    if (!h) return CGE_ERR_INVALID_ARG;
    snake::Params p;
    const bool aligned = !((obs_step_stride & 3) && h->ops.cells % 4 == 0);   // (odd grids: a step's N*G*G bytes need not be a multiple of 4)
    const int st = rollout_params(h, p, aligned, h->n * h->ops.cells, "cge_snake_rollout: bad k_steps / obs_step_stride", k_steps, action_seed, t0,
                                  obs_out, obs_step_stride, reward_traj_out, terminated_traj_out, reward_sum_out, done_count_out);
    if (st != CGE_OK || k_steps == 0) return st;
    DeviceGuard g(h->device);
    p.actions = actions;
    // Rings that hold less than one placement round are topped up before the launch's first step; everything else is left to
    // the in-loop refill (wave-convergent, ~0.25 / 64 per env-step).  Measured on 1M envs, us per step at k = 20 / 40 / 100 / 200
    // (gpurun_out/r3_ab_topup.txt, one box): threshold 8-16: 26.5-27.8 / 25.2-26.3 / 24.7-25.4 / 23.4-24.8; 32: 28.5-29.3 / 26.9-27.7 /
    // 25.1-25.9 / 23.4-25.7; 64 (every ring full at the start): 31.5 / 29.2 / 25.9 / 22.8-24.8 — topping every ring up at every
    // launch costs a block visit per env per launch for a handful of digits each.
    p.dq_topup = 12u;
#ifdef CGE_SNAKE_TOPUP_ENV                                        // A/B build only (tools/build_variant.sh): the threshold from the environment
    if (const char *ev = getenv("CGE_SNAKE_TOPUP")) p.dq_topup = (uint32_t)atoi(ev);
#endif
    h->ops.rollout(p, as_stream(stream), &h->last_kernel);
    return launched(h);
}

CGE_DEFINE_FINAL_OBS(snake, int8_t, 64)

int cge_snake_info(cge_snake *h, int32_t field_id, int32_t *out, void *stream) {
    if (!h) return CGE_ERR_INVALID_ARG;
    if (!out || field_id < 0 || field_id > CGE_SNAKE_INFO_NEEDS_RESET)
        return h->fail(CGE_ERR_INVALID_ARG, "cge_snake_info: bad field id / null out");
    DeviceGuard g(h->device);
    h->ops.info(h->state, h->n, field_id, out, as_stream(stream));
    return launched(h);
}

int cge_snake_render_rgb(cge_snake *h, uint8_t *rgb_out, void *stream) {
    if (!h) return CGE_ERR_INVALID_ARG;
    if (!rgb_out || (reinterpret_cast<uintptr_t>(rgb_out) & 3u)) return h->fail(CGE_ERR_INVALID_ARG, "cge_snake_render_rgb: null or unaligned rgb_out");
    DeviceGuard g(h->device);
    h->ops.render(h->state, h->n, reinterpret_cast<uint32_t *>(rgb_out), as_stream(stream));
    return launched(h);
}

CGE_DEFINE_RECORDS(snake)

CGE_DEFINE_ERROR_COUNT(snake)

}  // extern "C"
