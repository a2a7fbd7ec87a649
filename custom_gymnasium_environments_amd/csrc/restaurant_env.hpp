// restaurant_env.hpp — the record and the dynamics of one RestaurantEnv, plain C++ (host and device): restaurant.hip runs it one lane
// per env; tools/probes/restaurant_host_check.cpp replays the reference fixtures through the same code on the CPU.
//
// Re-expresses the reference's restaurant_env_updated/:
//   restaurant_env.py  reset :74-93, step :95-175, _update_environment :268-405, _calculate_efficiency_rewards :407-424,
//                      _get_observation :426-476, _get_info :478-494
//   entities.py        Customer :28-87, Waiter :89-138, Table :140-196, Order :198-224, Kitchen :226-278
// The reference's objects reduce to small lists and masks:
//   waiting line   at most 21 entries (tag, wait_time), FIFO.  One arrival per step at most and every wait grows by one per step, so
//                  the waits fall strictly from the head: only the head can reach the patience limit (20), one customer per step.
//   waiters        (task 0..3, remaining, table) + the wait_time of the customer a seating task carries (it leaves the line when
//                  the task is assigned, stays WAITING — its wait goes on — and is no longer checked for impatience)
//   tables         occupied / dirty / guest-is-eating masks, per table the steps of eating left (a guest served at step s leaves in
//                  the _update_customers of step s + 10) and the guest's wait_time, frozen at seating (_get_info sums it)
//   kitchen        cooking takes a constant 4 steps and at most one order is added per step (one action per step, seating takes a
//                  constant 2), so the cooking list is a 3-slot shift register by progress (1, 2, 3 after a step); an order is ready
//                  in the kitchen update of step order_time + 3, which is how the ready list gets its order_time back
//   ready list     at most 10 entries (tag, table, order_time), FIFO: one order per occupied table
//   ghosts         a seating task that finds its table taken does nothing (:312) and its customer stays WAITING in
//                  `self.customers` forever; only _get_info sees it: a count and a wait sum (sum += count per step)
//   tags           the id columns: one counter per env, restarted by reset, taken by arrivals and by Kitchen.add_order (mod 100)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CGE_HD __host__ __device__ __forceinline__
#else
#define CGE_HD inline
#endif

namespace cge {
namespace restaurant {

constexpr int NT = 10, NW = 10;             // tables, waiters (:19-20)
constexpr int MAXQ = 22;                    // waiting-line slots (21 used at most, see above), two per word
constexpr int QW = MAXQ / 2;
constexpr int NREADY = 10;
constexpr uint32_t SEAT = 1, SERVE = 2, CLEAN = 3;
constexpr uint32_t PATIENCE = 20, EATING = 10;
constexpr int REC_WORDS = 44;               // 11 uint4 columns
constexpr uint32_t CK_VALID = 0x8000u;

// 10-way selects by a runtime index, mask form (an indexed read of a register array would go to scratch)
template <int N>
CGE_HD uint32_t pick(const uint32_t (&a)[N], uint32_t i) {
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < N; ++k) v |= a[k] & (0u - (uint32_t)(i == (uint32_t)k));
    return v;
}
template <int N>
CGE_HD void put(uint32_t (&a)[N], uint32_t i, uint32_t v) {
#pragma unroll
    for (int k = 0; k < N; ++k) a[k] = i == (uint32_t)k ? v : a[k];
}

struct Env {
    uint32_t wq[QW];       // waiting line: entry j = half (j & 1) of wq[j / 2] = tag | wait << 8; entries >= nw are zero
    uint32_t wt[NW];       // waiter: task:2 | remaining:2 << 2 | table:4 << 4 | carried customer's wait << 8
    uint32_t occ, dirty, eating;   // one bit per table
    uint64_t eatc;         // 4 bits per table: _update_customers calls left before the guest leaves
    uint64_t gwait;        // 6 bits per table: the guest's wait_time
    uint32_t ck[3];        // cooking orders with progress 1, 2, 3: CK_VALID | tag | table << 8
    uint32_t rd[NREADY];   // ready list: tag | table << 8 | order_time << 16; entries >= nr are zero
    uint32_t nw, nr, t, serial, needs_reset;
    uint32_t served, left, cleaned, orders, ghosts, ghost_wait;
    double total, ret;     // total_reward (:174 and the completion rewards); the running episode's sum of returned rewards
    uint32_t mt_pos, mt_enc;   // MT19937 cursor and its encoded ready mark (cge_device.hpp)

    CGE_HD void clear() {                                            // reset :74-93 (draws nothing, the stream goes on)
#pragma unroll
        for (int k = 0; k < QW; ++k) wq[k] = 0;
#pragma unroll
        for (int k = 0; k < NW; ++k) { wt[k] = 0; rd[k] = 0; }
        occ = dirty = eating = 0; eatc = 0; gwait = 0;
        ck[0] = ck[1] = ck[2] = 0;
        nw = nr = t = serial = needs_reset = 0;
        served = left = cleaned = orders = ghosts = ghost_wait = 0;
        total = 0.0; ret = 0.0;
    }
    CGE_HD void unpack(const uint32_t (&w)[REC_WORDS]) {
#pragma unroll
        for (int k = 0; k < QW; ++k) wq[k] = w[k];
#pragma unroll
        for (int k = 0; k < NW; ++k) wt[k] = (w[11 + k / 2] >> (16 * (k & 1))) & 0xFFFFu;
        occ = w[16] & 1023u; dirty = (w[16] >> 10) & 1023u; eating = (w[16] >> 20) & 1023u; needs_reset = (w[16] >> 30) & 1u;
        eatc = (uint64_t)w[17] | (uint64_t)w[18] << 32;
        gwait = (uint64_t)w[19] | (uint64_t)w[20] << 32;
        ck[0] = w[21] & 0xFFFFu; ck[1] = w[21] >> 16; ck[2] = w[22] & 0xFFFFu;
        nw = (w[22] >> 16) & 255u; nr = w[22] >> 24;
#pragma unroll
        for (int k = 0; k < NREADY; ++k) rd[k] = w[23 + k];
        t = w[33] & 0xFFFFu; serial = w[33] >> 16;
        served = w[34] & 0xFFFFu; left = w[34] >> 16; cleaned = w[35] & 0xFFFFu; orders = w[35] >> 16;
        ghosts = w[36]; ghost_wait = w[37];
        uint64_t a = (uint64_t)w[38] | (uint64_t)w[39] << 32, b = (uint64_t)w[40] | (uint64_t)w[41] << 32;
        __builtin_memcpy(&total, &a, 8); __builtin_memcpy(&ret, &b, 8);
        mt_pos = w[42] & 1023u; mt_enc = (w[42] >> 10) & 31u;
    }
    CGE_HD void pack(uint32_t (&w)[REC_WORDS]) const {
#pragma unroll
        for (int k = 0; k < QW; ++k) w[k] = wq[k];
#pragma unroll
        for (int k = 0; k < NW / 2; ++k) w[11 + k] = wt[2 * k] | wt[2 * k + 1] << 16;
        w[16] = occ | dirty << 10 | eating << 20 | needs_reset << 30;
        w[17] = (uint32_t)eatc; w[18] = (uint32_t)(eatc >> 32); w[19] = (uint32_t)gwait; w[20] = (uint32_t)(gwait >> 32);
        w[21] = ck[0] | ck[1] << 16; w[22] = ck[2] | nw << 16 | nr << 24;
#pragma unroll
        for (int k = 0; k < NREADY; ++k) w[23 + k] = rd[k];
        w[33] = (t < 0xFFFFu ? t : 0xFFFFu) | serial << 16;       // saturates: a Disabled-mode batch nobody resets stays truncated, arrivals stay off
        w[34] = (served & 0xFFFFu) | left << 16; w[35] = (cleaned & 0xFFFFu) | orders << 16;
        w[36] = ghosts; w[37] = ghost_wait;
        uint64_t a, b;
        __builtin_memcpy(&a, &total, 8); __builtin_memcpy(&b, &ret, 8);
        w[38] = (uint32_t)a; w[39] = (uint32_t)(a >> 32); w[40] = (uint32_t)b; w[41] = (uint32_t)(b >> 32);
        w[42] = mt_pos | mt_enc << 10; w[43] = 0;
    }

    CGE_HD uint32_t take_serial() { const uint32_t s = serial; serial = s == 99u ? 0u : s + 1u; return s; }
    // entry `idx` of the waiting line leaves it; the entries behind move up
    CGE_HD void pop_waiting(uint32_t idx) {
#pragma unroll
        for (int j = 0; j < QW; ++j) {
            const uint32_t nxt = j + 1 < QW ? wq[j + 1 < QW ? j + 1 : j] : 0u;
            const uint32_t up = (wq[j] >> 16) | (nxt << 16), half = (wq[j] & 0xFFFFu) | (nxt << 16);
            wq[j] = 2u * j + 1u < idx ? wq[j] : 2u * j >= idx ? up : half;
        }
        nw -= 1;
    }
    CGE_HD uint32_t waiting_entry(uint32_t idx) const { return (pick(wq, idx >> 1) >> (16u * (idx & 1u))) & 0xFFFFu; }
    // index of the ready order of table tb, or NREADY (Kitchen.get_ready_order_for_table :251-256)
    CGE_HD uint32_t find_ready(uint32_t tb) const {
        uint32_t idx = NREADY;
#pragma unroll
        for (int j = NREADY - 1; j >= 0; --j) idx = ((uint32_t)j < nr && ((rd[j] >> 8) & 255u) == tb) ? (uint32_t)j : idx;
        return idx;
    }
    CGE_HD void pop_ready(uint32_t idx) {
#pragma unroll
        for (int j = 0; j < NREADY; ++j) rd[j] = (uint32_t)j >= idx ? (j + 1 < NREADY ? rd[j + 1 < NREADY ? j + 1 : j] : 0u) : rd[j];
        nr -= 1;
    }

    // one waiter's finished task, _handle_task_completion :292-350; `order`: the order a seating adds (at most one per step)
    CGE_HD void complete(uint32_t task, uint32_t tb, uint32_t cwait, uint32_t &order) {
        const uint32_t bit = 1u << tb;
        if (task == SEAT) {
            if (!((occ | dirty) & bit)) {                            // :312 (the carried customer exists and is WAITING)
                occ |= bit; eating &= ~bit;
                gwait = (gwait & ~((uint64_t)63u << (6u * tb))) | (uint64_t)cwait << (6u * tb);
                order = CK_VALID | take_serial() | tb << 8;
                total += 2.0;
                served += 1;
            } else {                                                 // the table was taken first: a ghost
                ghosts += 1;
                ghost_wait += cwait;
            }
        } else if (task == SERVE) {
            const uint32_t idx = find_ready(tb);
            if ((occ & bit) && idx < (uint32_t)NREADY) {             // :326-341
                const uint32_t otime = pick(rd, idx) >> 16;
                eating |= bit;
                eatc = (eatc & ~((uint64_t)15u << (4u * tb))) | (uint64_t)EATING << (4u * tb);
                pop_ready(idx);
                total += 1.5 + (t - otime <= 5u ? 0.5 : 0.0);
                orders += 1;
            }
        } else if ((dirty & bit) && !(occ & bit)) {                  // :343-350
            dirty &= ~bit;
            total += 1.0;
            cleaned += 1;
        }
    }

    // step :95-175 for the action (type, waiter_id, customer_id, table_id) and the step's random.random() u.
    // Returns the reward (float64, summed in the reference's order); `invalid`: a component is negative or not below its bound
    // (4, 10, 50, 10) — the action is then outside the Dict action space and has no effect; the step itself runs.
    CGE_HD double step(int32_t typ, int32_t wid, int32_t cid, int32_t tid, double u, bool &invalid) {
        double reward = 0.0;
        invalid = (typ | wid | cid | tid) < 0 || typ >= 4 || wid >= NW || cid >= 50 || tid >= NT;
        if (!invalid) {                                              // an action outside the action space does nothing
            const uint32_t w = pick(wt, (uint32_t)wid), bit = 1u << tid;
            if ((w & 3u) == 0u) {                                    // waiter.is_idle() :108
                uint32_t nwt = 0;
                if (typ == 0) {
                    if ((uint32_t)cid < nw) {
                        if (dirty & bit) reward += -1.5;             // :119-121
                        else if (!(occ & bit)) {
                            nwt = SEAT | 2u << 2 | (uint32_t)tid << 4 | (waiting_entry((uint32_t)cid) >> 8) << 8;
                            pop_waiting((uint32_t)cid);
                        }
                    }
                } else if (typ == 1) {                               // :132-149: occupied, guest ORDERED, a ready order
                    if ((occ & bit) && !(eating & bit) && find_ready((uint32_t)tid) < (uint32_t)NREADY) nwt = SERVE | 1u << 2 | (uint32_t)tid << 4;
                } else if (typ == 2) {
                    if ((dirty & bit) && !(occ & bit)) nwt = CLEAN | 3u << 2 | (uint32_t)tid << 4;
                }
                if (nwt) put(wt, (uint32_t)wid, nwt);
            }
        }
        uint32_t order = 0;
#pragma unroll
        for (int k = 0; k < NW; ++k) {                               // _update_waiters :285-290, Waiter.update_task :108-124
            const uint32_t w = wt[k];
            if (w & 3u) {
                const uint32_t rem = ((w >> 2) & 3u) - 1u;
                if (rem == 0u) { wt[k] = 0; complete(w & 3u, (w >> 4) & 15u, w >> 8, order); }
                else wt[k] = (w & ~12u) | rem << 2;
            }
        }
#pragma unroll
        for (int j = 0; j < QW; ++j)                                 // _update_customers :352-372: every WAITING customer waits one more
            wq[j] += (2u * j < nw ? 0x100u : 0u) + (2u * j + 1u < nw ? 0x1000000u : 0u);
#pragma unroll
        for (int k = 0; k < NW; ++k) wt[k] += (wt[k] & 3u) == SEAT ? 0x100u : 0u;
        ghost_wait += ghosts;
#pragma unroll
        for (int k = 0; k < NT; ++k) {                               // Customer.update_eating :68-75, Table.customer_leaves :166-171
            const uint32_t bit = 1u << k;
            if (eating & bit) {
                const uint64_t c = (eatc >> (4 * k)) & 15u;
                if (c == 0) { occ &= ~bit; eating &= ~bit; dirty |= bit; gwait &= ~((uint64_t)63u << (6 * k)); }
                else eatc -= (uint64_t)1 << (4 * k);
            }
        }
        if (ck[2] & CK_VALID) { put(rd, nr, (ck[2] & 0x7FFFu) | (t - 3u) << 16); nr += 1; }   // Kitchen.update_cooking :238-249
        ck[2] = ck[1]; ck[1] = ck[0]; ck[0] = order;
        const double p = t >= 1u && t <= 150u ? 0.12 : t >= 151u && t <= 350u ? 0.20 : t >= 351u && t <= 500u ? 0.08 : 0.0;   // :64-68, :374-387
        if (u < p) {
            const uint32_t e = take_serial();
#pragma unroll
            for (int j = 0; j < QW; ++j) wq[j] |= (nw >> 1) == (uint32_t)j ? e << (16u * (nw & 1u)) : 0u;
            nw += 1;
        }
        if (nw && ((wq[0] >> 8) & 255u) >= PATIENCE) {               // _handle_impatient_customers :389-405: the head only (see the top)
            pop_waiting(0);
            total += -5.0;
            left += 1;
        }
        double eff = 0.0;                                            // _calculate_efficiency_rewards :407-424
        if (dirty == 0u) eff += 0.5;
        if (nw == 0u) eff += 0.3;
        if (!((ck[0] & ck[1] & ck[2]) & CK_VALID)) eff += 0.2;       // queue length <= 2
        reward += eff;
        t += 1;
        reward += -0.1;
        total += reward;
        return reward;
    }

    CGE_HD uint32_t seat_tasks() const {
        uint32_t c = 0;
#pragma unroll
        for (int k = 0; k < NW; ++k) c += (wt[k] & 3u) == SEAT;
        return c;
    }
    CGE_HD uint32_t idle_waiters() const {
        uint32_t c = 0;
#pragma unroll
        for (int k = 0; k < NW; ++k) c += (wt[k] & 3u) == 0u;
        return c;
    }
    CGE_HD uint32_t cooking() const { return (ck[0] >> 15) + (ck[1] >> 15) + (ck[2] >> 15); }
    CGE_HD uint32_t bits10(uint32_t m) const {
        uint32_t c = 0;
#pragma unroll
        for (int k = 0; k < NT; ++k) c += (m >> k) & 1u;
        return c;
    }
    // len(self.customers) and the sum of their wait_time (:480-481): waiting, carried, seated and ghost customers
    CGE_HD uint32_t num_customers() const { return nw + seat_tasks() + bits10(occ) + ghosts; }
    CGE_HD uint32_t wait_sum() const {
        uint32_t s = ghost_wait;
#pragma unroll
        for (int j = 0; j < QW; ++j) s += ((wq[j] >> 8) & 255u) + (wq[j] >> 24);
#pragma unroll
        for (int k = 0; k < NW; ++k) s += (wt[k] & 3u) == SEAT ? wt[k] >> 8 : 0u;
#pragma unroll
        for (int k = 0; k < NT; ++k) s += (uint32_t)((gwait >> (6 * k)) & 63u);
        return s;
    }

    // _get_observation :426-476 as the bytes the store pass expands to int32: STG_WORDS words per env
    //   words 0..10  waiting line (tag, wait) pairs        11..19 waiter (busy, task, remaining) triples
    //   20..22 occupied, a byte per table   23..25 dirty   26..28 cooking (tag, table, progress) triples, oldest first
    //   29..33 ready (tag, table) pairs     (current_timestep leaves straight from the register)
    template <class W>
    CGE_HD void stage(W &&word) const {
#pragma unroll
        for (int j = 0; j < QW; ++j) word(j, wq[j]);
        uint32_t tr[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            const uint32_t w = k < NW ? wt[k < NW ? k : 0] : 0u, task = w & 3u;
            tr[k] = (task ? 1u : 0u) | task << 8 | ((w >> 2) & 3u) << 16;
        }
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            word(11 + 3 * g, tr[4 * g] | tr[4 * g + 1] << 24);
            word(12 + 3 * g, tr[4 * g + 1] >> 8 | tr[4 * g + 2] << 16);
            word(13 + 3 * g, tr[4 * g + 2] >> 16 | tr[4 * g + 3] << 8);
        }
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            const uint32_t o = occ >> (4 * g), d = dirty >> (4 * g);
            word(20 + g, (o & 1u) | (o & 2u) << 7 | (o & 4u) << 14 | (o & 8u) << 21);
            word(23 + g, (d & 1u) | (d & 2u) << 7 | (d & 4u) << 14 | (d & 8u) << 21);
        }
        uint32_t l[3] = {0, 0, 0}, n = 0;
#pragma unroll
        for (int s = 2; s >= 0; --s) {
            if (ck[s] & CK_VALID) { put(l, n, (ck[s] & 0x7FFFu) | (uint32_t)(s + 1) << 16); n += 1; }
        }
        word(26, l[0] | l[1] << 24); word(27, l[1] >> 8 | l[2] << 16); word(28, l[2] >> 16);
#pragma unroll
        for (int j = 0; j < NREADY / 2; ++j) word(29 + j, (rd[2 * j] & 0xFFFFu) | rd[2 * j + 1] << 16);
    }
};

constexpr int STG_WORDS = 35;               // 34 used; an odd stride keeps the lanes' rows on different LDS banks
// where a plane's bytes start in an env's staged row, and how many of them can be non-zero (the rest of the plane is padding)
constexpr int STG_WAITING = 0, STG_WAITERS = 44, STG_OCC = 80, STG_DIRTY = 92, STG_COOKING = 104, STG_READY = 116;
constexpr int LIM_WAITING = 44, LIM_WAITERS = 30, LIM_TABLES = 10, LIM_COOKING = 12, LIM_READY = 20;

}  // namespace restaurant
}  // namespace cge
