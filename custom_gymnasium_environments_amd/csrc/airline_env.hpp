// airline_env.hpp — the record and the dynamics of one AirlineOperationsEnv, plain C++ (host and device): airline.hip runs it one lane
// per env; tools/probes/airline_host_check.cpp replays the reference fixtures through the same code on the CPU.
//
// Re-expresses the reference's airline_operations_env/airline_env.py:
//   _initialize_network :192-272, reset :274-336, _generate_weather_systems :338-352, _get_observation :354-396, step :398-443,
//   _process_action :445-511, _update_weather :513-548, _update_aircraft :550-576, _update_flights :578-599, _update_crew :601-616,
//   _calculate_metrics :618-630, _calculate_reward :632-666, _check_termination :668-686
// Only what an observation, a reward or a flag can see is state:
//   aircraft  one word (airport:4 | destination:4 | in flight:1 | steps flown:5 | delay minutes:18), the fuel level (float64) and the
//             maintenance hours as m0 (float64) with maintenance_status = m0 - 0.5 * t, t the steps since reset(): the reference
//             subtracts 0.5 per step from a draw in [50, 200) or from 100, every intermediate value is a multiple of the draw's last
//             place and smaller than the draw, so each subtraction is exact and so is the closed form; a maintenance event at step t
//             sets m0 = 100 + 0.5 * t.  Nothing is written per step.  A count of aircraft at or below 0.2 fuel stands for :663.
//             Airport and destination survive reset().  passengers_onboard is zeroed before it is paid (:562, :569):
//             daily_revenue is 0.0 for ever, only the draw behind it is consumed.  The delay saturates at 262,143 minutes, which only
//             a Disabled-mode env that is never reset can reach.
//   airports  gate availability, fuel price (float64), weather severity (float32: it is only ever cast on assignment, :371)
//   flights   one word (origin:4 | destination:4 | passengers:8 | due quarter hour:7 | on time after s + 0.25:1 | status:3 | aircraft:5).
//             `current_hour >= scheduled_time` is `4 * hour >= ceil(4 * scheduled)`: the hour is a multiple of 0.25, so both sides are
//             exact, also after the hour has wrapped at midnight.  `abs((s + 0.25) - s) < 0.25` is decided by float64 rounding once.
//             A flight leaves "scheduled" at most once, so on_time_performance is two counters.  Flights 0..9 (priority is 1.0 for
//             all and sorted() is stable) keep their float64 scheduled_time for the observation.
//   crew      nothing (assigned_flight is never set: crews only rest, fatigue and overtime stay 0); the draws are consumed.
//   weather   at most three systems: x, y, radius, movement x / y.  The distance is sqrt(dx * dx + dy * dy); the reference's dx ** 2
//             goes through libm pow, which differs in the last place now and then — the stated departure (README).
// The memory a runtime index reaches (aircraft words, per-airport masks of grounded aircraft, fuel prices, flight words) is behind the
// accessor M: LDS rows and HBM columns on the device, plain arrays on the host.  Everything else is indexed at compile time.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CGE_HD __host__ __device__ __forceinline__
#else
#define CGE_HD inline
#endif

namespace cge {
namespace airline {

constexpr int NA = 25, NP = 15, NF = 150, NC = 40, NWX = 3, OBS = 160;
constexpr int NPRI = 10;                                          // flights in the observation
constexpr int arrive_steps() {                                    // flight_progress += 0.05 from 0.0 until >= 1.0 (:555-557), in float64
    double p = 0.0;
    int k = 0;
    while (p < 1.0) { p += 0.05; ++k; }
    return k;
}
constexpr uint32_t ARRIVE = (uint32_t)arrive_steps();
enum : uint32_t { SCHEDULED = 0, BOARDING = 1, DEPARTED = 2, CANCELLED = 3, DELAYED_ACTION = 4, DELAYED_NO_AIRCRAFT = 5 };
constexpr uint32_t DELAY_MAX = 0x3FFFFu;
constexpr int AIRCRAFT_BATCH = 25;                                // maintenance bases fetched together (independent loads)
constexpr int FLIGHT_BATCH = 30;                                  // flight words fetched together before their turns (independent loads)

// the record: 32-bit columns [word][env]
constexpr int W_AC = 0, W_FUEL = W_AC + NA, W_MAINT = W_FUEL + 2 * NA /* m0 */, W_GATE = W_MAINT + 2 * NA, W_PRICE = W_GATE + 2 * NP,
              W_SEV = W_PRICE + 2 * NP, W_WX = W_SEV + NP, W_SCAL = W_WX + 10 * NWX, W_SCHED = W_SCAL + 14, W_FLIGHT = W_SCHED + 2 * NPRI,
              REC_WORDS = W_FLIGHT + NF;
static_assert(REC_WORDS == 414, "documented as 1,656 bytes per env");

CGE_HD double fuel_use(int a) { return a < 8 ? 2.0 : a < 20 ? 1.0 : 0.5; }       // :64-79
CGE_HD double airport_x(int p) {                                  // :196-219; 700 + 400 * cos(2 pi i / 10) as CPython computes it
    constexpr double x[NP] = {700.0, 300.0, 1100.0, 300.0, 1100.0, 0x1.1300000000000p+10, 0x1.ffcdab8c75b92p+9, 0x1.9bcdab8c75b92p+9, 0x1.203254738a46fp+9,
                              0x1.7864a8e7148dep+8, 0x1.2c00000000000p+8, 0x1.7864a8e7148dcp+8, 0x1.203254738a46ep+9, 0x1.9bcdab8c75b91p+9, 0x1.ffcdab8c75b91p+9};
    return x[p];
}
CGE_HD double airport_y(int p) {                                  // 500 + 300 * sin(2 pi i / 10)
    constexpr double y[NP] = {500.0, 300.0, 300.0, 700.0, 700.0, 0x1.f400000000000p+8, 0x1.522af424e617ap+9, 0x1.88a891fa504e6p+9, 0x1.88a891fa504e7p+9,
                              0x1.522af424e617ap+9, 0x1.f400000000001p+8, 0x1.43aa17b633d0ep+8, 0x1.ad5db816bec66p+7, 0x1.ad5db816bec64p+7, 0x1.43aa17b633d0cp+8};
    return y[p];
}

// aircraft word
CGE_HD uint32_t ac_airport(uint32_t w) { return w & 15u; }
CGE_HD uint32_t ac_dest(uint32_t w) { return (w >> 4) & 15u; }
CGE_HD bool ac_flying(uint32_t w) { return (w >> 8) & 1u; }
CGE_HD uint32_t ac_prog(uint32_t w) { return (w >> 9) & 31u; }
CGE_HD uint32_t ac_delay(uint32_t w) { return w >> 14; }
CGE_HD uint32_t ac_add_delay(uint32_t w, uint32_t m) {
    const uint32_t d = ac_delay(w) + m;
    return (w & 0x3FFFu) | ((d < DELAY_MAX ? d : DELAY_MAX) << 14);
}
// flight word
CGE_HD uint32_t fl_make(uint32_t org, uint32_t dst, uint32_t pax, uint32_t due, bool ontime) { return org | dst << 4 | pax << 8 | due << 16 | (ontime ? 1u : 0u) << 23; }
CGE_HD uint32_t fl_origin(uint32_t w) { return w & 15u; }
CGE_HD uint32_t fl_dest(uint32_t w) { return (w >> 4) & 15u; }
CGE_HD uint32_t fl_pax(uint32_t w) { return (w >> 8) & 255u; }
CGE_HD uint32_t fl_due(uint32_t w) { return (w >> 16) & 127u; }
CGE_HD bool fl_ontime(uint32_t w) { return (w >> 23) & 1u; }
CGE_HD uint32_t fl_status(uint32_t w) { return (w >> 24) & 7u; }
CGE_HD uint32_t fl_aircraft(uint32_t w) { return w >> 27; }
CGE_HD uint32_t fl_set(uint32_t w, uint32_t status, uint32_t aircraft) { return (w & 0xFFFFFFu) | status << 24 | aircraft << 27; }

// CPython's random on a source of tempered MT19937 words, R::next()
template <class R>
CGE_HD uint32_t randbelow(R &r, uint32_t n, int kbits) {           // Random._randbelow_with_getrandbits(n), kbits = n.bit_length()
    uint32_t v = r.next() >> (32 - kbits);
    while (v >= n) v = r.next() >> (32 - kbits);
    return v;
}
template <class R>
CGE_HD double uniform(R &r, double lo, double width) {             // random.uniform(lo, lo + width) = lo + width * random()
    const uint32_t a = r.next() >> 5, b = r.next() >> 6;
    return lo + width * (((double)a * 67108864.0 + (double)b) / 9007199254740992.0);
}

struct Env {
    double gate[NP];
    double wx[NWX][5];                       // x, y, radius, movement x, movement y
    double sat, costs, comp, fuel_costs, ret;
    uint32_t h4, nwx, disruption, needs_reset, t, left, ontime, low, mt_pos;

    CGE_HD double otp() const { return left ? (double)ontime / (double)left : 0.95; }   // keeps 0.95 while no flight has left "scheduled" (:622)

    // the scalar columns W_SCAL .. W_SCAL + 13, as put(word, value) / get(word)
    template <class F>
    CGE_HD void pack_scalars(F put) const {
        const double d[5] = {sat, costs, comp, fuel_costs, ret};
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            uint64_t u;
            __builtin_memcpy(&u, &d[k], 8);
            put(2 * k, (uint32_t)u);
            put(2 * k + 1, (uint32_t)(u >> 32));
        }
        put(10, h4 | nwx << 7 | disruption << 9 | needs_reset << 10);
        put(11, t);
        put(12, left | ontime << 8 | low << 16);
        put(13, mt_pos);
    }
    template <class F>
    CGE_HD void unpack_scalars(F get) {
        double d[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const uint64_t u = (uint64_t)get(2 * k) | (uint64_t)get(2 * k + 1) << 32;
            __builtin_memcpy(&d[k], &u, 8);
        }
        sat = d[0]; costs = d[1]; comp = d[2]; fuel_costs = d[3]; ret = d[4];
        const uint32_t m = get(10), c = get(12);
        h4 = m & 127u; nwx = (m >> 7) & 3u; disruption = (m >> 9) & 1u; needs_reset = (m >> 10) & 1u;
        t = get(11);
        left = c & 255u; ontime = (c >> 8) & 255u; low = c >> 16;
        mt_pos = get(13);
    }
};

// a flight leaves "scheduled": the two counters behind on_time_performance (:621-625)
CGE_HD uint32_t leave(Env &e, uint32_t w, uint32_t status, uint32_t aircraft) {
    e.left += 1;
    e.ontime += (status == BOARDING || status == CANCELLED || (status == DELAYED_NO_AIRCRAFT && fl_ontime(w))) ? 1u : 0u;
    return fl_set(w, status, aircraft);
}

// reset() :274-336 with _generate_weather_systems.  Aircraft keep their airport and destination.
template <class M, class R>
CGE_HD void reset_episode(Env &e, M &m, R &r) {
    e.h4 = 24; e.t = 0; e.left = 0; e.ontime = 0; e.low = 0; e.disruption = 0; e.needs_reset = 0;
    e.sat = 1.0; e.costs = 0.0; e.comp = 0.0; e.fuel_costs = 0.0; e.ret = 0.0;
    for (int p = 0; p < NP; ++p) m.set_avail(p, 0u);
#pragma unroll 1
    for (int a = 0; a < NA; ++a) {
        const uint32_t w = m.ac(a) & 255u;                          // not in flight, no progress, no delay
        m.set_ac(a, w);
        m.set_avail(ac_airport(w), m.avail(ac_airport(w)) | 1u << a);
        m.set_fuel(a, uniform(r, 0.7, 1.0 - 0.7));
        m.set_maint0(a, uniform(r, 50.0, 150.0));
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        e.gate[p] = uniform(r, 0.7, 1.0 - 0.7);
        randbelow(r, 901u, 10);                                     // passenger_volume = randint(100, 1000)
        m.set_price(p, uniform(r, 2.0, 1.0));
        m.set_sev(p, 0.0f);
    }
    for (int f = 0; f < NF; ++f) m.set_flight(f, m.flight(f) & 0xFFFFFFu);
    for (int c = 0; c < NC; ++c) uniform(r, 8.0, 4.0);              // crew.duty_time_remaining
    e.nwx = randbelow(r, 4u, 3);
#pragma unroll
    for (int s = 0; s < NWX; ++s) {
        const bool on = (uint32_t)s < e.nwx;
        double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        if (on) {
            v[0] = uniform(r, 100.0, 1200.0); v[1] = uniform(r, 100.0, 800.0); v[2] = uniform(r, 100.0, 200.0);
            randbelow(r, 4u, 3);                                    // severity = choice of four
            v[3] = uniform(r, -20.0, 40.0); v[4] = uniform(r, -20.0, 40.0);
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) e.wx[s][k] = v[k];
    }
}

// random.seed(s); AirlineOperationsEnv(): _initialize_network :221-272 and the constructor's own reset() (:190), whose state the
// visible reset() overwrites.  The stream must be at its start.
template <class M, class R>
CGE_HD void draw_network(Env &e, M &m, R &r) {
    for (int a = 0; a < NA; ++a) {
        const uint32_t ap = a < 8 ? randbelow(r, 5u, 3) : a < 20 ? randbelow(r, 15u, 4) : 5u + randbelow(r, 10u, 4);
        const uint32_t de = a < 20 ? randbelow(r, 15u, 4) : 5u + randbelow(r, 10u, 4);
        uniform(r, 0.0, 1.0);                                       // maintenance_status: reset() draws it again
        m.set_ac(a, ap | de << 4);
    }
    for (int f = 0; f < NF; ++f) {
        const uint32_t org = randbelow(r, 15u, 4);
        uint32_t dst = randbelow(r, 15u, 4);
        while (dst == org) dst = randbelow(r, 15u, 4);
        const double s = uniform(r, 6.0, 16.0);
        const uint32_t pax = 50u + randbelow(r, 201u, 8);
        const double late = s + 0.25;                                // :593, rounded to float64 before :624 subtracts
        m.set_flight(f, fl_make(org, dst, pax, (uint32_t)ceil(s * 4.0), fabs(late - s) < 0.25));
        if (f < NPRI) m.set_sched(f, s);
    }
    for (int c = 0; c < NC; ++c) {
        randbelow(r, 3u, 2);                                         // choice(list(CrewType))
        randbelow(r, 15u, 4);
        uniform(r, 8.0, 4.0);
    }
    reset_episode(e, m, r);
}

// step() :398-443 up to the flags; `valid` false skips _process_action (an action outside 0..44).  Returns the reward.
template <class M, class R>
CGE_HD double env_step(Env &e, M &m, R &r, int32_t action, bool valid, bool &terminated) {
    double reward = 0.0;
    const uint32_t a = (uint32_t)action;
    if (!valid) {
    } else if (a < 25u) {                                            // :449-461 reassign an aircraft on the ground
        const uint32_t w = m.ac(a);
        if (!ac_flying(w)) {
            const uint32_t d = randbelow(r, 15u, 4);
            if (d != ac_airport(w)) {
                m.set_ac(a, (w & ~(15u << 4) & ~(31u << 9)) | d << 4 | 1u << 8);
                m.set_avail(ac_airport(w), m.avail(ac_airport(w)) & ~(1u << a));
                if (a < 8u) randbelow(r, 251u, 8); else if (a < 20u) randbelow(r, 101u, 7); else randbelow(r, 21u, 5);   // passengers_onboard
                reward += 100.0;
            }
        }
    } else if (a < 35u) {                                            // :463-478 cancel / delay one of flights 0..50
        const uint32_t f = randbelow(r, 51u, 6);
        const uint32_t w = m.flight(f);
        if (fl_status(w) == SCHEDULED) {
            if (a < 30u) {
                m.set_flight(f, leave(e, w, CANCELLED, 0u));
                e.sat *= 0.9;
                e.comp += (double)(fl_pax(w) * 200u);
                reward -= 5000.0;
            } else {
                m.set_flight(f, leave(e, w, DELAYED_ACTION, 0u));
                reward -= 100.0;
            }
        }
    } else if (a < 40u) {                                            // :480-485
#pragma unroll
        for (int p = 0; p < 5; ++p) {
            if (a == 35u + (uint32_t)p) { const double g = e.gate[p] + 0.2; e.gate[p] = g < 1.0 ? g : 1.0; }   // min(1.0, g)
        }
        reward += 50.0;
    } else if (a == 40u) {
        e.disruption = 1; reward -= 200.0;
    } else if (a == 41u) {
        if (e.costs < 500000.0) { e.costs += 50000.0; reward += 200.0; }
    } else if (a == 42u) {
        e.comp += 10000.0;
        const double s = e.sat + 0.05;
        e.sat = s < 1.0 ? s : 1.0;
        reward -= 100.0;
    } else if (a == 43u) {
#pragma unroll
        for (int k = 0; k < NA; ++k) { const uint32_t w = m.ac(k); if (!ac_flying(w)) m.set_ac(k, ac_add_delay(w, 30u)); }
        reward -= 500.0;
    } else {
        e.disruption = 0; reward += 50.0;
    }
    e.h4 += 1;                                                       // :406-408
    if (e.h4 >= 96u) e.h4 -= 96u;
    e.t += 1;
#pragma unroll
    for (int s = 0; s < NWX; ++s) {                                  // :513-529 (absent systems are zeros and stay zeros)
        e.wx[s][0] += e.wx[s][3] * 0.1;
        e.wx[s][1] += e.wx[s][4] * 0.1;
    }
#pragma unroll 1
    for (int p = 0; p < NP; ++p) {                                   // :532-540, the last system in range wins
        double sev = 0.0;
#pragma unroll
        for (int s = 0; s < NWX; ++s) {
            const double dx = airport_x(p) - e.wx[s][0], dy = airport_y(p) - e.wx[s][1];
            const double dist = sqrt(dx * dx + dy * dy);
            if ((uint32_t)s < e.nwx && dist < e.wx[s][2]) sev = 1.0 - dist / e.wx[s][2];
        }
        m.set_sev(p, (float)sev);
    }
    static_assert(NA % AIRCRAFT_BATCH == 0, "whole batches");
#pragma unroll 1
    for (int kb = 0; kb < NA; kb += AIRCRAFT_BATCH) {                // :550-576
    double m0[AIRCRAFT_BATCH];
#pragma unroll
    for (int j = 0; j < AIRCRAFT_BATCH; ++j) m0[j] = m.maint0(kb + j);   // independent loads
#pragma unroll
    for (int j = 0; j < AIRCRAFT_BATCH; ++j) {
        const int k = kb + j;
        uint32_t w = m.ac(k);
        if (ac_flying(w)) {
            w += 1u << 9;
            if (ac_prog(w) >= ARRIVE) {
                const uint32_t d = ac_dest(w);
                w = (w & ~15u & ~(1u << 8) & ~(31u << 9)) | d;
                m.set_avail(d, m.avail(d) | 1u << k);
                const double old = m.fuel(k), f = old - 0.1 * fuel_use(k), left = f > 0.1 ? f : 0.1;   // max(0.1, f)
                m.set_fuel(k, left);
                e.low += old > 0.2 && !(left > 0.2) ? 1u : 0u;
            }
        }
        if (m0[j] - 0.5 * (double)e.t <= 0.0) {                      // maintenance_status -= 0.5, t times since reset()
            w = ac_add_delay(w, 120u);
            m.set_maint0(k, 100.0 + 0.5 * (double)e.t);              // maintenance_status = 100
            e.costs += 10000.0;
        }
        m.set_ac(k, w);
    }
    }
    static_assert(NF % FLIGHT_BATCH == 0, "whole batches");
#pragma unroll 1
    for (int b = 0; b < NF; b += FLIGHT_BATCH) {                     // :578-599, in flight order; a flight's word changes only in its own turn
    uint32_t fw[FLIGHT_BATCH], todo = 0;                             // the flights of the batch that do something in this step
#pragma unroll
    for (int j = 0; j < FLIGHT_BATCH; ++j) fw[j] = m.flight(b + j);
#pragma unroll
    for (int j = 0; j < FLIGHT_BATCH; ++j) {
        const uint32_t st = fl_status(fw[j]);
        todo |= ((st == SCHEDULED && e.h4 >= fl_due(fw[j])) || st == BOARDING ? 1u : 0u) << j;
    }
    while (todo) {
        const uint32_t j = (uint32_t)__builtin_ctz(todo);
        todo &= todo - 1u;
        const int f = b + (int)j;
        uint32_t w = 0;
#pragma unroll
        for (int q = 0; q < FLIGHT_BATCH; ++q) w |= fw[q] & (0u - (uint32_t)(j == (uint32_t)q));   // fw[j], mask form: no indexed register array
        const uint32_t st = fl_status(w);
        if (st == SCHEDULED) {
            if (e.h4 >= fl_due(w)) {
                const uint32_t free = m.avail(fl_origin(w));         // a boarding aircraft is still "not in flight": it can be taken again
                if (free) {
                    const uint32_t k = (uint32_t)__builtin_ctz(free);
                    m.set_flight(f, leave(e, w, BOARDING, k));
                    m.set_ac(k, (m.ac(k) & ~(15u << 4)) | fl_dest(w) << 4);
                } else {
                    m.set_flight(f, leave(e, w, DELAYED_NO_AIRCRAFT, 0u));
                }
            }
        } else if (st == BOARDING) {
            const uint32_t k = fl_aircraft(w), c = m.ac(k);
            m.set_flight(f, fl_set(w, DEPARTED, k));
            m.set_ac(k, c | 1u << 8);
            m.set_avail(ac_airport(c), m.avail(ac_airport(c)) & ~(1u << k));
        }
    }
    }
    double total = 0.0;                                              // :628-630: sum() from int 0, left to right; 0 + x is x
#pragma unroll 1
    for (int k = 0; k < NA; ++k) {
        const uint32_t w = m.ac(k);
        if (!ac_flying(w)) total = total + fuel_use(k) * m.price(ac_airport(w));
    }
    e.fuel_costs = total * 100.0;
    e.costs += (e.fuel_costs + e.comp) + 0.0;                        // + crew_overtime, which stays 0
    const double otp = e.otp();                                      // :632-666
    reward += otp > 0.95 ? 500.0 : otp > 0.90 ? 200.0 : otp < 0.70 ? -500.0 : 0.0;
    reward += e.sat > 0.9 ? 300.0 : e.sat < 0.6 ? -1000.0 : 0.0;
    reward += 0.0 - e.costs < -100000.0 ? -500.0 : 0.0;             // profit = daily_revenue - daily_costs
    reward += e.low == 0u ? 100.0 : 0.0;                             // all(fuel_level > 0.2)
    terminated = e.h4 >= 95u || e.sat < 0.6;                         // :668-686; the crew and the financial exits cannot fire
    return reward;
}

// _get_observation :354-396 in four parts of 40 floats, out(k, value) with k the index inside the part:
//   0 aircraft 0..9, 1 aircraft 10..19, 2 aircraft 20..24 + airports 0..9, 3 airports 10..14 + flights 0..9 + the ten global values
constexpr int PARTS = 4, PART_FLOATS = OBS / PARTS;
template <class M, class F>
CGE_HD void observe_aircraft(const Env &e, M &m, F &out, int k, int at) {
    const uint32_t w = m.ac(k);
    out(at, (float)((double)ac_airport(w) / 15.0));
    out(at + 1, (float)m.fuel(k));
    out(at + 2, (float)((double)ac_delay(w) / 240.0));
    out(at + 3, (float)((m.maint0(k) - 0.5 * (double)e.t) / 200.0));
}
template <int PART, class M, class F>
CGE_HD void observe_part(const Env &e, M &m, F out) {
    if (PART < 2) {
#pragma unroll
        for (int j = 0; j < 10; ++j) observe_aircraft(e, m, out, 10 * PART + j, 4 * j);
    } else if (PART == 2) {
#pragma unroll
        for (int j = 0; j < 5; ++j) observe_aircraft(e, m, out, 20 + j, 4 * j);
#pragma unroll
        for (int p = 0; p < 10; ++p) { out(20 + 2 * p, m.sev(p)); out(21 + 2 * p, (float)e.gate[p]); }
    } else {
#pragma unroll
        for (int p = 10; p < NP; ++p) { out(2 * (p - 10), m.sev(p)); out(2 * (p - 10) + 1, (float)e.gate[p]); }
#pragma unroll
        for (int f = 0; f < NPRI; ++f) {
            const uint32_t w = m.flight(f), st = fl_status(w);
            const double s = m.sched(f);
            const double actual = st == DELAYED_ACTION ? s + 0.5 : st == DELAYED_NO_AIRCRAFT ? s + 0.25 : s;
            out(10 + 2 * f, (float)((actual - s) / 4.0));
            out(11 + 2 * f, (float)((double)fl_pax(w) / 300.0));
        }
        uint32_t flying = 0;
#pragma unroll
        for (int k = 0; k < NA; ++k) flying += ac_flying(m.ac(k)) ? 1u : 0u;
        out(30, (float)e.otp());
        out(31, (float)e.sat);
        out(32, (float)(((double)e.h4 * 0.25) / 24.0));
        out(33, (float)((double)flying / 25.0));
        out(34, 0.0f);                                              // daily_revenue / 1e6
        out(35, (float)(e.costs / 1000000.0));
        out(36, (float)(e.fuel_costs / 100000.0));
        out(37, (float)(e.comp / 100000.0));
        out(38, e.disruption ? 1.0f : 0.0f);
        out(39, (float)((double)e.nwx / 5.0));
    }
}


// Canonical records (cge_records_airline_*, lane_records.hip): what a record's body must satisfy before it may become an env, so that
// no kernel of the type reads or writes out of range.  get(w) is word w of the body.  The fields a kernel uses as an index or a bound:
//   airport, destination (aircraft word, 4 bits each)   the airport rows (masks of grounded aircraft, fuel prices): 0..NP-1
//   origin, destination (flight word, 4 bits each)      the airport rows; the destination becomes an aircraft's: 0..NP-1
//   aircraft (flight word, 5 bits)                      a boarding flight indexes the aircraft rows by it: 0..NA-1
// The number of weather systems (2 bits) is compared with compile-time indices only, the hour wraps by comparison, the flight an
// action picks is drawn below 51.  No kernel calls this.
enum { RECORD_OK = 0, RECORD_AIRCRAFT_AIRPORT = 16, RECORD_FLIGHT_AIRPORT = 17, RECORD_FLIGHT_AIRCRAFT = 18 };
template <class G>
CGE_HD int record_refusal(G get) {
    for (int a = 0; a < NA; ++a) {
        const uint32_t w = get(W_AC + a);
        if (ac_airport(w) >= (uint32_t)NP || ac_dest(w) >= (uint32_t)NP) return RECORD_AIRCRAFT_AIRPORT;
    }
    for (int f = 0; f < NF; ++f) {
        const uint32_t w = get(W_FLIGHT + f);
        if (fl_origin(w) >= (uint32_t)NP || fl_dest(w) >= (uint32_t)NP) return RECORD_FLIGHT_AIRPORT;
        if (fl_aircraft(w) >= (uint32_t)NA) return RECORD_FLIGHT_AIRCRAFT;
    }
    return RECORD_OK;
}
inline const char *record_refusal_text(int code) {
    return code == RECORD_AIRCRAFT_AIRPORT ? "an aircraft's airport or destination is above 14"
           : code == RECORD_FLIGHT_AIRPORT ? "a flight's origin or destination is above 14"
           : code == RECORD_FLIGHT_AIRCRAFT ? "a flight's aircraft is above 24" : "bad record";
}
constexpr int RECORD_CURSOR_FIRST = W_SCAL + 13, RECORD_CURSOR_WORDS = 1;   // mt_pos; the type keeps no ready mark

}  // namespace airline
}  // namespace cge
