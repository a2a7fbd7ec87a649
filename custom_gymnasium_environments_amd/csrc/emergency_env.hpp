// emergency_env.hpp — the record and the dynamics of one EmergencyResponseEnv, plain C++ (host and device): emergency.hip runs it one
// lane per env; tools/probes/emergency_host_check.cpp replays the reference fixtures through the same code on the CPU.  Compile it
// without FP contraction: every product and sum below is rounded where the reference rounds it.
//
// Re-expresses the reference's emergency_response_env/emergency_env.py:
//   _initialize_city :192-218, _initialize_units :220-265, _initialize_hospitals :267-283, _generate_emergencies :285-301,
//   _create_emergency :303-356, _get_required_units :358-399, _update_cascade_effects :401-419, _escalate_emergency :421-428,
//   _trigger_cascade_event :430-463, _update_units :465-494, _work_on_incident :496-522, _get_observation :524-587,
//   _calculate_reward :589-646, _execute_action :648-690, _dispatch_unit :692-736, _update_weather :768-780, _update_traffic :782-806,
//   _check_termination :808-827, reset :829-881, step :883-922
// Only what an observation, a reward, a flag or an info value can see is state (DESIGN.md §3.16 argues each point):
//   network    the station coordinates of units 30..39, 5 bits each.  population_density (900 draws) feeds only incident.casualties,
//              which nothing reads; the hospitals' capacities (32 draws) are at their cap from reset() on, both ratios are 1.0.
//   incidents  at most 20 in dict insertion order, compacted in place.  Word 0: x:5 | y:5 | type:3 | severity:4 | fire trucks
//              required:3 | police cars required:3 | sum of required units:4 — the requirement as computed at creation or at the last
//              escalation (work lowers the severity without touching it).  Word 1: the units ever dispatched to it (bit u, u < 20).
//              Word 2: start time.  "Contained" is severity 0.  escalation_risk is recomputed for every incident in every step before
//              the reward reads it, and incidents added later in the step carry 0.0: a mask that lives for one step.
//   units      0..19 (fire trucks 0..11, police cars 12..19: what actions 0..19 reach).  One word: x:5 | y:5 | busy:1 | incident
//              slot:5 | travel time:6, and the fatigue (float64).  Readiness is max(0.3, 1.0 - fatigue) whenever a unit works — it
//              was busy at its last update — plus the bonus of action 44 / 47 of the same step.  A freed unit stays where it is.
//              Units 20..39 never move; mutual-aid and National-Guard units cost four randint(0, 29) each and are never seen.
//   the rest   25 traffic values, visibility / precipitation / wind (road conditions follow from the precipitation), the cascade
//              multiplier, broadcast reach, cellular coverage, the counters with their _prev_ copies (which survive reset()), the sum,
//              count and last value of response_times (integers, exact in float64), the flags.
// Dead in the reference and left out: `cellular_coverage < 0.7` (the value only rises from 0.95); "three busy unit types" (only fire
// trucks and police cars can be busy); a busy unit whose incident is gone (an incident goes only when contained, which frees its units).
// The memory a runtime index reaches (incident words, unit words, fatigue) is behind the accessor M: LDS rows on the device, plain
// arrays on the host.  Everything else is indexed at compile time.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CGE_HD __host__ __device__ __forceinline__
#else
#define CGE_HD inline
#endif

namespace cge {
namespace emergency {

constexpr int NI = 20, NU = 20, NT = 25, NH = 8, OBS = 276, ACTIONS = 50;
enum : uint32_t { FIRE = 0, ACCIDENT = 1, CHEMICAL = 2, FLOOD = 3, QUAKE = 4, GAS = 5, MEDICAL = 6, UNREST = 7 };
enum : uint32_t { REASON_NONE = 0, REASON_SUCCESS = 1, REASON_CASUALTIES = 2, REASON_OVERWHELMED = 3, REASON_TIMEOUT = 4 };
constexpr uint32_t FIRE_TRUCKS = 0xFFFu, POLICE_CARS = 0xFF000u;

// the record: 32-bit columns [word][env]
constexpr int W_INC = 0, W_UNIT = W_INC + 3 * NI, W_FAT = W_UNIT + NU, W_TRAFFIC = W_FAT + 2 * NU, W_SCAL = W_TRAFFIC + 2 * NT, N_SCAL = 32,
              REC_WORDS = W_SCAL + N_SCAL;
static_assert(REC_WORDS == 202, "documented as 808 bytes per env");

// incident word 0
CGE_HD uint32_t in_x(uint32_t w) { return w & 31u; }
CGE_HD uint32_t in_y(uint32_t w) { return (w >> 5) & 31u; }
CGE_HD uint32_t in_kind(uint32_t w) { return (w >> 10) & 7u; }
CGE_HD uint32_t in_sev(uint32_t w) { return (w >> 13) & 15u; }
CGE_HD uint32_t in_fire(uint32_t w) { return (w >> 17) & 7u; }
CGE_HD uint32_t in_police(uint32_t w) { return (w >> 20) & 7u; }
CGE_HD uint32_t in_sum(uint32_t w) { return (w >> 23) & 15u; }
CGE_HD uint32_t in_set_sev(uint32_t w, uint32_t s) { return (w & ~(15u << 13)) | s << 13; }
CGE_HD uint32_t imin(uint32_t a, uint32_t b) { return a < b ? a : b; }
CGE_HD uint32_t imax(uint32_t a, uint32_t b) { return a > b ? a : b; }
// _get_required_units :358-399 as fire:3 | police:3 | sum:4, at bit 17 of the incident word (floods and earthquakes are never created)
CGE_HD uint32_t required(uint32_t kind, uint32_t s) {
    uint32_t f = 0, p = 0, rest = 0;
    if (kind == FIRE) { f = imin(4u, imax(2u, s / 3u)); rest = imin(2u, imax(1u, s / 5u)) + (s > 7u ? 1u : 0u); }
    else if (kind == ACCIDENT) { p = imin(3u, imax(1u, s / 4u)); rest = imin(4u, imax(1u, s / 3u)); f = s > 6u ? 1u : 0u; }
    else if (kind == CHEMICAL) { f = 1u; rest = imin(2u, imax(1u, s / 5u)) + 1u; }
    else if (kind == GAS) { f = imin(2u, imax(1u, s / 4u)); rest = 1u; }
    else if (kind == MEDICAL) { rest = imin(3u, imax(1u, s / 4u)); }
    else { p = imin(5u, imax(2u, s / 2u)); rest = 1u; }
    return f | p << 3 | (f + p + rest) << 6;
}
CGE_HD uint32_t in_make(uint32_t x, uint32_t y, uint32_t kind, uint32_t sev) { return x | y << 5 | kind << 10 | sev << 13 | required(kind, sev) << 17; }
// unit word
constexpr uint32_t U_BUSY = 1u << 10;
CGE_HD uint32_t un_x(uint32_t w) { return w & 31u; }
CGE_HD uint32_t un_y(uint32_t w) { return (w >> 5) & 31u; }
CGE_HD uint32_t un_slot(uint32_t w) { return (w >> 11) & 31u; }
CGE_HD uint32_t un_travel(uint32_t w) { return (w >> 16) & 63u; }
CGE_HD uint32_t home_x(int u) {                                    // :240-251, units 0..29
    constexpr uint8_t x[30] = {5, 25, 5, 25, 5, 25, 5, 25, 5, 25, 5, 25, 10, 20, 15, 10, 20, 15, 10, 20, 8, 22, 8, 22, 15, 8, 22, 8, 22, 15};
    return x[u];
}
CGE_HD uint32_t home_y(int u) {
    constexpr uint8_t y[30] = {5, 5, 25, 25, 5, 5, 25, 25, 5, 5, 25, 25, 10, 10, 20, 10, 10, 20, 10, 10, 8, 8, 22, 22, 15, 8, 8, 22, 22, 15};
    return y[u];
}
CGE_HD int hospital_x(int h) { constexpr int8_t x[NH] = {7, 23, 7, 23, 15, 10, 20, 15}; return x[h]; }   // :270-273
CGE_HD int hospital_y(int h) { constexpr int8_t y[NH] = {7, 7, 23, 23, 10, 15, 20, 25}; return y[h]; }

// CPython's random on a source of tempered MT19937 words: R::next(), and R::run(w) for W words the caller will consume in order
template <class R>
CGE_HD uint32_t randbelow(R &r, uint32_t n, int kbits) {           // Random._randbelow_with_getrandbits(n), kbits = n.bit_length()
    uint32_t v = r.next() >> (32 - kbits);
    while (v >= n) v = r.next() >> (32 - kbits);
    return v;
}
CGE_HD double random53(uint32_t w0, uint32_t w1) { return ((double)(w0 >> 5) * 67108864.0 + (double)(w1 >> 6)) / 9007199254740992.0; }
template <class R>
CGE_HD double random01(R &r) {
    const uint32_t a = r.next(), b = r.next();
    return random53(a, b);
}
CGE_HD double dmin(double cap, double v) { return v < cap ? v : cap; }   // Python's min(cap, v)
CGE_HD double dmax(double floor_, double v) { return v > floor_ ? v : floor_; }   // Python's max(floor, v)
constexpr double WIDE = 0.1 - (-0.1), NARROW = 0.05 - (-0.05);     // uniform(a, b) = a + (b - a) * random()

struct Env {
    double traffic[NT];
    double vis, precip, wind, cm, reach, cell, ret;
    uint32_t t, casualties, resolved, lives, prev_resolved, prev_lives, prev_casualties, rt_sum, rt_count, rt_last;
    uint32_t ninc, evac, soe, mutual, guard, needs_reset, reason;
    uint32_t station[4];                                           // units 30..39: x, y of unit 30 + j at 5-bit fields 2j, 2j + 1, six fields a word
    uint32_t mt_pos, mt_ready;

    CGE_HD double road() const { return dmax(0.5, 1.0 - precip * 0.5); }   // :777; 1.0 after reset (precipitation 0.0)
    CGE_HD double avg_rt() const { return rt_count ? (double)rt_sum / (double)rt_count : 0.0; }   // np.mean of small integers
    CGE_HD uint32_t station_field(int f) const { return (station[f / 6] >> (5 * (f % 6))) & 31u; }

    // the scalar columns W_SCAL .. W_SCAL + 31, as put(word, value) / get(word)
    template <class F>
    CGE_HD void pack_scalars(F put) const {
        const double d[7] = {vis, precip, wind, cm, reach, cell, ret};
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            uint64_t u;
            __builtin_memcpy(&u, &d[k], 8);
            put(2 * k, (uint32_t)u);
            put(2 * k + 1, (uint32_t)(u >> 32));
        }
        put(14, t); put(15, casualties); put(16, resolved); put(17, lives); put(18, prev_resolved); put(19, prev_lives); put(20, prev_casualties);
        put(21, rt_sum); put(22, rt_count); put(23, rt_last);
        put(24, ninc | evac << 5 | soe << 11 | mutual << 12 | guard << 13 | needs_reset << 14 | reason << 15);
        put(25, station[0]); put(26, station[1]); put(27, station[2]); put(28, station[3]);
        put(29, mt_pos); put(30, mt_ready); put(31, 0u);
    }
    template <class F>
    CGE_HD void unpack_scalars(F get) {
        double d[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const uint64_t u = (uint64_t)get(2 * k) | (uint64_t)get(2 * k + 1) << 32;
            __builtin_memcpy(&d[k], &u, 8);
        }
        vis = d[0]; precip = d[1]; wind = d[2]; cm = d[3]; reach = d[4]; cell = d[5]; ret = d[6];
        t = get(14); casualties = get(15); resolved = get(16); lives = get(17); prev_resolved = get(18); prev_lives = get(19); prev_casualties = get(20);
        rt_sum = get(21); rt_count = get(22); rt_last = get(23);
        const uint32_t f = get(24);
        ninc = f & 31u; evac = (f >> 5) & 63u; soe = (f >> 11) & 1u; mutual = (f >> 12) & 1u; guard = (f >> 13) & 1u; needs_reset = (f >> 14) & 1u;
        reason = (f >> 15) & 7u;
        station[0] = get(25); station[1] = get(26); station[2] = get(27); station[3] = get(28);
        mt_pos = get(29); mt_ready = get(30);
    }
};

template <class M>
CGE_HD void add_incident(Env &e, M &m, uint32_t x, uint32_t y, uint32_t kind, uint32_t sev) {
    m.set_inc(e.ninc, in_make(x, y, kind, sev));
    m.set_mask(e.ninc, 0u);
    m.set_start(e.ninc, e.t);
    e.ninc += 1;
}

// _create_emergency :303-356.  The thresholds are the reference's running float sums.
template <class M, class R>
CGE_HD void create_emergency(Env &e, M &m, R &r) {
    const uint32_t x = randbelow(r, 30u, 5), y = randbelow(r, 30u, 5);
    const double v = random01(r);
    uint32_t kind;
    if (x < 10u || x > 20u) {
        constexpr double c0 = 0.0 + 0.3, c1 = c0 + 0.4, c2 = c1 + 0.2, c3 = c2 + 0.1;
        kind = v <= c0 ? FIRE : v <= c1 ? MEDICAL : v <= c2 ? GAS : v <= c3 ? UNREST : FIRE;
    } else if (x <= 15u) {
        constexpr double c0 = 0.0 + 0.25, c1 = c0 + 0.3, c2 = c1 + 0.25, c3 = c2 + 0.2;
        kind = v <= c0 ? FIRE : v <= c1 ? ACCIDENT : v <= c2 ? MEDICAL : v <= c3 ? UNREST : FIRE;
    } else {
        constexpr double c0 = 0.0 + 0.3, c1 = c0 + 0.2, c2 = c1 + 0.25, c3 = c2 + 0.25;
        kind = v <= c0 ? CHEMICAL : v <= c1 ? FIRE : v <= c2 ? GAS : v <= c3 ? ACCIDENT : CHEMICAL;
    }
    add_incident(e, m, x, y, kind, 1u + randbelow(r, 10u, 4));
}

// reset() :829-881 without its draws: no incident yet.  The network and the _prev_ counters stay.
template <class M>
CGE_HD void clear_episode(Env &e, M &m) {
    e.t = 0; e.ninc = 0; e.casualties = 0; e.resolved = 0; e.lives = 0; e.rt_sum = 0; e.rt_count = 0; e.rt_last = 0;
    e.soe = 0; e.mutual = 0; e.guard = 0; e.evac = 0; e.needs_reset = 0; e.reason = 0;
    e.cm = 1.0; e.vis = 1.0; e.precip = 0.0; e.wind = 0.0; e.cell = 0.95; e.reach = 0.90; e.ret = 0.0;
#pragma unroll
    for (int k = 0; k < NT; ++k) e.traffic[k] = 0.3;
#pragma unroll 1
    for (int u = 0; u < NU; ++u) {
        m.set_unit(u, home_x(u) | home_y(u) << 5);
        m.set_fatigue(u, 0.0);
    }
}
template <class M, class R>
CGE_HD void reset_episode(Env &e, M &m, R &r) {
    clear_episode(e, m);
    const uint32_t n = 1u + randbelow(r, 3u, 2);
    for (uint32_t k = 0; k < n; ++k) create_emergency(e, m, r);
}

// random.seed(s); EmergencyResponseEnv(): the constructor's draws.  It does not reset: the env is left without an incident, as a
// fresh object is, until the reset() that follows.  The stream must be at its start.
template <class M, class R>
CGE_HD void draw_network(Env &e, M &m, R &r) {
    clear_episode(e, m);
#pragma unroll 1
    for (int i = 0; i < 30; ++i) {
        const uint32_t n = i < 10 || i > 20 ? 201u : i <= 15 ? 451u : 81u;
        const int bits = i < 10 || i > 20 ? 8 : i <= 15 ? 9 : 7;
#pragma unroll 1
        for (int j = 0; j < 30; ++j) randbelow(r, n, bits);         // population_density
    }
    e.station[0] = e.station[1] = e.station[2] = e.station[3] = 0u;
#pragma unroll
    for (int f = 0; f < 20; ++f) e.station[f / 6] |= (5u + randbelow(r, 21u, 5)) << (5 * (f % 6));
#pragma unroll 1
    for (int h = 0; h < NH; ++h) { randbelow(r, 101u, 7); randbelow(r, 21u, 5); randbelow(r, 121u, 7); randbelow(r, 26u, 5); }
    e.prev_resolved = 0; e.prev_lives = 0; e.prev_casualties = 0;   // a fresh object has no _prev_ attributes
}

// _dispatch_unit :692-736
template <class M>
CGE_HD void dispatch(Env &e, M &m, uint32_t u) {
    const uint32_t w = m.unit(u);
    if (w & U_BUSY) return;
    const uint32_t mine = u < 12u ? FIRE_TRUCKS : POLICE_CARS;
    const int ux = (int)un_x(w), uy = (int)un_y(w);
    uint32_t best = NI;
    double best_d = INFINITY;
#pragma unroll 1
    for (uint32_t s = 0; s < e.ninc; ++s) {
        const uint32_t iw = m.inc(s);
        const uint32_t need = u < 12u ? in_fire(iw) : in_police(iw);   // 0: the type is not in required_units
        if ((uint32_t)__builtin_popcount(m.mask(s) & mine) >= need) continue;
        const int dx = ux - (int)in_x(iw), dy = uy - (int)in_y(iw);
        const double d = sqrt((double)(dx * dx + dy * dy));
        if (d < best_d) { best_d = d; best = s; }
    }
    if (best < NI) {
        const int tt = (int)(best_d * (2.0 - e.road()));
        m.set_unit(u, (w & 1023u) | U_BUSY | best << 11 | (uint32_t)(tt > 1 ? tt : 1) << 16);
        m.set_mask(best, m.mask(best) | 1u << u);
    }
}

// np.mean of 25 float64: NumPy's pairwise sum — eight strided partial sums over the first 24, combined as a tree, then the 25th
CGE_HD double mean25(const double (&v)[NT]) {
    double r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = (v[j] + v[8 + j]) + v[16 + j];
    return ((((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))) + v[24]) / 25.0;
}

// step() :883-922 up to the observation; `valid` false is an action outside 0..49, which falls through every branch.  Returns the reward.
template <class M, class R>
CGE_HD double env_step(Env &e, M &m, R &r, int32_t action, bool valid, uint32_t max_timesteps, bool &terminated) {
    const uint32_t a = valid ? (uint32_t)action : 49u;
    bool bonus44 = false;
    if (a < 20u) {                                                   // :648-690
        dispatch(e, m, a);
    } else if (a < 26u) {
        e.evac |= 1u << (a - 20u);
    } else if (a < 32u) {
        if (!e.mutual) {
            e.mutual = 1;
#pragma unroll 1
            for (int k = 0; k < 20; ++k) randbelow(r, 30u, 5);       // five units: x, y, home_x, home_y
        }
    } else if (a < 38u) {                                            // beds_available is at its cap already
    } else if (a < 44u) {
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            if (a == 38u + (uint32_t)k) e.traffic[k] *= 0.7;
        }
    } else if (a == 44u) {
        if (!e.soe) { e.soe = 1; bonus44 = true; }
    } else if (a == 45u) {
        e.reach = dmin(1.0, e.reach + 0.1);
    } else if (a == 46u) {
        if (!e.guard && e.soe) {
            e.guard = 1;
#pragma unroll 1
            for (int k = 0; k < 40; ++k) randbelow(r, 30u, 5);       // ten units
        }
    } else if (a == 48u) {
        e.cell = dmin(1.0, e.cell + 0.05);
    }
    double rate = 0.02 * e.cm;                                       // :285-301
    if (e.precip > 0.7) rate *= 1.5;
    if (e.wind > 0.8) rate *= 1.3;
    if (random01(r) < rate && e.ninc < (uint32_t)NI) create_emergency(e, m, r);
    uint32_t risky = 0;                                              // bit s: escalation_risk > 0.8 (:401-419)
    const uint32_t n0 = e.ninc;                                      // the incidents a cascade adds are not visited
#pragma unroll 1
    for (uint32_t s = 0; s < n0; ++s) {
        uint32_t iw = m.inc(s);
        const double tf = (double)(e.t - m.start(s)) / 60.0, sf = (double)in_sev(iw) / 10.0;
        const double rf = (double)__builtin_popcount(m.mask(s)) / (double)imax(1u, in_sum(iw));
        const double risk = tf * sf * (1.0 - rf);                    // min(1.0, .) changes neither comparison
        if (risk > 0.8) {
            risky |= 1u << s;
            if (random01(r) < 0.1) {                                 // :421-428
                const uint32_t sev = imin(10u, in_sev(iw) + 1u);
                randbelow(r, 5u, 3);                                 // incident.casualties
                e.casualties += 1u + randbelow(r, 5u, 3);
                iw = in_make(in_x(iw), in_y(iw), in_kind(iw), sev);
                m.set_inc(s, iw);
            }
        }
        if (risk > 0.6 && random01(r) < 0.05 && e.ninc < (uint32_t)NI) {   // :430-463
            const int x = (int)in_x(iw) + (int)randbelow(r, 7u, 3) - 3, y = (int)in_y(iw) + (int)randbelow(r, 7u, 3) - 3;
            const uint32_t k = in_kind(iw), sev = 3u + randbelow(r, 5u, 3);
            randbelow(r, 4u, 3);                                     // casualties
            add_incident(e, m, (uint32_t)(x < 0 ? 0 : x > 29 ? 29 : x), (uint32_t)(y < 0 ? 0 : y > 29 ? 29 : y),
                         k == FIRE || k == QUAKE || k == GAS ? FIRE : k == ACCIDENT ? ACCIDENT : k == CHEMICAL ? GAS : MEDICAL, sev);
            e.cm = dmin(3.0, e.cm + 0.1);
        }
    }
    const double road = e.road();
    bool removed = false;
#pragma unroll 1
    for (uint32_t u = 0; u < (uint32_t)NU; ++u) {                    // :465-522
        uint32_t w = m.unit(u);
        if (w & U_BUSY) {
            if (un_travel(w)) {
                w -= 1u << 16;
                m.set_unit(u, w);
            } else {
                const uint32_t s = un_slot(w);
                uint32_t iw = m.inc(s);
                w = (w & ~1023u) | in_x(iw) | in_y(iw) << 5;
                m.set_unit(u, w);
                double ready = dmax(0.3, 1.0 - m.fatigue(u));
                if (bonus44) ready = dmin(1.0, ready + 0.2);
                if (a == 47u && u < 12u) ready = dmin(1.0, ready + 0.1);
                if (random01(r) < ready * e.vis * road * 0.1) {
                    iw = in_set_sev(iw, in_sev(iw) - 1u);             // a worked incident has severity >= 1
                    m.set_inc(s, iw);
                    if (random01(r) < 0.3) e.lives += 1;
                }
                if (in_sev(iw) == 0u) {
                    e.resolved += 1;
                    e.rt_last = e.t - m.start(s);
                    e.rt_sum += e.rt_last;
                    e.rt_count += 1;
                    removed = true;
                    uint32_t bits = m.mask(s);
                    while (bits) {
                        const uint32_t k = (uint32_t)__builtin_ctz(bits);
                        bits &= bits - 1u;
                        m.set_unit(k, m.unit(k) & ~U_BUSY);
                    }
                    w = m.unit(u);
                }
            }
        }
        const double f = m.fatigue(u);
        m.set_fatigue(u, (w & U_BUSY) ? dmin(1.0, f + 0.01) : dmax(0.0, f - 0.005));
    }
    {                                                                // :768-780 and :782-806: 3 + 25 uniforms, 56 words in order
        uint32_t q[16];
        r.run(q);
        e.vis = dmax(0.3, dmin(1.0, e.vis + (-0.1 + WIDE * random53(q[0], q[1]))));
        e.precip = dmax(0.0, dmin(1.0, e.precip + (-0.05 + NARROW * random53(q[2], q[3]))));
        e.wind = dmax(0.0, dmin(1.0, e.wind + (-0.1 + WIDE * random53(q[4], q[5]))));
        const uint32_t hour = (e.t / 60u) % 24u;
        const double base = (hour >= 7u && hour <= 9u) || (hour >= 17u && hour <= 19u) ? 0.7 : hour >= 22u || hour <= 5u ? 0.1 : 0.3;
        const double target0 = base + (double)e.ninc * 0.05 + e.precip * 0.3;   // a contained incident still counts
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const double tg = dmax(0.0, dmin(1.0, target0 + (-0.1 + WIDE * random53(q[6 + 2 * i], q[7 + 2 * i]))));
            e.traffic[i] = e.traffic[i] * 0.8 + tg * 0.2;
        }
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            uint32_t p[20];
            r.run(p);
#pragma unroll
            for (int i = 0; i < 10; ++i) {
                const double tg = dmax(0.0, dmin(1.0, target0 + (-0.1 + WIDE * random53(p[2 * i], p[2 * i + 1]))));
                e.traffic[5 + 10 * b + i] = e.traffic[5 + 10 * b + i] * 0.8 + tg * 0.2;
            }
        }
    }
    if (removed) {                                                   // :894-898, from the back: slots behind a removed one move up
#pragma unroll 1
        for (uint32_t s = e.ninc; s-- > 0u;) {
            if (in_sev(m.inc(s))) continue;
#pragma unroll 1
            for (uint32_t k = s + 1u; k < e.ninc; ++k) { m.set_inc(k - 1u, m.inc(k)); m.set_mask(k - 1u, m.mask(k)); m.set_start(k - 1u, m.start(k)); }
#pragma unroll 1
            for (uint32_t u = 0; u < (uint32_t)NU; ++u) {
                const uint32_t w = m.unit(u);
                if (un_slot(w) > s) m.set_unit(u, w - (1u << 11));
            }
            risky = (risky & ((1u << s) - 1u)) | (risky >> (s + 1u)) << s;
            e.ninc -= 1;
        }
    }
    double reward = 0.0;                                             // :589-646
    if (e.resolved > e.prev_resolved) reward += 2000.0 * (double)(e.resolved - e.prev_resolved);
    if (e.lives > e.prev_lives) reward += 5000.0 * (double)(e.lives - e.prev_lives);
    if (e.rt_count && e.rt_last <= 15u) reward += 1000.0;
    if (e.cm < 1.2) reward += 300.0;
    if (e.casualties > e.prev_casualties) reward -= 10000.0 * (double)(e.casualties - e.prev_casualties);
    reward -= 2000.0 * (double)__builtin_popcount(risky);
    uint32_t over = 0;
#pragma unroll 1
    for (uint32_t s = 0; s < e.ninc; ++s) over += (double)__builtin_popcount(m.mask(s)) > (double)in_sum(m.inc(s)) * 1.5 ? 1u : 0u;
    reward -= 1000.0 * (double)over;
    if (mean25(e.traffic) > 0.8) reward -= 500.0;
    e.prev_resolved = e.resolved; e.prev_lives = e.lives; e.prev_casualties = e.casualties;
    e.reason = e.ninc == 0u && e.t > 60u ? REASON_SUCCESS                                  // :808-827, before the clock moves
               : e.casualties > 50u ? REASON_CASUALTIES
               : e.avg_rt() > 45.0 ? REASON_OVERWHELMED
               : e.t >= max_timesteps ? REASON_TIMEOUT : REASON_NONE;
    terminated = e.reason != REASON_NONE;
    e.t += 1;
    return reward;
}

// _get_observation :524-587 as three groups, out(k, value) with k the element's index in the row:
//   incidents [0, 80): four floats each; units [80, 200): three floats each; the rest [200, 276): traffic 25, hospitals 24, weather 5,
//   zones 12, communication 10
template <class M, class F>
CGE_HD void observe_incident(const Env &e, M &m, F &out, int s) {
    const bool on = (uint32_t)s < e.ninc;
    const uint32_t w = on ? m.inc(s) : 0u;
    out(4 * s, (float)((double)in_x(w) / 30.0));
    out(4 * s + 1, (float)((double)in_y(w) / 30.0));
    out(4 * s + 2, (float)((double)in_kind(w) / 7.0));
    out(4 * s + 3, (float)((double)in_sev(w) / 10.0));
}
template <class M, class F>
CGE_HD void observe_unit(const Env &e, M &m, F &out, int u) {
    uint32_t x, y, busy = 0;
    if (u < NU) { const uint32_t w = m.unit(u); x = un_x(w); y = un_y(w); busy = w & U_BUSY; }
    else if (u < 30) { x = home_x(u); y = home_y(u); }
    else { x = e.station_field(2 * (u - 30)); y = e.station_field(2 * (u - 30) + 1); }
    out(80 + 3 * u, (float)((double)x / 30.0));
    out(81 + 3 * u, (float)((double)y / 30.0));
    out(82 + 3 * u, busy ? 1.0f : 0.0f);
}
template <class M, class F>
CGE_HD void observe_rest(const Env &e, M &m, F &out, uint32_t max_timesteps) {
#pragma unroll
    for (int k = 0; k < NT; ++k) out(200 + k, (float)e.traffic[k]);
    double sum[NH];
#pragma unroll
    for (int h = 0; h < NH; ++h) sum[h] = 0.0;
#pragma unroll 1
    for (uint32_t s = 0; s < e.ninc; ++s) {                          // sum() from int 0, left to right over the incidents
        const uint32_t w = m.inc(s);
#pragma unroll
        for (int h = 0; h < NH; ++h) {
            const int dx = (int)in_x(w) - hospital_x(h), dy = (int)in_y(w) - hospital_y(h);
            sum[h] = sum[h] + sqrt((double)(dx * dx + dy * dy));
        }
    }
#pragma unroll
    for (int h = 0; h < NH; ++h) {
        out(225 + 3 * h, 1.0f);
        out(226 + 3 * h, 1.0f);
        out(227 + 3 * h, (float)dmin(1.0, sum[h] / 100.0));
    }
    out(249, (float)e.vis); out(250, (float)e.road()); out(251, (float)e.wind); out(252, (float)e.precip); out(253, 0.5f);
#pragma unroll
    for (int z = 0; z < 6; ++z) { out(254 + 2 * z, (e.evac >> z) & 1u ? 1.0f : 0.0f); out(255 + 2 * z, 0.0f); }
    uint32_t busy = 0;
#pragma unroll
    for (int u = 0; u < NU; ++u) busy += m.unit(u) & U_BUSY ? 1u : 0u;
    out(266, (float)(8.0 / 10.0)); out(267, (float)e.cell); out(268, (float)e.reach);
    out(269, e.soe ? 1.0f : 0.0f); out(270, e.mutual ? 1.0f : 0.0f); out(271, e.guard ? 1.0f : 0.0f);
    out(272, (float)((double)e.ninc / 20.0)); out(273, (float)((double)busy / 40.0)); out(274, (float)((double)e.casualties / 100.0));
    out(275, (float)((double)e.t / (double)max_timesteps));
}


// Canonical records (cge_records_emergency_*, lane_records.hip): what a record's body must satisfy before it may become an env, so that
// no kernel of the type reads or writes out of range.  get(w) is word w of the body.  The fields a kernel uses as an index or a bound:
//   ninc (scalar word 24, 5 bits)   every walk over the incidents, add_incident's slot: rows 0..NI-1 of the incident words
//   mask (incident word 1)          the release walk of a contained incident indexes the unit rows by every set bit: bits 0..NU-1
//   slot (unit word, 5 bits)        a working unit indexes the incident rows by it: 0..NI-1
// Every slot of the twenty is checked, used or not: a stale one holds what a valid one held.  Nothing else in the record reaches an
// address: coordinates, kinds, severities and counters enter arithmetic only, the stations are indexed at compile time.  No kernel
// calls this.
enum { RECORD_OK = 0, RECORD_NINC = 16, RECORD_MASK = 17, RECORD_SLOT = 18 };
template <class G>
CGE_HD int record_refusal(G get) {
    if ((get(W_SCAL + 24) & 31u) > (uint32_t)NI) return RECORD_NINC;
    for (int s = 0; s < NI; ++s)
        if (get(W_INC + 3 * s + 1) >> NU) return RECORD_MASK;
    for (int u = 0; u < NU; ++u)
        if (un_slot(get(W_UNIT + u)) >= (uint32_t)NI) return RECORD_SLOT;
    return RECORD_OK;
}
inline const char *record_refusal_text(int code) {
    return code == RECORD_NINC ? "more than 20 active incidents" : code == RECORD_MASK ? "an incident's unit mask names a unit above 19"
           : code == RECORD_SLOT ? "a unit's incident slot is above 19" : "bad record";
}
constexpr int RECORD_CURSOR_FIRST = W_SCAL + 29, RECORD_CURSOR_WORDS = 2;   // mt_pos, mt_ready

}  // namespace emergency
}  // namespace cge
