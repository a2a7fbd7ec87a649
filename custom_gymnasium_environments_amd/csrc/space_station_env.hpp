// space_station_env.hpp — the record and the dynamics of one SpaceStationEnv, plain C++ (host and device): space_station.hip runs it
// one lane per env; tools/probes/space_station_host_check.cpp replays the reference fixtures through the same code on the CPU.
// Compile it without FP contraction: every product and sum below is rounded where the reference rounds it.
//
// Re-expresses the reference's space_station_env/station_env.py:
//   reset :247-308, step :310-349, _process_action :351-398, _update_orbital_position :400-420, _update_power_systems :422-443,
//   _update_life_support :445-479, _update_crew :481-523, _update_resources :525-556, _check_emergencies :558-601,
//   _update_system_degradation :603-621, _activate_emergency_protocols :623-638, _initiate_evacuation :640-651,
//   _calculate_reward :653-712, _check_termination :714-737, _get_observation :739-783, _get_info :785-797
// State is float64 throughout, in the reference's operation order (DESIGN.md §3.17 argues each point):
//   modules    8 x (oxygen_percent, co2_ppm, pressure, temperature)
//   crew       6 x (health, oxygen_level, fatigue); a task is one bit (only "emergency_response" is ever read); the module of a crew
//              member is one bit for all: member c is in module c until action 38 puts everybody in Docking, which no reset undoes;
//              x and y never change
//   systems    12 x (efficiency, maintenance_needed) and last_maintenance; power_draw and is_critical are constants
//   resources  water, food, oxygen_tanks, spare_parts, waste_capacity (nitrogen, medical_supplies and fuel stay at 100, 100, 200)
//   orbit      orbital_phase advances by exactly 20.0 mod 360: an index 0..17.  solar_angle is the phase of the last step and is NOT
//              reset, so it is a second index; cos, the solar efficiency and the radiation level are tables of 18 float64 constants
//              (no libm on the device; tests/test_space_station_cpu.py pins every entry against math.cos / math.sin).
//              radiation_level is not reset either: the table entry of the angle index, or a solar storm's 0.8 (one bit).
//   the rest   battery, total_power_consumption (not reset), episode_reward (never reset) and the episode's own return, the alerts,
//              counters, last_emergency_time (not reset).
// What a runtime index reaches — a system (actions 0..23, choice), a module (actions 30..35, choice), a crew member (choice) — is
// written through set_at() / update_at(): a compare and a select per element, so that every array stays in registers on the device and nothing is
// indexed in memory (no LDS rows, no scratch).  Everything else is indexed at compile time.
// The one libm call is log() in the 32 Gaussian draws of a reset: the host build uses glibc's, the device its own, which may differ in
// the last place; that touches the float64 module state after a reset and nothing else.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CGE_HD __host__ __device__ __forceinline__
#else
#define CGE_HD inline
#endif

namespace cge {
namespace station {

constexpr int NM = 8, NC = 6, NS = 12, OBS = 120, ACTIONS = 40, DOCKING = 6;
constexpr int O2_GEN = 0, CO2_SCRUB = 1, WATER_REC = 2, THERMAL = 4, WASTE = 7;
constexpr uint32_t CRITICAL = 0x33Fu;                               // systems 0..5, 8, 9 (:175-244)
enum : uint32_t { A_FIRE = 1u, A_DEPRESS = 2u, A_STORM = 4u, A_POWER = 8u, A_LIFE = 16u, A_MEDICAL = 32u };   // the alerts in the observation's order

// the record: 32-bit columns [word][env]
constexpr int W_MOD = 0, W_CREW = W_MOD + 8 * NM, W_SYS = W_CREW + 6 * NC, W_LM = W_SYS + 4 * NS, W_RES = W_LM + NS, W_PWR = W_RES + 10,
              W_SCAL = W_PWR + 8, N_SCAL = 10, REC_WORDS = W_SCAL + N_SCAL;
static_assert(REC_WORDS == 188, "documented as 752 bytes per env");

CGE_HD double power_draw(int s) {
    constexpr double w[NS] = {500.0, 300.0, 400.0, 0.0, 600.0, 200.0, 100.0, 350.0, 50.0, 800.0, 250.0, 1000.0};
    return w[s];
}
CGE_HD double crew_x(int c) { constexpr double x[NC] = {1.5, 5.0, 9.5, 1.5, 5.0, 8.5}; return x[c]; }   // :151-171: the centre of module c
CGE_HD double crew_y(int c) { constexpr double y[NC] = {1.5, 3.0, 2.0, 5.5, 8.0, 5.5}; return y[c]; }
// math.cos(math.radians(20.0 * k))
CGE_HD double cos_phase(uint32_t k) {
    constexpr double v[18] = {0x1.0000000000000p+0,  0x1.e11f642522d1cp-1,  0x1.8836fa2cf5039p-1,  0x1.0000000000001p-1,  0x1.63a1a7e0b738cp-3,
                              -0x1.63a1a7e0b7388p-3, -0x1.ffffffffffffcp-2, -0x1.8836fa2cf5038p-1, -0x1.e11f642522d1bp-1, -0x1.0000000000000p+0,
                              -0x1.e11f642522d1cp-1, -0x1.8836fa2cf5039p-1, -0x1.0000000000004p-1, -0x1.63a1a7e0b7389p-3, 0x1.63a1a7e0b737cp-3,
                              0x1.0000000000001p-1,  0x1.8836fa2cf5037p-1,  0x1.e11f642522d1cp-1};
    return v[k];
}
// solar_efficiency :411-414: 0.0 in the shadow (180 < phase < 270), otherwise max(0, cos)
CGE_HD double solar_eff(uint32_t k) {
    constexpr double v[18] = {0x1.0000000000000p+0, 0x1.e11f642522d1cp-1, 0x1.8836fa2cf5039p-1, 0x1.0000000000001p-1, 0x1.63a1a7e0b738cp-3, 0.0, 0.0, 0.0, 0.0,
                              0.0, 0.0, 0.0, 0.0, 0.0, 0x1.63a1a7e0b737cp-3, 0x1.0000000000001p-1, 0x1.8836fa2cf5037p-1, 0x1.e11f642522d1cp-1};
    return v[k];
}
// radiation_level :417-420: 0.3 + 0.2 * math.sin(math.radians(20.0 * k - 90)) for 90 < phase < 270, otherwise 0.2
CGE_HD double radiation_of(uint32_t k) {
    constexpr double v[18] = {0x1.999999999999ap-3, 0x1.999999999999ap-3, 0x1.999999999999ap-3, 0x1.999999999999ap-3, 0x1.999999999999ap-3,
                              0x1.56c35d9678b8ep-2, 0x1.9999999999999p-2, 0x1.d015fdab9534ap-2, 0x1.f3a6280edaba4p-2, 0x1.0000000000000p-1,
                              0x1.f3a6280edaba5p-2, 0x1.d015fdab9534ap-2, 0x1.9999999999999p-2, 0x1.56c35d9678b8dp-2, 0x1.999999999999ap-3,
                              0x1.999999999999ap-3, 0x1.999999999999ap-3, 0x1.999999999999ap-3};
    return v[k];
}

// NumPy's legacy draws on a source of tempered MT19937 words: R::next(), and R::run(w) for W words the caller will consume in order
CGE_HD double random53(uint32_t w0, uint32_t w1) { return ((double)(w0 >> 5) * 67108864.0 + (double)(w1 >> 6)) / 9007199254740992.0; }
template <class R>
CGE_HD double random01(R &r) {
    const uint32_t a = r.next(), b = r.next();
    return random53(a, b);
}
// RandomState.choice(seq) = randint(0, len): one 32-bit word per attempt, masked to the smallest 2^b - 1 >= len - 1, rejected above
template <class R>
CGE_HD uint32_t choice(R &r, uint32_t n, uint32_t mask) {
    uint32_t v = r.next() & mask;
    while (v >= n) v = r.next() & mask;
    return v;
}
// two values of legacy_gauss (polar method): the first call returns f * x2 and caches f * x1 for the second
template <class R>
CGE_HD void gauss_pair(R &r, double &first, double &second) {
    double x1, x2, r2;
    do {
        x1 = 2.0 * random01(r) - 1.0;
        x2 = 2.0 * random01(r) - 1.0;
        r2 = x1 * x1 + x2 * x2;
    } while (r2 >= 1.0 || r2 == 0.0);
    const double f = sqrt(-2.0 * log(r2) / r2);
    first = f * x2;
    second = f * x1;
}
CGE_HD double pymin(double cap, double v) { return v < cap ? v : cap; }        // Python's min(cap, v)
CGE_HD double pymax0(double v) { return v > 0.0 ? v : 0.0; }                   // Python's max(0, v)
CGE_HD double clip(double x, double lo, double hi) {                           // np.clip: min(max(x, lo), hi) as `a > b ? a : b`, `a < b ? a : b`
    const double t = x > lo ? x : lo;
    return t < hi ? t : hi;
}
template <int N>
CGE_HD void set_at(double (&v)[N], uint32_t k, double x) {                      // v[k] = x without an indexed register array
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = (uint32_t)j == k ? x : v[j];
}
// v[k] = f(v[k]): f is evaluated for every element and selected for one.  (Reading v[k] alone as a chain of selects is turned back
// into an indexed load by the compiler, and with it the whole record into scratch.)
template <int N, class F>
CGE_HD void update_at(double (&v)[N], uint32_t k, F f) {
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = (uint32_t)j == k ? f(v[j]) : v[j];
}

// np.mean in NumPy's summation order: a plain loop below eight values, the unrolled block of eight combined as a tree, the rest in turn
CGE_HD double mean6(const double (&v)[NC]) { return (((((v[0] + v[1]) + v[2]) + v[3]) + v[4]) + v[5]) / 6.0; }
CGE_HD double sum8(const double *v) { return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7])); }
CGE_HD double mean8(const double (&v)[NM]) { return sum8(v) / 8.0; }
CGE_HD double mean12(const double (&v)[NS]) { return ((((sum8(v) + v[8]) + v[9]) + v[10]) + v[11]) / 12.0; }

struct Env {
    double o2[NM], co2[NM], pres[NM], temp[NM];
    double health[NC], oxy[NC], fatigue[NC];
    double eff[NS], maint[NS];
    uint32_t last_maint[NS];
    double water, food, tanks, spare, waste;
    double battery, total_power, ret, ep_ret;                       // ret: the reference's episode_reward, never reset; ep_ret: this episode's
    uint32_t t, casualties, emergencies, failures, failure_mask, alerts, task, backup, success, evac, storm, needs_reset, phase, angle;
    int32_t last_emergency;
    uint32_t mt_pos, mt_ready;

    CGE_HD double radiation() const { return storm ? 0.8 : radiation_of(angle); }
    CGE_HD uint32_t alive() const {
        uint32_t n = 0;
#pragma unroll
        for (int c = 0; c < NC; ++c) n += health[c] > 0.0 ? 1u : 0u;
        return n;
    }

    // the scalar columns W_SCAL .. W_SCAL + 9, as put(word, value) / get(word)
    template <class F>
    CGE_HD void pack_scalars(F put) const {
        put(0, t); put(1, (uint32_t)last_emergency); put(2, casualties); put(3, emergencies); put(4, failures);
        put(5, failure_mask | alerts << 12 | task << 18 | backup << 24 | success << 25 | evac << 26 | storm << 27 | needs_reset << 28);
        put(6, phase | angle << 5);
        put(7, mt_pos); put(8, mt_ready); put(9, 0u);
    }
    template <class F>
    CGE_HD void unpack_scalars(F get) {
        t = get(0); last_emergency = (int32_t)get(1); casualties = get(2); emergencies = get(3); failures = get(4);
        const uint32_t f = get(5);
        failure_mask = f & 4095u; alerts = (f >> 12) & 63u; task = (f >> 18) & 63u; backup = (f >> 24) & 1u; success = (f >> 25) & 1u;
        evac = (f >> 26) & 1u; storm = (f >> 27) & 1u; needs_reset = (f >> 28) & 1u;
        const uint32_t o = get(6);
        phase = o & 31u; angle = (o >> 5) & 31u;
        mt_pos = get(7); mt_ready = get(8);
    }
    // every float64 of the record in its column order: f(word offset from W_MOD, value)
    template <class E, class F>
    static CGE_HD void each_double(E &e, F f) {
#pragma unroll
        for (int m = 0; m < NM; ++m) { f(W_MOD + 2 * m, e.o2[m]); f(W_MOD + 2 * (NM + m), e.co2[m]); f(W_MOD + 2 * (2 * NM + m), e.pres[m]); f(W_MOD + 2 * (3 * NM + m), e.temp[m]); }
#pragma unroll
        for (int c = 0; c < NC; ++c) { f(W_CREW + 2 * c, e.health[c]); f(W_CREW + 2 * (NC + c), e.oxy[c]); f(W_CREW + 2 * (2 * NC + c), e.fatigue[c]); }
#pragma unroll
        for (int s = 0; s < NS; ++s) { f(W_SYS + 2 * s, e.eff[s]); f(W_SYS + 2 * (NS + s), e.maint[s]); }
        f(W_RES, e.water); f(W_RES + 2, e.food); f(W_RES + 4, e.tanks); f(W_RES + 6, e.spare); f(W_RES + 8, e.waste);
        f(W_PWR, e.battery); f(W_PWR + 2, e.total_power); f(W_PWR + 4, e.ret); f(W_PWR + 6, e.ep_ret);
    }
};

// np.random.seed(s); SpaceStationEnv(): the constructor draws nothing (:56-135) and sets what reset() will not touch
CGE_HD void construct(Env &e) {
    e.ret = 0.0; e.ep_ret = 0.0; e.last_emergency = 0; e.evac = 0; e.angle = 0; e.storm = 0; e.total_power = 0.0; e.needs_reset = 0;
    e.t = 0; e.phase = 0; e.casualties = 0; e.emergencies = 0; e.failures = 0; e.failure_mask = 0; e.alerts = 0; e.task = 0; e.backup = 1; e.success = 0;
    e.water = 1000.0; e.food = 500.0; e.tanks = 20.0; e.spare = 50.0; e.waste = 100.0; e.battery = 100.0;
#pragma unroll
    for (int m = 0; m < NM; ++m) { e.o2[m] = 21.0; e.co2[m] = 400.0; e.pres[m] = 101.3; e.temp[m] = 22.0; }
#pragma unroll
    for (int c = 0; c < NC; ++c) { e.health[c] = 100.0; e.oxy[c] = 100.0; e.fatigue[c] = 0.0; }
#pragma unroll
    for (int s = 0; s < NS; ++s) { e.eff[s] = 100.0; e.maint[s] = 0.0; e.last_maint[s] = 0; }
}

// reset() :247-308: 32 normal draws (16 polar pairs: the cache is empty afterwards), then 24 uniform
template <class R>
CGE_HD void reset_episode(Env &e, R &r) {
    e.t = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (uint32_t m = 0; m < (uint32_t)NM; ++m) {
        double g0, g1, g2, g3;
        gauss_pair(r, g0, g1);
        gauss_pair(r, g2, g3);
        set_at(e.o2, m, 21.0 + (0.0 + 0.5 * g0));                   // normal(loc, scale) = loc + scale * gauss
        set_at(e.co2, m, 400.0 + (0.0 + 50.0 * g1));
        set_at(e.pres, m, 101.3 + (0.0 + 1.0 * g2));
        set_at(e.temp, m, 22.0 + (0.0 + 1.0 * g3));
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) { e.health[c] = 100.0; e.oxy[c] = 100.0; e.fatigue[c] = 0.0; }
    e.task = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (uint32_t s = 0; s < (uint32_t)NS; ++s) {
        const double u0 = random01(r), u1 = random01(r);
        set_at(e.eff, s, 100.0 - (0.0 + 5.0 * u0));                 // uniform(a, b) = a + (b - a) * random()
        set_at(e.maint, s, 0.0 + 10.0 * u1);
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) e.last_maint[s] = 0;
    e.water = 1000.0; e.food = 500.0; e.tanks = 20.0; e.spare = 50.0; e.waste = 100.0;
    e.battery = 100.0; e.backup = 1;
    e.phase = 0;
    e.alerts = 0; e.success = 0; e.casualties = 0; e.failures = 0; e.failure_mask = 0; e.emergencies = 0;
    e.needs_reset = 0;
    e.ep_ret = 0.0;
}

// step() :310-349 up to the observation; `valid` false is an action outside 0..39: _process_action is skipped.  Returns the reward.
template <class R>
CGE_HD double env_step(Env &e, R &r, int32_t action, bool valid, uint32_t max_steps, bool &terminated, bool &truncated) {
    const uint32_t a = valid ? (uint32_t)action : 39u;
    e.t += 1;
    if (a < 12u) {                                                   // :351-398
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if (a == (uint32_t)s) e.eff[s] = pymin(100.0, e.eff[s] + 10.0);
        }
    } else if (a < 24u) {
        if (e.spare > 0.0) {
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                if (a - 12u == (uint32_t)s) { e.maint[s] = pymax0(e.maint[s] - 20.0); e.last_maint[s] = e.t; }
            }
            e.spare -= 0.5;
        }
    } else if (a < 30u) {
        e.task |= 1u << (a - 24u);
    } else if (a < 36u) {
        uint32_t q[4];
        r.run(q);
        const uint32_t m = a - 30u;
        const double dt = -1.0 + 2.0 * random53(q[0], q[1]), dp = -0.5 + 1.0 * random53(q[2], q[3]);
        update_at(e.temp, m, [&](double v) { return clip(v + dt, 18.0, 26.0); });
        update_at(e.pres, m, [&](double v) { return clip(v + dp, 95.0, 108.0); });
    } else if (a == 36u) {                                           // :623-638
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if ((CRITICAL >> s) & 1u) e.eff[s] = pymin(100.0, e.eff[s] + 20.0);
        }
        if (e.tanks > 0.0) {
#pragma unroll
            for (int m = 0; m < NM; ++m) e.o2[m] = pymin(25.0, e.o2[m] + 2.0);
            e.tanks -= 0.5;
        }
        e.task = 63u;
    } else if (a == 37u) {
        if (e.backup) { e.battery = pymin(100.0, e.battery + 20.0); e.backup = 0; }
    } else if (a == 38u) {                                           // :640-651; the task "evacuation" is never read
        e.evac = 1; e.task = 0;
        e.pres[DOCKING] = 101.3; e.o2[DOCKING] = 21.0; e.temp[DOCKING] = 22.0;
    }
    e.phase = e.phase == 17u ? 0u : e.phase + 1u;                    // :400-420
    e.angle = e.phase; e.storm = 0;
    double total = power_draw(0) * (e.eff[0] / 100.0);               // :422-443: sum() from int 0, left to right
#pragma unroll
    for (int s = 1; s < NS; ++s) total = total + power_draw(s) * (e.eff[s] / 100.0);
    e.total_power = total;
    const double balance = 5000.0 * solar_eff(e.phase) - total;
    e.battery = clip(e.battery + (balance / 5000.0) * 10.0, 0.0, 100.0);
    if (e.battery < 10.0) {
        e.alerts |= A_POWER;
#pragma unroll
        for (int s = 0; s < NS; ++s) e.eff[s] *= 0.8;
    }
    {                                                                // :445-479
        const bool o2_on = e.eff[O2_GEN] > 50.0, co2_on = e.eff[CO2_SCRUB] > 50.0, thermal_on = e.eff[THERMAL] > 50.0;
        const double o2_add = (e.eff[O2_GEN] / 100.0) * 0.05, co2_sub = (e.eff[CO2_SCRUB] / 100.0) * 10.0, th = e.eff[THERMAL] / 100.0;
        uint32_t q[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) q[j] = 0u;
        if (!thermal_on) r.run(q);                                   // the temperature drifts: one uniform(-0.5, 0.5) per module
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            const uint32_t crew = e.evac ? (m == DOCKING ? (uint32_t)NC : 0u) : (m < NC ? 1u : 0u);
            if (o2_on) e.o2[m] += o2_add;
            e.o2[m] -= (double)crew * 0.01;
            if (co2_on) e.co2[m] -= co2_sub;
            e.co2[m] += (double)(crew * 5u);
            e.o2[m] = clip(e.o2[m], 0.0, 30.0);
            e.co2[m] = clip(e.co2[m], 0.0, 10000.0);
            if (thermal_on) e.temp[m] += (22.0 - e.temp[m]) * 0.1 * th;
            else e.temp[m] += -0.5 + 1.0 * random53(q[2 * m], q[2 * m + 1]);
            e.temp[m] = clip(e.temp[m], 10.0, 35.0);
        }
    }
    const double rad = e.radiation();
#pragma unroll
    for (int c = 0; c < NC; ++c) {                                   // :481-523
        const double mo2 = e.evac ? e.o2[DOCKING] : e.o2[c], mco2 = e.evac ? e.co2[DOCKING] : e.co2[c], mt = e.evac ? e.temp[DOCKING] : e.temp[c];
        if (mo2 < 19.0) e.oxy[c] -= 2.0;
        else if (mo2 > 19.0) e.oxy[c] = pymin(100.0, e.oxy[c] + 1.0);
        if (mco2 > 1000.0) e.health[c] -= 0.5;
        if (mco2 > 5000.0) e.health[c] -= 2.0;
        if (mt < 15.0 || mt > 30.0) e.health[c] -= 0.3;
        e.fatigue[c] += 0.1;
        if (e.fatigue[c] > 80.0) e.health[c] -= 0.2;
        if ((e.task >> c) & 1u) e.fatigue[c] = pymax0(e.fatigue[c] - 5.0);
        if (rad > 0.5) e.health[c] -= rad * 0.1;
        e.health[c] = clip(e.health[c], 0.0, 100.0);
        e.oxy[c] = clip(e.oxy[c], 0.0, 100.0);
        e.fatigue[c] = clip(e.fatigue[c], 0.0, 100.0);
        if (e.health[c] <= 0.0 || e.oxy[c] <= 0.0) e.casualties += 1;
    }
    e.task = 0;
    {                                                                // :525-556
        const uint32_t alive = e.alive();
        const double used = (double)alive * 0.02;
        if (e.eff[WATER_REC] > 50.0) e.water -= used - used * (e.eff[WATER_REC] / 100.0) * 0.9;
        else e.water -= used;
        e.food -= (double)alive * 0.01;
        if (e.alerts & A_LIFE) e.tanks -= 0.1;
        const double made = (double)alive * 0.05;
        if (e.eff[WASTE] > 50.0) e.waste -= (made - made * (e.eff[WASTE] / 100.0)) * 0.1;
        else e.waste -= made * 0.2;
        e.water = pymax0(e.water); e.food = pymax0(e.food); e.tanks = pymax0(e.tanks); e.spare = pymax0(e.spare); e.waste = pymax0(e.waste);
    }
    if (random01(r) < 0.001) {                                       // :558-601
        const uint32_t kind = choice(r, 4u, 3u);
        if (kind == 0u) {
            const uint32_t m = choice(r, (uint32_t)NM, 7u);
            update_at(e.pres, m, [](double v) { return v - 10.0; });
            e.alerts |= A_DEPRESS;
        } else if (kind == 1u) {
            const uint32_t s = choice(r, (uint32_t)NS, 15u);
            set_at(e.eff, s, 0.0);
            e.failures += 1;
            e.failure_mask |= 1u << s;
            if ((CRITICAL >> s) & 1u) e.alerts |= A_LIFE;
        } else if (kind == 2u) {
            const uint32_t c = choice(r, (uint32_t)NC, 7u);
            update_at(e.health, c, [](double v) { return v - 30.0; });
            e.alerts |= A_MEDICAL;
        } else {
            e.storm = 1;
            e.alerts |= A_STORM;
        }
        e.emergencies += 1;
    }
    if (mean8(e.o2) < 18.0) e.alerts |= A_LIFE;
    if (e.battery < 5.0) e.alerts |= A_POWER;
    {                                                                // :603-621: twelve random(), 24 words in order
        uint32_t q[24];
        r.run(q);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            e.eff[s] -= 0.01;
            e.maint[s] += 0.05;
            if ((int64_t)e.t - (int64_t)e.last_maint[s] > 200) { e.eff[s] -= 0.1; e.maint[s] += 0.2; }
            if (random53(q[2 * s], q[2 * s + 1]) < 0.001) e.eff[s] = pymax0(e.eff[s] - 20.0);
            e.eff[s] = clip(e.eff[s], 0.0, 100.0);
            e.maint[s] = clip(e.maint[s], 0.0, 100.0);
        }
    }
    const uint32_t alive = e.alive();                                // :653-712; every term is an integer: the order of the sum is free
    double reward = (double)(alive * 10u);
    const double avg_o2 = mean8(e.o2), avg_co2 = mean8(e.co2), avg_eff = mean12(e.eff);
    if (19.0 < avg_o2 && avg_o2 < 23.0) reward += 50.0;
    if (avg_co2 < 1000.0) reward += 30.0;
    if (avg_eff > 90.0) reward += 200.0;
    else if (avg_eff > 70.0) reward += 50.0;
    if (e.water > 20.0 && e.food > 20.0 && e.tanks > 20.0) reward += 100.0;
    if (e.alerts) {
        if ((int64_t)e.t - (int64_t)e.last_emergency > 10) e.last_emergency = (int32_t)e.t;
        else if (alive == (uint32_t)NC) reward += 500.0;
    }
    if (e.casualties) reward -= 5000.0 * (double)e.casualties;
    reward -= 2000.0 * (double)__builtin_popcount(e.alerts & (A_DEPRESS | A_LIFE)) + 500.0 * (double)__builtin_popcount(e.alerts & ~(A_DEPRESS | A_LIFE));
    reward -= 100.0 * (double)((e.water < 10.0) + (e.food < 10.0) + (e.tanks < 10.0) + (e.spare < 10.0) + (e.waste < 10.0));
    if (e.battery > 50.0 && avg_eff > 80.0 && alive == (uint32_t)NC && !e.alerts) reward += 500.0;
    e.ret += reward;
    e.ep_ret += reward;
    truncated = e.t >= max_steps;                                    // :714-737
    if (truncated) {
        e.success = 1;
        terminated = true;
    } else {
        bool dead = true;
        uint32_t failed = 0;
#pragma unroll
        for (int c = 0; c < NC; ++c) dead = dead && e.health[c] <= 0.0;
#pragma unroll
        for (int s = 0; s < NS; ++s) failed += ((CRITICAL >> s) & 1u) && e.eff[s] < 10.0 ? 1u : 0u;
        terminated = dead || failed >= 3u || avg_o2 < 15.0 || mean8(e.pres) < 80.0;
    }
    return reward;
}

// _get_observation :739-783, out(k, value) with k the element's index in the row: crew [0, 24), systems [24, 60), modules [60, 92),
// power, resources, orbit and alerts [92, 120)
template <class F>
CGE_HD void observe_crew(const Env &e, F &out) {
#pragma unroll
    for (int c = 0; c < NC; ++c) { out(4 * c, (float)crew_x(c)); out(4 * c + 1, (float)crew_y(c)); out(4 * c + 2, (float)e.health[c]); out(4 * c + 3, (float)e.oxy[c]); }
}
template <class F>
CGE_HD void observe_systems(const Env &e, F &out) {
#pragma unroll
    for (int s = 0; s < NS; ++s) { out(24 + 3 * s, (float)e.eff[s]); out(25 + 3 * s, (float)power_draw(s)); out(26 + 3 * s, (float)e.maint[s]); }
}
template <class F>
CGE_HD void observe_modules(const Env &e, F &out) {
#pragma unroll
    for (int m = 0; m < NM; ++m) { out(60 + 4 * m, (float)e.o2[m]); out(61 + 4 * m, (float)e.co2[m]); out(62 + 4 * m, (float)e.pres[m]); out(63 + 4 * m, (float)e.temp[m]); }
}
template <class F>
CGE_HD void observe_rest(const Env &e, F &out) {
    out(92, (float)solar_eff(e.phase)); out(93, (float)e.battery); out(94, (float)e.total_power); out(95, e.backup ? 1.0f : 0.0f); out(96, 5000.0f);
#pragma unroll
    for (int k = 97; k < 102; ++k) out(k, 0.0f);
    out(102, (float)e.water); out(103, (float)e.food); out(104, (float)e.tanks); out(105, 100.0f); out(106, 100.0f); out(107, (float)e.spare); out(108, 200.0f);
    out(109, (float)e.waste);
    out(110, (float)(20.0 * (double)e.phase / 360.0)); out(111, (float)cos_phase(e.angle)); out(112, e.phase >= 10u && e.phase <= 13u ? 1.0f : 0.0f);
    out(113, (float)e.radiation());
#pragma unroll
    for (int k = 0; k < 6; ++k) out(114 + k, (e.alerts >> k) & 1u ? 1.0f : 0.0f);
}

// _get_info :785-797: the nine values in the reference's order (system_failures as the list's length), then what else the record knows
enum { INFO_TIME_STEP = 0, INFO_DAY, INFO_CREW_ALIVE, INFO_SYSTEM_FAILURES, INFO_EMERGENCY_COUNT, INFO_MISSION_SUCCESS, INFO_EPISODE_REWARD, INFO_BATTERY_LEVEL,
       INFO_AVG_CREW_HEALTH, INFO_SYSTEM_FAILURE_MASK, INFO_NEEDS_RESET, INFO_CREW_CASUALTIES, INFO_EVACUATED, INFO_COUNT };
CGE_HD double info_value(const Env &e, int field) {
    switch (field) {
        case INFO_TIME_STEP: return (double)e.t;
        case INFO_DAY: return (double)((uint64_t)e.t * 5u / 1440u);
        case INFO_CREW_ALIVE: return (double)e.alive();
        case INFO_SYSTEM_FAILURES: return (double)e.failures;
        case INFO_EMERGENCY_COUNT: return (double)e.emergencies;
        case INFO_MISSION_SUCCESS: return (double)e.success;
        case INFO_EPISODE_REWARD: return e.ret;
        case INFO_BATTERY_LEVEL: return e.battery;
        case INFO_AVG_CREW_HEALTH: return mean6(e.health);
        case INFO_SYSTEM_FAILURE_MASK: return (double)e.failure_mask;
        case INFO_NEEDS_RESET: return (double)e.needs_reset;
        case INFO_CREW_CASUALTIES: return (double)e.casualties;
        case INFO_EVACUATED: return (double)e.evac;
    }
    return 0.0;
}


// Canonical records (cge_records_space_station_*, lane_records.hip): what a record's body must satisfy before it may become an env, so
// that no kernel of the type reads out of range.  get(w) is word w of the body.  The fields a kernel uses as an index:
//   phase, angle (scalar word 6, 5 bits each)   the three tables of eighteen orbit positions: 0..17
// Modules, crew and systems are indexed at compile time or by a draw below their count.  The type keeps no cached Gaussian: a
// reset's sixteen polar pairs leave none.  No kernel calls this.
enum { RECORD_OK = 0, RECORD_PHASE = 16 };
template <class G>
CGE_HD int record_refusal(G get) {
    const uint32_t o = get(W_SCAL + 6);
    return (o & 31u) >= 18u || ((o >> 5) & 31u) >= 18u ? RECORD_PHASE : RECORD_OK;
}
inline const char *record_refusal_text(int code) { return code == RECORD_PHASE ? "orbit phase or angle is above 17" : "bad record"; }
constexpr int RECORD_CURSOR_FIRST = W_SCAL + 7, RECORD_CURSOR_WORDS = 2;   // mt_pos, mt_ready

}  // namespace station
}  // namespace cge
