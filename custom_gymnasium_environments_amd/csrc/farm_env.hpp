// farm_env.hpp — the record and the dynamics of one AgriculturalFarmEnv, plain C++ (host and device): farm.hip runs it one lane per
// env; tools/probes/farm_host_check.cpp replays the reference fixtures through the same code on the CPU.
// Compile it without FP contraction: every product and sum below is rounded where the reference rounds it.
//
// Re-expresses the reference's agricultural_farm_env/farm_env.py:
//   __init__ :127-192, _initialize_fields :194-220, _initialize_equipment :222-232, _initialize_market :234-240, weather ranges :242-274,
//   _update_weather :276-316, _update_crop_growth :318-356, _update_soil_conditions :358-388, _update_market_prices :390-411,
//   _calculate_operating_costs :413-433, _get_observation :435-518, reset :520-566, step :568-627, _process_action :629-800,
//   _harvest_crop :802-845, _calculate_environmental_rewards :847-883, _update_sustainability_metrics :885-909, _get_info :911-935
// and crops/crop_data.py: CROP_DATA :57-167, get_crop_stage_duration :170-223, calculate_yield_modifier :226-282,
// get_market_price_multiplier :285-320.
// State is float64 throughout, in the reference's operation order (DESIGN.md §3.18 argues each point):
//   fields     4 x (health, yield_potential, moisture, ph, nitrogen, phosphorus, potassium, compaction, organic matter, pest, disease)
//              and the integers crop (-1 is None), stage, last_crop (-1 is None), days_to_harvest, days_since_planting,
//              last_fertilized_day, last_pesticide_day.  `if field.crop_type` is `crop > 0` (wheat is 0 and false),
//              `is not None` is `crop >= 0`.  last_irrigated_day is never read; operation_field is never set.
//   equipment  8 x (fuel_level, maintenance_needed), the location (two integers below 25) and one is_operating bit
//   weather    temperature, humidity, rainfall, wind_speed, frost_risk, the two day counters (solar_radiation stays 15.0)
//   market     5 x (current, predicted)
//   the rest   reservoir_level, water_quality (NOT reset), cash_flow, operating_costs, profit_margin, total_revenue, total_expenses,
//              carbon_sequestered, water_conservation_score, biodiversity_index, soil_health_trend, climate_change_factor, the
//              legacy Gaussian's cached second value with its flag (NOT reset: it belongs to the stream), this episode's return;
//              irrigation_capacity 1.0, groundwater_level 0.7, water_costs 10.0 and debt_level 0.0 are constants.
// Two streams: R is NumPy's legacy global one (np.random.seed), P is CPython's global `random` (random.seed), drawn from only by
// random.choice when an empty field is planted.
// Whatever a runtime index reaches — a field (actions 0..33), a machine (25..29), a crop — is reached by a compare in an unrolled loop
// or a chain of selects, so that on the device every array stays in registers and nothing is indexed in memory.
// The one libm call is log() in the Gaussian of a price: the host build uses glibc's, the device its own, which may differ in the last
// place.  The number of draws never depends on a price, so such a difference cannot move a stream.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CGE_HD __host__ __device__ __forceinline__
#else
#define CGE_HD inline
#endif
// A value read at a runtime index as a chain of selects is turned back into an indexed load by the compiler, and with it the whole
// record into scratch; on the device every link of such a chain passes through this, which the compiler cannot see through.
#if defined(__HIP_DEVICE_COMPILE__)
#define CGE_FARM_OPAQUE(x) asm volatile("" : "+v"(x))
#else
#define CGE_FARM_OPAQUE(x) ((void)0)
#endif

namespace cge {
namespace farm {

constexpr int NF = 4, NE = 8, NCROP = 5, OBS = 620, LIVE = 134, ACTIONS = 45;
constexpr int WHEAT = 0, SOYBEANS = 4, HARVEST_READY = 5, HARVESTED = 6, DORMANT = 7;

// the record: 32-bit columns [word][env]
constexpr int FIELD_DOUBLES = 11, W_FIELD = 0, W_EQ = W_FIELD + 2 * FIELD_DOUBLES * NF, W_WEATHER = W_EQ + 4 * NE, W_MARKET = W_WEATHER + 10,
              W_REST = W_MARKET + 4 * NCROP, N_REST = 14, W_INT = W_REST + 2 * N_REST, N_INT = 30, REC_WORDS = W_INT + N_INT;
static_assert(REC_WORDS == 208, "documented as 832 bytes per env");

// a value by crop / by season as a chain of selects
template <class T>
CGE_HD T by_crop(int c, T wheat, T corn, T tomatoes, T apples, T soybeans) { return c == 0 ? wheat : c == 1 ? corn : c == 2 ? tomatoes : c == 3 ? apples : soybeans; }
template <class T>
CGE_HD T by_season(uint32_t s, T spring, T summer, T fall, T winter) { return s == 0u ? spring : s == 1u ? summer : s == 2u ? fall : winter; }

// crop_data.py:57-167
CGE_HD int cycle_days(int c) { return by_crop(c, 90, 120, 60, 365, 100); }
CGE_HD double base_price(int c) { return by_crop(c, 250.0, 200.0, 800.0, 600.0, 400.0); }
CGE_HD double yield_per_hectare(int c) { return by_crop(c, 3.5, 10.0, 80.0, 40.0, 3.0); }
CGE_HD double carbon_of(int c) { return by_crop(c, 0.8, 1.2, 0.5, 2.5, 1.0); }
CGE_HD double need_n(int c) { return by_crop(c, 120.0, 180.0, 100.0, 80.0, 40.0); }
CGE_HD double need_p(int c) { return by_crop(c, 60.0, 80.0, 120.0, 40.0, 60.0); }
CGE_HD double need_k(int c) { return by_crop(c, 40.0, 90.0, 140.0, 100.0, 80.0); }
// get_crop_stage_duration :170-223: int(growth_cycle_days * percentage), one byte per stage 0..7 (0.1 where a stage is not listed);
// tests/test_farm_cpu.py pins all forty against Python
CGE_HD int stage_days(int c, int stage) {
    const uint64_t d = by_crop<uint64_t>(c, 0x09090412161f0904ull, 0x0c0c06151e300904ull, 0x0606030912130703ull, 0x33241d4936920703ull, 0x0a0a050f1e230a05ull);
    return (int)((d >> (8 * stage)) & 255u);
}
// get_market_price_multiplier :285-320
CGE_HD double season_mult(uint32_t s, int c) {
    return by_season(s, by_crop(c, 1.0, 0.9, 1.2, 1.1, 1.0), by_crop(c, 1.1, 1.0, 0.8, 0.9, 1.0), by_crop(c, 0.9, 1.2, 1.3, 1.2, 1.1), by_crop(c, 1.2, 1.3, 1.5, 1.0, 1.2));
}

// NumPy's legacy draws on a source of tempered MT19937 words: R::next()
CGE_HD double random53(uint32_t w0, uint32_t w1) { return ((double)(w0 >> 5) * 67108864.0 + (double)(w1 >> 6)) / 9007199254740992.0; }
template <class R>
CGE_HD double random01(R &r) {
    const uint32_t a = r.next(), b = r.next();
    return random53(a, b);
}
// RandomState.uniform(lo, hi) = lo + (hi - lo) * random_sample(), the range rounded on its own
template <class R>
CGE_HD double uniform(R &r, double lo, double hi) {
    const double range = hi - lo;
    return lo + range * random01(r);
}
// RandomState.randint(0, 25): one 32-bit word per attempt, masked to 31, rejected above 24
template <class R>
CGE_HD uint32_t randint25(R &r) {
    uint32_t v = r.next() & 31u;
    while (v > 24u) v = r.next() & 31u;
    return v;
}
// CPython's Random._randbelow_with_getrandbits(n) with k = n.bit_length(): the top k bits of a word, rejected at n and above
template <class P>
CGE_HD uint32_t randbelow(P &py, uint32_t n, int kbits) {
    uint32_t v = py.next() >> (32 - kbits);
    while (v >= n) v = py.next() >> (32 - kbits);
    return v;
}
CGE_HD double pymin(double a, double b) { return b < a ? b : a; }              // Python's min(a, b)
CGE_HD double pymax(double a, double b) { return b > a ? b : a; }              // Python's max(a, b)
CGE_HD double clip(double x, double lo, double hi) {                           // np.clip: min(max(x, lo), hi) as `a > b ? a : b`, `a < b ? a : b`
    const double t = x > lo ? x : lo;
    return t < hi ? t : hi;
}
// np.mean of four values: below eight NumPy's pairwise sum is a plain loop
CGE_HD double mean4(double a, double b, double c, double d) { return (((a + b) + c) + d) / 4.0; }

struct Field {
    double health, yp, moisture, ph, n, p, k, compaction, om, pest, disease;
    int32_t crop, stage, last_crop, dth, since, last_fert, last_pest;
};

struct Env {
    Field f[NF];
    double fuel[NE], maint[NE];
    uint32_t locx[NE], locy[NE], operating;                         // operating: bit q
    double temp, hum, rain, wind, frost;
    double price[NCROP], pred[NCROP];
    double reservoir, quality, cash, costs, margin, revenue, expenses, carbon, wcs, bio, trend, climate, gauss, ep_ret;
    uint32_t day, season, year, drought, rain_days, has_gauss, needs_reset;
    uint32_t mt_pos, mt_ready, py_pos, py_ready;

    // the integer columns W_INT .. W_INT + 29, as put(word, value) / get(word)
    template <class F>
    CGE_HD void pack_ints(F put) const {
#pragma unroll
        for (int k = 0; k < NF; ++k) {
            put(4 * k, (uint32_t)(f[k].crop + 1) | (uint32_t)f[k].stage << 4 | (uint32_t)(f[k].last_crop + 1) << 8 | (uint32_t)f[k].dth << 12);
            put(4 * k + 1, (uint32_t)f[k].since); put(4 * k + 2, (uint32_t)f[k].last_fert); put(4 * k + 3, (uint32_t)f[k].last_pest);
        }
        put(16, locx[0] | locx[1] << 8 | locx[2] << 16 | locx[3] << 24); put(17, locx[4] | locx[5] << 8 | locx[6] << 16 | locx[7] << 24);
        put(18, locy[0] | locy[1] << 8 | locy[2] << 16 | locy[3] << 24); put(19, locy[4] | locy[5] << 8 | locy[6] << 16 | locy[7] << 24);
        put(20, day); put(21, season | has_gauss << 2 | needs_reset << 3 | operating << 8 | year << 16);
        put(22, drought); put(23, rain_days);
        put(24, mt_pos); put(25, mt_ready); put(26, py_pos); put(27, py_ready); put(28, 0u); put(29, 0u);
    }
    template <class F>
    CGE_HD void unpack_ints(F get) {
#pragma unroll
        for (int k = 0; k < NF; ++k) {
            const uint32_t w = get(4 * k);
            f[k].crop = (int32_t)(w & 15u) - 1; f[k].stage = (int32_t)((w >> 4) & 15u); f[k].last_crop = (int32_t)((w >> 8) & 15u) - 1; f[k].dth = (int32_t)(w >> 12);
            f[k].since = (int32_t)get(4 * k + 1); f[k].last_fert = (int32_t)get(4 * k + 2); f[k].last_pest = (int32_t)get(4 * k + 3);
        }
        const uint32_t x0 = get(16), x1 = get(17), y0 = get(18), y1 = get(19);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            locx[q] = (x0 >> (8 * q)) & 255u; locx[4 + q] = (x1 >> (8 * q)) & 255u;
            locy[q] = (y0 >> (8 * q)) & 255u; locy[4 + q] = (y1 >> (8 * q)) & 255u;
        }
        day = get(20);
        const uint32_t g = get(21);
        season = g & 3u; has_gauss = (g >> 2) & 1u; needs_reset = (g >> 3) & 1u; operating = (g >> 8) & 255u; year = g >> 16;
        drought = get(22); rain_days = get(23);
        mt_pos = get(24); mt_ready = get(25); py_pos = get(26); py_ready = get(27);
    }
    // every float64 of the record in its column order: f(word offset, value)
    template <class E, class F>
    static CGE_HD void each_double(E &e, F f) {
#pragma unroll
        for (int k = 0; k < NF; ++k) {
            const int w = W_FIELD + 2 * FIELD_DOUBLES * k;
            f(w, e.f[k].health); f(w + 2, e.f[k].yp); f(w + 4, e.f[k].moisture); f(w + 6, e.f[k].ph); f(w + 8, e.f[k].n); f(w + 10, e.f[k].p);
            f(w + 12, e.f[k].k); f(w + 14, e.f[k].compaction); f(w + 16, e.f[k].om); f(w + 18, e.f[k].pest); f(w + 20, e.f[k].disease);
        }
#pragma unroll
        for (int q = 0; q < NE; ++q) { f(W_EQ + 2 * q, e.fuel[q]); f(W_EQ + 2 * (NE + q), e.maint[q]); }
        f(W_WEATHER, e.temp); f(W_WEATHER + 2, e.hum); f(W_WEATHER + 4, e.rain); f(W_WEATHER + 6, e.wind); f(W_WEATHER + 8, e.frost);
#pragma unroll
        for (int c = 0; c < NCROP; ++c) { f(W_MARKET + 2 * c, e.price[c]); f(W_MARKET + 2 * (NCROP + c), e.pred[c]); }
        f(W_REST, e.reservoir); f(W_REST + 2, e.quality); f(W_REST + 4, e.cash); f(W_REST + 6, e.costs); f(W_REST + 8, e.margin); f(W_REST + 10, e.revenue);
        f(W_REST + 12, e.expenses); f(W_REST + 14, e.carbon); f(W_REST + 16, e.wcs); f(W_REST + 18, e.bio); f(W_REST + 20, e.trend); f(W_REST + 22, e.climate);
        f(W_REST + 24, e.gauss); f(W_REST + 26, e.ep_ret);
    }
};

// legacy_gauss (polar method): the first call returns f * x2 and caches f * x1 for the second
template <class R>
CGE_HD double gauss(Env &e, R &r) {
    if (e.has_gauss) {
        const double g = e.gauss;
        e.has_gauss = 0; e.gauss = 0.0;
        return g;
    }
    double x1, x2, r2;
    do {
        x1 = 2.0 * random01(r) - 1.0;
        x2 = 2.0 * random01(r) - 1.0;
        r2 = x1 * x1 + x2 * x2;
    } while (r2 >= 1.0 || r2 == 0.0);
    const double f = sqrt(-2.0 * log(r2) / r2);
    e.gauss = f * x1; e.has_gauss = 1;
    return f * x2;
}

// what __init__ and reset() both do (:136-176, :524-561): the fields, the equipment and the market drawn in this order, everything
// else at its default.  water_quality and the Gaussian's cache are not touched.
template <class R>
CGE_HD void reset_episode(Env &e, R &r) {
    e.day = 0; e.season = 0; e.year = 1;
#pragma unroll
    for (int k = 0; k < NF; ++k) {
        Field &f = e.f[k];
        f.crop = k < 3 ? k : -1; f.stage = DORMANT; f.health = 1.0; f.yp = 1.0; f.dth = 0; f.since = 0; f.last_crop = -1;
        f.pest = 0.0; f.disease = 0.0; f.last_fert = -100; f.last_pest = -100;
        f.moisture = uniform(r, 0.3, 0.7);
        f.ph = uniform(r, 6.0, 7.0);
        f.n = uniform(r, 80.0, 120.0);
        f.p = uniform(r, 40.0, 60.0);
        f.k = uniform(r, 40.0, 60.0);
        f.compaction = uniform(r, 0.2, 0.4);
        f.om = uniform(r, 0.03, 0.05);
    }
#pragma unroll
    for (int q = 0; q < NE; ++q) {
        e.locx[q] = randint25(r); e.locy[q] = randint25(r);
        e.fuel[q] = uniform(r, 0.7, 1.0);
        e.maint[q] = uniform(r, 0.0, 0.2);
    }
    e.operating = 0;
    e.temp = 20.0; e.hum = 0.5; e.rain = 0.0; e.wind = 10.0; e.frost = 0.0; e.drought = 0; e.rain_days = 0;
    e.climate = 0.0;
#pragma unroll
    for (int c = 0; c < NCROP; ++c) {
        e.price[c] = base_price(c) * uniform(r, 0.9, 1.1);
        e.pred[c] = base_price(c) * uniform(r, 0.85, 1.15);
    }
    e.reservoir = 0.8;
    e.cash = 50000.0; e.costs = 0.0; e.margin = 0.0; e.revenue = 0.0; e.expenses = 0.0;
    e.carbon = 0.0; e.wcs = 0.0; e.bio = 0.5; e.trend = 0.0;
    e.needs_reset = 0;
    e.ep_ret = 0.0;
}

// random.seed(s); np.random.seed(s); AgriculturalFarmEnv(): sets what reset() will not touch and draws what reset() draws again
template <class R>
CGE_HD void construct(Env &e, R &r) {
    e.quality = 0.9; e.has_gauss = 0; e.gauss = 0.0;
    reset_episode(e, r);
}

// calculate_yield_modifier, crop_data.py:226-282
CGE_HD double yield_modifier(int c, const Field &f, double temperature) {
    double m = 1.0;
    const double tlo = by_crop(c, 10.0, 18.0, 18.0, 4.0, 20.0), thi = by_crop(c, 25.0, 32.0, 29.0, 24.0, 30.0);
    if (tlo <= temperature && temperature <= thi) m *= 1.0;
    else if (temperature < tlo) m *= pymax(0.3, 1.0 - (tlo - temperature) * 0.05);
    else m *= pymax(0.3, 1.0 - (temperature - thi) * 0.05);
    const double plo = by_crop(c, 6.0, 5.8, 6.0, 6.0, 6.0), phi = by_crop(c, 7.5, 7.0, 6.8, 7.0, 7.0);
    if (!(plo <= f.ph && f.ph <= phi)) m *= pymax(0.5, 1.0 - pymin(fabs(f.ph - plo), fabs(f.ph - phi)) * 0.15);
    if (!(0.4 <= f.moisture && f.moisture <= 0.8)) m *= pymax(0.4, 1.0 - fabs(f.moisture - 0.6));
    const double have[3] = {f.n, f.p, f.k}, need[3] = {need_n(c), need_p(c), need_k(c)};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double ratio = have[j] / need[j];
        if (0.8 <= ratio && ratio <= 1.2) m *= 1.0;
        else if (ratio < 0.8) m *= pymax(0.5, ratio);
        else m *= pymax(0.7, 2.0 - ratio);
    }
    m *= (1.0 - f.pest * 0.5);
    m *= (1.0 - f.disease * 0.5);
    return pymax(0.1, pymin(1.5, m));
}

// market.current_prices[crop]
CGE_HD double price_of(const Env &e, uint32_t crop) {
    double price = e.price[0];
#pragma unroll
    for (int j = 1; j < NCROP; ++j) {
        price = crop == (uint32_t)j ? e.price[j] : price;
        CGE_FARM_OPAQUE(price);
    }
    return price;
}

// _harvest_crop :802-845 of a field of `size` cells; returns the reward
CGE_HD double harvest(Env &e, Field &f, double size) {
    if (f.crop < 0) return 0.0;
    const int c = f.crop;
    const double base = yield_per_hectare(c) * (size / 625.0);
    const double actual = base * f.yp * f.health;
    const double price = price_of(e, (uint32_t)c);
    const double revenue = actual * price;
    e.cash += revenue;
    e.revenue += revenue;
    const double ratio = actual / base;
    double reward = ratio > 1.2 ? 5000.0 : ratio > 0.9 ? 2000.0 : ratio > 0.7 ? 1000.0 : -1000.0;
    const double avg = base_price(c);
    if (price > avg * 1.2) reward += 800.0;
    else if (price < avg * 0.8) reward -= 400.0;
    f.last_crop = c; f.crop = -1; f.stage = DORMANT; f.since = 0; f.health = 1.0; f.yp = 1.0;
    return reward;
}
CGE_HD double field_size(int k) { return k == 3 ? 157.0 : 156.0; }

// _process_action :629-800 for an action in 0..44; returns the reward
template <class P>
CGE_HD double process_action(Env &e, P &py, uint32_t a) {
    double reward = 0.0;
    const int32_t day = (int32_t)e.day;
    if (a <= 4u) {
#pragma unroll
        for (int k = 0; k < NF; ++k) {
            Field &f = e.f[k];
            if (a == (uint32_t)k && (f.crop < 0 || f.stage == HARVESTED) && e.season != 3u) {
                int crop;                                            // random.choice(suitable_crops)
                if (e.season == 0u) crop = (int)randbelow(py, 5u, 3);
                else if (e.season == 1u) { const uint32_t j = randbelow(py, 3u, 2); crop = j == 0u ? 1 : j == 1u ? 2 : 4; }
                else { randbelow(py, 1u, 1); crop = WHEAT; }
                f.crop = crop; f.stage = 0; f.since = 0; f.health = 1.0; f.yp = 1.0;
                e.cash -= 500.0;
                reward += 50.0;
                if (f.last_crop > 0 && f.last_crop != crop) reward += 100.0;   // `if field.last_crop`: wheat is false
            }
        }
    } else if (a <= 9u) {
#pragma unroll
        for (int k = 0; k < NF; ++k) {
            if (a - 5u == (uint32_t)k && e.f[k].stage == HARVEST_READY) reward += harvest(e, e.f[k], field_size(k));
        }
    } else if (a <= 14u) {
#pragma unroll
        for (int k = 0; k < NF; ++k) {
            Field &f = e.f[k];
            if (a - 10u == (uint32_t)k && day - f.last_fert > 14) {
                f.n += 30.0; f.p += 20.0; f.k += 20.0;
                f.last_fert = day;
                e.cash -= 300.0;
                reward += 20.0;
                if (f.n > 150.0) { reward -= 100.0; e.quality -= 0.02; }
            }
        }
    } else if (a <= 19u) {
#pragma unroll
        for (int k = 0; k < NF; ++k) {
            Field &f = e.f[k];
            if (a - 15u == (uint32_t)k && e.reservoir > 0.1) {
                const double amount = pymin(0.05, e.reservoir);
                f.moisture += amount * 2.0;
                f.moisture = pymin(1.0, f.moisture);
                e.reservoir -= amount;
                e.cash -= 10.0 * amount * 100.0;
                if (f.moisture < 0.3) reward += 50.0;
            }
        }
    } else if (a <= 24u) {
#pragma unroll
        for (int k = 0; k < NF; ++k) {
            Field &f = e.f[k];
            if (a - 20u == (uint32_t)k && day - f.last_pest > 21) {
                f.pest = pymax(0.0, f.pest - 0.5);
                f.disease = pymax(0.0, f.disease - 0.3);
                f.last_pest = day;
                e.cash -= 400.0;
                e.bio -= 0.02;
                e.quality -= 0.01;
                reward -= 50.0;
                if (f.pest > 0.5) reward += 200.0;
            }
        }
    } else if (a <= 29u) {
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            if (a - 25u == (uint32_t)q) {
                if (e.fuel[q] > 0.1 && e.maint[q] < 0.8) {
                    e.operating |= 1u << q;
                    e.fuel[q] -= 0.1;
                    e.maint[q] += 0.02;
                    reward += 10.0;
                } else {
                    reward -= 20.0;
                }
            }
        }
    } else if (a <= 34u) {
#pragma unroll
        for (int k = 0; k < NF; ++k) {
            if (a - 30u == (uint32_t)k) {
                reward += 15.0;
                e.cash -= 100.0;
                e.f[k].compaction = pymax(0.0, e.f[k].compaction - 0.1);
            }
        }
    } else if (a <= 39u) {
        if (e.cash < 10000.0) {
            const double revenue = price_of(e, a - 35u) * 10.0;
            e.cash += revenue;
            e.revenue += revenue;
            reward += 100.0;
        }
    } else if (a == 40u) {
#pragma unroll
        for (int k = 0; k < NF; ++k) {
            if (e.frost > 0.5 || e.rain_days > 3u) {
                e.f[k].health = pymax(e.f[k].health - 0.05, 0.5);
                reward += 50.0;
            }
        }
        e.cash -= 1000.0;
    } else if (a == 41u) {
        e.bio += 0.01;
        e.trend += 0.02;
        e.carbon += 1.0;
        reward += 500.0;
    } else if (a == 42u) {
#pragma unroll
        for (int k = 0; k < NF; ++k) {
            if (e.f[k].crop > 0) { e.f[k].yp *= 1.1; e.f[k].om -= 0.001; }
        }
        reward += 100.0;
    } else if (a == 43u) {
        uint32_t kinds = 0;
#pragma unroll
        for (int k = 0; k < NF; ++k) kinds |= e.f[k].crop > 0 ? 1u << e.f[k].crop : 0u;
        if (__builtin_popcount(kinds) >= 3) reward += 200.0;
    } else {
#pragma unroll
        for (int q = 0; q < NE; ++q) {
            if (e.maint[q] > 0.5) {
                e.maint[q] = 0.0;
                e.fuel[q] = 1.0;
                e.cash -= 500.0;
                reward += 30.0;
            }
        }
    }
    return reward;
}

// step() :568-627 up to the observation; `valid` false is an action outside 0..44: it falls through every branch of _process_action.
// Returns the reward.
template <class R, class P>
CGE_HD double env_step(Env &e, R &r, P &py, int32_t action, bool valid, uint32_t max_years, bool &terminated) {
    double reward = 0.0;
    if (valid) reward += process_action(e, py, (uint32_t)action);
    {                                                                // :276-316
        const uint32_t s = e.season;
        const double shift = e.climate * 2.0;
        const double t = uniform(r, by_season(s, 10.0, 20.0, 8.0, -5.0) + shift, by_season(s, 22.0, 35.0, 20.0, 10.0) + shift);
        e.temp = 0.7 * e.temp + (1.0 - 0.7) * t;
        const double h = uniform(r, by_season(s, 0.4, 0.3, 0.5, 0.6), by_season(s, 0.7, 0.6, 0.8, 0.9));
        e.hum = 0.7 * e.hum + (1.0 - 0.7) * h;
        if (random01(r) < 0.3) e.rain = uniform(r, 0.0, by_season(s, 15.0, 10.0, 20.0, 25.0));
        else e.rain = 0.0;
        e.wind = uniform(r, by_season(s, 5.0, 3.0, 8.0, 10.0), by_season(s, 20.0, 15.0, 25.0, 30.0));
        if (e.temp < 5.0) e.frost = uniform(r, by_season(s, 0.0, 0.0, 0.0, 0.2), by_season(s, 0.2, 0.0, 0.3, 0.7));
        else e.frost = 0.0;
        if (e.rain < 2.0) { e.drought += 1; e.rain_days = 0; }
        else if (e.rain > 15.0) { e.rain_days += 1; e.drought = 0; }
        else { e.drought = e.drought > 0u ? e.drought - 1u : 0u; e.rain_days = e.rain_days > 0u ? e.rain_days - 1u : 0u; }
    }
#pragma unroll
    for (int k = 0; k < NF; ++k) {                                   // :318-356
        Field &f = e.f[k];
        if (f.crop >= 0 && f.stage != HARVESTED) {
            f.since += 1;
            if (f.since % stage_days(f.crop, f.stage) == 0 && f.stage < HARVEST_READY) f.stage += 1;
            const int left = cycle_days(f.crop) - f.since;
            f.dth = left > 0 ? left : 0;
            f.yp = yield_modifier(f.crop, f, e.temp);
            f.health = pymax(0.0, pymin(1.0, f.health - 0.01 * (f.pest + f.disease)));
            if (random01(r) < 0.05) f.pest = pymin(1.0, f.pest + uniform(r, 0.01, 0.05));
            if (e.hum > 0.7 && e.temp > 15.0) f.disease = pymin(1.0, f.disease + 0.02);
        }
    }
#pragma unroll
    for (int k = 0; k < NF; ++k) {                                   // :358-388; operation_field is never set: nothing compacts
        Field &f = e.f[k];
        f.moisture += e.rain * 0.01;
        f.moisture -= (e.temp / 100.0) * (1.0 - e.hum);
        f.moisture = clip(f.moisture, 0.0, 1.0);
        if (f.crop >= 0) {
            f.n -= need_n(f.crop) * 0.001;
            f.p -= need_p(f.crop) * 0.001;
            f.k -= need_k(f.crop) * 0.001;
            if (f.crop == SOYBEANS) f.n += 0.5;
        }
        f.compaction = pymax(0.0, f.compaction - 0.001);
        if (f.last_crop >= 0) f.om += 0.0001;
        f.om = clip(f.om, 0.01, 0.1);
    }
#pragma unroll
    for (int c = 0; c < NCROP; ++c) {                                // :390-411
        const double base = base_price(c);
        const double change = 0.0 + (0.1 * base) * gauss(e, r);      // normal(loc, scale) = loc + scale * gauss
        double fresh = e.price[c] + change;
        fresh = 0.9 * fresh + 0.1 * (base * season_mult(e.season, c));
        e.price[c] = pymax(base * 0.5, pymin(base * 2.0, fresh));
        e.pred[c] = fresh * uniform(r, 0.9, 1.1);
    }
    e.reservoir += e.rain * 0.001;                                   // :581-589
    e.reservoir -= 0.01;
    e.reservoir = clip(e.reservoir, 0.0, 1.0);
    {                                                                // :413-433
        double costs = 0.0;
#pragma unroll
        for (int q = 0; q < NE; ++q) {
            if ((e.operating >> q) & 1u) costs += 50.0;
        }
        costs += 200.0;
        costs += 10.0 * (1.0 - e.reservoir) * 10.0;
#pragma unroll
        for (int q = 0; q < NE; ++q) {
            if (e.maint[q] > 0.5) costs += 100.0;
        }
        e.costs = costs;
        e.expenses += costs;
        e.cash -= costs;
    }
#pragma unroll
    for (int k = 0; k < NF; ++k) {                                   // :591-596
        if (e.f[k].stage == HARVEST_READY && e.f[k].dth <= 0) reward += harvest(e, e.f[k], field_size(k));
    }
    {                                                                // :847-883
        const double avg_om = mean4(e.f[0].om, e.f[1].om, e.f[2].om, e.f[3].om);
        if (avg_om > 0.045) reward += 500.0;
        else if (avg_om < 0.02) reward -= 2000.0;
        if (e.reservoir > 0.5 && e.drought > 10u) reward += 300.0;
        if (e.bio > 0.7) reward += 200.0;
        else if (e.bio < 0.3) reward -= 300.0;
#pragma unroll
        for (int k = 0; k < NF; ++k) {
            Field &f = e.f[k];
            if (f.crop > 0) {
                if (e.frost > 0.5 && (f.stage == 1 || f.stage == 3)) { f.health -= 0.2; reward -= 300.0; }
                if (e.drought > 20u && f.moisture < 0.2) { f.health -= 0.15; reward -= 300.0; }
                if (e.rain_days > 5u) { f.disease += 0.1; reward -= 200.0; }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NF; ++k) {                                   // :885-909
        if (e.f[k].crop > 0) e.carbon += carbon_of(e.f[k].crop) * 0.01;
    }
    if (1.0 - e.reservoir < 0.3) e.wcs = pymin(1.0, e.wcs + 0.01);
    else e.wcs = pymax(0.0, e.wcs - 0.01);
    e.trend = (mean4(e.f[0].om, e.f[1].om, e.f[2].om, e.f[3].om) * 10.0 - mean4(e.f[0].compaction, e.f[1].compaction, e.f[2].compaction, e.f[3].compaction)) / 2.0;
    e.margin = e.revenue > 0.0 ? (e.revenue - e.expenses) / e.revenue : -1.0;
    e.day += 1;                                                      // :604-621
    if (e.day % 90u == 0u) {
        e.season = (e.season + 1u) & 3u;
        if (e.season == 0u) { e.year += 1; e.climate += 0.05; }
    }
    terminated = false;
    if (e.year > max_years) {
        terminated = true;
    } else if (e.cash < -50000.0) {
        terminated = true;
        reward -= 5000.0;
    } else if (e.f[0].om < 0.01 && e.f[1].om < 0.01 && e.f[2].om < 0.01 && e.f[3].om < 0.01) {   // unreachable: the clip above
        terminated = true;
        reward -= 3000.0;
    }
    e.ep_ret += reward;
    return reward;
}

// _get_observation :435-518, out(k, value) with k the element's index in the row: fields [0, 60), weather [60, 70), equipment [70, 110),
// market [110, 120), water [120, 125), finances [125, 130), sustainability [130, 134).  Elements 134..619 are zero.
template <class F>
CGE_HD void observe(const Env &e, F &out) {
#pragma unroll
    for (int k = 0; k < NF; ++k) {
        const Field &f = e.f[k];
        const int o = 15 * k;
        out(o, (float)(f.crop > 0 ? f.crop : -1)); out(o + 1, (float)f.stage); out(o + 2, (float)f.health); out(o + 3, (float)f.yp); out(o + 4, (float)f.dth);
        out(o + 5, (float)f.moisture); out(o + 6, (float)f.ph); out(o + 7, (float)(f.n / 200.0)); out(o + 8, (float)(f.p / 100.0)); out(o + 9, (float)(f.k / 100.0));
        out(o + 10, (float)f.compaction); out(o + 11, (float)(f.om * 10.0)); out(o + 12, (float)f.pest); out(o + 13, (float)f.disease);
        out(o + 14, (float)((double)f.since / 365.0));
    }
    out(60, (float)(e.temp / 40.0)); out(61, (float)e.hum); out(62, (float)(e.rain / 30.0)); out(63, (float)(e.wind / 40.0)); out(64, 0.5f);
    out(65, (float)e.frost); out(66, (float)((double)e.drought / 30.0)); out(67, (float)((double)e.rain_days / 10.0)); out(68, (float)((double)e.season / 3.0));
    out(69, (float)((double)e.day / 365.0));
#pragma unroll
    for (int q = 0; q < NE; ++q) {
        out(70 + 5 * q, (float)((double)e.locx[q] / 25.0)); out(71 + 5 * q, (float)((double)e.locy[q] / 25.0)); out(72 + 5 * q, (float)e.fuel[q]);
        out(73 + 5 * q, (float)e.maint[q]); out(74 + 5 * q, (e.operating >> q) & 1u ? 1.0f : 0.0f);
    }
#pragma unroll
    for (int c = 0; c < NCROP; ++c) { out(110 + 2 * c, (float)(e.price[c] / 1000.0)); out(111 + 2 * c, (float)(e.pred[c] / 1000.0)); }
    out(120, (float)e.reservoir); out(121, 1.0f); out(122, (float)e.quality); out(123, (float)0.7); out(124, (float)(10.0 / 50.0));
    out(125, (float)(e.cash / 100000.0)); out(126, (float)(e.costs / 1000.0)); out(127, 0.0f); out(128, (float)e.margin);
    out(129, (float)((e.revenue - e.expenses) / 100000.0));
    out(130, (float)(e.carbon / 100.0)); out(131, (float)e.wcs); out(132, (float)e.bio); out(133, (float)e.trend);
}

// _get_info :911-935: the eleven scalar values in the reference's order (season as 0..3), field_status as crop (-1 for "None", which a
// wheat field prints too), stage, health and yield_potential of the four fields, then what else the record knows
enum { INFO_DAY = 0, INFO_SEASON, INFO_YEAR, INFO_CASH_FLOW, INFO_TOTAL_REVENUE, INFO_TOTAL_EXPENSES, INFO_PROFIT_MARGIN, INFO_CARBON_SEQUESTERED,
       INFO_WATER_CONSERVATION_SCORE, INFO_BIODIVERSITY_INDEX, INFO_SOIL_HEALTH_TREND, INFO_FIELD_CROP, INFO_FIELD_STAGE = INFO_FIELD_CROP + NF,
       INFO_FIELD_HEALTH = INFO_FIELD_STAGE + NF, INFO_FIELD_YIELD_POTENTIAL = INFO_FIELD_HEALTH + NF, INFO_NEEDS_RESET = INFO_FIELD_YIELD_POTENTIAL + NF,
       INFO_WATER_QUALITY, INFO_COUNT };
CGE_HD double info_value(const Env &e, int field) {
    if (field >= INFO_FIELD_CROP && field < INFO_NEEDS_RESET) {
        const int what = (field - INFO_FIELD_CROP) / NF, k = (field - INFO_FIELD_CROP) % NF;
        double v = 0.0;
#pragma unroll
        for (int j = 0; j < NF; ++j) {
            const Field &f = e.f[j];
            const double x = what == 0 ? (double)(f.crop > 0 ? f.crop : -1) : what == 1 ? (double)f.stage : what == 2 ? f.health : f.yp;
            v = j == k ? x : v;
        }
        return v;
    }
    switch (field) {
        case INFO_DAY: return (double)e.day;
        case INFO_SEASON: return (double)e.season;
        case INFO_YEAR: return (double)e.year;
        case INFO_CASH_FLOW: return e.cash;
        case INFO_TOTAL_REVENUE: return e.revenue;
        case INFO_TOTAL_EXPENSES: return e.expenses;
        case INFO_PROFIT_MARGIN: return e.margin;
        case INFO_CARBON_SEQUESTERED: return e.carbon;
        case INFO_WATER_CONSERVATION_SCORE: return e.wcs;
        case INFO_BIODIVERSITY_INDEX: return e.bio;
        case INFO_SOIL_HEALTH_TREND: return e.trend;
        case INFO_NEEDS_RESET: return (double)e.needs_reset;
        case INFO_WATER_QUALITY: return e.quality;
    }
    return 0.0;
}


// Canonical records (cge_records_farm_*, lane_records.hip): what a record's body must satisfy before it may become an env.  get(w) is
// word w of the body.  No field of a farm record reaches an address (crops, stages and seasons select among constants), but
//   stage (field word 0, 4 bits)                picks a byte of stage_days' 64-bit table, the divisor of `since % stage_days`: 0..7
//   crop, last_crop (field word 0, 4 bits each, stored + 1)   -1..4, the five crops and "none"
// has_gauss is one bit of integer word 21 and cannot be anything but 0 or 1.  No kernel calls this.
enum { RECORD_OK = 0, RECORD_STAGE = 16, RECORD_CROP = 17 };
template <class G>
CGE_HD int record_refusal(G get) {
    for (int k = 0; k < NF; ++k) {
        const uint32_t w = get(W_INT + 4 * k);
        if (((w >> 4) & 15u) > (uint32_t)DORMANT) return RECORD_STAGE;
        if ((w & 15u) > (uint32_t)NCROP || ((w >> 8) & 15u) > (uint32_t)NCROP) return RECORD_CROP;
    }
    return RECORD_OK;
}
inline const char *record_refusal_text(int code) {
    return code == RECORD_STAGE ? "a field's growth stage is above 7" : code == RECORD_CROP ? "a field's crop or last crop is not one of the five" : "bad record";
}
constexpr int RECORD_CURSOR_FIRST = W_INT + 24, RECORD_CURSOR_WORDS = 4;   // mt_pos, mt_ready, py_pos, py_ready

}  // namespace farm
}  // namespace cge
