// Replays a farm fixture through csrc/farm_env.hpp on the CPU (the code the kernels run, compiled for the host) and compares every
// step with what the reference recorded, bit for bit.  Driven by tools/probes/farm_host_check.py, which writes the input file:
//   int32 n, T, autoreset, nresets, max_years, npokes; float reset_obs[nresets][134]; npokes x {int32 env, int32 step, char name[24],
//   double value}: the named field of that env is set before that step; then per env: int32 seed, int32 actions[T],
//   int32 reset_at[T] (row of reset_obs or -1), float obs0[134], double info0[27], float obs[T][134], double reward[T],
//   uint8 terminated[T], double info[T][27].
// `--layout`: prints `name word-offset f64|u32` for every field a poke can name, the offsets found through the record's own packer.
// `--mean`: reads float64 vectors of 4 from stdin and writes mean4() of each to stdout (the order of NumPy's np.mean).
// `--stage-days`: writes the 5 x 8 int32 entries of stage_days() to stdout.
// `--randint S N`: writes N uint32 draws of randint25() after np.random.seed(S).  `--randbelow S n k N`: writes N uint32 draws of
// randbelow(n, k) after random.seed(S).
// `--record S0 N K`: reads int32 actions [K][N] from stdin, runs env i = 0 .. N - 1 seeded S0 + i through reset and K steps with an
// autoreset in the same step, and writes the 89 float64 of each record in column order (tools/probes/farm_timing.py compares them with
// the device's).
// The generators are MT19937 seeded as NumPy's legacy np.random.seed(int) (init_genrand) and as CPython's random.seed(int)
// (init_by_array over the 32-bit limbs) do.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../custom_gymnasium_environments_amd/csrc/farm_env.hpp"

using namespace cge::farm;

constexpr int NINFO = 27;

struct Mt {
    uint32_t mt[624];
    int idx = 624;
    void seed(uint32_t s) {                                          // init_genrand
        mt[0] = s;
        for (int i = 1; i < 624; ++i) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
        idx = 624;
    }
    void seed_python(uint64_t s) {                                   // init_by_array
        uint32_t key[2] = {(uint32_t)s, (uint32_t)(s >> 32)};
        const int len = key[1] ? 2 : 1;
        seed(19650218u);
        int i = 1, j = 0;
        for (int k = 624 > len ? 624 : len; k; --k) {
            mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1664525u)) + key[j] + (uint32_t)j;
            if (++i >= 624) { mt[0] = mt[623]; i = 1; }
            if (++j >= len) j = 0;
        }
        for (int k = 623; k; --k) {
            mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1566083941u)) - (uint32_t)i;
            if (++i >= 624) { mt[0] = mt[623]; i = 1; }
        }
        mt[0] = 0x80000000u;
        idx = 624;
    }
    uint32_t next() {
        if (idx >= 624) {
            for (int k = 0; k < 624; ++k) {
                const uint32_t y = (mt[k] & 0x80000000u) | (mt[(k + 1) % 624] & 0x7fffffffu);
                mt[k] = mt[(k + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
            }
            idx = 0;
        }
        uint32_t y = mt[idx++];
        y ^= y >> 11; y ^= (y << 7) & 0x9d2c5680u; y ^= (y << 15) & 0xefc60000u; y ^= y >> 18;
        return y;
    }
};

static void observe_row(const Env &e, float *o) {
    auto out = [&](int k, float v) { if (k < 0 || k >= LIVE) { printf("element %d\n", k); exit(3); } o[k] = v; };
    observe(e, out);
}

// through the packed record, as every launch does
static void repack(Env &e) {
    uint32_t w[REC_WORDS] = {};
    Env::each_double(e, [&](int k, const double &v) { memcpy(&w[k], &v, 8); });
    e.pack_ints([&](int k, uint32_t v) { w[W_INT + k] = v; });
    Env f{};
    Env::each_double(f, [&](int k, double &v) { memcpy(&v, &w[k], 8); });
    f.unpack_ints([&](int k) { return w[W_INT + k]; });
    e = f;
}

// every field a poke can name, as the header names it: f(name, the double or nullptr, the whole-word integer or nullptr)
template <class F>
static void each_named(Env &e, F f) {
    static const char *FD[] = {"health", "yp", "moisture", "ph", "n", "p", "k", "compaction", "om", "pest", "disease"};
    char name[24];
    for (int k = 0; k < NF; ++k) {
        double *d[] = {&e.f[k].health, &e.f[k].yp, &e.f[k].moisture, &e.f[k].ph, &e.f[k].n, &e.f[k].p, &e.f[k].k, &e.f[k].compaction, &e.f[k].om, &e.f[k].pest, &e.f[k].disease};
        for (int j = 0; j < FIELD_DOUBLES; ++j) { snprintf(name, sizeof name, "f%d.%s", k, FD[j]); f(name, d[j], (uint32_t *)nullptr); }
    }
    for (int q = 0; q < NE; ++q) {
        snprintf(name, sizeof name, "fuel%d", q); f(name, &e.fuel[q], (uint32_t *)nullptr);
        snprintf(name, sizeof name, "maint%d", q); f(name, &e.maint[q], (uint32_t *)nullptr);
    }
    const char *WD[] = {"temp", "hum", "rain", "wind", "frost", "reservoir", "quality", "cash", "bio", "trend", "climate"};
    double *wd[] = {&e.temp, &e.hum, &e.rain, &e.wind, &e.frost, &e.reservoir, &e.quality, &e.cash, &e.bio, &e.trend, &e.climate};
    for (int j = 0; j < 11; ++j) f(WD[j], wd[j], (uint32_t *)nullptr);
    f("day", (double *)nullptr, &e.day); f("drought", (double *)nullptr, &e.drought); f("rain_days", (double *)nullptr, &e.rain_days);
}

static bool poke(Env &e, const char *name, double value) {
    bool found = false;
    each_named(e, [&](const char *nm, double *d, uint32_t *u) {
        if (strcmp(nm, name)) return;
        found = true;
        if (d) *d = value; else *u = (uint32_t)value;
    });
    return found;
}

// the word of the record that holds each named field: a double by its address in each_double(), an integer by a marker through pack_ints()
static int layout() {
    Env e{};
    int bad = 0;
    each_named(e, [&](const char *nm, double *d, uint32_t *u) {
        int at = -1;
        if (d) {
            Env::each_double(e, [&](int w, double &v) { if (&v == d) at = w; });
        } else {
            const uint32_t keep = *u;
            *u = 0x5a5a5a5au;
            e.pack_ints([&](int k, uint32_t v) { if (v == 0x5a5a5a5au) at = W_INT + k; });
            *u = keep;
        }
        if (at < 0 || at >= REC_WORDS) { ++bad; return; }
        printf("%s %d %s\n", nm, at, d ? "f64" : "u32");
    });
    return bad ? 1 : 0;
}

struct Poke { int32_t env, step; char name[24]; double value; };
static_assert(sizeof(Poke) == 40, "as farm_host_check.py writes it");

static void info_row(const Env &e, double *gi) {
    for (int k = 0; k < NINFO; ++k) gi[k] = info_value(e, k);
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "--layout")) return layout();
    if (!strcmp(argv[1], "--mean")) {
        double v[4];
        while (fread(v, 8, 4, stdin) == 4) {
            const double mean = mean4(v[0], v[1], v[2], v[3]);
            fwrite(&mean, 8, 1, stdout);
        }
        return 0;
    }
    if (!strcmp(argv[1], "--stage-days")) {
        for (int c = 0; c < NCROP; ++c)
            for (int s = 0; s < 8; ++s) {
                const int32_t d = stage_days(c, s);
                fwrite(&d, 4, 1, stdout);
            }
        return 0;
    }
    if (!strcmp(argv[1], "--randint") && argc > 3) {
        Mt rng;
        rng.seed((uint32_t)atol(argv[2]));
        for (long k = atol(argv[3]); k > 0; --k) {
            const uint32_t v = randint25(rng);
            fwrite(&v, 4, 1, stdout);
        }
        return 0;
    }
    if (!strcmp(argv[1], "--randbelow") && argc > 5) {
        Mt py;
        py.seed_python((uint64_t)atoll(argv[2]));
        for (long k = atol(argv[5]); k > 0; --k) {
            const uint32_t v = randbelow(py, (uint32_t)atol(argv[3]), atoi(argv[4]));
            fwrite(&v, 4, 1, stdout);
        }
        return 0;
    }
    if (!strcmp(argv[1], "--record") && argc > 4) {
        const long s0 = atol(argv[2]), n = atol(argv[3]), K = atol(argv[4]);
        std::vector<int32_t> a((size_t)n * K);
        if (fread(a.data(), 4, a.size(), stdin) != a.size()) return 2;
        for (long i = 0; i < n; ++i) {
            Mt rng, py;
            rng.seed((uint32_t)(s0 + i));
            py.seed_python((uint64_t)(s0 + i));
            Env e{};
            construct(e, rng);
            reset_episode(e, rng);
            for (long t = 0; t < K; ++t) {
                bool term;
                const int32_t act = a[(size_t)t * n + i];
                env_step(e, rng, py, act, act >= 0 && act < ACTIONS, 1u, term);
                if (term) reset_episode(e, rng);
            }
            double rec[W_INT / 2];
            Env::each_double(e, [&](int w, const double &v) { rec[w / 2] = v; });
            fwrite(rec, 8, W_INT / 2, stdout);
        }
        return 0;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[6];
    if (fread(hd, 4, 6, f) != 6) return 2;
    const int n = hd[0], T = hd[1], autoreset = hd[2], nres = hd[3];
    const uint32_t max_years = (uint32_t)hd[4];
    std::vector<float> robs((size_t)nres * LIVE);
    if (fread(robs.data(), 4, robs.size(), f) != robs.size()) return 2;
    std::vector<Poke> pokes((size_t)hd[5]);
    if (fread(pokes.data(), sizeof(Poke), pokes.size(), f) != pokes.size()) return 2;
    long bad = 0;
    for (int i = 0; i < n; ++i) {
        int32_t seed;
        std::vector<int32_t> a(T), at(T);
        std::vector<float> obs0(LIVE), obs((size_t)T * LIVE);
        std::vector<double> r(T), info((size_t)T * NINFO), info0(NINFO);
        std::vector<uint8_t> tm(T);
        if (fread(&seed, 4, 1, f) != 1 || fread(a.data(), 4, T, f) != (size_t)T || fread(at.data(), 4, T, f) != (size_t)T ||
            fread(obs0.data(), 4, LIVE, f) != LIVE || fread(info0.data(), 8, NINFO, f) != NINFO || fread(obs.data(), 4, obs.size(), f) != obs.size() ||
            fread(r.data(), 8, T, f) != (size_t)T || fread(tm.data(), 1, T, f) != (size_t)T || fread(info.data(), 8, info.size(), f) != info.size()) return 2;
        Mt rng, py;
        rng.seed((uint32_t)seed);
        py.seed_python((uint64_t)seed);
        Env e{};
        construct(e, rng);
        reset_episode(e, rng);
        float got[LIVE];
        double gi[NINFO];
        observe_row(e, got);
        info_row(e, gi);
        if ((memcmp(got, obs0.data(), sizeof got) || memcmp(gi, info0.data(), sizeof gi)) && bad++ < 5) printf("env %d: reset observation or info differs\n", i);
        for (int t = 0; t < T; ++t) {
            for (Poke &p : pokes) {
                p.name[sizeof p.name - 1] = 0;
                if (p.env == i && p.step == t && !poke(e, p.name, p.value)) { printf("no field %s\n", p.name); return 2; }
            }
            repack(e);
            bool term;
            const double rew = env_step(e, rng, py, a[t], a[t] >= 0 && a[t] < ACTIONS, max_years, term);
            observe_row(e, got);
            info_row(e, gi);
            const bool ok = !memcmp(&rew, &r[t], 8) && term == (tm[t] != 0) && !memcmp(gi, &info[NINFO * (size_t)t], sizeof gi) && !memcmp(got, &obs[(size_t)LIVE * t], sizeof got);
            if (!ok && bad++ < 5) {
                printf("env %d step %d action %d: reward %.17g / %.17g terminated %d / %d\n", i, t, a[t], rew, r[t], (int)term, (int)tm[t]);
                for (int k = 0; k < NINFO; ++k) if (memcmp(&gi[k], &info[NINFO * (size_t)t + k], 8)) printf("  info %d: %.17g / %.17g\n", k, gi[k], info[NINFO * (size_t)t + k]);
                for (int k = 0; k < LIVE; ++k) if (memcmp(&got[k], &obs[(size_t)LIVE * t + k], 4)) printf("  obs %d: %.9g / %.9g\n", k, got[k], obs[(size_t)LIVE * t + k]);
            }
            if (term && autoreset) {
                reset_episode(e, rng);
                observe_row(e, got);
                if (!(at[t] >= 0 && !memcmp(got, &robs[(size_t)LIVE * at[t]], sizeof got)) && bad++ < 5) printf("env %d step %d: reset observation differs\n", i, t);
            }
        }
    }
    fclose(f);
    printf("%s: %d envs x %d steps, %ld mismatching steps\n", argv[1], n, T, bad);
    return bad ? 1 : 0;
}
