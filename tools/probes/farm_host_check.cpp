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
// The generators are MT19937 seeded as NumPy's legacy np.random.seed(int) and as CPython's random.seed(int) do.  The reader, the replay
// loop, the poke table, --layout, --record and the generator are those of lane_host_check.hpp.
#include "lane_host_check.hpp"

#include "../../custom_gymnasium_environments_amd/csrc/farm_env.hpp"

using namespace cge::farm;
using lane_check::Mt;

struct Sim {
    static constexpr int WIDTH = LIVE, NINFO = 27, EXTRA = 1;         // extra: max_years
    static constexpr bool INFO0 = true, TRUNCATED = false, POKES = true;
    static constexpr int REC_WORDS = cge::farm::REC_WORDS, REC_DOUBLES = W_INT / 2;
    static constexpr int32_t RECORD_EXTRA[EXTRA] = {1};
    Env e{};
    Mt rng, py;
    uint32_t max_years;
    Sim(uint64_t seed, const int32_t *extra) : max_years((uint32_t)extra[0]) {
        rng.seed_numpy((uint32_t)seed);
        py.seed_python(seed);
        construct(e, rng);
        reset_episode(e, rng);
    }
    double step(int32_t a, bool &term, bool &) { return env_step(e, rng, py, a, a >= 0 && a < ACTIONS, max_years, term); }
    void reset() { reset_episode(e, rng); }
    void observe(float *o) const {
        auto out = [&](int k, float v) { o[lane_check::element(k, LIVE)] = v; };
        cge::farm::observe(e, out);
    }
    void info(double *gi) const {
        for (int k = 0; k < NINFO; ++k) gi[k] = info_value(e, k);
    }
    void repack() {                                                  // through the packed record, as every launch does
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
    // the word of the record that holds a named integer: by a marker through pack_ints()
    static int int_word(Env &e, uint32_t *u) {
        int at = -1;
        const uint32_t keep = *u;
        *u = 0x5a5a5a5au;
        e.pack_ints([&](int k, uint32_t v) { if (v == 0x5a5a5a5au) at = W_INT + k; });
        *u = keep;
        return at;
    }
};

int main(int argc, char **argv) {
    if (argc < 2) return 2;
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
        rng.seed_numpy((uint32_t)atol(argv[2]));
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
    return lane_check::run<Sim>(argc, argv);
}
