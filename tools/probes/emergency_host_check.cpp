// Replays an emergency fixture through csrc/emergency_env.hpp on the CPU (the code the kernels run, compiled for the host) and compares
// every step with what the reference recorded, bit for bit.  Driven by tools/probes/emergency_host_check.py, which writes the input file:
//   int32 n, T, autoreset, nresets, max_timesteps; float reset_obs[nresets][276]; then per env: int32 seed, int32 actions[T],
//   int32 reset_at[T] (row of reset_obs or -1), float obs0[276], float obs[T][276], double reward[T], uint8 terminated[T], double info[T][6].
// `--mean`: reads float64 vectors of 25 from stdin and writes mean25() of each to stdout (the order of NumPy's np.mean).
// The generator is MT19937 seeded as CPython's random.seed(int) does.  The reader, the replay loop and the generator are those of
// lane_host_check.hpp.
#include "lane_host_check.hpp"

#include "../../custom_gymnasium_environments_amd/csrc/emergency_env.hpp"

using namespace cge::emergency;
using lane_check::Mt;

// the memory a runtime index reaches, as plain arrays; every index is checked
struct Mem {
    uint32_t iw[NI], im[NI], is[NI], uw[NU];
    double fa[NU];
    static int at(uint32_t i, int n) { if (i >= (uint32_t)n) { printf("index %u outside 0..%d\n", i, n - 1); exit(3); } return (int)i; }
    uint32_t inc(uint32_t s) const { return iw[at(s, NI)]; }
    void set_inc(uint32_t s, uint32_t w) { iw[at(s, NI)] = w; }
    uint32_t mask(uint32_t s) const { return im[at(s, NI)]; }
    void set_mask(uint32_t s, uint32_t w) { im[at(s, NI)] = w; }
    uint32_t start(uint32_t s) const { return is[at(s, NI)]; }
    void set_start(uint32_t s, uint32_t w) { is[at(s, NI)] = w; }
    uint32_t unit(uint32_t u) const { return uw[at(u, NU)]; }
    void set_unit(uint32_t u, uint32_t w) { uw[at(u, NU)] = w; }
    double fatigue(uint32_t u) const { return fa[at(u, NU)]; }
    void set_fatigue(uint32_t u, double v) { fa[at(u, NU)] = v; }
};

struct Sim {
    static constexpr int WIDTH = OBS, NINFO = 6, EXTRA = 1;           // extra: max_timesteps
    static constexpr bool INFO0 = false, TRUNCATED = false, POKES = false;
    Env e{};
    Mem m{};
    Mt rng;
    uint32_t max_t;
    Sim(uint64_t seed, const int32_t *extra) : max_t((uint32_t)extra[0]) {
        rng.seed_python((uint32_t)seed);
        draw_network(e, m, rng);
        reset_episode(e, m, rng);
    }
    double step(int32_t a, bool &term, bool &) { return env_step(e, m, rng, a, a >= 0 && a < ACTIONS, max_t, term); }
    void reset() { reset_episode(e, m, rng); }
    void observe(float *o) {
        auto out = [&](int k, float v) { o[lane_check::element(k, OBS)] = v; };
        for (int s = 0; s < NI; ++s) observe_incident(e, m, out, s);
        for (int u = 0; u < 40; ++u) observe_unit(e, m, out, u);
        observe_rest(e, m, out, max_t);
    }
    void info(double *gi) const {
        const double row[NINFO] = {(double)e.ninc, (double)e.casualties, (double)e.lives, (double)e.resolved, e.avg_rt(), (double)e.reason};
        memcpy(gi, row, sizeof row);
    }
    void repack() {                                                  // through the packed scalar words, as every launch does
        uint32_t w[N_SCAL];
        e.pack_scalars([&](int k, uint32_t v) { w[k] = v; });
        e.unpack_scalars([&](int k) { return w[k]; });
    }
};

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "--mean")) {
        double v[NT];
        while (fread(v, 8, NT, stdin) == (size_t)NT) {
            const double mean = mean25(v);
            fwrite(&mean, 8, 1, stdout);
        }
        return 0;
    }
    return lane_check::run<Sim>(argc, argv);
}
