// Replays an emergency fixture through csrc/emergency_env.hpp on the CPU (the code the kernels run, compiled for the host) and compares
// every step with what the reference recorded, bit for bit.  Driven by tools/probes/emergency_host_check.py, which writes the input file:
//   int32 n, T, autoreset, nresets, max_timesteps; float reset_obs[nresets][276]; then per env: int32 seed, int32 actions[T],
//   int32 reset_at[T] (row of reset_obs or -1), float obs0[276], float obs[T][276], double reward[T], uint8 terminated[T], double info[T][6].
// `--mean`: reads float64 vectors of 25 from stdin and writes mean25() of each to stdout (the order of NumPy's np.mean).
// The generator is MT19937 seeded as CPython's random.seed(int) does (init_by_array over the 32-bit digits of the seed).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../custom_gymnasium_environments_amd/csrc/emergency_env.hpp"

using namespace cge::emergency;

struct Mt {
    uint32_t mt[624];
    int idx = 624;
    void init(uint32_t s) {
        mt[0] = s;
        for (int i = 1; i < 624; ++i) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
    }
    void seed(uint32_t key) {                                        // init_by_array([key])
        init(19650218u);
        int i = 1;
        for (int k = 624; k; --k) {
            mt[i] = (mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1664525u)) + key;
            if (++i >= 624) { mt[0] = mt[623]; i = 1; }
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
    template <int W>
    void run(uint32_t (&w)[W]) { for (int k = 0; k < W; ++k) w[k] = next(); }
};

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

static void observe(const Env &e, Mem &m, float *o, uint32_t max_timesteps) {
    auto out = [&](int k, float v) { if (k < 0 || k >= OBS) { printf("element %d\n", k); exit(3); } o[k] = v; };
    for (int s = 0; s < NI; ++s) observe_incident(e, m, out, s);
    for (int u = 0; u < 40; ++u) observe_unit(e, m, out, u);
    observe_rest(e, m, out, max_timesteps);
}

// through the packed scalar words, as every launch does
static void repack(Env &e) {
    uint32_t w[N_SCAL];
    e.pack_scalars([&](int k, uint32_t v) { w[k] = v; });
    e.unpack_scalars([&](int k) { return w[k]; });
}

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
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[5];
    if (fread(hd, 4, 5, f) != 5) return 2;
    const int n = hd[0], T = hd[1], autoreset = hd[2], nres = hd[3];
    const uint32_t max_t = (uint32_t)hd[4];
    std::vector<float> robs((size_t)nres * OBS);
    if (fread(robs.data(), 4, robs.size(), f) != robs.size()) return 2;
    long bad = 0;
    for (int i = 0; i < n; ++i) {
        int32_t seed;
        std::vector<int32_t> a(T), at(T);
        std::vector<float> obs0(OBS), obs((size_t)T * OBS);
        std::vector<double> r(T), info((size_t)T * 6);
        std::vector<uint8_t> tm(T);
        if (fread(&seed, 4, 1, f) != 1 || fread(a.data(), 4, T, f) != (size_t)T || fread(at.data(), 4, T, f) != (size_t)T ||
            fread(obs0.data(), 4, OBS, f) != OBS || fread(obs.data(), 4, obs.size(), f) != obs.size() || fread(r.data(), 8, T, f) != (size_t)T ||
            fread(tm.data(), 1, T, f) != (size_t)T || fread(info.data(), 8, info.size(), f) != info.size()) return 2;
        Mt rng;
        rng.seed((uint32_t)seed);
        Env e{};
        Mem m{};
        draw_network(e, m, rng);
        reset_episode(e, m, rng);
        float got[OBS];
        observe(e, m, got, max_t);
        if (memcmp(got, obs0.data(), sizeof got) && bad++ < 5) printf("env %d: reset observation differs\n", i);
        for (int t = 0; t < T; ++t) {
            repack(e);
            bool term;
            const double rew = env_step(e, m, rng, a[t], a[t] >= 0 && a[t] < ACTIONS, max_t, term);
            observe(e, m, got, max_t);
            const double gi[6] = {(double)e.ninc, (double)e.casualties, (double)e.lives, (double)e.resolved, e.avg_rt(), (double)e.reason};
            bool ok = !memcmp(&rew, &r[t], 8) && term == (tm[t] != 0) && !memcmp(gi, &info[6 * (size_t)t], sizeof gi) && !memcmp(got, &obs[(size_t)OBS * t], sizeof got);
            if (!ok && bad++ < 5) {
                printf("env %d step %d action %d: reward %.17g / %.17g terminated %d / %d\n", i, t, a[t], rew, r[t], (int)term, (int)tm[t]);
                for (int k = 0; k < 6; ++k) if (memcmp(&gi[k], &info[6 * (size_t)t + k], 8)) printf("  info %d: %.17g / %.17g\n", k, gi[k], info[6 * (size_t)t + k]);
                for (int k = 0; k < OBS; ++k) if (memcmp(&got[k], &obs[(size_t)OBS * t + k], 4)) printf("  obs %d: %.9g / %.9g\n", k, got[k], obs[(size_t)OBS * t + k]);
            }
            if (term && autoreset) {
                reset_episode(e, m, rng);
                observe(e, m, got, max_t);
                if (!(at[t] >= 0 && !memcmp(got, &robs[(size_t)OBS * at[t]], sizeof got)) && bad++ < 5) printf("env %d step %d: reset observation differs\n", i, t);
            }
        }
    }
    fclose(f);
    printf("%s: %d envs x %d steps, %ld mismatching steps\n", argv[1], n, T, bad);
    return bad ? 1 : 0;
}
