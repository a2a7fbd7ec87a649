// Replays an airline fixture through csrc/airline_env.hpp on the CPU (the code the kernels run, compiled for the host) and compares every
// step with what the reference recorded, bit for bit.  Driven by tools/probes/airline_host_check.py, which writes the input file:
//   int32 n, T, autoreset, nresets; float reset_obs[nresets][160]; then per env: int32 seed, int32 actions[T], int32 reset_at[T] (row of
//   reset_obs or -1), float obs0[160], float obs[T][160], double reward[T], uint8 terminated[T], double info[T][5].
// The generator is MT19937 seeded as CPython's random.seed(int) does (init_by_array over the 32-bit digits of the seed).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../custom_gymnasium_environments_amd/csrc/airline_env.hpp"

using namespace cge::airline;

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
};

// the memory a runtime index reaches, as plain arrays; every index is checked
struct Mem {
    uint32_t acw[NA], av[NP], fl[NF];
    double pr[NP], sc[NPRI], fu[NA], m0[NA];
    float sv[NP];
    static int at(int i, int n) { if (i < 0 || i >= n) { printf("index %d outside 0..%d\n", i, n - 1); exit(3); } return i; }
    uint32_t ac(int a) const { return acw[at(a, NA)]; }
    void set_ac(int a, uint32_t w) { acw[at(a, NA)] = w; }
    uint32_t avail(int p) const { return av[at(p, NP)]; }
    void set_avail(int p, uint32_t m) { av[at(p, NP)] = m; }
    double price(int p) const { return pr[at(p, NP)]; }
    void set_price(int p, double v) { pr[at(p, NP)] = v; }
    float sev(int p) const { return sv[at(p, NP)]; }
    void set_sev(int p, float v) { sv[at(p, NP)] = v; }
    double fuel(int a) const { return fu[at(a, NA)]; }
    void set_fuel(int a, double v) { fu[at(a, NA)] = v; }
    double maint0(int a) const { return m0[at(a, NA)]; }
    void set_maint0(int a, double v) { m0[at(a, NA)] = v; }
    uint32_t flight(int f) const { return fl[at(f, NF)]; }
    void set_flight(int f, uint32_t w) { fl[at(f, NF)] = w; }
    double sched(int f) const { return sc[at(f, NPRI)]; }
    void set_sched(int f, double s) { sc[at(f, NPRI)] = s; }
};

static void observe(const Env &e, Mem &m, float *o) {
    observe_part<0>(e, m, [&](int k, float v) { o[k] = v; });
    observe_part<1>(e, m, [&](int k, float v) { o[40 + k] = v; });
    observe_part<2>(e, m, [&](int k, float v) { o[80 + k] = v; });
    observe_part<3>(e, m, [&](int k, float v) { o[120 + k] = v; });
}

// through the packed scalar words, as every launch does
static void repack(Env &e) {
    uint32_t w[14];
    e.pack_scalars([&](int k, uint32_t v) { w[k] = v; });
    e.unpack_scalars([&](int k) { return w[k]; });
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[4];
    if (fread(hd, 4, 4, f) != 4) return 2;
    const int n = hd[0], T = hd[1], autoreset = hd[2], nres = hd[3];
    std::vector<float> robs((size_t)nres * OBS);
    if (fread(robs.data(), 4, robs.size(), f) != robs.size()) return 2;
    long bad = 0;
    for (int i = 0; i < n; ++i) {
        int32_t seed;
        std::vector<int32_t> a(T), at(T);
        std::vector<float> obs0(OBS), obs((size_t)T * OBS);
        std::vector<double> r(T), info((size_t)T * 5);
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
        observe(e, m, got);
        if (memcmp(got, obs0.data(), sizeof got) && bad++ < 5) printf("env %d: reset observation differs\n", i);
        for (int t = 0; t < T; ++t) {
            repack(e);
            bool term;
            const double rew = env_step(e, m, rng, a[t], a[t] >= 0 && a[t] < 45, term);
            observe(e, m, got);
            const double gi[5] = {e.otp(), e.sat, 0.0, e.costs, (double)e.h4 * 0.25};
            bool ok = !memcmp(&rew, &r[t], 8) && term == (tm[t] != 0) && !memcmp(gi, &info[5 * (size_t)t], sizeof gi) && !memcmp(got, &obs[(size_t)OBS * t], sizeof got);
            if (term && autoreset) {
                reset_episode(e, m, rng);
                observe(e, m, got);
                ok = ok && at[t] >= 0 && !memcmp(got, &robs[(size_t)OBS * at[t]], sizeof got);
            }
            if (!ok && bad++ < 5) {
                printf("env %d step %d action %d: reward %.17g / %.17g terminated %d / %d\n", i, t, a[t], rew, r[t], (int)term, (int)tm[t]);
                for (int k = 0; k < 5; ++k) if (memcmp(&gi[k], &info[5 * (size_t)t + k], 8)) printf("  info %d: %.17g / %.17g\n", k, gi[k], info[5 * (size_t)t + k]);
                for (int k = 0; k < OBS; ++k) if (memcmp(&got[k], &obs[(size_t)OBS * t + k], 4)) printf("  obs %d: %.9g / %.9g\n", k, got[k], obs[(size_t)OBS * t + k]);
            }
        }
    }
    fclose(f);
    printf("%s: %d envs x %d steps, %ld mismatching steps\n", argv[1], n, T, bad);
    return bad ? 1 : 0;
}
