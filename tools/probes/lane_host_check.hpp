// The shared part of tools/probes/{airline,emergency,space_station,farm}_host_check.cpp: the generator, the reader of the file that
// tools/probes/lane_host_check.py::write_fixture writes, the replay loop with its mismatch report, the poke table with `--layout`, and
// `--record`.  A type's program includes its csrc/<type>_env.hpp, describes itself in a struct Sim and ends its main() in
// lane_check::run<Sim>(argc, argv).  Sim mirrors what the type gives lane_host_check.bind() in Python:
//   WIDTH (floats of an observation row), NINFO (doubles of an info row), EXTRA (int32 of the file's header behind n, T, autoreset,
//   nresets: they reach the constructor), INFO0 / TRUNCATED (those columns are in the file), POKES (a poke count and the poke table follow
//   the header; the program also has --layout and --record, and Sim has each_named(), int_word(), REC_DOUBLES and RECORD_EXTRA);
//   Sim(uint64_t seed, const int32_t *extra): seeds the generators, constructs the env and resets it for the first time;
//   double step(int32_t action, bool &terminated, bool &truncated); void reset(); void observe(float *) (element indices through
//   lane_check::element()); void info(double *); void repack() (the state through its packed words, as every launch does); Env e.
// The file: int32 n, T, autoreset, nresets, extra[EXTRA], [npokes]; float reset_obs[nresets][WIDTH]; [npokes x Poke: the named field of
// that env is set before that step]; then per env: int32 seed, int32 actions[T], int32 reset_at[T] (row of reset_obs or -1),
// float obs0[WIDTH], [double info0[NINFO]], float obs[T][WIDTH], double reward[T], uint8 terminated[T], [uint8 truncated[T]],
// double info[T][NINFO].  Exit status: 0, 1 a mismatching step, 2 bad input (an unknown poke name included), 3 an index out of range.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace lane_check {

struct Mt {                                                          // MT19937
    uint32_t mt[624];
    int idx = 624;
    void seed_numpy(uint32_t s) {                                    // init_genrand: NumPy's legacy np.random.seed(int)
        mt[0] = s;
        for (int i = 1; i < 624; ++i) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
        idx = 624;
    }
    void seed_python(uint64_t s) {                                   // init_by_array over the 32-bit limbs: CPython's random.seed(int)
        const uint32_t key[2] = {(uint32_t)s, (uint32_t)(s >> 32)};
        const int len = key[1] ? 2 : 1;
        seed_numpy(19650218u);
        int i = 1, j = 0;
        for (int k = 624; k; --k) {
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
    template <int W>
    void run(uint32_t (&w)[W]) { for (int k = 0; k < W; ++k) w[k] = next(); }
};

// the element index of an observation row, checked
inline int element(int k, int n) { if (k < 0 || k >= n) { printf("element %d\n", k); exit(3); } return k; }

struct Poke { int32_t env, step; char name[24]; double value; };
static_assert(sizeof(Poke) == 40, "as lane_host_check.py writes it");

// each_named(e, f) calls f(name, the double or nullptr, the whole-word integer or nullptr) for every field a poke can name
template <class S>
bool poke(S &s, const char *name, double value) {
    bool found = false;
    S::each_named(s.e, [&](const char *nm, double *d, uint32_t *u) {
        if (strcmp(nm, name)) return;
        found = true;
        if (d) *d = value; else *u = (uint32_t)value;
    });
    return found;
}

// `--layout`: the word of the record that holds each named field, a double by its address in each_double(), an integer by int_word()
template <class S>
int layout() {
    decltype(S::e) e{};
    int bad = 0;
    S::each_named(e, [&](const char *nm, double *d, uint32_t *u) {
        int at = -1;
        if (d) e.each_double(e, [&](int w, double &v) { if (&v == d) at = w; });
        else at = S::int_word(e, u);
        if (at < 0 || at + (d ? 1 : 0) >= S::REC_WORDS) { ++bad; return; }
        printf("%s %d %s\n", nm, at, d ? "f64" : "u32");
    });
    return bad ? 1 : 0;
}

// `--record S0 N K`: int32 actions [K][N] from stdin; env i = 0 .. N - 1 seeded S0 + i goes through reset and K steps with an autoreset
// in the same step; the REC_DOUBLES float64 slots of each record go to stdout in column order (a slot that holds no double as zero)
template <class S>
int record(long s0, long n, long K) {
    std::vector<int32_t> a((size_t)n * K);
    if (fread(a.data(), 4, a.size(), stdin) != a.size()) return 2;
    for (long i = 0; i < n; ++i) {
        S s((uint64_t)(s0 + i), S::RECORD_EXTRA);
        for (long t = 0; t < K; ++t) {
            bool term, trunc;
            s.step(a[(size_t)t * n + i], term, trunc);
            if (term) s.reset();
        }
        double rec[S::REC_DOUBLES] = {};
        s.e.each_double(s.e, [&](int w, const double &v) { rec[w / 2] = v; });
        fwrite(rec, 8, S::REC_DOUBLES, stdout);
    }
    return 0;
}

template <class T>
bool read(FILE *f, std::vector<T> &v) { return fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

template <class S>
int replay(const char *path) {
    constexpr int W = S::WIDTH, NI = S::NINFO;
    FILE *f = fopen(path, "rb");
    if (!f) return 2;
    std::vector<int32_t> hd(4 + S::EXTRA + (S::POKES ? 1 : 0));
    if (!read(f, hd)) return 2;
    const int n = hd[0], T = hd[1], autoreset = hd[2], nres = hd[3];
    if (n < 0 || T < 0 || nres < 0 || (S::POKES && hd[4 + S::EXTRA] < 0)) return 2;
    std::vector<float> robs((size_t)nres * W);
    std::vector<Poke> pokes(S::POKES ? (size_t)hd[4 + S::EXTRA] : 0);
    if (!read(f, robs) || !read(f, pokes)) return 2;
    for (Poke &p : pokes) p.name[sizeof p.name - 1] = 0;
    long bad = 0;
    for (int i = 0; i < n; ++i) {
        std::vector<int32_t> seed(1), a(T), at(T);
        std::vector<float> obs0(W), obs((size_t)T * W);
        std::vector<double> info0(S::INFO0 ? NI : 0), r(T), info((size_t)T * NI);
        std::vector<uint8_t> tm(T), tr(S::TRUNCATED ? T : 0);
        if (!read(f, seed) || !read(f, a) || !read(f, at) || !read(f, obs0) || !read(f, info0) || !read(f, obs) || !read(f, r) || !read(f, tm) ||
            !read(f, tr) || !read(f, info)) return 2;
        S s((uint64_t)(uint32_t)seed[0], hd.data() + 4);
        float got[W];
        double gi[NI];
        s.observe(got);
        s.info(gi);
        if ((memcmp(got, obs0.data(), sizeof got) || (S::INFO0 && memcmp(gi, info0.data(), sizeof gi))) && bad++ < 5)
            printf(S::INFO0 ? "env %d: reset observation or info differs\n" : "env %d: reset observation differs\n", i);
        for (int t = 0; t < T; ++t) {
            if constexpr (S::POKES)
                for (const Poke &p : pokes)
                    if (p.env == i && p.step == t && !poke(s, p.name, p.value)) { printf("no field %s\n", p.name); return 2; }
            s.repack();
            bool term = false, trunc = false;
            const double rew = s.step(a[t], term, trunc);
            s.observe(got);
            s.info(gi);
            const bool ok = !memcmp(&rew, &r[t], 8) && term == (tm[t] != 0) && (!S::TRUNCATED || trunc == (tr[t] != 0)) &&
                            !memcmp(gi, &info[NI * (size_t)t], sizeof gi) && !memcmp(got, &obs[(size_t)W * t], sizeof got);
            if (!ok && bad++ < 5) {
                printf("env %d step %d action %d: reward %.17g / %.17g terminated %d / %d", i, t, a[t], rew, r[t], (int)term, (int)tm[t]);
                if (S::TRUNCATED) printf(" truncated %d / %d", (int)trunc, (int)tr[t]);
                printf("\n");
                for (int k = 0; k < NI; ++k) if (memcmp(&gi[k], &info[NI * (size_t)t + k], 8)) printf("  info %d: %.17g / %.17g\n", k, gi[k], info[NI * (size_t)t + k]);
                for (int k = 0; k < W; ++k) if (memcmp(&got[k], &obs[(size_t)W * t + k], 4)) printf("  obs %d: %.9g / %.9g\n", k, got[k], obs[(size_t)W * t + k]);
            }
            if (term && autoreset) {
                s.reset();
                s.observe(got);
                if (!(at[t] >= 0 && at[t] < nres && !memcmp(got, &robs[(size_t)W * at[t]], sizeof got)) && bad++ < 5) printf("env %d step %d: reset observation differs\n", i, t);
            }
        }
    }
    fclose(f);
    printf("%s: %d envs x %d steps, %ld mismatching steps\n", path, n, T, bad);
    return bad ? 1 : 0;
}

// the modes every program has: a fixture file, and with a poke table --layout and --record S0 N K
template <class S>
int run(int argc, char **argv) {
    if constexpr (S::POKES) {
        if (!strcmp(argv[1], "--layout")) return layout<S>();
        if (!strcmp(argv[1], "--record") && argc > 4) return record<S>(atol(argv[2]), atol(argv[3]), atol(argv[4]));
    }
    return replay<S>(argv[1]);
}

}  // namespace lane_check
