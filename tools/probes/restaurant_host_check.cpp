// Replays a restaurant fixture through csrc/restaurant_env.hpp on the CPU (the code the kernels run, compiled for the host) and compares
// every step with what the reference recorded.  Driven by tools/probes/restaurant_host_check.py, which writes the input file:
//   int32 n, T, max_steps; then per env: int32 actions[T][4], double u[T], double reward[T], double total[T], int32 info[T][12],
//   int32 obs[T][340] (the six list planes in key order; the reference's step() returns the terminal observation).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../custom_gymnasium_environments_amd/csrc/restaurant_env.hpp"

using namespace cge::restaurant;

static void expand(const Env &e, int32_t *o) {
    uint32_t stg[STG_WORDS] = {0};
    e.stage([&](int k, uint32_t v) { stg[k] = v; });
    const uint8_t *b = reinterpret_cast<const uint8_t *>(stg);
    const int per[6] = {100, 30, 10, 10, 150, 40}, off[6] = {STG_WAITING, STG_WAITERS, STG_OCC, STG_DIRTY, STG_COOKING, STG_READY},
              lim[6] = {LIM_WAITING, LIM_WAITERS, LIM_TABLES, LIM_TABLES, LIM_COOKING, LIM_READY};
    for (int p = 0; p < 6; ++p)
        for (int k = 0; k < per[p]; ++k) *o++ = k < lim[p] ? b[off[p] + k] : 0;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hd[3];
    if (fread(hd, 4, 3, f) != 3) return 2;
    const int n = hd[0], T = hd[1], max_steps = hd[2];
    long bad = 0;
    for (int i = 0; i < n; ++i) {
        std::vector<int32_t> a(T * 4), info(T * 12), obs((size_t)T * 340);
        std::vector<double> u(T), r(T), tot(T);
        if (fread(a.data(), 4, a.size(), f) != a.size() || fread(u.data(), 8, T, f) != (size_t)T || fread(r.data(), 8, T, f) != (size_t)T ||
            fread(tot.data(), 8, T, f) != (size_t)T || fread(info.data(), 4, info.size(), f) != info.size() || fread(obs.data(), 4, obs.size(), f) != obs.size()) return 2;
        Env e;
        e.clear();
        e.mt_pos = e.mt_enc = 0;
        for (int t = 0; t < T; ++t) {
            uint32_t w[REC_WORDS];                       // through the packed record every step, as a step() call does
            e.pack(w);
            Env e2;
            e2.unpack(w);
            e = e2;
            bool invalid;
            const double rew = e.step(a[4 * t], a[4 * t + 1], a[4 * t + 2], a[4 * t + 3], u[t], invalid);
            int32_t got[340];
            expand(e, got);
            const int32_t gi[12] = {(int32_t)e.t, (int32_t)e.nw, (int32_t)e.idle_waiters(), (int32_t)e.cooking(), (int32_t)e.nr, (int32_t)e.bits10(e.dirty),
                                    (int32_t)e.served, (int32_t)e.left, (int32_t)e.cleaned, (int32_t)e.orders, (int32_t)e.wait_sum(), (int32_t)e.num_customers()};
            const bool ok = !memcmp(&rew, &r[t], 8) && !memcmp(&e.total, &tot[t], 8) && !memcmp(gi, &info[12 * t], sizeof gi) &&
                            !memcmp(got, &obs[(size_t)340 * t], sizeof got) && !invalid;
            if (!ok && bad++ < 5) {
                printf("env %d step %d: reward %.17g / %.17g total %.17g / %.17g\n", i, t, rew, r[t], e.total, tot[t]);
                for (int k = 0; k < 12; ++k) if (gi[k] != info[12 * t + k]) printf("  info %d: %d / %d\n", k, gi[k], info[12 * t + k]);
                for (int k = 0; k < 340; ++k) if (got[k] != obs[(size_t)340 * t + k]) printf("  obs %d: %d / %d\n", k, got[k], obs[(size_t)340 * t + k]);
            }
            if (e.t >= (uint32_t)max_steps) e.clear();
        }
    }
    printf("%s: %d envs x %d steps, %ld mismatching steps\n", argv[1], n, T, bad);
    return bad ? 1 : 0;
}
