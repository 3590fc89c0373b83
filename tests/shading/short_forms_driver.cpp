/* The short forms of the cornell-box kernel's shading arithmetic (include/tb_math.h; docs/experiments/r12.md) against the forms they stand for,
 * as bits, on the host:
 *   tb_sincos(x)          against tb_sin(x) and tb_cos(x);
 *   tb_div_pi(x)          against x / TB_PI_F, and tb_div_pi_fast(x) -- the three operations alone -- to find the numerators they are good for;
 *   tb_zero_over_sqrt(s)  against 0.0f / s for every s that is +0, denormal, normal, +inf or NaN, and for every s that tb_sqrt returns for one.
 *
 *   short_forms_driver full      every one of the 2^32 binary32 values for the division and the square roots, every 251st for tb_sincos
 *   short_forms_driver strided   every 4 093rd value and the edge values (the build under ASan + UBSan runs this one)
 *
 * Prints one "name value" line per answer; exit status 1 if any comparison failed. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <thread>
#include <utility>
#include <vector>

#include "tb_math.h"

namespace {

constexpr unsigned THREADS = 16;
typedef std::pair<uint32_t, uint32_t> Run; /* magnitudes first .. second, both included */

struct Tally {
    uint64_t sincos = 0, sincosBad = 0;      /* arguments compared, arguments whose sine or cosine differs */
    uint64_t div = 0, divBad = 0;            /* tb_div_pi */
    uint64_t fastBadInside = 0;              /* tb_div_pi_fast differs from the division where tb_div_pi takes it */
    uint64_t zero = 0, zeroBad = 0;          /* tb_zero_over_sqrt */
    uint64_t sqrtClasses[5] = {0, 0, 0, 0, 0}; /* +0, denormal, normal, +inf, NaN among the denominators seen */
    std::vector<Run> runs;                   /* maximal runs of magnitudes for which the three operations are right for both signs */
};

bool same_sincos(float x)
{
    float s, c;
    tb_sincos(x, &s, &c);
    return tb_f2u(s) == tb_f2u(tb_sin(x)) && tb_f2u(c) == tb_f2u(tb_cos(x));
}

bool fast_is_right(uint32_t bits)
{
    const float x = tb_u2f(bits);
    return tb_f2u(tb_div_pi_fast(x)) == tb_f2u(x / TB_PI_F);
}

bool div_pi_is_right(uint32_t bits)
{
    const float x = tb_u2f(bits);
    return tb_f2u(tb_div_pi(x)) == tb_f2u(x / TB_PI_F);
}

/* every value that is not negative and not -0, as the denominator itself and through tb_sqrt: a sum of two squares is +0, positive, +inf or NaN,
 * and so is its square root (which is never denormal: the value itself covers that class) */
void one_sqrt(uint32_t bits, Tally& t)
{
    const float x = tb_u2f(bits);
    if (x < 0.0f || bits == 0x80000000u) return;
    const float both[2] = {x, tb_sqrt(x)};
    for (const float s : both) {
        if (s != s && !(tb_f2u(s) & 0x00400000u)) continue; /* a signalling NaN: no operation returns one */
        const uint32_t u = tb_f2u(s);
        t.sqrtClasses[s != s ? 4 : u == 0x7f800000u ? 3 : u == 0 ? 0 : (u & 0x7f800000u) == 0 ? 1 : 2]++;
        t.zero++;
        if (tb_f2u(tb_zero_over_sqrt(s)) != tb_f2u(0.0f / s)) t.zeroBad++;
    }
}

/* magnitudes lo .. hi - 1, every `step`th; with step 1 the runs of the fast path are collected */
void sweep(uint64_t lo, uint64_t hi, uint64_t step, uint64_t sincosEvery, Tally& t)
{
    bool open = false;
    uint32_t first = 0;
    for (uint64_t m64 = lo; m64 < hi; m64 += step) {
        const uint32_t m = (uint32_t)m64;
        bool both = true;
        for (uint32_t sign = 0; sign < 2; sign++) {
            const uint32_t bits = m | sign << 31;
            t.div++;
            if (!div_pi_is_right(bits)) t.divBad++;
            const bool ok = fast_is_right(bits);
            both = both && ok;
            if (!ok && tb_div_pi_is_fast(tb_u2f(bits))) t.fastBadInside++;
            one_sqrt(bits, t);
            if (m64 % sincosEvery == 0) { t.sincos++; if (!same_sincos(tb_u2f(bits))) t.sincosBad++; }
        }
        if (step == 1) {
            if (both && !open) { open = true; first = m; }
            if (!both && open) { open = false; t.runs.push_back(Run(first, m - 1)); }
        }
    }
    if (open) t.runs.push_back(Run(first, (uint32_t)(hi - 1)));
}

void edges(Tally& t)
{
    const uint32_t e[] = {0x00000000u, 0x00000001u, 0x007fffffu, 0x00800000u, 0x00800001u, 0x00ffffffu, 0x01000000u, 0x3f800000u, 0x40490fdau, 0x40490fdbu,
                          0x4e6e6b28u /* 1e9 */, 0x4e6e6b27u, 0x7f7fffffu, 0x7f800000u, 0x7f800001u, 0x7fc00000u, 0x7fffffffu,
                          TB_DIV_PI_FAST_MIN_BITS, TB_DIV_PI_FAST_MIN_BITS - 1u, TB_DIV_PI_FAST_MAX_BITS, TB_DIV_PI_FAST_MAX_BITS + 1u};
    for (uint32_t m : e) sweep(m, (uint64_t)m + 1, 1, 1, t);
    t.runs.clear();
}

} // namespace

int main(int argc, char** argv)
{
    const bool full = argc > 1 && !strcmp(argv[1], "full");
    if (!full && !(argc > 1 && !strcmp(argv[1], "strided"))) { fprintf(stderr, "usage: %s full|strided\n", argv[0]); return 2; }
    const uint64_t N = 1ull << 31, step = full ? 1 : 4093, sincosEvery = full ? 251 : 1;
    std::vector<Tally> tallies(THREADS);
    std::vector<std::thread> pool;
    for (unsigned i = 0; i < THREADS; i++) {
        /* a thread's first magnitude is a multiple of the step, so the strided sweep is one progression */
        const uint64_t lo = (N / THREADS * i + step - 1) / step * step, hi = i + 1 == THREADS ? N : N / THREADS * (i + 1);
        pool.emplace_back([&tallies, lo, hi, step, sincosEvery, i]() { sweep(lo, hi, step, sincosEvery, tallies[i]); });
    }
    for (std::thread& th : pool) th.join();
    Tally all;
    edges(all);
    for (const Tally& t : tallies) {
        all.sincos += t.sincos; all.sincosBad += t.sincosBad; all.div += t.div; all.divBad += t.divBad; all.fastBadInside += t.fastBadInside;
        all.zero += t.zero; all.zeroBad += t.zeroBad;
        for (int k = 0; k < 5; k++) all.sqrtClasses[k] += t.sqrtClasses[k];
        for (const Run& r : t.runs) {   /* the threads' ranges follow one another: a run that ends where the next begins is one run */
            if (!all.runs.empty() && all.runs.back().second + 1u == r.first) all.runs.back().second = r.second;
            else all.runs.push_back(r);
        }
    }
    printf("sincos_compared %llu\nsincos_differ %llu\n", (unsigned long long)all.sincos, (unsigned long long)all.sincosBad);
    printf("div_pi_compared %llu\ndiv_pi_differ %llu\n", (unsigned long long)all.div, (unsigned long long)all.divBad);
    printf("fast_path_differs_where_taken %llu\n", (unsigned long long)all.fastBadInside);
    printf("zero_over_sqrt_compared %llu\nzero_over_sqrt_differ %llu\n", (unsigned long long)all.zero, (unsigned long long)all.zeroBad);
    printf("sqrt_classes_zero_denormal_normal_inf_nan %llu %llu %llu %llu %llu\n", (unsigned long long)all.sqrtClasses[0], (unsigned long long)all.sqrtClasses[1],
           (unsigned long long)all.sqrtClasses[2], (unsigned long long)all.sqrtClasses[3], (unsigned long long)all.sqrtClasses[4]);
    printf("header_interval 0x%08x 0x%08x\n", TB_DIV_PI_FAST_MIN_BITS, TB_DIV_PI_FAST_MAX_BITS);
    bool ok = all.sincosBad == 0 && all.divBad == 0 && all.fastBadInside == 0 && all.zeroBad == 0;
    for (int k = 0; k < 5; k++) ok = ok && all.sqrtClasses[k] > 0;
    if (full) {
        /* the domain of the three operations: the runs of magnitudes that are right for both signs, the longest first */
        Run best(1, 0);
        uint64_t bestLen = 0, rightMagnitudes = 0;
        for (const Run& r : all.runs) {
            const uint64_t len = (uint64_t)r.second - r.first + 1;
            rightMagnitudes += len;
            if (len > bestLen) { bestLen = len; best = r; }
        }
        printf("fast_path_runs %zu\nfast_path_right_magnitudes %llu\n", all.runs.size(), (unsigned long long)rightMagnitudes);
        printf("fast_path_longest_run 0x%08x 0x%08x %.9g %.9g\n", best.first, best.second, tb_u2f(best.first), tb_u2f(best.second));
        std::sort(all.runs.begin(), all.runs.end(), [](const Run& a, const Run& b) { return a.second - a.first > b.second - b.first; });
        for (size_t k = 1; k < all.runs.size() && k < 4; k++) printf("fast_path_next_run 0x%08x 0x%08x\n", all.runs[k].first, all.runs[k].second);
        printf("fast_path_plus_zero %d\nfast_path_minus_zero %d\n", (int)fast_is_right(0u), (int)fast_is_right(0x80000000u));
        ok = ok && best.first == TB_DIV_PI_FAST_MIN_BITS && best.second == TB_DIV_PI_FAST_MAX_BITS;
    }
    printf("ok %d\n", (int)ok);
    return ok ? 0 : 1;
}
