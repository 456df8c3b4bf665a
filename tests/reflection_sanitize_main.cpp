// Stand-alone program around csrc/reflection.hpp for tests/test_reflection_cpu.py, built there with -fsanitize=address,undefined: the
// prefilter and the lookup on the inputs a caller of the device forms can get wrong -- NaN, infinities, +-1e300, zero vectors, maps one
// texel wide, probe indices out of range.  Every array is exactly as large as its size says (heap arrays: a tap outside them is an error
// the sanitizer reports).  Probe i's map is L[b][c] = (7 i + 3 b + c + 1) / 8.
// stdin, first line: res num_levels probes, then num_levels lines: level_res level_ns; then one receiver per line: probe dx dy dz x.
// stdout: the chain, one line of three hex floats per texel, then one line per receiver: the three channels as hex floats (a probe
// outside 0 .. probes - 1: +0.0, the device form's rule).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "reflection.hpp"

int main()
{
    mcpt_reflection_chain c{};
    int probes;
    if (std::scanf("%d %d %d", &c.res, &c.num_levels, &probes) != 3) return 2;
    if (c.res < 1 || c.res > 64 || c.num_levels < 1 || c.num_levels > 8 || probes < 1 || probes > 8) return 2;
    for (int l = 0; l < c.num_levels; l++) {
        if (std::scanf("%d %d", &c.level_res[l], &c.level_ns[l]) != 2) return 2;
        if (c.level_res[l] < 1 || c.level_res[l] > 64 || c.level_ns[l] < 0 || c.level_ns[l] > 65535) return 2;
    }
    const int src = c.res * c.res, T = mcpt::reflection_chain_texels(c);
    std::vector<double> L(size_t(probes) * size_t(src) * 3), dw(size_t(src) * 4), chain(size_t(probes) * size_t(T) * 3);
    for (int i = 0; i < probes; i++)
        for (int b = 0; b < src; b++)
            for (int ch = 0; ch < 3; ch++) L[(size_t(i) * size_t(src) + size_t(b)) * 3 + size_t(ch)] = double(7 * i + 3 * b + ch + 1) / 8.0;
    for (int b = 0; b < src; b++) mcpt::reflection_texel(c.res, b, &dw[size_t(b) * 4], dw[size_t(b) * 4 + 3]);
    for (int l = 0, first = 0; l < c.num_levels; first += c.level_res[l] * c.level_res[l], l++)
        for (int o = 0; o < c.level_res[l] * c.level_res[l]; o++) {
            double r[3], w;
            mcpt::reflection_texel(c.level_res[l], o, r, w);
            for (int i = 0; i < probes; i++)
                mcpt::reflection_filter(dw.data(), L.data() + size_t(i) * size_t(src) * 3, src, r, c.level_ns[l],
                                        chain.data() + (size_t(i) * size_t(T) + size_t(first + o)) * 3);
        }
    for (size_t t = 0; t < size_t(probes) * size_t(T); t++) std::printf("%a %a %a\n", chain[t * 3], chain[t * 3 + 1], chain[t * 3 + 2]);
    char sd[3][64], sx[64];
    long long probe;
    while (std::scanf("%lld %63s %63s %63s %63s", &probe, sd[0], sd[1], sd[2], sx) == 5) {
        const double d[3] = {std::strtod(sd[0], nullptr), std::strtod(sd[1], nullptr), std::strtod(sd[2], nullptr)};
        double v[3] = {0.0, 0.0, 0.0};
        if (probe >= 0 && probe < probes) mcpt::reflection_lookup(c, chain.data() + size_t(probe) * size_t(T) * 3, d, std::strtod(sx, nullptr), v);
        std::printf("%a %a %a\n", v[0], v[1], v[2]);
    }
    return 0;
}
