// Stand-alone program around csrc/baked.hpp for tests/test_baked_cpu.py, built there with -fsanitize=address,undefined: the lightmap's
// lookup on the inputs a caller can get wrong -- NaN, infinities, +-1e300, maps one texel wide.  The map and the owner map are exactly as
// large as their size says (heap arrays: a tap outside them is an error the sanitizer reports), E[T][c] = (3 T + c + 1) / 4.
// stdin, one lookup per line: width height owner-mode u v   (owner-mode 0: none, 1: owner -1 on every third texel, 2: all -1)
// stdout, one line each: the three channels as hex floats and the taps.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "baked.hpp"

int main()
{
    char su[64], sv[64];
    int W, H, mode;
    while (std::scanf("%d %d %d %63s %63s", &W, &H, &mode, su, sv) == 5) {
        if (W < 1 || H < 1 || W > 4096 || H > 4096 || mode < 0 || mode > 2) return 2;
        const double u = std::strtod(su, nullptr), v = std::strtod(sv, nullptr);
        const size_t n = size_t(W) * size_t(H);
        std::vector<double> irr(n * 3);
        std::vector<int32_t> owner(n);
        for (size_t T = 0; T < n; T++) {
            for (size_t c = 0; c < 3; c++) irr[T * 3 + c] = double(3 * T + c + 1) / 4.0;
            owner[T] = mode == 2 || (mode == 1 && T % 3 == 0) ? -1 : int32_t(T % 7);
        }
        double E[3];
        const int taps = mcpt::baked_lightmap_lookup(W, H, irr.data(), mode ? owner.data() : nullptr, u, v, E);
        std::printf("%a %a %a %d\n", E[0], E[1], E[2], taps);
    }
    return 0;
}
