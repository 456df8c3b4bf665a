// tests/test_bounce_rank_cpu.py: prints bounce_first_rank (csrc/wave_rank.hpp) of every lane for each mask read from standard input
// (one hexadecimal mask per line in, 64 ranks per line out).
#include <cstdio>

#include "wave_rank.hpp"

int main()
{
    unsigned long long mask;
    while (std::scanf("%llx", &mask) == 1) {
        for (int lane = 0; lane < 64; lane++) std::printf("%u%c", mcpt::bounce_first_rank(mask, lane), lane == 63 ? '\n' : ' ');
    }
    return 0;
}
