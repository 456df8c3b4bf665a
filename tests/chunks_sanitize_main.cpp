// Stand-alone program around csrc/chunks.hpp for tests/test_chunks_cpu.py, built there with -fsanitize=address,undefined: the chunk plan
// at the edges of its arguments (a signed overflow anywhere in it is an error the sanitizer reports).
// stdin: one triple per line: workspace_rays rays_per_item n.
// stdout, per triple: per_chunk, the rays of a full chunk (per_chunk * rays_per_item, as the callers form it), and -- walked as the
// callers' loops walk, where that takes at most 2^20 steps, else -1 -1 -1 -- the number of chunks, the sum of their counts and the
// last chunk's count.
#include <cstdio>

#include "chunks.hpp"

int main()
{
    long long ws, item, n;
    while (std::scanf("%lld %lld %lld", &ws, &item, &n) == 3) {
        if (ws < 0 || ws > (1LL << 62) || item < 1 || item > (1LL << 62) || n < 1 || n > (1LL << 62)) return 2;
        const int64_t per = mcpt::chunk_plan(ws, item, n);
        long long chunks = -1, sum = -1, last = -1;
        if (n / per <= (1 << 20)) {
            chunks = sum = last = 0;
            for (int64_t first = 0; first < n; first += per, chunks++) {
                last = mcpt::chunk_count(per, n, first);
                if (last < 1 || last > per) return 3;
                sum += last;
            }
        }
        std::printf("%lld %lld %lld %lld %lld\n", (long long)per, (long long)(per * item), chunks, sum, last);
    }
    return 0;
}
