// Stand-alone program around csrc/chunks.hpp for tests/test_chunks_cpu.py, built there with -fsanitize=address,undefined: the chunk plan
// at the edges of its arguments (a signed overflow anywhere in it is an error the sanitizer reports).
// stdin: one triple per line: workspace_rays rays_per_item n.
// stdout, per triple: per_chunk, the rays of a full chunk (per_chunk * rays_per_item, as the callers form it), and -- walked as the
// callers' loop walks (chunks.hpp: chunk_walk, the loop itself), where that takes at most 2^20 steps, else -1 -1 -1 -- the number of
// chunks, the sum of their counts and the last chunk's count.
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
            sum = last = 0;
            int64_t next = 0;
            int walked = 0;
            const int rc = mcpt::chunk_walk(n, per, walked, [&](int64_t first, int64_t count) {
                if (first != next || count < 1 || count > per) return 3;
                next = first + count;
                sum += last = count;
                return 0;
            });
            if (rc != 0) return rc;
            chunks = walked;
        }
        std::printf("%lld %lld %lld %lld %lld\n", (long long)per, (long long)(per * item), chunks, sum, last);
    }
    return 0;
}
