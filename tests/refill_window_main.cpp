// tests/test_refill_window_cpu.py: checks csrc/refill_window.hpp against brute-force models and prints what it checked.
//   refill_window_main window          the ranking of a refill's window: every W, n_have and mask of the test's list
//   refill_window_main div <stride>    the multiply-shift quotient id / spp: every stride-th id of 0 .. 2^31 - 1 (1: all of them) and the
//                                      ids around every multiple boundary near both ends of the range
// Exit status 0 and a line "ok ..." when everything agrees; the first disagreement is printed and the status is 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "refill_window.hpp"

namespace {

// SplitMix64: seeded, the same masks in every run
uint64_t g_state = 20250u;
uint64_t rnd()
{
    uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

struct Mask { uint64_t v0, v1; };

Mask clip(Mask m, int W)       // no bit at or above W
{
    if (W <= 64) { m.v1 = 0; m.v0 = W == 64 ? m.v0 : m.v0 & ((1ull << W) - 1ull); }
    else if (W < 128) m.v1 &= (1ull << (W - 64)) - 1ull;
    return m;
}

int check_window()
{
    const int Ws[] = {1, 63, 64, 65, 127, 128};
    const int haves[] = {1, 2, 49, 63, 64};
    long long cases = 0;
    for (int W : Ws) {
        std::vector<Mask> masks;
        const uint64_t all = ~0ull, alt = 0x5555555555555555ull;
        masks.push_back({0, 0});                                    // empty
        masks.push_back({all, all});                                // full
        for (int n : {1, 2, 31, 48, 49, 50, 63, 64, 65, 100}) {     // prefix-only and suffix-only runs of n slots
            if (n > W) continue;
            Mask pre = {n >= 64 ? all : (1ull << n) - 1ull, n > 64 ? (1ull << (n - 64)) - 1ull : 0ull};
            masks.push_back(pre);
            Mask suf = {0, 0};
            for (int o = W - n; o < W; o++) (o < 64 ? suf.v0 : suf.v1) |= 1ull << (o & 63);
            masks.push_back(suf);
        }
        masks.push_back({alt, alt});
        masks.push_back({~alt, ~alt});
        masks.push_back({all, 0});
        masks.push_back({0, all});
        for (int i = 0; i < 4000; i++) {                            // every density: a random mask and-ed / or-ed with others
            const uint64_t a0 = rnd(), a1 = rnd(), b0 = rnd(), b1 = rnd(), c0 = rnd(), c1 = rnd();
            switch (i % 5) {
            case 0: masks.push_back({a0, a1}); break;
            case 1: masks.push_back({a0 & b0, a1 & b1}); break;
            case 2: masks.push_back({a0 | b0, a1 | b1}); break;
            case 3: masks.push_back({a0 & b0 & c0, a1 & b1 & c1}); break;
            default: masks.push_back({a0 | b0 | c0, a1 | b1 | c1}); break;
            }
        }
        for (const Mask& m0 : masks) {
            const Mask m = clip(m0, W);
            // the model: the window's rays in slot order
            std::vector<int> rays;
            for (int o = 0; o < W; o++) if (((o < 64 ? m.v0 : m.v1) >> (o & 63)) & 1ull) rays.push_back(o);
            for (int n_have : haves) {
                unsigned char off[64];
                std::memset(off, 0xff, sizeof off);
                int n_take = -1;
                const int used = mcpt::refill_window(m.v0, m.v1, n_have, W, off, &n_take);
                const int want_take = (int)rays.size() < n_have ? (int)rays.size() : n_have;
                const int want_used = (int)rays.size() <= n_have ? W : rays[n_have - 1] + 1;
                bool ok = n_take == want_take && used == want_used && used >= 1 && used <= W;
                for (int r = 0; ok && r < want_take; r++) ok = off[r] == rays[r];            // strictly increasing valid slots, none left out
                for (int r = want_take; ok && r < 64; r++) ok = off[r] == 0xff;             // nothing written beyond them
                // no ray below `used` is left out, none at or above it is taken
                int below = 0;
                for (int o : rays) below += o < used;
                ok = ok && below == want_take;
                if (!ok) {
                    std::printf("window: W %d n_have %d masks %016llx %016llx: used %d (want %d), n_take %d (want %d)\n", W, n_have,
                                (unsigned long long)m.v0, (unsigned long long)m.v1, used, want_used, n_take, want_take);
                    return 1;
                }
                cases++;
            }
        }
    }
    std::printf("ok window %lld cases\n", cases);
    return 0;
}

int check_div(long long stride)
{
    const unsigned int spps[] = {1, 2, 3, 4, 5, 7, 16, 63, 64, 65, 100, 192, 255, 256, 257, 1000, 4096, 65535, 65536, 65537, 1000003, 0x40000000u, 0x7fffffffu};
    const unsigned int full[] = {1, 3, 64, 192, 256};
    const unsigned int top = 0x7fffffffu;
    long long n_checked = 0;
    auto one = [&](unsigned int id, unsigned int d, const mcpt::DivMagic& dm) {
        const unsigned int q = mcpt::div_by_magic(id, dm.mul, dm.shift);
        if (q != id / d) { std::printf("div: %u / %u = %u, multiply-shift gives %u (mul %u shift %d)\n", id, d, id / d, q, dm.mul, dm.shift); return false; }
        n_checked++;
        return true;
    };
    for (unsigned int d : spps) {
        const mcpt::DivMagic dm = mcpt::div_magic(d);
        if (dm.shift < 31 || dm.shift > 62) { std::printf("div: shift %d for %u\n", dm.shift, d); return 1; }
        // around the first and the last multiples of d in the range, and the ends of the range
        for (unsigned int k = 0; k < 2000; k++) {
            const unsigned long long lo = (unsigned long long)k * d, hi = (unsigned long long)(top / d - (k < top / d ? k : 0)) * d;
            for (int e = -2; e <= 2; e++) {
                const long long a = (long long)lo + e, b = (long long)hi + e;
                if (a >= 0 && a <= (long long)top && !one((unsigned int)a, d, dm)) return 1;
                if (b >= 0 && b <= (long long)top && !one((unsigned int)b, d, dm)) return 1;
            }
        }
        if (!one(0u, d, dm) || !one(top, d, dm)) return 1;
    }
    for (unsigned int d : full) {
        const mcpt::DivMagic dm = mcpt::div_magic(d);
        for (unsigned long long id = 0; id <= top; id += (unsigned long long)stride)
            if (!one((unsigned int)id, d, dm)) return 1;
    }
    std::printf("ok div %lld quotients, stride %lld\n", n_checked, stride);
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc >= 2 && !std::strcmp(argv[1], "window")) return check_window();
    if (argc >= 3 && !std::strcmp(argv[1], "div")) { const long long s = std::atoll(argv[2]); return s >= 1 ? check_div(s) : 2; }
    std::printf("usage: refill_window_main window | div <stride>\n");
    return 2;
}
