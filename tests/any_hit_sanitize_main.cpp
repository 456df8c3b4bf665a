// Stand-alone program around the host-compiled parts of csrc/any_hit.hpp for tests/test_any_hit_cpu.py, built there with
// -fsanitize=address,undefined: pair_ray on the values a caller can get wrong, and the word and bit indexing of the packed matrix at the
// count bounds.  Every array is a heap array exactly as large as its size says: a read or write outside it is an error the sanitizer
// reports; an index computed past its bound, or a shift past 63, is reported or fails the program's own checks.
// stdin, one pair per line: t0 t1  ax ay az  bx by bz      stdout, one line each: o, d and tmax as hex floats.
// After the pairs: the indexing checks (exit status 3 when one fails), then a small matrix packed through the helpers and printed as hex.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "any_hit.hpp"

static int check_indexing()
{
    using namespace mcpt;
    const int64_t M = kPairCountMax;
    // the row lengths of the tests and the bounds: words a row, the last column's word and bit, the masks
    const int64_t nbs[] = {1, 3, 63, 64, 65, 129, 257, M - 1, M};
    for (const int64_t nb : nbs) {
        const int64_t W = pair_row_words(nb);
        if (W != (nb + 63) / 64 || W < 1 || W > (int64_t(1) << 25)) return 1;
        const int64_t last = nb - 1;
        if (pair_word_index(0, W, last) != W - 1) return 2;
        if (pair_bit(last) != uint64_t(1) << (last % 64)) return 3;
        uint64_t all = 0;
        for (int64_t j = (W - 1) * 64; j < nb; j++) all |= pair_bit(j);
        if (pair_word_mask(nb, W - 1) != all) return 4;
        if (W > 1 && pair_word_mask(nb, 0) != ~uint64_t(0)) return 5;
        if (pair_word_mask(nb, W) != 0) return 6;
    }
    // na * W = 2^31 - 1 without allocating: 2^31 - 1 rows of one word, and one row short of the bound with two words a row refused
    if (!pair_words_ok(M, 1) || !pair_words_ok(M, 64) || pair_words_ok(M, 65)) return 7;
    if (pair_word_index(M - 1, 1, 63) != M - 1) return 8;
    if (!pair_words_ok(1, M) || pair_row_words(M) != (int64_t(1) << 25)) return 9;
    if (!pair_words_ok(63, M) || pair_words_ok(64, M)) return 10;                 // 63 * 2^25 < 2^31 - 1 < 64 * 2^25
    if (pair_word_index(62, pair_row_words(M), M - 1) != 63 * (int64_t(1) << 25) - 1) return 11;
    if (pair_words_ok(M, M)) return 12;                                            // (2^31 - 1) * 2^25: no overflow, refused
    if (!pair_words_ok(0, M) || !pair_words_ok(M, 0) || pair_row_words(0) != 0) return 13;
    return 0;
}

int main()
{
    char s[8][64];
    while (std::scanf("%63s %63s %63s %63s %63s %63s %63s %63s", s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7]) == 8) {
        double v[8];
        for (int i = 0; i < 8; i++) v[i] = std::strtod(s[i], nullptr);
        const std::vector<double> a{v[2], v[3], v[4]}, b{v[5], v[6], v[7]};
        const mcpt::PairRay r = mcpt::pair_ray(a.data(), b.data(), v[0], v[1]);
        std::printf("%a %a %a %a %a %a %a\n", r.o[0], r.o[1], r.o[2], r.d[0], r.d[1], r.d[2], r.tmax);
    }
    if (const int bad = check_indexing()) {
        std::fprintf(stderr, "indexing check %d failed\n", bad);
        return 3;
    }
    // a 5 x 65 matrix whose pair (i, j) is set when (i + j) % 3 == 0, in an array of exactly na * W words
    const int64_t na = 5, nb = 65, W = mcpt::pair_row_words(nb);
    std::vector<uint64_t> bits(size_t(na * W), 0);
    for (int64_t i = 0; i < na; i++)
        for (int64_t j = 0; j < nb; j++)
            if ((i + j) % 3 == 0) bits[size_t(mcpt::pair_word_index(i, W, j))] |= mcpt::pair_bit(j);
    for (int64_t i = 0; i < na; i++)
        for (int64_t w = 0; w < W; w++)
            if (bits[size_t(i * W + w)] & ~mcpt::pair_word_mask(nb, w)) return 4;
    std::printf("matrix");
    for (const uint64_t w : bits) std::printf(" %llx", (unsigned long long)w);
    std::printf("\n");
    return 0;
}
