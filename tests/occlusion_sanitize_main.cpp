// Stand-alone program around csrc/occlusion.hpp for tests/test_occlusion_cpu.py, built there with -fsanitize=address,undefined: the fold
// of one entry on the values a caller can get wrong -- NaN, infinities, +-1e300, 1e-300, zero normals.  Every array is a heap array
// exactly as large as its size says: a read outside it is an error the sanitizer reports.
// stdin, one entry per line: falloff max_distance  nx ny nz  dx dy dz  t hit  fx fy fz
//   the entry's normal n and three samples: (d, t, hit, f), (-d, t, hit, f) and (d, t / 2, hit, f), f the hit face's normal.
// stdout, one line each: ao, stderr and the bent normal as hex floats, hits and back.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "occlusion.hpp"

int main()
{
    char s[12][64];
    int falloff, hit;
    while (std::scanf("%d %63s %63s %63s %63s %63s %63s %63s %63s %d %63s %63s %63s", &falloff, s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], &hit, s[8], s[9],
                      s[10]) == 13) {
        if (falloff < 0 || falloff > 2) return 2;
        double v[11];
        for (int i = 0; i < 11; i++) v[i] = std::strtod(s[i], nullptr);
        const int spp = 3;
        const std::vector<double> nrm{v[1], v[2], v[3]};
        std::vector<double> d(spp * 3), t(spp), f(spp * 3);
        for (int k = 0; k < spp; k++) {
            for (int c = 0; c < 3; c++) {
                d[k * 3 + c] = k == 1 ? -v[4 + c] : v[4 + c];
                f[k * 3 + c] = v[8 + c];
            }
            t[k] = k == 2 ? v[7] / 2.0 : v[7];
        }
        mcpt::OccSums a;
        mcpt::occlusion_clear(a);
        for (int k = 0; k < spp; k++) mcpt::occlusion_add(a, mcpt::occlusion_sample(falloff, v[0], d.data() + k * 3, hit != 0, t[k], f.data() + k * 3));
        std::vector<double> bent(3);
        mcpt::occlusion_bent(a.b, nrm.data(), bent.data());
        std::printf("%a %a %a %a %a %d %d\n", a.s1 / spp, mcpt::occlusion_stderr(a.s1, a.s2, spp), bent[0], bent[1], bent[2], a.hits, a.back);
    }
    return 0;
}
