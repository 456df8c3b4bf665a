// Stand-alone program around the host-compiled parts of csrc/direct.hpp for tests/test_direct_cpu.py, built there with
// -fsanitize=address,undefined: direct_prepare, direct_normal and direct_slot on the values a caller can get wrong, and the fold into heap
// arrays exactly as large as their sizes say (n * 3, n * nl * 3, n * nl): a read or write outside them is an error the sanitizer reports.
// stdin, a sequence of records:
//   slot type flags  px py pz  dx dy dz  ux uy uz  vx vy vz  cos_inner cos_outer range  ax ay az  bx by bz  bias xi1 xi2
//        -> one line: o, d, tmax, g as hex floats
//   fold n spp nl, then nl times "type flags cr cg cb", then n * R times "g occluded"
//        -> n lines: E[3] stderr[3] per_light[nl][3] visibility[nl] as hex floats
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "direct.hpp"

static bool number(double& v)
{
    char s[64];
    if (std::scanf("%63s", s) != 1) return false;
    v = std::strtod(s, nullptr);
    return true;
}

static int do_slot()
{
    double v[26];
    for (double& x : v)
        if (!number(x)) return 2;
    mcpt_direct_light L;
    std::memset(&L, 0, sizeof L);
    L.type = int32_t(v[0]); L.flags = int32_t(v[1]);
    for (int c = 0; c < 3; c++) { L.position[c] = v[2 + c]; L.direction[c] = v[5 + c]; L.u[c] = v[8 + c]; L.v[c] = v[11 + c]; L.color[c] = 1.0; }
    L.cos_inner = v[14]; L.cos_outer = v[15]; L.range = v[16];
    const std::vector<double> a{v[17], v[18], v[19]}, b{v[20], v[21], v[22]};
    std::vector<double> nh(3);
    const mcpt::DirectLight D = mcpt::direct_prepare(L);
    mcpt::direct_normal(b.data(), nh.data());
    const mcpt::DirectSlot s = mcpt::direct_slot(D, a.data(), nh.data(), v[23], v[24], v[25]);
    std::printf("%a %a %a %a %a %a %a %a\n", s.o[0], s.o[1], s.o[2], s.d[0], s.d[1], s.d[2], s.tmax, s.g);
    return 0;
}

static int do_fold()
{
    double hn, hspp, hnl;
    if (!number(hn) || !number(hspp) || !number(hnl)) return 2;
    const int64_t n = int64_t(hn);
    const int32_t spp = int32_t(hspp), nl = int32_t(hnl);
    std::vector<mcpt::DirectLight> lights;
    int64_t R = 0;
    for (int32_t l = 0; l < nl; l++) {
        double t, f, c[3];
        if (!number(t) || !number(f) || !number(c[0]) || !number(c[1]) || !number(c[2])) return 2;
        mcpt::DirectLight D;
        std::memset(&D, 0, sizeof D);
        D.type = int32_t(t); D.flags = int32_t(f);
        D.color[0] = c[0]; D.color[1] = c[1]; D.color[2] = c[2];
        lights.push_back(D);
        R += mcpt::direct_light_slots(D.type, spp);
    }
    std::vector<double> g(size_t(n * R));
    std::vector<uint8_t> occ(size_t(n * R));
    for (int64_t k = 0; k < n * R; k++) {
        double o;
        if (!number(g[size_t(k)]) || !number(o)) return 2;
        occ[size_t(k)] = o != 0.0;
    }
    std::vector<double> E(size_t(n * 3)), err(size_t(n * 3)), pl(size_t(n * nl * 3)), vis(size_t(n * nl));
    for (int64_t i = 0; i < n; i++) {
        mcpt::DirectFold f;
        f.begin();
        int64_t at = i * R;
        for (int32_t l = 0; l < nl; l++) {
            const mcpt::DirectLight& D = lights[size_t(l)];
            f.light_begin();
            for (int32_t j = 0; j < mcpt::direct_light_slots(D.type, spp); j++, at++) f.add(D, g[size_t(at)], occ[size_t(at)] != 0);
            f.light_end(D, spp);
            for (int c = 0; c < 3; c++) pl[size_t((i * nl + l) * 3 + c)] = f.El[c];
            vis[size_t(i * nl + l)] = f.vis;
        }
        if (at != (i + 1) * R) return 3;
        for (int c = 0; c < 3; c++) { E[size_t(i * 3 + c)] = f.E[c]; err[size_t(i * 3 + c)] = std::sqrt(f.V[c]); }
    }
    for (int64_t i = 0; i < n; i++) {
        for (int c = 0; c < 3; c++) std::printf("%a ", E[size_t(i * 3 + c)]);
        for (int c = 0; c < 3; c++) std::printf("%a ", err[size_t(i * 3 + c)]);
        for (int64_t k = 0; k < int64_t(nl) * 3; k++) std::printf("%a ", pl[size_t(i * nl * 3 + k)]);
        for (int32_t l = 0; l < nl; l++) std::printf("%a ", vis[size_t(i * nl + l)]);
        std::printf("\n");
    }
    return 0;
}

int main()
{
    char word[16];
    while (std::scanf("%15s", word) == 1) {
        int rc = 1;
        if (!std::strcmp(word, "slot")) rc = do_slot();
        else if (!std::strcmp(word, "fold")) rc = do_fold();
        if (rc) {
            std::fprintf(stderr, "record '%s' failed: %d\n", word, rc);
            return rc;
        }
    }
    return 0;
}
