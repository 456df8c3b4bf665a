// Stand-alone check of csrc/pre_test.hpp (the trace engines' conservative fp32 pre-test of a leaf triangle, branch-free) against the
// short-circuit form it replaced, which is kept here verbatim as the model.  For every input the two must return the same bool and
// write the same eight debug words, bit for bit (a NaN word: NaN in both).  Build with -ffp-contract=off (tests/test_pre_test_cpu.py does).
//
//   pre_test random [n]   n (default 1 200 000) seeded tuples (record, ray, limit, margin) around cornell-box's extents
//   pre_test edges        the hand-made inputs: pre-test off, det = 0 and denormal, ray out of range, limit = +inf and 0, a NaN in every
//                         input position, a triangle seen edge-on, every comparison at, just below and just above its bound
// Prints "ok <mode> <cases> <rejected>" and returns 0, or the first difference and 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <string>

#include "pre_test.hpp"

using mcpt::PreRay;
using mcpt::PreRec;

// ---- the model: tri_pre_reject as it stood before the branch-free form (its float4 loads spelled as a struct of the same words)
struct F4 { float x, y, z, w; };
static bool model_pre_reject(const F4 w[3], const PreRay& R, float limit_f, float* dbg = nullptr)
{
    const F4 A = w[0], B = w[1], C = w[2];             // v0 a1 | e1 a2 | e2 -
    const float a1 = A.w, a2 = B.w;
    const float tx = R.o[0] - A.x, ty = R.o[1] - A.y, tz = R.o[2] - A.z;
    const float px = fmaf(R.d[1], C.z, -(R.d[2] * C.y)), py = fmaf(R.d[2], C.x, -(R.d[0] * C.z)), pz = fmaf(R.d[0], C.y, -(R.d[1] * C.x));
    const float det = fmaf(B.z, pz, fmaf(B.y, py, B.x * px));
    const float u = fmaf(tz, pz, fmaf(ty, py, tx * px));
    const float qx = fmaf(ty, B.z, -(tz * B.y)), qy = fmaf(tz, B.x, -(tx * B.z)), qz = fmaf(tx, B.y, -(ty * B.x));
    const float v = fmaf(R.d[2], qz, fmaf(R.d[1], qy, R.d[0] * qx));
    const float tq = fmaf(C.z, qz, fmaf(C.y, qy, C.x * qx));
    const float T = fmaxf(fmaxf(fabsf(tx), fabsf(ty)), fabsf(tz));
    const float base = fmaf(T, 0x1p-18f, R.eta4);
    const float da1 = R.dm * a1, da2 = R.dm * a2;
    const float Eu = da2 * base, Ev = da1 * base, X = da2 * a1, Etq = (a1 * a2) * base;
    const float Dt = fabsf(det);
    const bool neg = det < 0.0f;
    const float U = neg ? -u : u, V = neg ? -v : v, TQ = neg ? -tq : tq;
    const bool clear = Dt > 0x1p-9f * X;                    // (i); false as well when a1 = +inf or anything is NaN
    bool rej = U < -Eu || V < -Ev || (U + V) - Dt > (Eu + Ev) + 0x1p-19f * X;
    rej = rej || TQ + Etq < -((R.margin * Dt) * 1.002f) || TQ - Etq > (limit_f * Dt) * 1.002f;
    if (dbg) { dbg[0] = U + Eu; dbg[1] = V + Ev; dbg[2] = ((Eu + Ev) + 0x1p-19f * X) - ((U + V) - Dt); dbg[3] = TQ + Etq + (R.margin * Dt) * 1.002f;
               dbg[4] = (limit_f * Dt) * 1.002f - (TQ - Etq); dbg[5] = Dt - 0x1p-9f * X; dbg[6] = TQ / Dt; dbg[7] = Dt; }
    return clear && rej;
}

// ---- one input as 22 floats, so that "every input position" is a loop: record 0..10, ray o 11..13, d 14..16, dm 17, eta4 18, margin 19, limit 20
enum { kV0 = 0, kA1 = 3, kE1 = 4, kA2 = 7, kE2 = 8, kO = 11, kD = 14, kDm = 17, kEta4 = 18, kMargin = 19, kLimit = 20, kWords = 21 };
struct Input { float f[kWords]; };

static long long g_cases = 0, g_rejected = 0;

static bool check(const Input& in, const char* what)
{
    const float* f = in.f;
    const F4 w[3] = {{f[0], f[1], f[2], f[3]}, {f[4], f[5], f[6], f[7]}, {f[8], f[9], f[10], 0.0f}};
    const PreRec rec{{f[0], f[1], f[2]}, f[3], {f[4], f[5], f[6]}, f[7], {f[8], f[9], f[10]}};
    PreRay R;
    for (int i = 0; i < 3; i++) { R.o[i] = f[kO + i]; R.d[i] = f[kD + i]; }
    R.dm = f[kDm]; R.eta4 = f[kEta4]; R.margin = f[kMargin];
    float dm[8], dn[8];
    const bool m = model_pre_reject(w, R, f[kLimit], dm);
    const bool n = mcpt::pre_reject(rec, R, f[kLimit], dn);
    const bool n_plain = mcpt::pre_reject(rec, R, f[kLimit]);
    g_cases++;
    g_rejected += m;
    // bit for bit -- but where a word is NaN in both, its sign and payload are not compared: IEEE 754 leaves those of an operation's
    // result open, and the host compiler is free to commute the operands of an addition, which on x86 decides whose NaN comes out
    bool same = m == n && n == n_plain;
    for (int i = 0; i < 8; i++) same = same && (std::memcmp(&dm[i], &dn[i], sizeof(float)) == 0 || (std::isnan(dm[i]) && std::isnan(dn[i])));
    if (same) return true;
    std::printf("DIFFERENT (%s): model %d, header %d (without dbg %d)\n input:", what, (int)m, (int)n, (int)n_plain);
    for (int i = 0; i < kWords; i++) std::printf(" %a", f[i]);
    std::printf("\n dbg model :");
    for (float x : dm) std::printf(" %a", x);
    std::printf("\n dbg header:");
    for (float x : dn) std::printf(" %a", x);
    std::printf("\n");
    return false;
}

// the ray words make_pre_ray (trace_fast.hpp) derives: dm, eta4 from the origin and the scene's extent S
static void derive(Input& in, float S)
{
    float* f = in.f;
    f[kDm] = fmaxf(fmaxf(fabsf(f[kD]), fabsf(f[kD + 1])), fabsf(f[kD + 2]));
    const float omax = fmaxf(fmaxf(fabsf(f[kO]), fabsf(f[kO + 1])), fabsf(f[kO + 2]));
    const bool in_range = omax <= 4.0f * S && S >= 1e-6f && S <= 1e6f && f[kDm] >= 1e-6f && f[kDm] <= 1e6f;
    f[kEta4] = in_range ? 0x1p-20f * (omax + S) * 1.0001f : std::numeric_limits<float>::infinity();
}

static int run_random(long long n)
{
    std::mt19937_64 rng(20240611);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::normal_distribution<double> N(0.0, 1.0);
    const double lo[3] = {-1.0, 0.0, -1.0}, hi[3] = {1.0, 2.0, 1.0};       // cornell-box
    const float S = 2.0f, inf = std::numeric_limits<float>::infinity();
    for (long long i = 0; i < n; i++) {
        Input in;
        double v[3][3], o[3], d[3];
        const double len = std::pow(10.0, -2.5 + 2.8 * U(rng));              // edges of 0.003 .. 2
        for (int a = 0; a < 3; a++) {
            v[0][a] = lo[a] + (hi[a] - lo[a]) * U(rng);
            v[1][a] = v[0][a] + len * N(rng);
            v[2][a] = v[0][a] + len * N(rng);
            o[a] = lo[a] + (hi[a] - lo[a]) * U(rng);
        }
        if (i % 3 == 0) {
            for (int a = 0; a < 3; a++) d[a] = N(rng);
        } else {                                                             // aimed at the triangle's plane, weights in [-0.1, 1.1]
            const double b = -0.1 + 1.2 * U(rng), c = -0.1 + 1.2 * U(rng);
            for (int a = 0; a < 3; a++) d[a] = v[0][a] + b * (v[1][a] - v[0][a]) + c * (v[2][a] - v[0][a]) - o[a];
            if (i % 16 == 1) for (int a = 0; a < 3; a++) d[a] = -d[a];        // ... or away from it
        }
        const double dl = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        double s1 = 0, s2 = 0;
        for (int a = 0; a < 3; a++) {
            in.f[kV0 + a] = (float)v[0][a];
            in.f[kE1 + a] = (float)(v[1][a] - v[0][a]);
            in.f[kE2 + a] = (float)(v[2][a] - v[0][a]);
            in.f[kO + a] = (float)o[a];
            in.f[kD + a] = (float)(d[a] / dl);
            s1 += std::fabs(v[1][a] - v[0][a]); s2 += std::fabs(v[2][a] - v[0][a]);
        }
        in.f[kA1] = std::nextafter((float)(s1 * (1 + 0x1p-20)), inf);
        in.f[kA2] = std::nextafter((float)(s2 * (1 + 0x1p-20)), inf);
        if (i % 97 == 0) in.f[kA1] = inf;
        derive(in, S);
        const double rmax = 1.0 / std::fmin(std::fmin(std::fabs(in.f[kD]), std::fabs(in.f[kD + 1])), std::fabs(in.f[kD + 2]));
        in.f[kMargin] = rmax <= 1e6 ? (float)(1.0000001e-9 * 2.0 * rmax) : inf;
        // the limit: none, or around the distance to the triangle's first vertex
        double dist = 0;
        for (int a = 0; a < 3; a++) dist += (v[0][a] - o[a]) * (v[0][a] - o[a]);
        in.f[kLimit] = i % 2 == 0 ? inf : (float)(std::sqrt(dist) * (0.5 + U(rng)));
        if (!check(in, "random")) return 1;
    }
    std::printf("ok random %lld %lld\n", g_cases, g_rejected);
    return g_rejected > g_cases / 10 && g_rejected < g_cases - g_cases / 10 ? 0 : 1;       // both answers occur, often
}

// A triangle and a ray whose intermediate values are small integers times powers of two: v0 = 0, e1 = x, e2 = y, a1 = a2 = 1, a ray
// along -z from (ox, oy, oz).  Then det = 1 (= -d.z), u = ox, v = oy, tq = oz, T = max |o_i|, X = 1, and with eta4 = 2^-10 - 2^-18 and
// T = 1 the error terms are Eu = Ev = Etq = 2^-10 exactly: every comparison can be put on its bound by hand.
static Input unit_case(float ox, float oy, float oz)
{
    Input in = {};
    in.f[kE1] = 1.0f; in.f[kE2 + 1] = 1.0f; in.f[kA1] = 1.0f; in.f[kA2] = 1.0f;
    in.f[kO] = ox; in.f[kO + 1] = oy; in.f[kO + 2] = oz;
    in.f[kD + 2] = -1.0f; in.f[kDm] = 1.0f;
    in.f[kEta4] = 0x1p-10f - 0x1p-18f;
    in.f[kMargin] = 0.0f;
    in.f[kLimit] = std::numeric_limits<float>::infinity();
    return in;
}

// input word `at` moved through the 2 * span + 1 floats around its value
static bool sweep(Input in, int at, int span, const char* what, int* flips)
{
    float x = in.f[at];
    for (int i = 0; i < span; i++) x = std::nextafter(x, -std::numeric_limits<float>::infinity());
    bool first = true, last = false;
    for (int i = 0; i <= 2 * span; i++) {
        in.f[at] = x;
        const long long before = g_rejected;
        if (!check(in, what)) return false;
        const bool r = g_rejected != before;
        if (!first && r != last) (*flips)++;
        first = false; last = r;
        x = std::nextafter(x, std::numeric_limits<float>::infinity());
    }
    return true;
}

static int run_edges()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float E = 0x1p-10f;
    // inside the triangle, in front: nothing rejects
    const Input inside = unit_case(0.25f, 0.25f, 1.0f);
    // clearly outside (u < 0): rejected by the first comparison alone, ... by the second, the third, behind, beyond
    const Input out1 = unit_case(-0.5f, 0.25f, 1.0f), out2 = unit_case(0.25f, -0.5f, 1.0f), out3 = unit_case(1.0f, 1.0f, 1.0f);
    const Input behind = unit_case(0.25f, 0.25f, -1.0f);
    Input beyond = unit_case(0.25f, 0.25f, 1.0f);
    beyond.f[kLimit] = 0.5f;
    const Input bases[] = {inside, out1, out2, out3, behind, beyond};
    const char* names[] = {"inside", "u<0", "v<0", "u+v>1", "behind", "beyond"};
    long long want_rej = 0;
    for (int b = 0; b < 6; b++) {
        if (!check(bases[b], names[b])) return 1;
        want_rej += b > 0;
    }
    if (g_rejected != want_rej) { std::printf("the hand-made cases are not what they say: %lld of 5 rejected\n", g_rejected); return 1; }

    for (int b = 0; b < 6; b++) {
        Input in = bases[b];
        // pre-test off; ray out of range; no limit, limit 0
        in.f[kA1] = inf; if (!check(in, "a1 = +inf")) return 1;
        in = bases[b]; in.f[kEta4] = inf; if (!check(in, "eta4 = +inf")) return 1;
        in = bases[b]; in.f[kLimit] = inf; if (!check(in, "limit = +inf")) return 1;
        in = bases[b]; in.f[kLimit] = 0.0f; if (!check(in, "limit = 0")) return 1;
        in = bases[b]; in.f[kMargin] = inf; if (!check(in, "margin = +inf")) return 1;
        // det = 0 and +-denormal (det = -d.z here), with the ray along x
        const float dets[] = {0.0f, -0.0f, 1e-42f, -1e-42f, std::numeric_limits<float>::denorm_min(), -std::numeric_limits<float>::denorm_min(),
                              std::numeric_limits<float>::min(), -std::numeric_limits<float>::min()};
        for (float dz : dets) {
            in = bases[b]; in.f[kD] = 1.0f; in.f[kD + 2] = dz;
            if (!check(in, "det = 0 or denormal")) return 1;
        }
        // NaN, and the infinities, in every input position, one at a time
        for (int at = 0; at < kWords; at++)
            for (float bad : {nan, -nan, inf, -inf}) {
                in = bases[b]; in.f[at] = bad;
                if (!check(in, "NaN or inf in one position")) return 1;
            }
    }
    const long long before_sweeps = g_rejected;
    int flips = 0;
    // edge-on: d = (1, 0, dz), dm = 1, X = 1, |det| = |dz| around 2^-9: `clear` turns true just above it (u < 0 otherwise rejects)
    for (float sign : {1.0f, -1.0f}) {
        Input in = out1;
        in.f[kD] = 1.0f; in.f[kD + 2] = sign * 0x1p-9f;
        const int f0 = flips;
        if (!sweep(in, kD + 2, 40, "edge-on, |det| around 2^-9 X", &flips)) return 1;
        if (flips != f0 + 1) { std::printf("edge-on sweep: %d changes of the answer, not 1\n", flips - f0); return 1; }
    }
    // each comparison on its bound (T = 1 in all of them: one coordinate of the origin is +-1)
    struct { Input in; int at; const char* what; } bounds[] = {
        {unit_case(-E, 0.0f, 1.0f), kO, "U = -Eu"},
        {unit_case(0.0f, -E, 1.0f), kO + 1, "V = -Ev"},
        {unit_case(0.5f, 0.5f + 0x1p-9f + 0x1p-19f, 1.0f), kO + 1, "U + V - Dt = Eu + Ev + 2^-19 X"},
        {unit_case(1.0f, 0.0f, -E), kO + 2, "TQ + Etq = 0 (margin 0)"},
        {unit_case(1.0f, 0.0f, 0.5f + E), kO + 2, "TQ - Etq = limit (limit 0.5 / 1.002)"},
    };
    bounds[4].in.f[kLimit] = 0.5f / 1.002f;
    for (auto& b : bounds) {
        const int f0 = flips;
        if (!sweep(b.in, b.at, 40, b.what, &flips)) return 1;
        if (flips != f0 + 1) { std::printf("%s: %d changes of the answer in the sweep, not 1\n", b.what, flips - f0); return 1; }
        // the same with the triangle's edges exchanged (det = -1: u, v, tq change sign before they are compared, U = o.y, V = o.x)
        Input m = b.in;
        for (int k = 0; k < 3; k++) { const float t = m.f[kE1 + k]; m.f[kE1 + k] = m.f[kE2 + k]; m.f[kE2 + k] = t; }
        { const float t = m.f[kO]; m.f[kO] = m.f[kO + 1]; m.f[kO + 1] = t; }
        const int at = b.at == kO ? kO + 1 : b.at == kO + 1 ? kO : b.at;
        const int f1 = flips;
        if (!sweep(m, at, 40, b.what, &flips)) return 1;
        if (flips != f1 + 1) { std::printf("%s, edges exchanged: %d changes of the answer in the sweep, not 1\n", b.what, flips - f1); return 1; }
    }
    // the limit and the margin through their own bounds
    {
        Input in = unit_case(1.0f, 0.0f, 0.75f);
        in.f[kLimit] = (0.75f - E) / 1.002f;
        const int f0 = flips;
        if (!sweep(in, kLimit, 40, "limit around (TQ - Etq) / 1.002", &flips)) return 1;
        if (flips != f0 + 1) { std::printf("limit sweep: %d changes, not 1\n", flips - f0); return 1; }
        in = unit_case(1.0f, 0.0f, -0.75f);
        in.f[kMargin] = (0.75f - E) / 1.002f;
        const int f1 = flips;
        if (!sweep(in, kMargin, 40, "margin around -(TQ + Etq) / 1.002", &flips)) return 1;
        if (flips != f1 + 1) { std::printf("margin sweep: %d changes, not 1\n", flips - f1); return 1; }
    }
    if (g_rejected == before_sweeps) { std::printf("no sweep rejected anything\n"); return 1; }
    std::printf("ok edges %lld %lld\n", g_cases, g_rejected);
    return 0;
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "random") return run_random(argc > 2 ? std::atoll(argv[2]) : 1200000);
    if (mode == "edges") return run_edges();
    std::fprintf(stderr, "usage: pre_test random [n] | edges\n");
    return 2;
}
