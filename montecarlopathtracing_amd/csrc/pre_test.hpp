// The arithmetic of the conservative fp32 pre-test of a leaf triangle (trace_fast.hpp derives it and its error budget; tri_pre_reject
// there loads a record and calls this).
//
// pre_reject() evaluates the five rejection comparisons and `clear` unconditionally and combines them with | and &: no branch stands
// between two triangles of a round, so the records of a round can be requested together (trace_persistent.hpp: leaf_survivors), and a
// wave in which one lane still needs the later comparisons -- nearly every wave -- pays no mask bookkeeping for the others.  The truth
// value is that of the short-circuit form  clear && (c1 || c2 || c3 || c4 || c5)  for every input: each c_k is a comparison of values
// computed by IEEE operations that neither trap nor have any other effect, so evaluating one that || would have skipped changes nothing
// but time, and on bools a | b == a || b, a & b == a && b.  A NaN operand makes its comparison false in both forms (only <, > are
// used, never their negations), and `clear` is false when a1 = +inf or anything that reaches it is NaN.
//
// Pure, and compiled by the host compiler too (tests/test_pre_test_cpu.py holds it to the short-circuit form, input for input).  The
// operations, their operands and their order are fixed: fmaf is one rounding on both sides, nothing else may be contracted
// (-ffp-contract=off).
#pragma once

#include <math.h>

namespace mcpt {

#ifdef __HIPCC__
#define MCPT_PRE_FN __host__ __device__ __forceinline__
#else
#define MCPT_PRE_FN inline
#endif

struct PreRay { float o[3], d[3], dm, eta4, margin; };
// the record of a triangle as three 16-byte words (device_scene.hpp: DTriPre): v0 a1 | e1 a2 | e2 -
struct PreRec { float v0[3], a1, e1[3], a2, e2[3]; };

// true: the triangle cannot become the closest hit.  dbg (self-check builds): the margins of the six comparisons, t and |det|.
MCPT_PRE_FN bool pre_reject(const PreRec& q, const PreRay& R, float limit_f, float* dbg = nullptr)
{
    const float a1 = q.a1, a2 = q.a2;
    const float tx = R.o[0] - q.v0[0], ty = R.o[1] - q.v0[1], tz = R.o[2] - q.v0[2];
    const float px = fmaf(R.d[1], q.e2[2], -(R.d[2] * q.e2[1])), py = fmaf(R.d[2], q.e2[0], -(R.d[0] * q.e2[2])),
                pz = fmaf(R.d[0], q.e2[1], -(R.d[1] * q.e2[0]));
    const float det = fmaf(q.e1[2], pz, fmaf(q.e1[1], py, q.e1[0] * px));
    const float u = fmaf(tz, pz, fmaf(ty, py, tx * px));
    const float qx = fmaf(ty, q.e1[2], -(tz * q.e1[1])), qy = fmaf(tz, q.e1[0], -(tx * q.e1[2])), qz = fmaf(tx, q.e1[1], -(ty * q.e1[0]));
    const float v = fmaf(R.d[2], qz, fmaf(R.d[1], qy, R.d[0] * qx));
    const float tq = fmaf(q.e2[2], qz, fmaf(q.e2[1], qy, q.e2[0] * qx));
    const float T = fmaxf(fmaxf(fabsf(tx), fabsf(ty)), fabsf(tz));
    const float base = fmaf(T, 0x1p-18f, R.eta4);
    const float da1 = R.dm * a1, da2 = R.dm * a2;
    const float Eu = da2 * base, Ev = da1 * base, X = da2 * a1, Etq = (a1 * a2) * base;
    const float Dt = fabsf(det);
    const bool neg = det < 0.0f;
    const float U = neg ? -u : u, V = neg ? -v : v, TQ = neg ? -tq : tq;
    const bool clear = Dt > 0x1p-9f * X;                    // (i); false as well when a1 = +inf or anything is NaN
    const bool c1 = U < -Eu, c2 = V < -Ev, c3 = (U + V) - Dt > (Eu + Ev) + 0x1p-19f * X;
    const bool c4 = TQ + Etq < -((R.margin * Dt) * 1.002f), c5 = TQ - Etq > (limit_f * Dt) * 1.002f;
    if (dbg) { dbg[0] = U + Eu; dbg[1] = V + Ev; dbg[2] = ((Eu + Ev) + 0x1p-19f * X) - ((U + V) - Dt); dbg[3] = TQ + Etq + (R.margin * Dt) * 1.002f;
               dbg[4] = (limit_f * Dt) * 1.002f - (TQ - Etq); dbg[5] = Dt - 0x1p-9f * X; dbg[6] = TQ / Dt; dbg[7] = Dt; }
    return clear & (c1 | c2 | c3 | c4 | c5);
}

#undef MCPT_PRE_FN

}  // namespace mcpt
