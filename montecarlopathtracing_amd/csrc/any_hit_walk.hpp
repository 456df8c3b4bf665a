// Any-hit rays (mcpt.h: any-hit rays): the walk that answers one ray per lane (any_lane_fast), built from the closest-hit engines' own
// pieces, unchanged (trace_fast.hpp: fast_rcp, make_rayf, cw_step, own_box_hit; dev_common.hpp: tri_hit, trace_closest).  Device code.
// fp64 at the leaves, no contraction (-ffp-contract=off).
//
// THE RULE.  A ray with limit tmax is occluded iff mcpt_trace_closest of the same ray on the same device state answers face >= 0 and
// t < tmax (IEEE: a NaN limit is never occluded).  The closest hit is the minimum of t_k over the accepted candidates, each with t_k > 0,
// so this is: there EXISTS a leaf k whose own box passes the reference's slab test (own_box_hit), whose triangle test passes (tri_hit),
// and whose t_k = (p.x - o.x) / d.x has t_k > 0 and t_k < tmax.  No ordering between candidates is involved: the walk stops at the first.
//
// Why the early exit is exact.  trace_fast.hpp's contract carries over with the fixed tmax in the place of the moving best_t:
//   * inner nodes are culled conservatively on the compressed 4-wide hierarchy (cw_step): a box the reference would accept is never
//     rejected for its position, and by monotonicity no leaf below it is lost;
//   * by distance a box is pruned only when the lower bound of its entry lies beyond limit = tmax + margin, margin = 1e-9 * scale /
//     min|d_k| (>= 1e6 times the rounding error of t_k relative to the slab entry; +inf, so no pruning at all, when min|d_k| < 1e-6).
//     Every leaf k below such a box has t_k >= entry - error > tmax: it is no witness, so dropping it changes no answer.  In
//     trace_lane_fast the same test with best_t drops leaves that cannot beat the leader; here the "leader" is the caller's limit and
//     never moves, which is why limit and limit_f are formed once, before the first step;
//   * at a leaf the conditions are a conjunction of pure tests, so their order is free: the triangle test, then the sign of
//     ta = (p.x - o.x) * (1/d.x) (the sign of t_k: better_candidate), then a skip when ta is certainly not below tmax (ta beyond tmax by
//     more than the 2^-48 band, product and quotient differing by < 2^-50 relative; only for ta in the normal range, where "relative"
//     means something), then the own box, then t_k itself by the reference's division and the two comparisons of the rule;
//   * a ray outside fast_path_ok's ranges is answered by the definition: trace_closest(S, r, h, w) && h.t < tmax.
// tri_pre_reject is not used: the plain walk is the starting point.
#pragma once
#include "trace_fast.hpp"

namespace mcpt {

// ---- the walk ---------------------------------------------------------------------------------------------------------------------
// One ray per lane, start to finish (while-while over the compressed hierarchy): trace_lane_fast's steps, the limit fixed, the first
// witness ends it.  stack: this lane's LDS words, stack[i * stride], kFastMaxDepth of them: fast_walk_enabled keeps cw_stack_need below
// that, so no push can pass the end and there is no hand-over (MCPT_TEST_STACK_CAP does not apply here).
__device__ __forceinline__ bool any_lane_fast(const DScene& S, const Ray& r, double tmax, Work& w, int* __restrict__ stack, int stride)
{
    if (!(tmax > 0.0)) return false;                        // NaN, zero, negative: no t_k > 0 lies below it
    const DFast& F = S.fast;
    if (!fast_path_ok(F, r)) {
        Hit h;
        return trace_closest(S, r, h, w) && h.t < tmax;
    }
    const CwNode* __restrict__ nodes = F.cw;
    const DTri* __restrict__ tris = F.tris;
    const V3 rcp = mk(fast_rcp(r.d.x), fast_rcp(r.d.y), fast_rcp(r.d.z));
    const double rmax = fmax(fmax(fabs(rcp.x), fabs(rcp.y)), fabs(rcp.z));
    const double scale = fmax(fmax(F.absmax, fabs(r.o.x)), fmax(fabs(r.o.y), fabs(r.o.z)));
    const double margin = rmax <= 1e6 ? 1.0000001e-9 * scale * rmax : __builtin_inf();
    const RayF rf = make_rayf(F, r, rcp);
    const double limit = tmax + margin;
    const float limit_f = __double2float_ru(limit);
    const double band = tmax + tmax * 0x1p-48;              // (+inf for tmax = +inf: nothing lies beyond it)
    int sp = 0, cur = 0;
    for (;;) {
        while (cur >= 0) {
            w.nodes++;
            const CwHits h = cw_step(nodes + cur, rf, limit_f);
            if (h.ref[3] != MCPT_FAST_EMPTY) { stack[sp * stride] = h.ref[3]; sp++; }
            if (h.ref[2] != MCPT_FAST_EMPTY) { stack[sp * stride] = h.ref[2]; sp++; }
            if (h.ref[1] != MCPT_FAST_EMPTY) { stack[sp * stride] = h.ref[1]; sp++; }
            cur = h.ref[0];
            if (cur == MCPT_FAST_EMPTY && sp > 0) { sp--; cur = stack[sp * stride]; }
        }
        if (cur == MCPT_FAST_EMPTY) break;
        const int ref = -1 - cur;
        const int first = ref >> 4, count = (ref & 7) + 1;
        w.tris += count;
        for (int i = 0; i < count; i++) {
            const DTri* tr = tris + first + i;
            V3 p;
            if (!tri_hit(tr, r, p)) continue;
            const double ta = (p.x - r.o.x) * rcp.x;        // same sign as t, within 2^-50 of it
            if (!(ta > 0.0)) continue;
            if (ta > band && ta > 0x1p-1000) continue;      // t is certainly not below tmax
            if (!own_box_hit(tr, r, rcp)) continue;
            const double t = (p.x - r.o.x) / r.d.x;         // pathTracing.cpp:347
            if (t > 0 && t < tmax) return true;
        }
        if (sp > 0) { sp--; cur = stack[sp * stride]; }
        else break;
    }
    return false;
}

// the reference-shaped form: the definition itself (MCPT_TRACE_REFERENCE, devices without the fast hierarchy)
__device__ __forceinline__ bool any_lane_reference(const DScene& S, const Ray& r, double tmax, Work& w)
{
    if (!(tmax > 0.0)) return false;
    Hit h;
    return trace_closest(S, r, h, w) && h.t < tmax;
}

}  // namespace mcpt
