// MCPT_LIGHTS_TREE: the arithmetic host and device share (include/mcpt.h: light sampling).  The tree is built by light_sampling.cpp, the
// descent is vertex.hpp's light_pick_at, the host's walk over every light is light_sampling.cpp's tree_pdf.  Only + - * / and comparisons
// in fp64, in one fixed order, under -ffp-contract=off: g++, hipcc and a numpy restatement give the same bits.
#pragma once
#include "device_scene.hpp"

#if defined(__HIPCC__)
#define MCPT_HD __host__ __device__ __forceinline__
#else
#define MCPT_HD inline
#endif

namespace mcpt {

MCPT_HD double lt_abs(double x) { return x < 0.0 ? -x : x; }
MCPT_HD double lt_max(double a, double b) { return a < b ? b : a; }

// Importance of node n seen from the vertex (p, pn): W / D, D = max(1, |c - p|^2, |h|^2) (c the box's centre, h its half extent), or 0 when
// the whole box lies below the vertex's horizon: s = (c - p) . pn + h . |pn| is the largest (x - p) . pn over the box, and the node is
// culled only when s is below -1e-9 * |pn|_1 * (|p|_inf + |c|_inf + |h|_inf) -- some 10^6 rounding errors of s, and of light_sample's own
// direction . pn on a point of the box: the rule can only cull less than the exact one.
MCPT_HD double light_node_importance(const DLightNode& n, double px, double py, double pz, double nx, double ny, double nz)
{
    const double cx = (n.lo[0] + n.hi[0]) * 0.5, cy = (n.lo[1] + n.hi[1]) * 0.5, cz = (n.lo[2] + n.hi[2]) * 0.5;
    const double hx = (n.hi[0] - n.lo[0]) * 0.5, hy = (n.hi[1] - n.lo[1]) * 0.5, hz = (n.hi[2] - n.lo[2]) * 0.5;
    const double dx = cx - px, dy = cy - py, dz = cz - pz;
    const double ax = lt_abs(nx), ay = lt_abs(ny), az = lt_abs(nz);
    const double s = ((dx * nx + dy * ny) + dz * nz) + ((hx * ax + hy * ay) + hz * az);
    const double pinf = lt_max(lt_max(lt_abs(px), lt_abs(py)), lt_abs(pz));
    const double cinf = lt_max(lt_max(lt_abs(cx), lt_abs(cy)), lt_abs(cz));
    const double hinf = lt_max(lt_max(hx, hy), hz);
    const double margin = (1e-9 * ((ax + ay) + az)) * ((pinf + cinf) + hinf);
    if (s < -margin) return 0.0;
    const double d2 = (dx * dx + dy * dy) + dz * dz, h2 = (hx * hx + hy * hy) + hz * hz;
    return n.w / lt_max(1.0, lt_max(d2, h2));
}

// The probability of going to the left child L of a node whose right child is R.  Both culled: their weights stand in (the pick is then
// wasted on a light below the horizon, which gives nothing anyway).  One culled, or of weight 0: 1.0 or 0.0 exactly.
MCPT_HD double light_tree_left(const DLightNode& L, const DLightNode& R, double px, double py, double pz, double nx, double ny, double nz)
{
    double iL = light_node_importance(L, px, py, pz, nx, ny, nz), iR = light_node_importance(R, px, py, pz, nx, ny, nz);
    if (iL == 0.0 && iR == 0.0) { iL = L.w; iR = R.w; }
    if (iR == 0.0) return 1.0;
    if (iL == 0.0) return 0.0;
    return iL / (iL + iR);
}

}  // namespace mcpt
