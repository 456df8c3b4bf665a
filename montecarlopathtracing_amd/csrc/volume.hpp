// Irradiance volumes (mcpt.h: irradiance volumes): the arithmetic of a regular probe grid and of the trilinear lookup between its probes,
// the one copy of it -- volume.hip compiles it for the GPU, volume_api.cpp for mcpt_volume_points and mcpt_volume_irradiance_host -- and
// the launch interface of the two kernels.  fp64, no contraction (-ffp-contract=off), IEEE division, every expression in the order mcpt.h
// writes it; tests/volume_ref.py restates it in numpy.
#pragma once
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mcpt.h"
#include "sh_math.hpp"

namespace mcpt {

// the number of probes of a valid grid (at most 2^31 - 1)
MCPT_HD int64_t volume_probes(const mcpt_volume_grid& g) { return (int64_t(g.nx) * g.ny) * g.nz; }

// the position of probe i along axis a
MCPT_HD double volume_coord(const mcpt_volume_grid& g, int a, int i) { return g.origin[a] + double(i) * g.spacing[a]; }

// One axis of a lookup: the two probes i0, i1 around coordinate x of an axis of n probes and their weights w0, w1.  A coordinate outside
// the grid takes the border's; a NaN (the device form does not look) lands on probe 0, never outside the grid.
MCPT_HD void volume_axis(double x, double origin, double spacing, int n, int* i, double* w)
{
    const double top = double(n - 1);
    double g = (x - origin) / spacing;
    g = g > 0.0 ? g : 0.0;
    g = g < top ? g : top;
    double f = 0.0;
    i[0] = i[1] = 0;
    if (n >= 2) {
        const int fl = int(floor(g));
        i[0] = fl < n - 2 ? fl : n - 2;
        i[1] = i[0] + 1;
        f = g - double(i[0]);
        // a coordinate that is a probe's own, bit for bit, gets that probe alone: (x - origin) / spacing does not give the probe's index
        // back exactly unless origin and spacing are dyadic ((0.1 + 0.3 - 0.1) / 0.3 is 1 + 2^-52)
        if (x == origin + double(i[0]) * spacing) f = 0.0;
        else if (x == origin + double(i[1]) * spacing) f = 1.0;
    }
    w[0] = 1.0 - f;
    w[1] = f;
}

// The eight corners of a receiver at x: probe P[j] and weight w[j] of corner j = dz * 4 + dy * 2 + dx, after the mask (valid: one byte
// per probe, or null).  Returns the number of corners whose weight is > 0; 0 under a mask that leaves nothing: every weight is then 0.0
// and the receiver's outputs are +0.0.
MCPT_HD int volume_corners(const mcpt_volume_grid& g, const uint8_t* valid, const double* x, int32_t* P, double* w)
{
    int ix[2], iy[2], iz[2];
    double wx[2], wy[2], wz[2];
    volume_axis(x[0], g.origin[0], g.spacing[0], g.nx, ix, wx);
    volume_axis(x[1], g.origin[1], g.spacing[1], g.ny, iy, wy);
    volume_axis(x[2], g.origin[2], g.spacing[2], g.nz, iz, wz);
    for (int j = 0; j < 8; j++) {
        const int dx = j & 1, dy = (j >> 1) & 1, dz = j >> 2;
        P[j] = (iz[dz] * g.ny + iy[dy]) * g.nx + ix[dx];
        w[j] = (wx[dx] * wy[dy]) * wz[dz];
    }
    if (valid) {
        double W = 0.0;
        for (int j = 0; j < 8; j++) {
            if (valid[P[j]] == 0) w[j] = 0.0;
            W += w[j];
        }
        const bool any = W > 0.0;
        for (int j = 0; j < 8; j++) w[j] = any ? w[j] / W : 0.0;
    }
    int c = 0;
    for (int j = 0; j < 8; j++) c += w[j] > 0.0 ? 1 : 0;
    return c;
}

// A(i) * Y_i(n^) of a receiver's normal b, i = 0..8: mcpt_sh_irradiance's expressions
MCPT_HD void volume_lobe9(const double* b, double* AY)
{
    const double l = sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]);
    double Y[MCPT_SH_N];
    sh_basis9(b[0] / l, b[1] / l, b[2] / l, Y);
    for (int i = 0; i < MCPT_SH_N; i++) AY[i] = sh_cosine_factor(i) * Y[i];
}

// E[3] from the corners' coefficients sh27 [probe][9][3]: per channel the blend c in j order, the sum over i in i order, the clamp last.
// lit == false (nothing valid around the receiver): +0.0.
MCPT_HD void volume_eval(const double* sh27, const int32_t* P, const double* w, const double* AY, bool lit, bool clamp, double* E)
{
    for (int c = 0; c < 3; c++) E[c] = 0.0;
    if (!lit) return;
    for (int i = 0; i < MCPT_SH_N; i++)
        for (int c = 0; c < 3; c++) {
            double s = 0.0;
            for (int j = 0; j < 8; j++) s += w[j] * sh27[size_t(P[j]) * (MCPT_SH_N * 3) + size_t(i * 3 + c)];
            E[c] += AY[i] * s;
        }
    if (clamp)
        for (int c = 0; c < 3; c++) E[c] = E[c] > 0.0 ? E[c] : 0.0;
}

// d_p3[P] = the position of probe P for every probe of g (valid), one lane per probe
void launch_volume_points(const mcpt_volume_grid& g, double* d_p3, hipStream_t st);
// d_e3[r] and d_corners[r] (may be null) of receivers r = 0 .. n-1 (n >= 1), q6 = position, normal; d_valid may be null
void launch_volume_irradiance(const mcpt_volume_grid& g, const double* d_sh27, const uint8_t* d_valid, const double* d_q6, int64_t n, double* d_e3,
                              int32_t* d_corners, hipStream_t st);

}  // namespace mcpt
