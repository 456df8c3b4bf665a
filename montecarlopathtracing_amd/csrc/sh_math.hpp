// The real spherical-harmonic basis of bands 0..2 (mcpt.h: light probes), the one copy of it: query.hip compiles it for the probe fold,
// sh_api.cpp for mcpt_sh_basis / _radiance / _irradiance.  fp64, no contraction (-ffp-contract=off), in the index order and the operation
// order mcpt.h writes out; tests/sh_ref.py restates it in numpy.
#pragma once

#ifndef MCPT_HD
#if defined(__HIPCC__)
#define MCPT_HD __host__ __device__ __forceinline__
#else
#define MCPT_HD inline
#endif
#endif

namespace mcpt {

#define MCPT_SH_N 9

// Y_i(d), i = 0..8, of the unit direction (x, y, z)
MCPT_HD void sh_basis9(double x, double y, double z, double* Y)
{
    Y[0] = 0.28209479177387814;
    Y[1] = 0.4886025119029199 * y;
    Y[2] = 0.4886025119029199 * z;
    Y[3] = 0.4886025119029199 * x;
    Y[4] = 1.0925484305920792 * (x * y);
    Y[5] = 1.0925484305920792 * (y * z);
    Y[6] = 0.31539156525252005 * (3.0 * (z * z) - 1.0);
    Y[7] = 1.0925484305920792 * (x * z);
    Y[8] = 0.5462742152960396 * (x * x - y * y);
}

// A_l of coefficient i: the cosine lobe's zonal factors pi, 2 pi / 3, pi / 4
MCPT_HD double sh_cosine_factor(int i) { return i == 0 ? 3.141592653589793 : (i < 4 ? 2.0943951023931953 : 0.7853981633974483); }

}  // namespace mcpt
