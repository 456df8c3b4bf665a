// C ABI, light probes on the host (include/mcpt.h: mcpt_sh_basis, mcpt_sh_radiance, mcpt_sh_irradiance): what a receiver does with the
// coefficients mcpt_query_sh returns.  No device is needed.  The basis is sh_math.hpp's, the copy the probe fold compiles for the GPU.
#include <cmath>
#include <string>

#include "handles.hpp"
#include "sh_math.hpp"

using namespace mcpt;

static int finite_check(const double* a, int64_t n, int per, const char* what)
{
    for (int64_t i = 0; i < n * per; i++)
        if (!std::isfinite(a[i])) return fail(MCPT_ERR_ARG, std::string(what) + " " + std::to_string(i / per) + ": component that is not finite");
    return MCPT_OK;
}

extern "C" {

int mcpt_sh_basis(const double* d3, int64_t n, double* y9)
{
    if (n < 0) return fail(MCPT_ERR_ARG, "n must be >= 0");
    if (!d3 || !y9) return fail(MCPT_ERR_ARG, "null argument");
    if (const int rc = finite_check(d3, n, 3, "direction")) return rc;
    for (int64_t i = 0; i < n; i++) sh_basis9(d3[i * 3], d3[i * 3 + 1], d3[i * 3 + 2], y9 + i * MCPT_SH_N);
    return MCPT_OK;
}

int mcpt_sh_radiance(const double* sh27, const double* d3, int64_t n, double* rgb3)
{
    if (n < 0) return fail(MCPT_ERR_ARG, "n must be >= 0");
    if (!sh27 || !d3 || !rgb3) return fail(MCPT_ERR_ARG, "null argument");
    if (const int rc = finite_check(sh27, n, MCPT_SH_N * 3, "probe")) return rc;
    if (const int rc = finite_check(d3, n, 3, "direction")) return rc;
    for (int64_t i = 0; i < n; i++) {
        double Y[MCPT_SH_N];
        sh_basis9(d3[i * 3], d3[i * 3 + 1], d3[i * 3 + 2], Y);
        const double* sh = sh27 + i * MCPT_SH_N * 3;
        for (int c = 0; c < 3; c++) {
            double s = 0.0;
            for (int j = 0; j < MCPT_SH_N; j++) s += sh[j * 3 + c] * Y[j];
            rgb3[i * 3 + c] = s;
        }
    }
    return MCPT_OK;
}

int mcpt_sh_irradiance(const double* sh27, const double* n3, int64_t n, double* e3)
{
    if (n < 0) return fail(MCPT_ERR_ARG, "n must be >= 0");
    if (!sh27 || !n3 || !e3) return fail(MCPT_ERR_ARG, "null argument");
    if (const int rc = finite_check(sh27, n, MCPT_SH_N * 3, "probe")) return rc;
    if (const int rc = finite_check(n3, n, 3, "normal")) return rc;
    for (int64_t i = 0; i < n; i++) {
        const double* b = n3 + i * 3;
        const double l = std::sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]);
        if (!(std::isfinite(l) && l > 0.0)) return fail(MCPT_ERR_ARG, "normal " + std::to_string(i) + ": the normal must have a non-zero finite length");
    }
    for (int64_t i = 0; i < n; i++) {
        const double* b = n3 + i * 3;
        const double l = std::sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]);
        double Y[MCPT_SH_N];
        sh_basis9(b[0] / l, b[1] / l, b[2] / l, Y);
        const double* sh = sh27 + i * MCPT_SH_N * 3;
        for (int c = 0; c < 3; c++) {
            double s = 0.0;
            for (int j = 0; j < MCPT_SH_N; j++) s += (sh_cosine_factor(j) * Y[j]) * sh[j * 3 + c];
            e3[i * 3 + c] = s;
        }
    }
    return MCPT_OK;
}

}  // extern "C"
