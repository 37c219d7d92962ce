// The coefficients of the scaled Chebyshev filter on the stored states (wafer_filter_states, wafer_batch_filter_states; Zhou, Saad,
// Tiago, Chelikowsky 2006).  Plain C++, no HIP: wafer_filter_coefficients() of the C ABI serves it without a GPU.
//
// [a, b] is the interval to damp, a0 < a the anchor at which the degree-m polynomial has magnitude 1.  In this order, every
// operation a double operation of its own (the build passes -ffp-contract=off):
//   e = (b - a) / 2    cc = (b + a) / 2    sigma = e / (a0 - cc)    gamma = 2 / sigma
//   step 1:      al = sigma / e                                             y_1 = al (H - cc) y_0
//   step i >= 2: s2 = 1 / (gamma - sigma)   al = (2 s2) / e   be = sigma s2   sigma = s2
//                                                                           y_i = al (H - cc) y_(i-1) - be y_(i-2)
// al[i], be[i] are step i + 1's; be[0] = 0.  Nothing is written on failure.
#pragma once
#include <cmath>
#include <cstdint>

#ifndef WAFER_FILTER_MAX_DEGREE
#define WAFER_FILTER_MAX_DEGREE 256
#endif

// one step's coefficients of one member, as the kernels read them
struct WaferFilterCoef {
    double al, be, cc;
};

enum { WAFER_FILTER_OK = 0, WAFER_FILTER_BAD_DEGREE = 1, WAFER_FILTER_BAD_INTERVAL = 2 };

// a0 < a < b, all finite
static inline bool wafer_filter_interval_ok(double a, double b, double a0)
{
    return std::isfinite(a) && std::isfinite(b) && std::isfinite(a0) && a0 < a && a < b;
}

static inline int wafer_filter_coefficients_host(uint32_t degree, double a, double b, double a0, double *al, double *be, double *cc)
{
    if (degree == 0 || degree > WAFER_FILTER_MAX_DEGREE) return WAFER_FILTER_BAD_DEGREE;
    if (!wafer_filter_interval_ok(a, b, a0)) return WAFER_FILTER_BAD_INTERVAL;
    const double e = (b - a) / 2.0;
    const double c = (b + a) / 2.0;
    double sigma = e / (a0 - c);
    const double gamma = 2.0 / sigma;
    al[0] = sigma / e;
    be[0] = 0.0;
    for (uint32_t i = 1; i < degree; ++i) {
        const double s2 = 1.0 / (gamma - sigma);
        al[i] = (2.0 * s2) / e;
        be[i] = sigma * s2;
        sigma = s2;
    }
    *cc = c;
    return WAFER_FILTER_OK;
}
