// pg_kaiser.h -- the Kaiser-windowed sinc of pg_resample and pg_varispeed, evaluated in double on the HOST (not part of the ABI):
//     h(t) = r sinc(r t) I0(beta sqrt(1 - (t/Z)^2)) / I0(beta) for |t| <= Z, else 0.
// One definition, so that the polyphase bank of resample.hip and the interpolation table of varispeed.hip sample the same filter.
#pragma once
#include <math.h>

struct RsFilter { int Z; double beta, rolloff; };
// resampy's published kaiser_best / kaiser_fast parameters, indexed by PG_RS_KAISER_BEST / PG_RS_KAISER_FAST
constexpr RsFilter RS_FILTERS[2] = {{64, 14.769656459379492, 0.9475937167399596}, {16, 8.555504641634386, 0.85}};

inline double rs_i0(double x) {                                   // modified Bessel function I0 by its power series (x <= 15)
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

// h(t) with i0b = rs_i0(beta) formed once by the caller
inline double rs_h(double t, double Z, double beta, double rolloff, double i0b) {
    double h = 0.0;
    if (fabs(t) <= Z) {
        const double u = t / Z, a = M_PI * rolloff * t;
        const double sinc = a == 0.0 ? 1.0 : sin(a) / a;
        const double c = 1.0 - u * u;
        h = rolloff * sinc * rs_i0(beta * sqrt(c > 0.0 ? c : 0.0)) / i0b;
    }
    return h;
}
