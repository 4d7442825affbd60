// f64_sincos.hpp — sin and cos of an f64 over the range a physics env meets (|x| up to a few hundred: the quadrant count must stay
// below 2^20 for the reduction to be exact), bit-reproducible on the host: every operation is one f64 `+ - *`, a `rint` under
// round-to-nearest-even or a sign flip, in one fixed order and uncontracted, so that numpy float64 scalars spelling the same
// operations (np.rint for rint) give the same bits (tests/acrobot_reference.py: poly_sincos).
//
//   k = rint(x * (2 / pi))                         the nearest quadrant
//   r = (x - k * C1) - k * C2                      C1 + C2 = pi / 2 to 2^-86: C1 is its leading 33 bits, so k * C1 is exact and so is
//                                                  the first difference; |r| <= pi / 4 (+ one rounding of x * (2 / pi))
//   s = r * P(r^2), c = Q(r^2)                     Horner, the Taylor coefficients 1 / n! through r^17 and r^16: the first dropped
//                                                  terms, r^19 / 19! < 9e-20 and r^18 / 18! < 3e-18 at pi / 4, are below half an ulp
//   k & 3 = 0: (s, c)   1: (c, -s)   2: (-s, -c)   3: (-c, s)
//
// The result is within a few roundings of libm's (measured: tests/test_acrobot_cpu.py), which is all a reproducible env needs.
#pragma once

namespace pfa {

__device__ __forceinline__ void f64_sincos(double x, double &sn, double &cs) {
#pragma clang fp contract(off)
    constexpr double kTwoOverPi = 0.63661977236758138;        // 2 / pi in f64
    constexpr double kC1 = 1.5707963267341256;                // the leading 33 bits of pi / 2 (fdlibm's pio2_1)
    constexpr double kC2 = 6.0771005065061922e-11;            // pi / 2 - kC1 in f64 (fdlibm's pio2_1t)
    const double k = rint(x * kTwoOverPi);
    const double r = (x - k * kC1) - k * kC2;
    const double z = r * r;
    double p = 1.0 / 355687428096000.0;       // 1 / 17!
    p = p * z + -1.0 / 1307674368000.0;       // 15!
    p = p * z + 1.0 / 6227020800.0;           // 13!
    p = p * z + -1.0 / 39916800.0;            // 11!
    p = p * z + 1.0 / 362880.0;               // 9!
    p = p * z + -1.0 / 5040.0;
    p = p * z + 1.0 / 120.0;
    p = p * z + -1.0 / 6.0;
    p = p * z + 1.0;
    const double s = r * p;
    double q = 1.0 / 20922789888000.0;        // 1 / 16!
    q = q * z + -1.0 / 87178291200.0;         // 14!
    q = q * z + 1.0 / 479001600.0;            // 12!
    q = q * z + -1.0 / 3628800.0;             // 10!
    q = q * z + 1.0 / 40320.0;                // 8!
    q = q * z + -1.0 / 720.0;
    q = q * z + 1.0 / 24.0;
    q = q * z + -1.0 / 2.0;
    q = q * z + 1.0;
    const int n = (int)k & 3;
    const double a = (n & 1) ? q : s, b = (n & 1) ? s : q;          // |sin|, |cos| carriers of this quadrant
    sn = (n & 2) ? -a : a;
    cs = ((n + 1) & 2) ? -b : b;
}

}  // namespace pfa
