// Python's round(v, 5) on the device, for the candidate-table builder (woa_prep.hip) and the scorer over service ids
// (services.hip): both round rows of the service table the way WOA._prepare does.
#pragma once
#include "common.h"

namespace {
// Python's round(x, 5) bit for bit (CPython rounds the exact binary value, ties to even, and returns the double nearest to
// the decimal result).  p + e = x * 10^5 exactly (e by fma); n = rint(p), r = p - n is exact and |r| <= 0.5.  The decision
// reads r and e separately: r + e could round onto 0.5.  For 2^52 <= |p| < 2^53, p is an integer and r = 0, |e| <= 0.5: an
// exact half there is a tie between n and n +- 1, broken to the even one.  n < 2^53 is exact, so n / 10^5 (IEEE division) is
// the double nearest to n * 10^-5.  From |p| >= 2^53 on x itself is what Python returns (and NaN / inf stay as they are).
__device__ __forceinline__ double round5(double x) {
    const double p = __dmul_rn(x, 1e5);
    if (!(fabs(p) < 9007199254740992.0)) return x;
    const double e = fma(x, 1e5, -p);
    double n = rint(p);
    const double r = __dsub_rn(p, n);
    if (r > 0.5 || (r == 0.5 && e > 0.0)) n = __dadd_rn(n, 1.0);
    else if (r < -0.5 || (r == -0.5 && e < 0.0)) n = __dsub_rn(n, 1.0);
    else if (r == 0.0 && fabs(e) == 0.5 && fmod(n, 2.0) != 0.0) n = __dadd_rn(n, e > 0.0 ? 1.0 : -1.0);
    return n / 1e5;
}
}  // namespace
