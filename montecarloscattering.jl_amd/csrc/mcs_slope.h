// The least-squares slope rule of include/mcs.h ("Slope of frame m"), stated once: over the entries l_lo <= l < l_hi that valid(l)
// admits, in ascending l, with x(l) and y(l) -- every operation a separate rounding, serial sums that start from 0:
//   xbar = (sum x) / k;  ybar = (sum y) / k;  Sxx = sum (x - xbar)(x - xbar);  Sxy = sum (x - xbar)(y - ybar);  slope = Sxy / Sxx
// Fewer than three valid entries give a quiet NaN.  The entries are walked twice; valid, x and y give the same bits each time.
// Used by the products and escape samples of the ensemble statistics (mcs_ensemble.hip) and by K12 (mcs_consumers.hip).
#pragma once
#include <hip/hip_runtime.h>

template <class Valid, class X, class Y>
__device__ __forceinline__ double mcs_slope_rule(int l_lo, int l_hi, Valid valid, X x, Y y) {
  int k = 0;
  double sx = 0.0, sy = 0.0;
  for (int l = l_lo; l < l_hi; ++l)
    if (valid(l)) { sx = sx + x(l); sy = sy + y(l); ++k; }
  if (k < 3) return __builtin_nan("");
  const double xbar = sx / (double)k, ybar = sy / (double)k;
  double sxx = 0.0, sxy = 0.0;
  for (int l = l_lo; l < l_hi; ++l)
    if (valid(l)) {
      const double dx = x(l) - xbar;
      sxx = sxx + dx * dx;
      sxy = sxy + dx * (y(l) - ybar);
    }
  return sxy / sxx;
}
