// Scalar math of ap_per_class (utils/metrics.py:21-114 of the reference) -- plain C++ (host + device) so that tests/native can
// compile it with g++ and compare it with the reference's numpy on the CPU.  Everything is double, in numpy's operation
// order, and must be compiled with -ffp-contract=off.
//
// The curves are handed in as accessors over ONE class's predictions in sorted order (conf descending, ties by ascending row
// index -- this package's rule; numpy's argsort leaves ties in introsort order):
//   tpc(i)   int     inclusive count of true positives among predictions 0..i        (fpc = i + 1 - tpc)
//   env(i)   double  max over k >= i of precision(k): the reverse running maximum of compute_ap's mpre without its sentinels
//   conf(i)  double  the confidence, widened from float
// np.interp's contract (numpy/core/src/multiarray/compiled_base.c, arr_interp): j = the last index with xp[j] <= x; the last
// point and an exact hit return fp[j]; otherwise slope * (x - xp[j]) + fp[j] with slope = (fp[j+1] - fp[j]) / (xp[j+1] - xp[j]).
#pragma once
#include "obb_device.h"

namespace obb {
namespace apm {

constexpr int kApPoints = 101;    // np.linspace(0, 1, 101)
constexpr int kPrPoints = 1000;   // np.linspace(0, 1, 1000)
constexpr double kEps = 1e-16;

// np.linspace(0, 1, num)[k]: k * step with step = 1 / (num - 1), the last point set to 1.0
OBB_HD double ap_x(int k) { return k >= kApPoints - 1 ? 1.0 : k * 0.01; }
OBB_HD double pr_x(int k) { return k >= kPrPoints - 1 ? 1.0 : k * (1.0 / 999); }

OBB_HD double recall_of(int tpc, double nl_eps) { return (double)tpc / nl_eps; }                  // tpc / (n_l + eps)
OBB_HD double precision_of(int tpc, int64_t rank) { return (double)tpc / (double)rank; }          // tpc / (tpc + fpc)
OBB_HD double f1_of(double p, double r) { return 2 * p * r / (p + r + kEps); }

// np.interp(x, mrec, mpre) of compute_ap for 0 <= x <= 1: mrec = [0, recall..., 1], mpre = envelope of [1, precision..., 0]
// (mpre[0] = 1 because no precision exceeds 1).  recall is non-decreasing but may pass 1 when a caller hands in more true
// positives than labels; the closing sentinel 1.0 then breaks the order of mrec, and numpy's bisection never reaches it unless
// every recall is <= x -- so j is searched among [0, recall...] and moves to the sentinel only from the last recall.
template <typename Tpc, typename Env>
OBB_HD double ap_interp(double x, int64_t np, double nl_eps, Tpc tpc, Env env) {
  int64_t lo = 0, hi = np;                       // the number of recalls <= x
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (recall_of(tpc(mid), nl_eps) <= x) lo = mid + 1; else hi = mid;
  }
  int64_t j = lo;                                // index into mrec / mpre
  if (j == np && 1.0 <= x) return 0.0;           // the closing sentinel: fp[len - 1]
  const double xj = j ? recall_of(tpc(j - 1), nl_eps) : 0.0;
  const double yj = j ? env(j - 1) : 1.0;
  if (xj == x) return yj;
  const double xn = j < np ? recall_of(tpc(j), nl_eps) : 1.0;
  const double yn = j < np ? env(j) : 0.0;
  const double slope = (yn - yj) / (xn - xj);
  return slope * (x - xj) + yj;
}

// np.trapz(y, x) over the 101 points: (d * (y[1:] + y[:-1]) / 2.0).sum() with numpy's pairwise summation of 100 doubles
// (eight running sums over the first 96, combined as a tree, then the last four in order).
OBB_HD double trapz101(const double* y) {
  double r[8];
  double res = 0.0;
  for (int k = 0; k < 100; k++) {
    const double d = ap_x(k + 1) - ap_x(k);
    const double t = d * (y[k + 1] + y[k]) / 2.0;
    if (k < 8) r[k] = t;
    else if (k < 96) r[k & 7] += t;
    else {
      if (k == 96) res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
      res += t;
    }
  }
  return res;
}

// np.interp(-px, -conf, curve, left=left): xp = -conf ascends; beyond the last xp the last curve value.
template <typename Conf, typename Curve>
OBB_HD double pr_interp(double px, int64_t np, Conf conf, Curve curve, double left) {
  const double x = -px;
  if (x < -conf(0)) return left;
  if (x > -conf(np - 1)) return curve(np - 1);
  int64_t lo = 0, hi = np;                       // the number of xp <= x (at least 1 here)
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (-conf(mid) <= x) lo = mid + 1; else hi = mid;
  }
  const int64_t j = lo - 1;
  const double xj = -conf(j), yj = curve(j);
  if (j == np - 1 || xj == x) return yj;
  const double slope = (curve(j + 1) - yj) / (-conf(j + 1) - xj);
  return slope * (x - xj) + yj;
}

// tp = (r * n_l).round(), fp = (tp / (p + eps) - tp).round() at the best-F1 index (np.round: half to even)
OBB_HD double tp_of(double r, int64_t n_l) { return rint(r * (double)n_l); }
OBB_HD double fp_of(double tp, double p) { return rint(tp / (p + kEps) - tp); }

// the sort key of a confidence: unsigned, ascending key = descending conf; -0 and +0 are one value as they are for numpy
OBB_HD uint32_t conf_key_desc(float conf) {
  union { float f; uint32_t u; } v;
  v.f = conf + 0.0f;
  const uint32_t asc = (v.u & 0x80000000u) ? ~v.u : (v.u | 0x80000000u);
  return ~asc;
}

}  // namespace apm
}  // namespace obb
