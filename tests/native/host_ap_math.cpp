// Host build of the PRODUCT's ap_per_class arithmetic (yolov5_obb_amd/csrc/ap_math.h): a serial driver with the outputs of
// obb_ap_per_class_f32, so that tests/test_ap_math_host.py can compare it with the reference's numpy on the CPU (no GPU needed).
#include <algorithm>
#include <vector>

#include "ap_math.h"

namespace {
struct TpcAt {
  const int* p; int64_t stride;
  int operator()(int64_t i) const { return p[i * stride]; }
};
struct EnvAt {
  const double* p; int64_t stride;
  double operator()(int64_t i) const { return p[i * stride]; }
};
struct ConfAt {
  const float* conf; const int* idx;
  double operator()(int64_t i) const { return (double)conf[idx[i]]; }
};
struct RecallAt {
  TpcAt tpc; double nl_eps;
  double operator()(int64_t i) const { return obb::apm::recall_of(tpc(i), nl_eps); }
};
struct PrecisionAt {
  TpcAt tpc;
  double operator()(int64_t i) const { return obb::apm::precision_of(tpc(i), i + 1); }
};
}  // namespace

extern "C" {
// tp (n, niou) bytes, conf (n), pred_cls (n), target_cls (m) -> ap [nc_max][niou], prf [nc_max][5], counts [2][nc_max], info [4]
// (layouts of include/obb_hip.h: obb_ap_per_class_f32).  Returns 0, or -1 for a class id outside [0, nc_max).
int hc_ap_per_class(const unsigned char* tp, const float* conf, const float* pred_cls, long n, int niou, const float* target_cls, long m,
                    int nc_max, double* ap, double* prf, int* counts, int* info) {
  using namespace obb::apm;
  std::fill(ap, ap + (size_t)nc_max * niou, 0.0);
  std::fill(prf, prf + (size_t)nc_max * 5, 0.0);
  std::fill(counts, counts + 2 * nc_max, 0);
  std::fill(info, info + 4, 0);
  for (long i = 0; i < m; i++) {
    const int c = (int)target_cls[i];
    if (c < 0 || c >= nc_max || (float)c != target_cls[i]) return -1;
    counts[c]++;
  }
  std::vector<unsigned long long> key(n);
  std::vector<int> idx(n);
  for (long i = 0; i < n; i++) {
    const int c = (int)pred_cls[i];
    if (c < 0 || c >= nc_max || (float)c != pred_cls[i]) return -1;
    counts[nc_max + c]++;
    key[i] = ((unsigned long long)c << 32) | conf_key_desc(conf[i]);
    idx[i] = (int)i;
    info[1] += tp[(size_t)i * niou] ? 1 : 0;
  }
  std::sort(idx.begin(), idx.end(), [&](int a, int b) { return key[a] < key[b] || (key[a] == key[b] && a < b); });
  std::vector<double> curves((size_t)3 * nc_max * kPrPoints, 0.0);
  const size_t plane = (size_t)nc_max * kPrPoints;
  long first = 0;
  for (int c = 0; c < nc_max; first += counts[nc_max + c], c++) {
    const long np = counts[nc_max + c], n_l = counts[c];
    if (!np || !n_l) continue;
    std::vector<int> tpc((size_t)np * niou);
    std::vector<double> env((size_t)np * niou);
    for (int j = 0; j < niou; j++) {
      int run = 0;
      for (long i = 0; i < np; i++) tpc[i * niou + j] = run += tp[(size_t)idx[first + i] * niou + j] ? 1 : 0;
      double mx = 0.0;
      for (long i = np - 1; i >= 0; i--) env[i * niou + j] = mx = std::max(mx, precision_of(tpc[i * niou + j], i + 1));
      double y[kApPoints];
      const TpcAt t = {tpc.data() + j, niou};
      const EnvAt e = {env.data() + j, niou};
      for (int k = 0; k < kApPoints; k++) y[k] = ap_interp(ap_x(k), np, (double)n_l + kEps, t, e);
      ap[c * niou + j] = trapz101(y);
    }
    const TpcAt t0 = {tpc.data(), niou};
    const ConfAt cf = {conf, idx.data() + first};
    const RecallAt rc = {t0, (double)n_l + kEps};
    const PrecisionAt pc = {t0};
    for (int k = 0; k < kPrPoints; k++) {
      const double r = pr_interp(pr_x(k), np, cf, rc, 0.0), p = pr_interp(pr_x(k), np, cf, pc, 1.0);
      curves[(size_t)c * kPrPoints + k] = p;
      curves[plane + (size_t)c * kPrPoints + k] = r;
      curves[2 * plane + (size_t)c * kPrPoints + k] = f1_of(p, r);
    }
  }
  int best = 0, ncls = 0;
  for (int c = 0; c < nc_max; c++) ncls += counts[c] > 0;
  double best_v = -1.0;
  for (int k = 0; k < kPrPoints && ncls; k++) {
    double sum = 0.0;
    for (int c = 0; c < nc_max; c++)
      if (counts[c] > 0) sum += curves[2 * plane + (size_t)c * kPrPoints + k];
    if (sum / ncls > best_v) best_v = sum / ncls, best = k;
  }
  info[0] = best;
  for (int c = 0; c < nc_max; c++) {
    if (!counts[c]) continue;
    const double p = curves[(size_t)c * kPrPoints + best], r = curves[plane + (size_t)c * kPrPoints + best];
    const double tpn = tp_of(r, counts[c]);
    double* o = prf + (size_t)c * 5;
    o[0] = p, o[1] = r, o[2] = curves[2 * plane + (size_t)c * kPrPoints + best], o[3] = tpn, o[4] = fp_of(tpn, p);
  }
  return 0;
}
}
