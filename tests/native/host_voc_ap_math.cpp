// Host build of the PRODUCT's VOC AP arithmetic (yolov5_obb_amd/csrc/voc_ap_math.h) behind array drivers, so that
// tests/test_voc_ap_math_host.py can compare it with numpy on the CPU (no GPU needed).  The file is also a program of its own:
// main() walks the same functions over seeded curves and sums of every length class and holds the explicit-stack summation to a
// plain recursive one; the test builds it with -fsanitize=address,undefined and runs it once.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "voc_ap_math.h"

using namespace obb::vap;

extern "C" {

double hc_np_sum(const double* a, long n) {
  SumStack s;
  return np_sum([&](long long i) { return a[i]; }, n, &s);
}

double hc_ap11(const double* rec, const double* prec, long n) {
  return ap11(n, [&](long long i) { return rec[i]; }, [&](long long i) { return prec[i]; });
}

double hc_ap_all(const double* rec, const double* prec, long n) {
  std::vector<double> terms((size_t)n + 1);
  SumStack s;
  return ap_all(n, [&](long long i) { return rec[i]; }, [&](long long i) { return prec[i]; }, terms.data(), &s);
}

// rec / prec of voc_eval's tail from inclusive counts
void hc_curve(const long long* tp, const long long* fp, long n, long long npos, double* rec, double* prec) {
  for (long i = 0; i < n; i++) rec[i] = rec_of(tp[i], npos), prec[i] = prec_of(tp[i], fp[i]);
}

void hc_score_key(const double* s, long n, unsigned long long* out) {
  for (long i = 0; i < n; i++) out[i] = score_key_desc(s[i]);
}

void hc_index_of(const double* v, long n, long long lim, long long* out) {
  for (long i = 0; i < n; i++) out[i] = index_of(v[i], lim);
}

}  // extern "C"

static double pairwise_rec(const double* a, long n) {
  if (n <= kLeaf) return sum_leaf([&](long long i) { return a[i]; }, 0, (int)n);
  long n2 = n / 2;
  n2 -= n2 % 8;
  return pairwise_rec(a, n2) + pairwise_rec(a + n2, n - n2);
}

static unsigned long long bits(double v) { return __builtin_bit_cast(unsigned long long, v); }

int main() {
  unsigned long long x = 88172645463325252ull;
  auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (double)(x >> 11) / 9007199254740992.0; };
  const long lens[] = {0, 1, 7, 8, 9, 127, 128, 129, 257, 1000, 8191, 8192, 8193, 16385, 100003};
  for (long n : lens) {
    std::vector<double> a((size_t)n);
    for (auto& v : a) v = (rnd() - 0.5) * (rnd() < 0.3 ? 1e9 : 1e-3);
    double want = 0.0;
    for (long o = 0; o < n; o += kNpBuf) want = want + pairwise_rec(a.data() + o, n - o < kNpBuf ? n - o : kNpBuf);
    const double got = hc_np_sum(a.data(), n);
    if (bits(got) != bits(want)) { printf("np_sum differs at n = %ld\n", n); return 1; }
  }
  for (long n : {0L, 1L, 5L, 300L, 9000L, 20000L}) {
    for (long long npos : {0LL, 1LL, 7LL, (long long)n}) {
      std::vector<long long> tp((size_t)n), fp((size_t)n);
      long long t = 0, f = 0;
      for (long i = 0; i < n; i++) { (rnd() < 0.6 ? t : f)++; tp[i] = t; fp[i] = f; }
      std::vector<double> rec((size_t)n), prec((size_t)n);
      hc_curve(tp.data(), fp.data(), n, npos, rec.data(), prec.data());
      const double a11 = hc_ap11(rec.data(), prec.data(), n), aall = hc_ap_all(rec.data(), prec.data(), n);
      if (npos > 0 && npos >= t && !(a11 >= 0. && a11 <= 1.0000001 && aall >= 0. && aall <= 1.0000001)) {
        printf("ap out of range at n = %ld npos = %lld: %g %g\n", n, npos, a11, aall);
        return 1;
      }
    }
  }
  const double s[] = {1.0, 0.5, 0.0, -0.0, -1.0, __builtin_inf(), -__builtin_inf(), __builtin_nan("")};
  unsigned long long k[8];
  hc_score_key(s, 8, k);
  if (!(k[5] < k[0] && k[0] < k[1] && k[1] < k[2] && k[2] == k[3] && k[3] < k[4] && k[4] < k[6] && k[6] < k[7])) { printf("score_key order\n"); return 1; }
  printf("host_voc_ap_math ok\n");
  return 0;
}
