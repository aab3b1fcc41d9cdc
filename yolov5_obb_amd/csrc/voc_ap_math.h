// Scalar math of voc_ap and of the tail of voc_eval (DOTA_devkit/dota_evaluation_task1.py:54-86, :235-249 of the reference) -- plain
// C++ (host + device) so that tests/native can compile it with g++ and compare it with numpy on the CPU.  Everything is IEEE
// double, in numpy's operation order, and must be compiled with -ffp-contract=off.  Used by csrc/task1_eval.h.
//
// np.sum of a contiguous double array of n elements (numpy/core/src/umath/loops_utils.h.src, checked against numpy 2.2.6):
// the array goes through the reduction in chunks of kNpBuf = 8192 elements, the result starts from +0.0 and takes the chunks'
// sums left to right; one chunk is summed by pairwise_sum:
//   n < 8      a plain loop starting from -0.0
//   n <= 128   eight accumulators over the full groups of 8, ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the
//              remainder one element at a time
//   else       n2 = n / 2, n2 -= n2 % 8; pairwise(a, n2) + pairwise(a + n2, n - n2)
// A pairwise recursion over the whole array is NOT np.sum above 8192 elements.
//
// The recursion is walked with an explicit stack (SumStack: the kernel keeps it in LDS, no scratch memory, no device recursion).
#pragma once
#include "obb_device.h"

namespace obb {
namespace vap {

constexpr double kEps = 2.220446049250313e-16;   // np.finfo(np.float64).eps
constexpr int kPoints11 = 11;                    // np.arange(0., 1.1, 0.1)
constexpr long long kNpBuf = 8192;               // numpy's default reduction buffer, in elements
constexpr int kLeaf = 128;                       // PW_BLOCKSIZE
constexpr int kSumDepth = 16;                    // a chunk of 8192 splits at most 8 times

// np.maximum of doubles: a NaN operand is the result
OBB_HD double np_max(double a, double b) { return (a >= b || a != a) ? a : b; }

// np.arange(0., 1.1, 0.1)[i] = 0. + i * 0.1, computed in double
OBB_HD double thr11(int i) { return (double)i * 0.1; }

// :238-241  rec = tp / float(npos) (npos == 0: NaN or inf, as numpy), prec = tp / np.maximum(tp + fp, eps); tp, fp counts
OBB_HD double rec_of(long long tp, long long npos) { return (double)tp / (double)npos; }
OBB_HD double prec_of(long long tp, long long fp) {
  const double s = (double)tp + (double)fp;
  return (double)tp / np_max(s, kEps);
}

// ---- 11-point metric (:60-69) ----
// p = np.max(prec[rec >= t]) or 0 when nothing qualifies; a running pair (m, any) takes the qualifying values in any order
// (np.max propagates NaN, and so does every grouping of np_max).
OBB_HD void max_take(double& m, bool& any, double v) {
  m = any ? np_max(m, v) : v;
  any = true;
}
OBB_HD void max_join(double& m, bool& any, double om, bool oany) {
  if (oany) max_take(m, any, om);
}
// ap = 0.; for t: ap = ap + p / 11.
OBB_HD double ap11_of(const double* p, unsigned any_mask) {
  double ap = 0.;
  for (int t = 0; t < kPoints11; t++) ap = ap + (((any_mask >> t) & 1u) ? p[t] : 0.) / 11.;
  return ap;
}
template <typename Rec, typename Prec>
OBB_HD double ap11(long long n, Rec rec, Prec prec) {
  double p[kPoints11];
  unsigned mask = 0;
  for (int t = 0; t < kPoints11; t++) {
    const double th = thr11(t);
    double m = 0.;
    bool any = false;
    for (long long i = 0; i < n; i++)
      if (rec(i) >= th) max_take(m, any, prec(i));
    p[t] = m;
    if (any) mask |= 1u << t;
  }
  return ap11_of(p, mask);
}

// ---- all-point metric (:70-85) ----
// mrec = [0, rec.., 1], mpre = [0, prec.., 0]; k in 0 .. n + 1
template <typename Rec> OBB_HD double mrec_at(long long k, long long n, Rec rec) { return k == 0 ? 0. : (k == n + 1 ? 1. : rec(k - 1)); }
template <typename Prec> OBB_HD double mpre_at(long long k, long long n, Prec prec) { return (k == 0 || k == n + 1) ? 0. : prec(k - 1); }
// term e in 0 .. n of the sum, kept where mrec[e + 1] != mrec[e] (a NaN differs from everything): env = the reverse running
// np.maximum of mpre at e + 1
OBB_HD bool term_kept(double r1, double r0) { return r1 != r0; }
OBB_HD double term_of(double r1, double r0, double env) { return (r1 - r0) * env; }

// pairwise_sum of n <= kLeaf elements
template <typename A>
OBB_HD double sum_leaf(A a, long long o, int n) {
  if (n < 8) {
    double res = -0.0;
    for (int i = 0; i < n; i++) res += a(o + i);
    return res;
  }
  double r0 = a(o), r1 = a(o + 1), r2 = a(o + 2), r3 = a(o + 3), r4 = a(o + 4), r5 = a(o + 5), r6 = a(o + 6), r7 = a(o + 7);
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
    r0 += a(o + i); r1 += a(o + i + 1); r2 += a(o + i + 2); r3 += a(o + i + 3);
    r4 += a(o + i + 4); r5 += a(o + i + 5); r6 += a(o + i + 6); r7 += a(o + i + 7);
  }
  double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
  for (; i < n; i++) res += a(o + i);
  return res;
}

struct SumStack {
  long long off[kSumDepth];
  int len[kSumDepth];
  int state[kSumDepth];       // 0: entered, 1: the left half is in `ret`, 2: the right half is
  double left[kSumDepth];
};

// pairwise_sum of one chunk (n <= kNpBuf), the recursion on an explicit stack
template <typename A>
OBB_HD double sum_chunk(A a, long long o, int n, SumStack* s) {
  int sp = 0;
  double ret = 0.;
  s->off[0] = o; s->len[0] = n; s->state[0] = 0;
  for (;;) {
    const int len = s->len[sp], st = s->state[sp];
    if (st == 0 && len <= kLeaf) {
      ret = sum_leaf(a, s->off[sp], len);
    } else if (st < 2) {
      int n2 = len / 2;
      n2 -= n2 % 8;
      if (st == 1) s->left[sp] = ret;
      s->state[sp] = st + 1;
      s->off[sp + 1] = st == 0 ? s->off[sp] : s->off[sp] + n2;
      s->len[sp + 1] = st == 0 ? n2 : len - n2;
      s->state[sp + 1] = 0;
      sp++;
      continue;
    } else {
      ret = s->left[sp] + ret;
    }
    if (sp == 0) return ret;
    sp--;
  }
}

// np.sum(a[0 .. n))
template <typename A>
OBB_HD double np_sum(A a, long long n, SumStack* s) {
  double res = 0.0;                                // the reduction's identity: the empty sum, and a sum of -0.0s, are +0.0
  for (long long o = 0; o < n; o += kNpBuf) {
    const long long m = n - o < kNpBuf ? n - o : kNpBuf;
    res = res + sum_chunk(a, o, (int)m, s);
  }
  return res;
}

// voc_ap(rec, prec, use_07_metric=False) in one thread: `terms` takes the kept terms (n + 1 doubles at most).  The kernel
// produces the same terms with a workgroup (task1_eval.h: k_t1_ap) and sums them with np_sum.
template <typename Rec, typename Prec>
OBB_HD double ap_all(long long n, Rec rec, Prec prec, double* terms, SumStack* s) {
  long long kept = 0;
  for (long long e = 0; e <= n; e++) kept += term_kept(mrec_at(e + 1, n, rec), mrec_at(e, n, rec)) ? 1 : 0;
  double env = mpre_at(n + 1, n, prec);
  long long w = kept;
  for (long long e = n; e >= 0; e--) {
    if (e < n) env = np_max(mpre_at(e + 1, n, prec), env);
    const double r1 = mrec_at(e + 1, n, rec), r0 = mrec_at(e, n, rec);
    if (term_kept(r1, r0)) terms[--w] = term_of(r1, r0, env);
  }
  return np_sum([&](long long i) { return terms[i]; }, kept, s);
}

// the sort key of a score: unsigned, ascending key = descending score; -0 and +0 are one value, NaN sorts last (np.argsort(-score))
OBB_HD unsigned long long score_key_desc(double score) {
  if (score != score) return ~0ull;
  union { double f; unsigned long long u; } v;
  v.f = score + 0.0;
  const unsigned long long asc = (v.u & 0x8000000000000000ull) ? ~v.u : (v.u | 0x8000000000000000ull);
  return ~asc;
}

// a class or image index as a row carries it (a double): an integer in [0, lim), else -1 (NaN fails every comparison)
OBB_HD long long index_of(double v, long long lim) {
  if (!(v >= 0.0 && v < (double)lim)) return -1;
  const long long c = (long long)v;
  return (double)c == v ? c : -1;
}

}  // namespace vap
}  // namespace obb
