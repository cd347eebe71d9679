// Energy / kurtosis statistics over the augmented population, and the z-normalisation of the packed corpus
// (DESIGN.md section 15): what the reference computes after it has written every variant as a file.
//
// Reference (host, one file per variant):
//   Preprocessor.build_from_path (scripts/preprocessor/preprocessor.py:113-144): per file _remove_outlier (:647-660,
//     np.percentile 25 / 75, fences at 1.5 IQR, both comparisons strict), StandardScaler.partial_fit over what is
//     left, then _normalize (:624-645): (x - mean) / std over every file, min and max of the results.
// A variant's energy array is the base's under the character map sigma of augment.hip, so nothing has to exist but
// the base corpus and the plan: one workgroup per plan row gathers the row's values into LDS, sorts a copy, takes
// numpy's two quartiles operation for operation in fp64, and leaves (kept count, mean, M2, min, max) of the row in
// the workspace; a second launch folds the rows with Chan's pairwise update in one fixed order.  No atomics, no
// order that depends on scheduling: two runs give the same bits.
//
// This file is compiled with -ffp-contract=off (Makefile) and the fences are written with the _rn intrinsics:
// a product fused into a sum would move a fence by an ulp, and the comparisons against it are strict.

#include "vo_common.h"

#include <math.h>

namespace vo {

constexpr int ST_THREADS = 256;
constexpr int ST_REC = 5;  // doubles of a row's record: kept count, mean, M2, min, max

struct StatRow {
  int status;
  int co, n1, L, pos, m;  // first character of src, n', characters out
};

// augment.hip's aug_row without the frames: the same refusals in the same order, the products in 64 bits with each
// factor bounded before the next product.  An accepted row has 1 <= L <= VO_STATS_MAX_CHARS and sigma < n.
__device__ __forceinline__ StatRow stat_row(const vo_corpus& c, const int32_t* __restrict__ plan, int b) {
  StatRow r = {};
  const int32_t* p = plan + (int64_t)b * 5;
  const int src = p[0], pos = p[1], m = p[2], mm = p[3], rep = p[4];
  r.status = VO_AUG_BAD_ROW;
  if (src < 0 || src >= c.U || m < 0 || mm < 0 || rep < 1) return r;
  const int co = c.char_off[src], n = c.char_off[src + 1] - co;
  if (pos < 0 || pos >= n) return r;
  const int64_t n1 = (int64_t)n + m;  // >= 1
  r.status = VO_STATS_CHARS_OVER;
  if (n1 > VO_STATS_MAX_CHARS || n1 * rep > VO_STATS_MAX_CHARS) return r;
  r.status = VO_AUG_OK;
  r.co = co, r.n1 = (int)n1, r.L = (int)(n1 * rep), r.pos = pos, r.m = m;
  return r;
}

__device__ __forceinline__ int stat_sigma(const StatRow& r, int jp) {
  return r.co + (jp < r.pos ? jp : (jp <= r.pos + r.m ? r.pos : jp - r.m));
}

// np.percentile(v, 100 q), method "linear", on the sorted keys of a row without NaN: the virtual index (L - 1) q is
// exact for q = 0.25, 0.75 and L <= 4096, and _lerp's two branches are kept as they are.  L = 1 is numpy's
// "index above bounds" case: both neighbours are the last element.
__device__ __forceinline__ double stat_quantile(const float* key, int L, double q) {
  if (L == 1) return (double)key[0];
  const double h = __dmul_rn((double)(L - 1), q);
  const int lo = (int)h;  // h >= 0: the floor; lo + 1 <= L - 1 as h < L - 1
  const double t = h - (double)lo;
  const double a = (double)key[lo], b = (double)key[lo + 1];
  const double d = __dsub_rn(b, a);
  return t < 0.5 ? __dadd_rn(a, __dmul_rn(d, t)) : __dsub_rn(b, __dmul_rn(d, __dsub_rn(1.0, t)));
}

// sum over the workgroup in a fixed tree; every thread gets it.  red: ST_THREADS doubles.
__device__ __forceinline__ double block_sum(double v, double* red, int tid) {
  __syncthreads();  // red may still be read from the previous use
  red[tid] = v;
  __syncthreads();
  for (int s = ST_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  return red[0];
}

__global__ void __launch_bounds__(ST_THREADS) corpus_stats_rows_kernel(vo_corpus c, const int32_t* __restrict__ plan,
                                                                      const float* __restrict__ x,
                                                                      double* __restrict__ rec,
                                                                      int32_t* __restrict__ status) {
  __shared__ float raw[VO_STATS_MAX_CHARS];  // the row's values in the row's order
  __shared__ float key[VO_STATS_MAX_CHARS];  // sorted
  __shared__ double red[ST_THREADS];
  __shared__ float red_mn[ST_THREADS], red_mx[ST_THREADS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const StatRow r = stat_row(c, plan, b);  // uniform over the workgroup
  double* out = rec + (int64_t)b * ST_REC;
  if (tid == 0 && status) status[b] = r.status;
  if (r.status != VO_AUG_OK) {  // contributes nothing
    if (tid == 0) out[0] = 0.0, out[1] = 0.0, out[2] = 0.0, out[3] = INFINITY, out[4] = -INFINITY;
    return;
  }
  const int L = r.L;
  int P = 2;
  while (P < L) P <<= 1;  // <= VO_STATS_MAX_CHARS, a power of two

  float mn = INFINITY, mx = -INFINITY;
  int nan = 0;
  for (int j = tid; j < P; j += ST_THREADS) {
    float v = INFINITY;  // the padding sorts behind every value
    if (j < L) {
      v = x[stat_sigma(r, j % r.n1)];
      raw[j] = v;
      mn = fminf(mn, v), mx = fmaxf(mx, v);
      nan |= v != v;
    }
    key[j] = v;
  }
  nan = __syncthreads_or(nan);  // also the barrier behind the gather

  // bitonic network over P keys: step (k, j) compares i and i + j for every i with bit j clear, ascending where bit
  // k of i is clear.  A step reads what the step before wrote in other threads: one barrier a step, and P is
  // uniform, so every thread meets every barrier.
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (P >> 1); t += ST_THREADS) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const float a = key[i], bb = key[i + j];
        if ((a > bb) == ((i & k) == 0)) key[i] = bb, key[i + j] = a;
      }
      __syncthreads();
    }
  }

  // every thread takes the quartiles itself (broadcast reads): no barrier for them
  const double p25 = stat_quantile(key, L, 0.25), p75 = stat_quantile(key, L, 0.75);
  const double iqr15 = __dmul_rn(1.5, __dsub_rn(p75, p25));
  const double lower = __dsub_rn(p25, iqr15), upper = __dadd_rn(p75, iqr15);

  // the kept count and sum, then M2 about the kept mean: each thread its strided elements in order, then the tree
  double cnt = 0.0, s = 0.0;
  if (!nan)  // numpy's percentile of a row with a NaN is NaN: every comparison fails
    for (int j = tid; j < L; j += ST_THREADS) {
      const double v = (double)raw[j];
      if (v > lower && v < upper) cnt += 1.0, s += v;
    }
  const double k = block_sum(cnt, red, tid);  // exact: integers up to 4096
  const double sum = block_sum(s, red, tid);
  const double mean = k > 0.0 ? sum / k : 0.0;
  double q = 0.0;
  if (!nan)
    for (int j = tid; j < L; j += ST_THREADS) {
      const double v = (double)raw[j];
      if (v > lower && v < upper) q += (v - mean) * (v - mean);
    }
  const double M2 = block_sum(q, red, tid);

  red_mn[tid] = mn, red_mx[tid] = mx;
  __syncthreads();
  for (int st = ST_THREADS / 2; st > 0; st >>= 1) {
    if (tid < st) {
      red_mn[tid] = fminf(red_mn[tid], red_mn[tid + st]);
      red_mx[tid] = fmaxf(red_mx[tid], red_mx[tid + st]);
    }
    __syncthreads();
  }
  if (tid == 0) out[0] = k, out[1] = mean, out[2] = M2, out[3] = (double)red_mn[0], out[4] = (double)red_mx[0];
}

struct StatAcc {
  double k, mean, M2, mn, mx, used;
};

// Chan, Golub and LeVeque's update of (count, mean, M2) for the union of two sets; an empty side leaves the other
__device__ __forceinline__ StatAcc stat_merge(const StatAcc& a, const StatAcc& b) {
  StatAcc o;
  o.mn = fmin(a.mn, b.mn), o.mx = fmax(a.mx, b.mx), o.used = a.used + b.used;
  if (b.k == 0.0) {
    o.k = a.k, o.mean = a.mean, o.M2 = a.M2;
  } else if (a.k == 0.0) {
    o.k = b.k, o.mean = b.mean, o.M2 = b.M2;
  } else {
    const double n = a.k + b.k, delta = b.mean - a.mean;
    o.k = n;
    o.mean = a.mean + delta * (b.k / n);
    o.M2 = a.M2 + b.M2 + delta * delta * (a.k * b.k / n);
  }
  return o;
}

// One workgroup: thread t folds rows t, t + 256, ... in order, then the 256 partial results fold in a tree.  The
// order depends on n_rows alone.
__global__ void __launch_bounds__(ST_THREADS) corpus_stats_combine_kernel(const double* __restrict__ rec, int n_rows,
                                                                         double* __restrict__ out) {
  __shared__ StatAcc acc[ST_THREADS];
  const int tid = threadIdx.x;
  StatAcc a = {0.0, 0.0, 0.0, INFINITY, -INFINITY, 0.0};
  for (int64_t row = tid; row < n_rows; row += ST_THREADS) {
    const double* p = rec + row * ST_REC;
    const StatAcc b = {p[0], p[1], p[2], p[3], p[4], p[0] > 0.0 ? 1.0 : 0.0};
    a = stat_merge(a, b);
  }
  acc[tid] = a;
  __syncthreads();
  for (int s = ST_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) acc[tid] = stat_merge(acc[tid], acc[tid + s]);
    __syncthreads();
  }
  if (tid == 0) {
    const StatAcc t = acc[0];
    double sd = t.k > 0.0 ? sqrt(t.M2 / t.k) : 0.0;
    if (sd == 0.0) sd = 1.0;  // StandardScaler's handling of a zero variance
    out[0] = t.k, out[1] = t.mean, out[2] = sd, out[3] = t.mn, out[4] = t.mx, out[5] = t.used;
  }
}

__global__ void __launch_bounds__(256) corpus_normalize_kernel(float* __restrict__ values, int64_t n,
                                                               const double* __restrict__ stats) {
  const double mean = stats[1], sd = stats[2];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) values[i] = (float)__ddiv_rn(__dsub_rn((double)values[i], mean), sd);
}

}  // namespace vo

using namespace vo;

extern "C" int64_t vo_corpus_stats_workspace_size(int n_rows) {
  return n_rows > 0 ? (int64_t)n_rows * ST_REC * (int64_t)sizeof(double) : 0;
}

extern "C" int vo_corpus_stats(const vo_corpus* c, const int32_t* plan, int n_rows, int feature, void* workspace,
                               int64_t workspace_bytes, double* out, int32_t* status, void* stream) {
  VO_CHECK_ARG(c && plan && workspace && out, "corpus_stats: null pointer");
  VO_CHECK_ARG(c->char_off, "corpus_stats: null pointer in the corpus");
  VO_CHECK_ARG(c->U > 0, "corpus_stats: empty corpus");
  VO_CHECK_ARG(feature == VO_STATS_ENERGY || feature == VO_STATS_KURTOSIS,
               "corpus_stats: feature %d is neither energy (0) nor kurtosis (1)", feature);
  const float* x = feature == VO_STATS_ENERGY ? c->ch_energy : c->ch_kurtosis;
  VO_CHECK_ARG(x, "corpus_stats: the corpus was packed without %s", feature == VO_STATS_ENERGY ? "energy" : "kurtosis");
  VO_CHECK_ARG(n_rows > 0, "corpus_stats: n_rows %d", n_rows);
  VO_CHECK_ARG(reinterpret_cast<uintptr_t>(workspace) % 8 == 0 && reinterpret_cast<uintptr_t>(out) % 8 == 0,
               "corpus_stats: workspace and out must be 8-byte aligned");
  VO_CHECK_ARG(workspace_bytes >= vo_corpus_stats_workspace_size(n_rows),
               "corpus_stats: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
               (long long)vo_corpus_stats_workspace_size(n_rows));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  double* rec = static_cast<double*>(workspace);
  hipLaunchKernelGGL(corpus_stats_rows_kernel, dim3((unsigned)n_rows), dim3(ST_THREADS), 0, st, *c, plan, x, rec,
                     status);
  hipLaunchKernelGGL(corpus_stats_combine_kernel, dim3(1), dim3(ST_THREADS), 0, st, rec, n_rows, out);
  VO_RETURN_LAUNCH();
}

extern "C" int vo_corpus_normalize(float* values, int64_t n, const double* stats, void* stream) {
  VO_CHECK_ARG(values && stats, "corpus_normalize: null pointer");
  VO_CHECK_ARG(reinterpret_cast<uintptr_t>(stats) % 8 == 0, "corpus_normalize: stats must be 8-byte aligned");
  VO_CHECK_ARG(n > 0 && (n + 255) / 256 < ((int64_t)1 << 31), "corpus_normalize: n %lld", (long long)n);
  hipLaunchKernelGGL(corpus_normalize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), values, n, stats);
  VO_RETURN_LAUNCH();
}
