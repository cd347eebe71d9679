// BatchNorm with batch statistics over channels-last rows (x: M rows x C channels), training-step glue that
// round 1 left on PyTorch-ROCm (config C4 / C5 backward): forward (Welford partials per row block merged in a
// fixed order -> mean / biased var, the running statistics update of nn.BatchNorm*, normalize + affine) and
// backward (dx = g rstd (dy - mean(dy) - xhat mean(dy xhat)), dgamma = sum dy xhat, dbeta = sum dy):
// PostNet's BatchNorm1d on (B, T, C) activations (scripts/transformer/Layers.py:67-137) and the glyph
// encoder's single-channel BatchNorm2d (scripts/model/visual_feature_extractor.py:40-47, C = 1: rows = every
// pixel).  Everything deterministic (no atomics).

#include <algorithm>

#include "vo_common.h"

namespace vo {

struct Welford {
  float n, mean, m2;
};

__device__ __forceinline__ Welford wf_merge(Welford a, Welford b) {
  if (b.n == 0.f) return a;
  if (a.n == 0.f) return b;
  const float n = a.n + b.n;
  const float d = b.mean - a.mean;
  const float fb = b.n / n;
  return Welford{n, a.mean + d * fb, a.m2 + b.m2 + d * d * a.n * fb};
}

// block: 256 threads = CT channels x (256 / CT) row lanes; rows [blockIdx.x * RB, +RB)
template <typename TX, int CT>
__global__ void __launch_bounds__(256) bn_stats_kernel(const TX* __restrict__ x, int M, int C, int RB,
                                                       float* __restrict__ part) {
  constexpr int RS = 256 / CT;
  __shared__ float sn[256], sm[256], s2[256];
  const int tid = threadIdx.x;
  const int cl = tid % CT, rl = tid / CT;
  const int c = blockIdx.y * CT + cl;
  const int r0 = blockIdx.x * RB;
  const int r1 = min(r0 + RB, M);
  Welford w{0.f, 0.f, 0.f};
  if (c < C) {
    for (int r = r0 + rl; r < r1; r += RS) {
      const float v = to_f32(x[(int64_t)r * C + c]);
      w.n += 1.f;
      const float d = v - w.mean;
      w.mean += d / w.n;
      w.m2 += d * (v - w.mean);
    }
  }
  sn[tid] = w.n; sm[tid] = w.mean; s2[tid] = w.m2;
  __syncthreads();
  if (rl == 0 && c < C) {
    for (int k = 1; k < RS; ++k) w = wf_merge(w, Welford{sn[k * CT + cl], sm[k * CT + cl], s2[k * CT + cl]});
    float* p = part + ((int64_t)blockIdx.x * C + c) * 3;
    p[0] = w.n; p[1] = w.mean; p[2] = w.m2;
  }
}

// per channel: merge the row-block partials in order; mean / rstd for the normalisation and the
// backward; running statistics: (1 - m) r + m stat, the variance unbiased (n / (n - 1))
__global__ void bn_finalize_kernel(const float* __restrict__ part, int nb, int C, float eps, float momentum,
                                   float* __restrict__ mean_rstd, float* __restrict__ run_mean,
                                   float* __restrict__ run_var, int64_t* __restrict__ nbt) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c == 0 && nbt) nbt[0] += 1;
  if (c >= C) return;
  Welford w{0.f, 0.f, 0.f};
  for (int b = 0; b < nb; ++b) {
    const float* p = part + ((int64_t)b * C + c) * 3;
    w = wf_merge(w, Welford{p[0], p[1], p[2]});
  }
  const float var = w.n > 0.f ? w.m2 / w.n : 0.f;
  mean_rstd[c] = w.mean;
  mean_rstd[C + c] = rsqrtf(var + eps);
  if (run_mean) {
    run_mean[c] = (1.f - momentum) * run_mean[c] + momentum * w.mean;
    const float unb = w.n > 1.f ? w.m2 / (w.n - 1.f) : var;
    run_var[c] = (1.f - momentum) * run_var[c] + momentum * unb;
  }
}

template <typename TX>
__global__ void __launch_bounds__(256) bn_apply_kernel(const TX* __restrict__ x, int64_t total, int C,
                                                       const float* __restrict__ mean_rstd,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       TX* __restrict__ y) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % C);
    float v = (to_f32(x[i]) - mean_rstd[c]) * mean_rstd[C + c];
    if (gamma) v = v * gamma[c] + beta[c];
    y[i] = from_f32<TX>(v);
  }
}

// backward partial sums per row block: [sum dy, sum dy * xhat] per channel
template <typename TX, typename TG, int CT>
__global__ void __launch_bounds__(256) bn_bwd_stats_kernel(const TX* __restrict__ x, const TG* __restrict__ dy,
                                                           int M, int C, int RB, const float* __restrict__ mean_rstd,
                                                           float* __restrict__ part) {
  constexpr int RS = 256 / CT;
  __shared__ float sa[256], sb[256];
  const int tid = threadIdx.x;
  const int cl = tid % CT, rl = tid / CT;
  const int c = blockIdx.y * CT + cl;
  const int r0 = blockIdx.x * RB;
  const int r1 = min(r0 + RB, M);
  float a = 0.f, bsum = 0.f;
  if (c < C) {
    const float mu = mean_rstd[c], rs = mean_rstd[C + c];
    for (int r = r0 + rl; r < r1; r += RS) {
      const int64_t i = (int64_t)r * C + c;
      const float g = to_f32(dy[i]);
      a += g;
      bsum += g * (to_f32(x[i]) - mu) * rs;
    }
  }
  sa[tid] = a; sb[tid] = bsum;
  __syncthreads();
  if (rl == 0 && c < C) {
    for (int k = 1; k < RS; ++k) {
      a += sa[k * CT + cl];
      bsum += sb[k * CT + cl];
    }
    float* p = part + ((int64_t)blockIdx.x * C + c) * 2;
    p[0] = a; p[1] = bsum;
  }
}

__global__ void bn_bwd_finalize_kernel(const float* __restrict__ part, int nb, int C, float* __restrict__ dgamma,
                                       float* __restrict__ dbeta) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float a = 0.f, b = 0.f;
  for (int k = 0; k < nb; ++k) {
    a += part[((int64_t)k * C + c) * 2];
    b += part[((int64_t)k * C + c) * 2 + 1];
  }
  dbeta[c] = a;
  dgamma[c] = b;
}

template <typename TX, typename TG>
__global__ void __launch_bounds__(256) bn_bwd_apply_kernel(const TX* __restrict__ x, const TG* __restrict__ dy,
                                                           int64_t total, int C, float inv_m,
                                                           const float* __restrict__ mean_rstd,
                                                           const float* __restrict__ gamma,
                                                           const float* __restrict__ dgamma,
                                                           const float* __restrict__ dbeta, TX* __restrict__ dx) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % C);
    const float rs = mean_rstd[C + c];
    const float xh = (to_f32(x[i]) - mean_rstd[c]) * rs;
    const float g = gamma ? gamma[c] : 1.f;
    const float v = g * rs * (to_f32(dy[i]) - dbeta[c] * inv_m - xh * dgamma[c] * inv_m);
    dx[i] = from_f32<TX>(v);
  }
}

// ---- vectorised BatchNorm (16-byte vectors: 8 bf16 / 4 fp32 channels per lane).  The scalar kernels
// above read 2-4 bytes per lane and run a division per element (Welford) and serial partial merges:
// at PostNet's 16384 x 512 bf16 a forward took 71 us and a backward 75 us (C4 trace, round 5).  Here
// each lane sums (v - k) and (v - k)^2 against the first value it read (k), converted to a Welford
// triple once; the row lanes of a block, the blocks and (FLAT: C = 1, every element one channel) the
// lanes of a vector merge in a fixed order, so results stay deterministic.
// (BnVec, one 16-byte vector of a lane: vo_common.h -- vo_dropout reads and writes the same vectors)

constexpr int BN_NB = 128;  // row blocks (partials per channel) of the vectorised kernels
constexpr int BN_CMAX = 2048;  // channels of the vectorised kernels (C / V <= 256 vector columns)

// part[block][c] = (n, mean, m2).  Non-FLAT: CV = C / V vector columns, RL = 256 / CV row lanes, rows
// [blockIdx.x RB, +RB) of M.  FLAT (C = 1): the M elements as M / V rows of one vector.
template <typename TX, bool FLAT>
__global__ void __launch_bounds__(256) bn_stats_v_kernel(const TX* __restrict__ x, int rows, int C, int RB,
                                                         float* __restrict__ part) {
  using VT = BnVec<TX>;
  constexpr int V = VT::V;
  __shared__ float sn[256], sm[256 * V], s2[256 * V];
  const int CV = FLAT ? 1 : C / V, RL = 256 / CV;
  const int tid = threadIdx.x, vc = tid % CV, rl = tid / CV;
  const int r0 = blockIdx.x * RB, r1 = min(r0 + RB, rows);
  float k[V], a1[V], a2[V];
  int n = 0;
#pragma unroll
  for (int e = 0; e < V; ++e) k[e] = a1[e] = a2[e] = 0.f;
  if (rl < RL && r0 + rl < r1) {
    VT::load(x + ((int64_t)(r0 + rl) * CV + vc) * V, k);
    for (int r = r0 + rl; r < r1; r += RL) {
      float v[V];
      VT::load(x + ((int64_t)r * CV + vc) * V, v);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const float d = v[e] - k[e];
        a1[e] += d;
        a2[e] = fmaf(d, d, a2[e]);
      }
      ++n;
    }
  }
  // the lane's Welford triple per vector element
  const float fn = (float)n, inv = n ? 1.f / fn : 0.f;
  if (FLAT) {  // merge the V elements (one channel) in order
    Welford w{0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < V; ++e) w = wf_merge(w, Welford{fn, k[e] + a1[e] * inv, a2[e] - a1[e] * a1[e] * inv});
    sn[tid] = w.n; sm[tid] = w.mean; s2[tid] = w.m2;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {  // pairwise tree over the 256 lanes (fixed order)
      if (tid < h) {
        const Welford m = wf_merge(Welford{sn[tid], sm[tid], s2[tid]}, Welford{sn[tid + h], sm[tid + h], s2[tid + h]});
        sn[tid] = m.n; sm[tid] = m.mean; s2[tid] = m.m2;
      }
      __syncthreads();
    }
    if (tid == 0) {
      float* p = part + (int64_t)blockIdx.x * 3;
      p[0] = sn[0]; p[1] = sm[0]; p[2] = s2[0];
    }
    return;
  }
  sn[tid] = fn;
#pragma unroll
  for (int e = 0; e < V; ++e) {
    sm[tid * V + e] = k[e] + a1[e] * inv;
    s2[tid * V + e] = a2[e] - a1[e] * a1[e] * inv;
  }
  __syncthreads();
  for (int c = tid; c < C; c += 256) {  // channel c = vector column c / V, element c % V: merge the row lanes
    const int cv = c / V, e = c % V;
    Welford w{0.f, 0.f, 0.f};
    for (int l = 0; l < RL; ++l) {
      const int t = l * CV + cv;
      w = wf_merge(w, Welford{sn[t], sm[t * V + e], s2[t * V + e]});
    }
    float* p = part + ((int64_t)blockIdx.x * C + c) * 3;
    p[0] = w.n; p[1] = w.mean; p[2] = w.m2;
  }
}

// finalize: 8 lanes per channel, lane s merging partials s, s + 8, .. (loads issued ahead), then the 8
// lane results merged in lane order -- a fixed order (deterministic).  One lane walking all 128
// partials took 17 us (serial merges with a division each, behind one load latency per step).
constexpr int BN_FL = 8;
__global__ void __launch_bounds__(256) bn_finalize_v_kernel(const float* __restrict__ part, int nb, int C, float eps,
                                                            float momentum, float* __restrict__ mean_rstd,
                                                            float* __restrict__ run_mean, float* __restrict__ run_var,
                                                            int64_t* __restrict__ nbt) {
  __shared__ float sn[256], sm[256], s2[256];
  const int tid = threadIdx.x, sl = tid % BN_FL;
  const int c = blockIdx.x * (256 / BN_FL) + tid / BN_FL;
  if (blockIdx.x == 0 && tid == 0 && nbt) nbt[0] += 1;
  Welford w{0.f, 0.f, 0.f};
  if (c < C) {
    for (int b0 = sl; b0 < nb; b0 += 4 * BN_FL) {
      float q[4][3];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int b = min(b0 + i * BN_FL, nb - 1);
        const float* p = part + ((int64_t)b * C + c) * 3;
        q[i][0] = p[0]; q[i][1] = p[1]; q[i][2] = p[2];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (b0 + i * BN_FL < nb) w = wf_merge(w, Welford{q[i][0], q[i][1], q[i][2]});
    }
  }
  sn[tid] = w.n; sm[tid] = w.mean; s2[tid] = w.m2;
  __syncthreads();
  if (sl != 0 || c >= C) return;
  for (int k = 1; k < BN_FL; ++k) w = wf_merge(w, Welford{sn[tid + k], sm[tid + k], s2[tid + k]});
  const float var = w.n > 0.f ? w.m2 / w.n : 0.f;
  mean_rstd[c] = w.mean;
  mean_rstd[C + c] = rsqrtf(var + eps);
  if (run_mean) {
    run_mean[c] = (1.f - momentum) * run_mean[c] + momentum * w.mean;
    const float unb = w.n > 1.f ? w.m2 / (w.n - 1.f) : var;
    run_var[c] = (1.f - momentum) * run_var[c] + momentum * unb;
  }
}

// apply: the grid's thread count is a multiple of CV (the launcher rounds it), so a thread's vector
// column -- and its channels' parameters, loaded once -- stays the same over the grid-stride loop
// (per-element parameter loads, 8 channels 32 bytes apart per lane, ran the kernel at 59 us)
template <typename TX, bool FLAT>
__global__ void __launch_bounds__(256) bn_apply_v_kernel(const TX* __restrict__ x, int nvec, int C,
                                                         const float* __restrict__ mean_rstd,
                                                         const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, TX* __restrict__ y) {
  using VT = BnVec<TX>;
  constexpr int V = VT::V;
  const int CV = FLAT ? 1 : C / V;
  const int i0 = blockIdx.x * 256 + threadIdx.x;
  const int c0 = FLAT ? 0 : (i0 % CV) * V;
  // the block's copy of the per-channel parameters (coalesced), then 8 consecutive per thread from LDS
  // (each thread loading its own 8-channel run from global was the kernel's cost: 32 scattered loads)
  __shared__ float sp[4][BN_CMAX];
  for (int c = threadIdx.x; c < C; c += 256) {
    sp[0][c] = mean_rstd[c]; sp[1][c] = mean_rstd[C + c];
    sp[2][c] = gamma ? gamma[c] : 1.f; sp[3][c] = gamma ? beta[c] : 0.f;
  }
  __syncthreads();
  float mu[V], rs[V], ga[V], be[V];
#pragma unroll
  for (int e = 0; e < V; ++e) {
    const int c = FLAT ? 0 : c0 + e;
    mu[e] = sp[0][c]; rs[e] = sp[1][c]; ga[e] = sp[2][c]; be[e] = sp[3][c];
  }
  // four vectors in flight per thread (one load, wait, compute, store at a time ran at 0.9 TB/s)
  const int stride = gridDim.x * 256;
  for (int i = i0; i < nvec; i += 4 * stride) {
    float v[4][V];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (i + u * stride < nvec) VT::load(x + (int64_t)(i + u * stride) * V, v[u]);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const float t = (v[u][e] - mu[e]) * rs[e];
        v[u][e] = gamma ? t * ga[e] + be[e] : t;
      }
      if (i + u * stride < nvec) VT::store(y + (int64_t)(i + u * stride) * V, v[u]);
    }
  }
}

// one vector of dy beside a vector of x: the same width, or (x fp32, 4 per vector; dy bf16) an 8-byte load
template <typename TX, typename TG>
__device__ __forceinline__ void bn_load_dy(const TG* p, float (&gv)[BnVec<TX>::V]) {
  if constexpr (sizeof(TG) == sizeof(TX)) {
    BnVec<TG>::load(p, gv);
  } else {
    const uint2 u = *reinterpret_cast<const uint2*>(p);
    gv[0] = __uint_as_float(u.x << 16); gv[1] = __uint_as_float(u.x & 0xffff0000u);
    gv[2] = __uint_as_float(u.y << 16); gv[3] = __uint_as_float(u.y & 0xffff0000u);
  }
}

// backward partials per row block: part[block][c] = (sum dy, sum dy xhat); FLAT: as doubles
template <typename TX, typename TG, bool FLAT>
__global__ void __launch_bounds__(256) bn_bwd_stats_v_kernel(const TX* __restrict__ x, const TG* __restrict__ dy,
                                                             int rows, int C, int RB,
                                                             const float* __restrict__ mean_rstd,
                                                             float* __restrict__ part) {
  constexpr int V = BnVec<TX>::V;
  static_assert(BnVec<TG>::V >= V, "dy vector at least as wide as x's");
  __shared__ float sa[256 * V], sb[256 * V];
  const int CV = FLAT ? 1 : C / V, RL = 256 / CV;
  const int tid = threadIdx.x, vc = tid % CV, rl = tid / CV;
  const int r0 = blockIdx.x * RB, r1 = min(r0 + RB, rows);
  if constexpr (FLAT) {
    // C = 1 (the glyph encoder's maps): xhat, the products and both sums in double, the partials doubles too.
    // Where another batch-statistics BatchNorm follows, d gamma is the small remainder of cancelling terms
    // (sum |dy xhat| = 1700 |d gamma| at 2400 elements): fp32 terms and sums leave it 1e-5 off.
    __shared__ double da[256], db[256];
    const double mu = mean_rstd[0], rs = mean_rstd[1];
    double a = 0., b = 0.;
    for (int r = r0 + tid; r < r1; r += 256) {
      const int64_t o = (int64_t)r * V;
      float xv[V], gv[V];
      BnVec<TX>::load(x + o, xv);
      bn_load_dy<TX, TG>(dy + o, gv);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        a += (double)gv[e];
        b = fma((double)gv[e], ((double)xv[e] - mu) * rs, b);
      }
    }
    da[tid] = a; db[tid] = b;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {  // pairwise tree over the 256 lanes (fixed order)
      if (tid < h) { da[tid] += da[tid + h]; db[tid] += db[tid + h]; }
      __syncthreads();
    }
    if (tid == 0) {
      double* p = reinterpret_cast<double*>(part) + (int64_t)blockIdx.x * 2;
      p[0] = da[0]; p[1] = db[0];
    }
    return;
  }
  float mu[V], rs[V], a[V], b[V];
#pragma unroll
  for (int e = 0; e < V; ++e) {
    const int c = vc * V + e;
    mu[e] = mean_rstd[c]; rs[e] = mean_rstd[C + c];
    a[e] = b[e] = 0.f;
  }
  if (rl < RL)
    for (int r = r0 + rl; r < r1; r += RL) {
      const int64_t o = ((int64_t)r * CV + vc) * V;
      float xv[V], gv[V];
      BnVec<TX>::load(x + o, xv);
      bn_load_dy<TX, TG>(dy + o, gv);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        a[e] += gv[e];
        b[e] = fmaf(gv[e], (xv[e] - mu[e]) * rs[e], b[e]);
      }
    }
#pragma unroll
  for (int e = 0; e < V; ++e) { sa[tid * V + e] = a[e]; sb[tid * V + e] = b[e]; }
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    const int cv = c / V, e = c % V;
    float ta = 0.f, tb = 0.f;
    for (int l = 0; l < RL; ++l) {
      const int t = (l * CV + cv) * V + e;
      ta += sa[t]; tb += sb[t];
    }
    float* p = part + ((int64_t)blockIdx.x * C + c) * 2;
    p[0] = ta; p[1] = tb;
  }
}

__global__ void __launch_bounds__(256) bn_bwd_finalize_v_kernel(const float* __restrict__ part, int nb, int C,
                                                                float* __restrict__ dgamma, float* __restrict__ dbeta) {
  __shared__ float sa[256], sb[256];
  const int tid = threadIdx.x, sl = tid % BN_FL;
  const int c = blockIdx.x * (256 / BN_FL) + tid / BN_FL;
  float a = 0.f, b = 0.f;
  if (c < C) {
    for (int k0 = sl; k0 < nb; k0 += 4 * BN_FL) {
      float q[4][2];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = min(k0 + i * BN_FL, nb - 1);
        q[i][0] = part[((int64_t)k * C + c) * 2];
        q[i][1] = part[((int64_t)k * C + c) * 2 + 1];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (k0 + i * BN_FL < nb) { a += q[i][0]; b += q[i][1]; }
    }
  }
  sa[tid] = a; sb[tid] = b;
  __syncthreads();
  if (sl != 0 || c >= C) return;
  for (int k = 1; k < BN_FL; ++k) { a += sa[tid + k]; b += sb[tid + k]; }
  dbeta[c] = a;
  dgamma[c] = b;
}

// FLAT: the nb <= BN_NB double partials summed by a fixed tree; tot = (sum dy, sum dy xhat) stays in double
// for the apply kernel (one ulp of fp32 on d gamma of the second glyph BatchNorm is 3e-6 on the first's)
__global__ void __launch_bounds__(BN_NB) bn_bwd_finalize_flat_kernel(const double* __restrict__ part, int nb,
                                                                     float* __restrict__ dgamma,
                                                                     float* __restrict__ dbeta, double* __restrict__ tot) {
  __shared__ double sa[BN_NB], sb[BN_NB];
  const int tid = threadIdx.x;
  sa[tid] = tid < nb ? part[2 * tid] : 0.;
  sb[tid] = tid < nb ? part[2 * tid + 1] : 0.;
  __syncthreads();
  for (int h = BN_NB / 2; h >= 1; h >>= 1) {
    if (tid < h) { sa[tid] += sa[tid + h]; sb[tid] += sb[tid + h]; }
    __syncthreads();
  }
  if (tid == 0) {
    tot[0] = sa[0]; tot[1] = sb[0];
    dbeta[0] = (float)sa[0];
    dgamma[0] = (float)sb[0];
  }
}

// tot: FLAT only (bn_bwd_finalize_flat_kernel's sums)
template <typename TX, typename TG, bool FLAT>
__global__ void __launch_bounds__(256) bn_bwd_apply_v_kernel(const TX* __restrict__ x, const TG* __restrict__ dy,
                                                             int nvec, int C, float inv_m,
                                                             const float* __restrict__ mean_rstd,
                                                             const float* __restrict__ gamma,
                                                             const float* __restrict__ dgamma,
                                                             const float* __restrict__ dbeta,
                                                             const double* __restrict__ tot, TX* __restrict__ dx) {
  constexpr int V = BnVec<TX>::V;
  const int i0 = blockIdx.x * 256 + threadIdx.x;
  if constexpr (FLAT) {  // every element in double from the double sums, rounded once
    const double im = 1. / ((double)nvec * V);
    const double mu = mean_rstd[0], rs = mean_rstd[1], gr = (gamma ? (double)gamma[0] : 1.) * rs;
    const double db = tot[0] * im, dg = tot[1] * im;
    for (int i = i0; i < nvec; i += gridDim.x * 256) {
      float xv[V], gv[V];
      BnVec<TX>::load(x + (int64_t)i * V, xv);
      bn_load_dy<TX, TG>(dy + (int64_t)i * V, gv);
#pragma unroll
      for (int e = 0; e < V; ++e) xv[e] = (float)(gr * ((double)gv[e] - db - ((double)xv[e] - mu) * rs * dg));
      BnVec<TX>::store(dx + (int64_t)i * V, xv);
    }
    return;
  }
  const int CV = C / V;
  const int c0 = (i0 % CV) * V;
  __shared__ float sp[5][BN_CMAX];  // per-channel parameters staged once per block (see bn_apply_v_kernel)
  for (int c = threadIdx.x; c < C; c += 256) {
    sp[0][c] = mean_rstd[c]; sp[1][c] = mean_rstd[C + c];
    sp[2][c] = (gamma ? gamma[c] : 1.f) * mean_rstd[C + c];
    sp[3][c] = dbeta[c] * inv_m; sp[4][c] = dgamma[c] * inv_m;
  }
  __syncthreads();
  float mu[V], rs[V], gr[V], db[V], dg[V];  // gr = gamma rstd, db / dg = dbeta / M, dgamma / M
#pragma unroll
  for (int e = 0; e < V; ++e) {
    const int c = c0 + e;
    mu[e] = sp[0][c]; rs[e] = sp[1][c]; gr[e] = sp[2][c]; db[e] = sp[3][c]; dg[e] = sp[4][c];
  }
  const int stride = gridDim.x * 256;
  for (int i = i0; i < nvec; i += 2 * stride) {  // two vectors of x and dy in flight per thread
    float xv[2][V], gv[2][V];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (i + u * stride >= nvec) continue;
      const int64_t o = (int64_t)(i + u * stride) * V;
      BnVec<TX>::load(x + o, xv[u]);
      bn_load_dy<TX, TG>(dy + o, gv[u]);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (i + u * stride >= nvec) continue;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const float xh = (xv[u][e] - mu[e]) * rs[e];
        xv[u][e] = gr[e] * (gv[u][e] - db[e] - xh * dg[e]);
      }
      BnVec<TX>::store(dx + (int64_t)(i + u * stride) * V, xv[u]);
    }
  }
}

}  // namespace vo

using namespace vo;

// ---- BatchNorm: x (M, C) channels-last, dtype VO_F32 / VO_BF16; workspace: bn workspace size
// the vectorised kernels cover C % V == 0 with C / V <= 256 vector columns (V = 8 bf16 / 4 fp32), and
// C = 1 with M % V == 0 (FLAT); other shapes take the scalar kernels
static bool bn_vec_ok(int M, int C, int dtype, bool* flat) {
  const int V = dtype == VO_BF16 ? 8 : 4;
  *flat = C == 1;
  if (C == 1) return M % V == 0;
  return C % V == 0 && C / V <= 256;
}

// apply grid: at most 2048 blocks, the thread count a multiple of the CV vector columns (so that every
// thread keeps one column: bn_apply_v_kernel)
static unsigned bn_apply_blocks(int nvec, int CV) {
  int g = 256, c = CV;
  while (c) { const int t = g % c; g = c; c = t; }  // gcd(256, CV)
  const int step = CV / g;
  int64_t blk = std::min<int64_t>((nvec + 1023) / 1024, 1024);  // ~4 vectors per thread (4096 blocks: 3x slower)
  blk = (blk + step - 1) / step * step;
  return (unsigned)std::max<int64_t>(blk, step);
}

static void bn_vec_geometry(int M, int C, int dtype, bool flat, int* rows, int* RB, int* nb) {
  const int V = dtype == VO_BF16 ? 8 : 4;
  *rows = flat ? M / V : M;
  const int RL = flat ? 256 : 256 / (C / V);
  int rb = (*rows + BN_NB - 1) / BN_NB;
  rb = (rb + RL - 1) / RL * RL;  // whole passes of the block's row lanes
  *RB = rb > 0 ? rb : RL;
  *nb = (*rows + *RB - 1) / *RB;
}

// the scalar kernels: CT channels x 256 / CT row lanes per block, RB rows per block
static void bn_geometry(int M, int C, int* CT, int* RB, int* nb) {
  *CT = C == 1 ? 1 : 64;
  *RB = C == 1 ? 8192 : 512;
  *nb = (M + *RB - 1) / *RB;
}

// 3 values per channel and row block: the scalar route's nb, the vector kernels' <= BN_NB (C = 1: doubles, backward)
extern "C" int64_t vo_bn_workspace_size(int M, int C) {
  int CT, RB, nb;
  bn_geometry(M, C, &CT, &RB, &nb);
  return std::max<int64_t>(nb, BN_NB) * C * 3 * (int64_t)(C == 1 ? sizeof(double) : sizeof(float));
}

// The route of a forward (dy_dtype < 0) or backward call and its geometry: what vo_bn_route reports and
// what vo_bn_train_fwd / vo_bn_bwd launch (include/vonoma.h).  Host arithmetic only.
enum { BN_SCALAR = 0, BN_VEC = 1, BN_FLAT = 2 };
struct BnRoute {
  int route, V, CV, RL, RB, nb, apply_blocks, CT;
};

static bool bn_aligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }  // NULL: aligned

static BnRoute bn_route(int M, int C, int x_dtype, int dy_dtype, const void* x, const void* dy, const void* out) {
  BnRoute r{};
  bool flat = false;
  bool vec = bn_vec_ok(M, C, x_dtype, &flat);
  // backward: x's vector width sets the layout; dy bf16 under fp32 x is read 4 per lane (8 bytes); bf16 x with
  // fp32 dy has no vector form
  if (dy_dtype >= 0 && x_dtype == VO_BF16 && dy_dtype == VO_F32) vec = false;
  // 16-byte loads and stores of x and the output, 16- or 8-byte loads of dy
  if (vec && !(bn_aligned(x, 16) && bn_aligned(out, 16) &&
               bn_aligned(dy, x_dtype == VO_F32 && dy_dtype == VO_BF16 ? 8 : 16)))
    vec = false;
  if (vec) {
    int rows;
    r.route = flat ? BN_FLAT : BN_VEC;
    r.V = x_dtype == VO_BF16 ? 8 : 4;
    r.CV = flat ? 1 : C / r.V;
    r.RL = 256 / r.CV;
    bn_vec_geometry(M, C, x_dtype, flat, &rows, &r.RB, &r.nb);
    r.apply_blocks = (int)bn_apply_blocks((int)((int64_t)M * C / r.V), r.CV);
    return r;
  }
  r.route = BN_SCALAR;
  bn_geometry(M, C, &r.CT, &r.RB, &r.nb);
  r.RL = 256 / r.CT;
  r.apply_blocks = (int)std::min<int64_t>(((int64_t)M * C + 255) / 256, 4096);
  return r;
}

extern "C" int vo_bn_route(int M, int C, int x_dtype, int dy_dtype, const void* x, const void* dy, const void* out,
                           int32_t* rec, int n) {
  const int m = std::max(0, std::min(n, VO_BN_ROUTE_FIELDS));
  if (rec) std::fill(rec, rec + m, 0);
  const bool ok = M > 0 && C > 0 && (x_dtype == VO_F32 || x_dtype == VO_BF16) &&
                  (dy_dtype < 0 || dy_dtype == VO_F32 || dy_dtype == VO_BF16);
  if (!ok) {
    vo_set_error("bn_route: M, C > 0, x fp32 / bf16, dy fp32 / bf16 or < 0 (forward)");
    return VO_ERR_INVALID;
  }
  const BnRoute r = bn_route(M, C, x_dtype, dy_dtype, x, dy, out);
  const int32_t f[VO_BN_ROUTE_FIELDS] = {r.route, r.V, r.CV, r.RL, r.RB, r.nb, r.apply_blocks, r.CT};
  if (!rec) return 0;
  std::copy(f, f + m, rec);
  return m;
}


// ---- launches, each from the BnRoute record vo_bn_route reports: its fields, or plain arithmetic on M, C and its V
struct BnFwdArgs {
  const void* x;
  int M, C;
  const float *gamma, *beta;
  float eps, momentum;
  float *run_mean, *run_var;
  int64_t* nbt;
  float *mean_rstd, *ws;
  void* y;
  hipStream_t st;
};
struct BnBwdArgs {
  const void *x, *dy;
  int M, C;
  const float *gamma, *mean_rstd;
  float *ws, *dgamma, *dbeta;
  void* dx;
  hipStream_t st;
};

template <typename TX, bool FLAT>
static void bn_fwd_vec(const BnRoute& rt, const BnFwdArgs& a) {
  const int rows = FLAT ? a.M / rt.V : a.M;
  const int nvec = (int)((int64_t)a.M * a.C / rt.V);
  hipLaunchKernelGGL((bn_stats_v_kernel<TX, FLAT>), dim3((unsigned)rt.nb), dim3(256), 0, a.st, (const TX*)a.x, rows,
                     a.C, rt.RB, a.ws);
  hipLaunchKernelGGL(bn_finalize_v_kernel, dim3((unsigned)((a.C + 31) / 32)), dim3(256), 0, a.st, a.ws, rt.nb, a.C,
                     a.eps, a.momentum, a.mean_rstd, a.run_mean, a.run_var, a.nbt);
  hipLaunchKernelGGL((bn_apply_v_kernel<TX, FLAT>), dim3((unsigned)rt.apply_blocks), dim3(256), 0, a.st,
                     (const TX*)a.x, nvec, a.C, a.mean_rstd, a.gamma, a.beta, (TX*)a.y);
}

template <typename TX>
static void bn_fwd_scalar(const BnRoute& rt, const BnFwdArgs& a) {
  const dim3 grid((unsigned)rt.nb, (unsigned)((a.C + rt.CT - 1) / rt.CT));
  with_bool(rt.CT == 1, [&](auto one) {
    hipLaunchKernelGGL((bn_stats_kernel<TX, decltype(one)::value ? 1 : 64>), grid, dim3(256), 0, a.st, (const TX*)a.x,
                       a.M, a.C, rt.RB, a.ws);
    return 0;
  });
  hipLaunchKernelGGL(bn_finalize_kernel, dim3((unsigned)((a.C + 255) / 256)), dim3(256), 0, a.st, a.ws, rt.nb, a.C,
                     a.eps, a.momentum, a.mean_rstd, a.run_mean, a.run_var, a.nbt);
  hipLaunchKernelGGL((bn_apply_kernel<TX>), dim3((unsigned)rt.apply_blocks), dim3(256), 0, a.st, (const TX*)a.x,
                     (int64_t)a.M * a.C, a.C, a.mean_rstd, a.gamma, a.beta, (TX*)a.y);
}

// FLAT: the workspace as doubles -- BN_NB partial pairs, then the pair of totals
template <typename TX, typename TG, bool FLAT>
static void bn_bwd_vec(const BnRoute& rt, const BnBwdArgs& a) {
  const int rows = FLAT ? a.M / rt.V : a.M;
  const int nvec = (int)((int64_t)a.M * a.C / rt.V);
  const float inv_m = 1.f / (float)a.M;
  double* tot = FLAT ? reinterpret_cast<double*>(a.ws) + 2 * BN_NB : nullptr;
  hipLaunchKernelGGL((bn_bwd_stats_v_kernel<TX, TG, FLAT>), dim3((unsigned)rt.nb), dim3(256), 0, a.st,
                     (const TX*)a.x, (const TG*)a.dy, rows, a.C, rt.RB, a.mean_rstd, a.ws);
  if (FLAT)
    hipLaunchKernelGGL(bn_bwd_finalize_flat_kernel, dim3(1), dim3(BN_NB), 0, a.st, (const double*)a.ws, rt.nb,
                       a.dgamma, a.dbeta, tot);
  else
    hipLaunchKernelGGL(bn_bwd_finalize_v_kernel, dim3((unsigned)((a.C + 31) / 32)), dim3(256), 0, a.st, a.ws, rt.nb,
                       a.C, a.dgamma, a.dbeta);
  hipLaunchKernelGGL((bn_bwd_apply_v_kernel<TX, TG, FLAT>), dim3((unsigned)rt.apply_blocks), dim3(256), 0, a.st,
                     (const TX*)a.x, (const TG*)a.dy, nvec, a.C, inv_m, a.mean_rstd, a.gamma, a.dgamma, a.dbeta,
                     (const double*)tot, (TX*)a.dx);
}

template <typename TX, typename TG>
static void bn_bwd_scalar(const BnRoute& rt, const BnBwdArgs& a) {
  const dim3 grid((unsigned)rt.nb, (unsigned)((a.C + rt.CT - 1) / rt.CT));
  with_bool(rt.CT == 1, [&](auto one) {
    hipLaunchKernelGGL((bn_bwd_stats_kernel<TX, TG, decltype(one)::value ? 1 : 64>), grid, dim3(256), 0, a.st,
                       (const TX*)a.x, (const TG*)a.dy, a.M, a.C, rt.RB, a.mean_rstd, a.ws);
    return 0;
  });
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((unsigned)((a.C + 255) / 256)), dim3(256), 0, a.st, a.ws, rt.nb,
                     a.C, a.dgamma, a.dbeta);
  hipLaunchKernelGGL((bn_bwd_apply_kernel<TX, TG>), dim3((unsigned)rt.apply_blocks), dim3(256), 0, a.st,
                     (const TX*)a.x, (const TG*)a.dy, (int64_t)a.M * a.C, a.C, 1.f / (float)a.M, a.mean_rstd, a.gamma,
                     a.dgamma, a.dbeta, (TX*)a.dx);
}

extern "C" int vo_bn_train_fwd(const void* x, int dtype, int M, int C, const float* gamma, const float* beta,
                               float eps, float momentum, float* run_mean, float* run_var, int64_t* nbt,
                               float* mean_rstd, float* workspace, void* y, void* stream) {
  VO_CHECK_ARG(x && y && mean_rstd && workspace && M > 0 && C > 0, "bn_train_fwd: bad arguments");
  VO_CHECK_ARG(dtype == VO_F32 || dtype == VO_BF16, "bn_train_fwd: dtype");
  VO_CHECK_ARG((gamma == nullptr) == (beta == nullptr), "bn_train_fwd: gamma and beta together");
  VO_CHECK_ARG((run_mean == nullptr) == (run_var == nullptr), "bn_train_fwd: running stats together");
  const BnFwdArgs a{x, M, C, gamma, beta, eps, momentum, run_mean, run_var, nbt, mean_rstd, workspace, y,
                    (hipStream_t)stream};
  const BnRoute rt = bn_route(M, C, dtype, -1, x, nullptr, y);
  return with_dtype(dtype, "bn_train_fwd", [&](auto tx) {
    using TX = typename decltype(tx)::type;
    if (rt.route == BN_SCALAR) bn_fwd_scalar<TX>(rt, a);
    else if (rt.route == BN_FLAT) bn_fwd_vec<TX, true>(rt, a);
    else bn_fwd_vec<TX, false>(rt, a);
    VO_RETURN_LAUNCH();
  });
}

extern "C" int vo_bn_bwd(const void* x, int x_dtype, const void* dy, int dy_dtype, int M, int C, const float* gamma,
                         const float* mean_rstd, float* workspace, float* dgamma, float* dbeta, void* dx, void* stream) {
  VO_CHECK_ARG(x && dy && mean_rstd && workspace && dgamma && dbeta && dx && M > 0 && C > 0, "bn_bwd: bad arguments");
  VO_CHECK_ARG((x_dtype == VO_F32 || x_dtype == VO_BF16) && (dy_dtype == VO_F32 || dy_dtype == VO_BF16),
               "bn_bwd: dtypes");
  const BnBwdArgs a{x, dy, M, C, gamma, mean_rstd, workspace, dgamma, dbeta, dx, (hipStream_t)stream};
  const BnRoute rt = bn_route(M, C, x_dtype, dy_dtype, x, dy, dx);
  VO_CHECK_ARG(rt.route != BN_FLAT || reinterpret_cast<uintptr_t>(workspace) % 8 == 0,
               "bn_bwd: workspace must be 8-byte aligned");
  return with_dtypes(x_dtype, dy_dtype, "bn_bwd", [&](auto tx, auto tg) {
    using TX = typename decltype(tx)::type;
    using TG = typename decltype(tg)::type;
    if (rt.route == BN_SCALAR) bn_bwd_scalar<TX, TG>(rt, a);
    // never reached: bn_route sends bf16 x with fp32 dy to the scalar kernels, and no vector kernel is compiled for it
    else if constexpr (std::is_same_v<TX, bf16_t> && std::is_same_v<TG, float>) return (int)VO_ERR_INVALID;
    else if (rt.route == BN_FLAT) bn_bwd_vec<TX, TG, true>(rt, a);
    else bn_bwd_vec<TX, TG, false>(rt, a);
    VO_RETURN_LAUNCH();
  });
}
