// Training-step glue that round 1 left on PyTorch-ROCm (config C4 / C5 backward):
//
//  * counter-based dropout (vo_dropout);
//  * the glyph encoder's 1 -> 1 channel 3 x 3 Conv2d (pad 1) forward and backward (input, weight
//    and bias gradients; the weight / bias sums as per-block partials added in a fixed order);
//  * the backward of the HiFi-GAN training log-mel (vo_stft_mel_ex with mag_eps): per frame the
//    forward spectrum is recomputed, dL/d|X| = fb (g / melsum) on the bins whose mel sum passed the
//    log floor, dX = dL/d|X| X / |X|, the one-sided inverse DFT of dX (a 1024-point complex FFT
//    in LDS) times the window gives the frame gradient; a second kernel gathers the (<= n_fft / hop)
//    overlapping frames and the reflect-padded mirror positions of every sample in a fixed order.
// Everything deterministic (no atomics).  (BatchNorm: batchnorm.hip.)

#include <algorithm>

#include "vo_common.h"

namespace vo {

// ------------------------------------------------------------------------------- dropout
// Counter-based dropout (nn.Dropout / F.dropout in training, scripts/transformer/SubLayers.py:38,87,
// scripts/transformer/Layers.py:129-131, scripts/model/modules.py:52-56): element i is kept iff
// hash(seed, i) >= p 2^32, y = keep ? x / (1 - p) : 0.  The mask is a pure function of (seed, i), so
// the backward is the same call on dy -- no mask tensor is written or read (ATen's fused_dropout writes
// one byte per element and its masked_scale reads it back).  seed: a device int64 drawn per call from
// torch's generator (graph-safe: every replay draws a new one).
// (drop_mix / drop_hash / drop_keys: vo_common.h -- the LayerNorm kernels apply the same mask in-pass)

template <typename T>
__global__ void __launch_bounds__(256) dropout_kernel(const T* __restrict__ x, int64_t n, uint32_t thr, float scale,
                                                      const int64_t* __restrict__ seed, uint32_t salt,
                                                      T* __restrict__ y) {
  using VT = BnVec<T>;
  constexpr int V = VT::V;
  uint32_t s0, s1;
  drop_keys(seed, salt, s0, s1);
  const int64_t nv = n / V;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += 4 * stride) {  // 4 vectors in flight
    float v[4][V];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (i + u * stride < nv) VT::load(x + (i + u * stride) * V, v[u]);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t iv = i + u * stride;
      if (iv >= nv) continue;
#pragma unroll
      for (int e = 0; e < V; ++e) v[u][e] = drop_hash(s0, s1, (uint32_t)(iv * V + e)) >= thr ? v[u][e] * scale : 0.f;
      VT::store(y + iv * V, v[u]);
    }
  }
  const int64_t t = nv * V + threadIdx.x;  // the n % V tail, one element a thread of block 0
  if (blockIdx.x == 0 && t < n) y[t] = from_f32<T>(drop_hash(s0, s1, (uint32_t)t) >= thr ? to_f32(x[t]) * scale : 0.f);
}

// ------------------------------------------------------------------------------- 3 x 3 single-channel conv

constexpr int VC_TILE = 256;  // pixels per block (the weight / bias partials: one row per block)

__global__ void __launch_bounds__(VC_TILE) vfe_conv_fwd_kernel(const float* __restrict__ x, int N, int H, int W,
                                                               const float* __restrict__ w, float* __restrict__ y) {
  const int64_t total = (int64_t)N * H * W;
  const int64_t i = (int64_t)blockIdx.x * VC_TILE + threadIdx.x;
  if (i >= total) return;
  const int wq = (int)(i % W), hq = (int)((i / W) % H);
  const int64_t base = i - (int64_t)hq * W - wq;
  float s = w[9];  // bias
#pragma unroll
  for (int di = -1; di <= 1; ++di)
#pragma unroll
    for (int dj = -1; dj <= 1; ++dj) {
      const int h = hq + di, ww = wq + dj;
      if (h >= 0 && h < H && ww >= 0 && ww < W) s += w[(di + 1) * 3 + (dj + 1)] * x[base + (int64_t)h * W + ww];
    }
  y[i] = s;
}

// dx = correlation of dy with the flipped kernel; per block: the 10 weight / bias partial sums
__global__ void __launch_bounds__(VC_TILE) vfe_conv_bwd_kernel(const float* __restrict__ x,
                                                               const float* __restrict__ dy, int N, int H, int W,
                                                               const float* __restrict__ w, float* __restrict__ dx,
                                                               float* __restrict__ part) {
  __shared__ float red[10][VC_TILE / 64];
  const int64_t total = (int64_t)N * H * W;
  const int64_t i = (int64_t)blockIdx.x * VC_TILE + threadIdx.x;
  float pw[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) pw[k] = 0.f;
  if (i < total) {
    const int wq = (int)(i % W), hq = (int)((i / W) % H);
    const int64_t base = i - (int64_t)hq * W - wq;
    float s = 0.f;
    const float g = dy[i];
#pragma unroll
    for (int di = -1; di <= 1; ++di)
#pragma unroll
      for (int dj = -1; dj <= 1; ++dj) {
        const int h = hq + di, ww = wq + dj;
        if (h >= 0 && h < H && ww >= 0 && ww < W) {
          // y[h, ww] used x[hq, wq] with kernel tap (-di, -dj): dx += w[1 - di][1 - dj] dy[h, ww]
          s += w[(1 - di) * 3 + (1 - dj)] * dy[base + (int64_t)h * W + ww];
          // dW[di + 1][dj + 1] += dy[hq, wq] x[hq + di, wq + dj]
          pw[(di + 1) * 3 + (dj + 1)] = g * x[base + (int64_t)h * W + ww];
        }
      }
    pw[9] = g;
    dx[i] = s;
  }
#pragma unroll
  for (int k = 0; k < 10; ++k) {
    const float v = wave_sum(pw[k]);
    if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x < 10) {
    float v = 0.f;
    for (int q = 0; q < VC_TILE / 64; ++q) v += red[threadIdx.x][q];
    part[(int64_t)blockIdx.x * 10 + threadIdx.x] = v;
  }
}

__global__ void vfe_conv_wgrad_finalize_kernel(const float* __restrict__ part, int nb, float* __restrict__ dw) {
  // one wave per weight: lanes stride over blocks in order, a fixed-shape tree inside the wave
  const int k = blockIdx.x;
  float s = 0.f;
  for (int b = threadIdx.x; b < nb; b += 64) s += part[(int64_t)b * 10 + k];
  s = wave_sum(s);
  if (threadIdx.x == 0) dw[k] = s;
}

// ------------------------------------------------------------------------------- kh x kw single-channel conv
// The general Conv2d(1, 1, (kh, kw), padding ((kh-1)/2, (kw-1)/2)): w[kh kw + 1] = row-major taps, then the bias.

constexpr int VC_MAXK = 9;
constexpr int VC_MAXT = VC_MAXK * VC_MAXK + 1;  // partial sums per block: the taps and the bias

__global__ void __launch_bounds__(VC_TILE) vfe_conv_fwd_ex_kernel(const float* __restrict__ x, int N, int H, int W,
                                                                  int kh, int kw, const float* __restrict__ w,
                                                                  float* __restrict__ y) {
  const int64_t total = (int64_t)N * H * W;
  const int64_t i = (int64_t)blockIdx.x * VC_TILE + threadIdx.x;
  if (i >= total) return;
  const int wq = (int)(i % W), hq = (int)((i / W) % H);
  const int64_t base = i - (int64_t)hq * W - wq;
  const int ph = (kh - 1) / 2, pw = (kw - 1) / 2;
  // summed in double and rounded once: up to 81 taps, and the training path's BatchNorm gradients are cancelling
  // sums that magnify every rounding of the maps (bn_bwd_stats_v_kernel)
  double s = w[kh * kw];  // bias
  for (int a = 0; a < kh; ++a) {
    const int h = hq + a - ph;
    if (h < 0 || h >= H) continue;
    for (int b = 0; b < kw; ++b) {
      const int ww = wq + b - pw;
      if (ww >= 0 && ww < W) s = fma((double)w[a * kw + b], (double)x[base + (int64_t)h * W + ww], s);
    }
  }
  y[i] = (float)s;
}

// dx[h, w] = sum_ab w[a][b] dy[h - (a - ph), w - (b - pw)]; per block and tap the partial
// dW[a][b] = sum dy[h, w] x[h + a - ph, w + b - pw], one tap at a time: the wave reduction inside the tap loop,
// so no per-tap register array
__global__ void __launch_bounds__(VC_TILE) vfe_conv_bwd_ex_kernel(const float* __restrict__ x,
                                                                  const float* __restrict__ dy, int N, int H, int W,
                                                                  int kh, int kw, const float* __restrict__ w,
                                                                  float* __restrict__ dx, float* __restrict__ part) {
  __shared__ float red[VC_MAXT][VC_TILE / 64];
  const int64_t total = (int64_t)N * H * W;
  const int64_t i = (int64_t)blockIdx.x * VC_TILE + threadIdx.x;
  const bool live = i < total;
  const int64_t ic = live ? i : total - 1;
  const int wq = (int)(ic % W), hq = (int)((ic / W) % H);
  const int64_t base = ic - (int64_t)hq * W - wq;
  const int ph = (kh - 1) / 2, pw = (kw - 1) / 2, nt = kh * kw;
  const float g = live ? dy[ic] : 0.f;
  const int wave = threadIdx.x >> 6;
  const bool lead = (threadIdx.x & 63) == 0;
  double s = 0.;  // dx in double, rounded once (as the forward)
  for (int a = 0; a < kh; ++a)
    for (int b = 0; b < kw; ++b) {
      const int hx = hq + a - ph, wx = wq + b - pw;  // the x this pixel's dy multiplies for tap (a, b)
      const int hy = hq - a + ph, wy = wq - b + pw;  // the dy that reached this pixel's x through tap (a, b)
      float p = 0.f;
      if (live && hx >= 0 && hx < H && wx >= 0 && wx < W) p = g * x[base + (int64_t)hx * W + wx];
      if (live && hy >= 0 && hy < H && wy >= 0 && wy < W) s = fma((double)w[a * kw + b], (double)dy[base + (int64_t)hy * W + wy], s);
      p = wave_sum(p);
      if (lead) red[a * kw + b][wave] = p;
    }
  {
    const float p = wave_sum(g);
    if (lead) red[nt][wave] = p;
  }
  if (live) dx[i] = (float)s;
  __syncthreads();
  if ((int)threadIdx.x <= nt) {
    float v = 0.f;
    for (int q = 0; q < VC_TILE / 64; ++q) v += red[threadIdx.x][q];
    part[(int64_t)blockIdx.x * (nt + 1) + threadIdx.x] = v;
  }
}

__global__ void vfe_conv_wgrad_finalize_ex_kernel(const float* __restrict__ part, int nb, int nk,
                                                  float* __restrict__ dw) {
  // as vfe_conv_wgrad_finalize_kernel, nk partials per block
  const int k = blockIdx.x;
  float s = 0.f;
  for (int b = threadIdx.x; b < nb; b += 64) s += part[(int64_t)b * nk + k];
  s = wave_sum(s);
  if (threadIdx.x == 0) dw[k] = s;
}

// ------------------------------------------------------------------------------- STFT log-mel backward

constexpr int SMB_MAX_N = 2048;

__device__ __forceinline__ int reflect_idx(int i, int n) {
  if (i < 0) i = -i;
  if (i >= n) i = 2 * (n - 1) - i;
  return i;
}

// in-place-free radix-2 Stockham FFT of length L (power of two) on buf[src]; sign -1 forward,
// +1 inverse (unnormalised); returns the buffer holding the result
__device__ int fft_stockham(float2 (*buf)[SMB_MAX_N], int L, float sign, int tid, int nthreads) {
  int src = 0;
  for (int ns = 1; ns < L; ns <<= 1) {
    for (int j = tid; j < L / 2; j += nthreads) {
      const int k = j & (ns - 1);
      const float2 u = buf[src][j];
      const float2 v = buf[src][j + L / 2];
      float s, c;
      sincospif(sign * (float)k / (float)ns, &s, &c);
      const float2 tv = make_float2(v.x * c - v.y * s, v.x * s + v.y * c);
      const int out = (j - k) * 2 + k;
      buf[src ^ 1][out] = make_float2(u.x + tv.x, u.y + tv.y);
      buf[src ^ 1][out + ns] = make_float2(u.x - tv.x, u.y - tv.y);
    }
    __syncthreads();
    src ^= 1;
  }
  return src;
}

// one workgroup per (frame, utterance): gframe[b][f][n] = d loss / d x_frame[n] (after the window)
__global__ void __launch_bounds__(256) stft_mel_bwd_frame_kernel(const float* __restrict__ wav, int N, int F,
                                                                 const float* __restrict__ window,
                                                                 const float* __restrict__ fb, int n_fft, int hop,
                                                                 int n_mels, int pad, float mag_eps, float log_floor,
                                                                 const float* __restrict__ gmel,
                                                                 float* __restrict__ gframe) {
  __shared__ float2 buf[2][SMB_MAX_N];
  __shared__ float mag[SMB_MAX_N / 2 + 1];
  __shared__ float xre[SMB_MAX_N / 2 + 1], xim[SMB_MAX_N / 2 + 1];
  __shared__ float dm[256];  // d loss / d melsum per mel bin (n_mels <= 256)
  const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int n = n_fft, half = n / 2;
  const float* x = wav + (int64_t)b * N;
  const int start = f * hop - pad;

  // forward: full n-point complex FFT of the windowed real frame
  for (int m = tid; m < n; m += 256) buf[0][m] = make_float2(x[reflect_idx(start + m, N)] * window[m], 0.f);
  __syncthreads();
  int s = fft_stockham(buf, n, -1.f, tid, 256);
  for (int k = tid; k <= half; k += 256) {
    const float2 z = buf[s][k];
    xre[k] = z.x;
    xim[k] = z.y;
    mag[k] = sqrtf(z.x * z.x + z.y * z.y + mag_eps);
  }
  __syncthreads();
  // mel sums and their log-floor derivative
  const int lane = tid & 63, wave = tid >> 6;
  const int nf = half + 1;
  for (int m = wave; m < n_mels; m += 4) {
    float acc = 0.f;
    for (int k = lane; k < nf; k += 64) acc += fb[(int64_t)k * n_mels + m] * mag[k];
    acc = wave_sum(acc);
    if (lane == 0) dm[m] = acc >= log_floor ? gmel[((int64_t)b * n_mels + m) * F + f] / acc : 0.f;
  }
  __syncthreads();
  // dX[k] = (fb dm)[k] X[k] / |X[k]| for k <= n/2, zero above: the inverse DFT's real part is the
  // gradient w.r.t. the windowed frame (Re sum_k conj-free D_k e^{+2 pi i k t / n})
  for (int k = tid; k < n; k += 256) {
    float2 d = make_float2(0.f, 0.f);
    if (k <= half) {
      float g = 0.f;
      for (int m = 0; m < n_mels; ++m) g += fb[(int64_t)k * n_mels + m] * dm[m];
      const float sc = g / mag[k];
      d = make_float2(sc * xre[k], sc * xim[k]);
    }
    buf[0][k] = d;
  }
  __syncthreads();
  s = fft_stockham(buf, n, 1.f, tid, 256);
  float* out = gframe + ((int64_t)b * F + f) * n;
  for (int m = tid; m < n; m += 256) out[m] = buf[s][m].x * window[m];
}

// dwav[b][i] = sum over padded positions p with reflect(p - pad) == i and frames f covering p
// (f hop <= p < f hop + n_fft) of gframe[b][f][p - f hop], in a fixed order
__global__ void __launch_bounds__(256) stft_mel_bwd_gather_kernel(const float* __restrict__ gframe, int N, int F,
                                                                  int n_fft, int hop, int pad,
                                                                  float* __restrict__ dwav) {
  const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (i >= N) return;
  const float* gf = gframe + (int64_t)b * F * n_fft;
  float s = 0.f;
  int ps[3];
  int np = 0;
  ps[np++] = i + pad;                                    // the sample itself
  if (i >= 1 && i <= pad) ps[np++] = pad - i;            // mirrored into the left pad
  if (i <= N - 2 && i >= N - 1 - pad) ps[np++] = pad + 2 * (N - 1) - i;  // mirrored into the right pad
  for (int q = 0; q < np; ++q) {
    const int p = ps[q];
    int f0 = p - n_fft + 1;
    f0 = f0 <= 0 ? 0 : (f0 + hop - 1) / hop;
    const int f1 = min(p / hop, F - 1);
    for (int f = f0; f <= f1; ++f) s += gf[(int64_t)f * n_fft + (p - f * hop)];
  }
  dwav[(int64_t)b * N + i] = s;
}

// ------------------------------------------------------------------------------- STFT magnitude
// torch.stft(center=True, reflect pad n_fft / 2, onesided) of a window zero-padded to n_fft, and
// mag = sqrt(max(|X|^2, eps)): the multi-resolution STFT loss of Parallel WaveGAN-style vocoder
// training.  One workgroup per (frame, utterance); mag laid out (B, F, n_fft / 2 + 1).
__global__ void __launch_bounds__(256) stft_mag_kernel(const float* __restrict__ wav, int N, int F,
                                                       const float* __restrict__ window, int n_fft, int hop,
                                                       float eps, float* __restrict__ mag) {
  __shared__ float2 buf[2][SMB_MAX_N];
  const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int n = n_fft, half = n / 2;
  const float* x = wav + (int64_t)b * N;
  const int start = f * hop - half;
  for (int m = tid; m < n; m += 256) buf[0][m] = make_float2(x[reflect_idx(start + m, N)] * window[m], 0.f);
  __syncthreads();
  const int s = fft_stockham(buf, n, -1.f, tid, 256);
  float* out = mag + ((int64_t)b * F + f) * (half + 1);
  for (int k = tid; k <= half; k += 256) {
    const float2 z = buf[s][k];
    out[k] = sqrtf(fmaxf(z.x * z.x + z.y * z.y, eps));
  }
}

// frame gradient of the magnitude: dX = gmag X / |X| where |X|^2 > eps (the clamp passes no
// gradient below it), zero above n / 2; the inverse DFT's real part times the window
__global__ void __launch_bounds__(256) stft_mag_bwd_frame_kernel(const float* __restrict__ wav, int N, int F,
                                                                 const float* __restrict__ window, int n_fft,
                                                                 int hop, float eps, const float* __restrict__ gmag,
                                                                 float* __restrict__ gframe) {
  __shared__ float2 buf[2][SMB_MAX_N];
  const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int n = n_fft, half = n / 2;
  const float* x = wav + (int64_t)b * N;
  const int start = f * hop - half;
  for (int m = tid; m < n; m += 256) buf[0][m] = make_float2(x[reflect_idx(start + m, N)] * window[m], 0.f);
  __syncthreads();
  int s = fft_stockham(buf, n, -1.f, tid, 256);
  const float* gm = gmag + ((int64_t)b * F + f) * (half + 1);
  float2 d[SMB_MAX_N / 256];
#pragma unroll
  for (int u = 0; u < SMB_MAX_N / 256; ++u) {
    const int k = tid + u * 256;
    d[u] = make_float2(0.f, 0.f);
    if (k <= half) {
      const float2 z = buf[s][k];
      const float p = z.x * z.x + z.y * z.y;
      const float sc = p > eps ? gm[k] * rsqrtf(p) : 0.f;
      d[u] = make_float2(sc * z.x, sc * z.y);
    }
  }
  __syncthreads();  // every spectrum read done before the buffer is reused
#pragma unroll
  for (int u = 0; u < SMB_MAX_N / 256; ++u) {
    const int k = tid + u * 256;
    if (k < n) buf[0][k] = d[u];
  }
  __syncthreads();
  s = fft_stockham(buf, n, 1.f, tid, 256);
  float* out = gframe + ((int64_t)b * F + f) * n;
  for (int m = tid; m < n; m += 256) out[m] = buf[s][m].x * window[m];
}

// multi-resolution STFT loss terms of one resolution over n magnitudes (x = generated, y =
// target): part[block] = (sum (y - x)^2, sum y^2, sum |log y - log x|); one wave adds the block
// partials in order into out[0..3)
__global__ void __launch_bounds__(256) stft_loss_reduce_kernel(const float* __restrict__ xm,
                                                               const float* __restrict__ ym, int64_t n,
                                                               float* __restrict__ part) {
  __shared__ float red[3][4];
  float a = 0.f, c = 0.f, l = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float x = xm[i], y = ym[i];
    a += (y - x) * (y - x);
    c += y * y;
    l += fabsf(__logf(y) - __logf(x));
  }
  a = wave_sum(a);
  c = wave_sum(c);
  l = wave_sum(l);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = a;
    red[1][threadIdx.x >> 6] = c;
    red[2][threadIdx.x >> 6] = l;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const float* r = red[threadIdx.x];
    part[(int64_t)blockIdx.x * 3 + threadIdx.x] = r[0] + r[1] + r[2] + r[3];
  }
}

__global__ void __launch_bounds__(64) stft_loss_final_kernel(const float* __restrict__ part, int nb,
                                                             float* __restrict__ out) {
  for (int k = 0; k < 3; ++k) {
    float v = 0.f;
    for (int i = threadIdx.x; i < nb; i += 64) v += part[(int64_t)i * 3 + k];
    v = wave_sum(v);
    if (threadIdx.x == 0) out[k] = v;
  }
}

// d/dx of w_sc * sqrt(A) / sqrt(C) + w_mag * L / n, A / C / L the sums above:
//   w_sc (x - y) / (sqrt(A) sqrt(C)) + w_mag sign(log x - log y) / (n x)
__global__ void __launch_bounds__(256) stft_loss_grad_kernel(const float* __restrict__ xm,
                                                             const float* __restrict__ ym, int64_t n,
                                                             const float* __restrict__ sums,
                                                             const float* __restrict__ w, float* __restrict__ gx) {
  const float w_sc = w[0], w_mag = w[1];  // device scalars: the incoming loss gradients (graph-safe)
  const float sa = sqrtf(sums[0]), sc = sqrtf(sums[1]);
  const float k_sc = sa > 0.f && sc > 0.f ? w_sc / (sa * sc) : 0.f;
  const float k_mag = w_mag / (float)n;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float x = xm[i], y = ym[i];
    const float dl = __logf(x) - __logf(y);
    gx[i] = k_sc * (x - y) + (dl > 0.f ? k_mag : (dl < 0.f ? -k_mag : 0.f)) / x;
  }
}

}  // namespace vo

using namespace vo;

extern "C" int64_t vo_vfe_conv_workspace_size(int N, int H, int W) {
  const int64_t nb = ((int64_t)N * H * W + VC_TILE - 1) / VC_TILE;
  return nb * 10 * (int64_t)sizeof(float);
}

extern "C" int vo_vfe_conv_fwd(const float* x, int N, int H, int W, const float* w, float* y, void* stream) {
  VO_CHECK_ARG(x && w && y && N > 0 && H > 0 && W > 0, "vfe_conv_fwd: bad arguments");
  const int64_t total = (int64_t)N * H * W;
  hipLaunchKernelGGL(vfe_conv_fwd_kernel, dim3((unsigned)((total + VC_TILE - 1) / VC_TILE)), dim3(VC_TILE), 0,
                     reinterpret_cast<hipStream_t>(stream), x, N, H, W, w, y);
  VO_RETURN_LAUNCH();
}

extern "C" int vo_vfe_conv_bwd(const float* x, const float* dy, int N, int H, int W, const float* w, float* dx,
                               float* dw, float* workspace, void* stream) {
  VO_CHECK_ARG(x && dy && w && dx && dw && workspace && N > 0 && H > 0 && W > 0, "vfe_conv_bwd: bad arguments");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t total = (int64_t)N * H * W;
  const int nb = (int)((total + VC_TILE - 1) / VC_TILE);
  hipLaunchKernelGGL(vfe_conv_bwd_kernel, dim3((unsigned)nb), dim3(VC_TILE), 0, st, x, dy, N, H, W, w, dx, workspace);
  hipLaunchKernelGGL(vfe_conv_wgrad_finalize_kernel, dim3(10), dim3(64), 0, st, workspace, nb, dw);
  VO_RETURN_LAUNCH();
}

// ---- the general glyph-encoder conv: kh x kw odd taps up to 9, w[kh kw + 1] = row-major kernel + bias
static bool vfe_conv_ex_args(int N, int H, int W, int kh, int kw) {
  return N > 0 && H > 0 && W > 0 && kh >= 1 && kw >= 1 && kh % 2 == 1 && kw % 2 == 1 && kh <= VC_MAXK && kw <= VC_MAXK &&
         ((int64_t)N * H * W + VC_TILE - 1) / VC_TILE <= INT32_MAX;
}

extern "C" int64_t vo_vfe_conv_workspace_size_ex(int N, int H, int W, int kh, int kw) {
  if (!vfe_conv_ex_args(N, H, W, kh, kw)) return -1;
  const int64_t nb = ((int64_t)N * H * W + VC_TILE - 1) / VC_TILE;
  return nb * (kh * kw + 1) * (int64_t)sizeof(float);
}

extern "C" int vo_vfe_conv_fwd_ex(const float* x, int N, int H, int W, int kh, int kw, const float* w, float* y,
                                  void* stream) {
  VO_CHECK_ARG(x && w && y, "vfe_conv_fwd_ex: null pointer");
  VO_CHECK_ARG(vfe_conv_ex_args(N, H, W, kh, kw), "vfe_conv_fwd_ex: N=%d H=%d W=%d, kernel %dx%d (odd sizes up to %d)", N,
               H, W, kh, kw, VC_MAXK);
  const int64_t total = (int64_t)N * H * W;
  hipLaunchKernelGGL(vfe_conv_fwd_ex_kernel, dim3((unsigned)((total + VC_TILE - 1) / VC_TILE)), dim3(VC_TILE), 0,
                     reinterpret_cast<hipStream_t>(stream), x, N, H, W, kh, kw, w, y);
  VO_RETURN_LAUNCH();
}

extern "C" int vo_vfe_conv_bwd_ex(const float* x, const float* dy, int N, int H, int W, int kh, int kw, const float* w,
                                  float* dx, float* dw, float* workspace, void* stream) {
  VO_CHECK_ARG(x && dy && w && dx && dw && workspace, "vfe_conv_bwd_ex: null pointer");
  VO_CHECK_ARG(vfe_conv_ex_args(N, H, W, kh, kw), "vfe_conv_bwd_ex: N=%d H=%d W=%d, kernel %dx%d (odd sizes up to %d)", N,
               H, W, kh, kw, VC_MAXK);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t total = (int64_t)N * H * W;
  const int nb = (int)((total + VC_TILE - 1) / VC_TILE), nk = kh * kw + 1;
  hipLaunchKernelGGL(vfe_conv_bwd_ex_kernel, dim3((unsigned)nb), dim3(VC_TILE), 0, st, x, dy, N, H, W, kh, kw, w, dx,
                     workspace);
  hipLaunchKernelGGL(vfe_conv_wgrad_finalize_ex_kernel, dim3((unsigned)nk), dim3(64), 0, st, workspace, nb, nk, dw);
  VO_RETURN_LAUNCH();
}

// ---- log-mel backward (the framing of vo_stft_mel_ex, clip off): gmel (B, n_mels, F) -> dwav (B, N)
extern "C" int64_t vo_stft_mel_bwd_workspace_size(int B, int N, int n_fft, int hop, int pad) {
  const int64_t F = 1 + (N + 2 * (int64_t)pad - n_fft) / hop;
  return (int64_t)B * F * n_fft * (int64_t)sizeof(float);
}

extern "C" int vo_stft_mel_bwd(const float* wav, int B, int N, const float* window, const float* fb, int n_fft, int hop,
                               int n_mels, int pad, float mag_eps, float log_floor, const float* gmel, float* dwav,
                               float* workspace, void* stream) {
  VO_CHECK_ARG(wav && window && fb && gmel && dwav && workspace, "stft_mel_bwd: null pointer");
  VO_CHECK_ARG(n_fft >= 8 && n_fft <= SMB_MAX_N && (n_fft & (n_fft - 1)) == 0, "stft_mel_bwd: n_fft=%d", n_fft);
  VO_CHECK_ARG(hop > 0 && n_mels > 0 && n_mels <= 256 && B > 0 && pad >= 0 && N > pad && N + 2 * pad >= n_fft,
               "stft_mel_bwd: bad sizes");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int F = 1 + (N + 2 * pad - n_fft) / hop;
  hipLaunchKernelGGL(stft_mel_bwd_frame_kernel, dim3((unsigned)F, (unsigned)B), dim3(256), 0, st, wav, N, F, window,
                     fb, n_fft, hop, n_mels, pad, mag_eps, log_floor, gmel, workspace);
  hipLaunchKernelGGL(stft_mel_bwd_gather_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)B), dim3(256), 0, st,
                     workspace, N, F, n_fft, hop, pad, dwav);
  VO_RETURN_LAUNCH();
}

// ---- STFT magnitude (multi-resolution STFT loss): wav (B, N) -> mag (B, 1 + N / hop, n_fft / 2 + 1)
extern "C" int vo_stft_mag(const float* wav, int B, int N, const float* window, int n_fft, int hop, float eps,
                           float* mag, void* stream) {
  VO_CHECK_ARG(wav && window && mag, "stft_mag: null pointer");
  VO_CHECK_ARG(n_fft >= 8 && n_fft <= SMB_MAX_N && (n_fft & (n_fft - 1)) == 0, "stft_mag: n_fft=%d", n_fft);
  VO_CHECK_ARG(B > 0 && hop > 0 && N > n_fft / 2, "stft_mag: bad sizes (reflect padding needs N > n_fft / 2)");
  const int F = 1 + N / hop;
  hipLaunchKernelGGL(stft_mag_kernel, dim3((unsigned)F, (unsigned)B), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), wav, N, F, window, n_fft, hop, eps, mag);
  VO_RETURN_LAUNCH();
}

extern "C" int64_t vo_stft_mag_bwd_workspace_size(int B, int N, int n_fft, int hop) {
  const int64_t F = 1 + N / hop;
  return (int64_t)B * F * n_fft * (int64_t)sizeof(float);
}

extern "C" int vo_stft_mag_bwd(const float* wav, int B, int N, const float* window, int n_fft, int hop, float eps,
                               const float* gmag, float* dwav, float* workspace, void* stream) {
  VO_CHECK_ARG(wav && window && gmag && dwav && workspace, "stft_mag_bwd: null pointer");
  VO_CHECK_ARG(n_fft >= 8 && n_fft <= SMB_MAX_N && (n_fft & (n_fft - 1)) == 0, "stft_mag_bwd: n_fft=%d", n_fft);
  VO_CHECK_ARG(B > 0 && hop > 0 && N > n_fft / 2, "stft_mag_bwd: bad sizes");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int F = 1 + N / hop;
  hipLaunchKernelGGL(stft_mag_bwd_frame_kernel, dim3((unsigned)F, (unsigned)B), dim3(256), 0, st, wav, N, F, window,
                     n_fft, hop, eps, gmag, workspace);
  hipLaunchKernelGGL(stft_mel_bwd_gather_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)B), dim3(256), 0, st,
                     workspace, N, F, n_fft, hop, n_fft / 2, dwav);
  VO_RETURN_LAUNCH();
}

// ---- one resolution's loss sums: out[3] = (sum (y-x)^2, sum y^2, sum |log y - log x|); workspace >= 3 * 512 floats
extern "C" int vo_stft_loss(const float* xm, const float* ym, int64_t n, float* out, float* workspace, void* stream) {
  VO_CHECK_ARG(xm && ym && out && workspace && n > 0, "stft_loss: bad arguments");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int nb = (int)std::min<int64_t>((n + 255) / 256, 512);
  hipLaunchKernelGGL(stft_loss_reduce_kernel, dim3((unsigned)nb), dim3(256), 0, st, xm, ym, n, workspace);
  hipLaunchKernelGGL(stft_loss_final_kernel, dim3(1), dim3(64), 0, st, workspace, nb, out);
  VO_RETURN_LAUNCH();
}

extern "C" int vo_stft_loss_grad(const float* xm, const float* ym, int64_t n, const float* sums, const float* w,
                                 float* gx, void* stream) {
  VO_CHECK_ARG(xm && ym && sums && w && gx && n > 0, "stft_loss_grad: bad arguments");
  const unsigned nb = (unsigned)std::min<int64_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(stft_loss_grad_kernel, dim3(nb), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), xm, ym, n,
                     sums, w, gx);
  VO_RETURN_LAUNCH();
}

extern "C" int vo_dropout(const void* x, int dtype, int64_t n, float p, const int64_t* seed, unsigned salt, void* y,
                          void* stream) {
  VO_CHECK_ARG(x && y && seed && n >= 0, "dropout: bad arguments");
  VO_CHECK_ARG(dtype == VO_F32 || dtype == VO_BF16, "dropout: dtype");
  VO_CHECK_ARG(p >= 0.f && p < 1.f, "dropout: p = %g outside [0, 1)", p);
  VO_CHECK_ARG(n < (1LL << 32), "dropout: %lld elements (the mask index is 32-bit)", (long long)n);
  VO_CHECK_ARG(((uintptr_t)x % 16) == 0 && ((uintptr_t)y % 16) == 0, "dropout: x / y must be 16-byte aligned");
  if (n == 0) return VO_OK;
  const uint32_t thr = (uint32_t)std::min(4294967295.0, (double)p * 4294967296.0);
  const float scale = 1.f / (1.f - p);
  const int V = dtype == VO_BF16 ? 8 : 4;
  const unsigned g = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n / V + 255) / 256, 8192));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == VO_BF16)
    hipLaunchKernelGGL(dropout_kernel<bf16_t>, dim3(g), dim3(256), 0, st, (const bf16_t*)x, n, thr, scale, seed,
                       (uint32_t)salt, (bf16_t*)y);
  else
    hipLaunchKernelGGL(dropout_kernel<float>, dim3(g), dim3(256), 0, st, (const float*)x, n, thr, scale, seed,
                       (uint32_t)salt, (float*)y);
  VO_RETURN_LAUNCH();
}
