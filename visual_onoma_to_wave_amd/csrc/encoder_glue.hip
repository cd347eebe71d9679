// Encoder front: the visual feature extractor's per-glyph stencil stack, and the
// positional / class embedding adds.
//
// vfe_stencil replaces VisualFeatureExtractor.forward up to the bridge Linear
// (scripts/model/visual_feature_extractor.py:60-80): the Python loop that slices the
// strip into 102-px character columns becomes the grid (one workgroup per slice), and
// the three Conv2d(1->1, 3x3, pad 1) -> BatchNorm2d(eval) -> ReLU layers run in LDS on
// the 24 x 102 tile with a zero border.  Output is the flattened (h*W + w) row the
// bridge GEMM reads.

#include "vo_common.h"

namespace vo {

constexpr int VFE_MAXH = 32;
constexpr int VFE_MAXW = 128;

template <typename TY>
__global__ void __launch_bounds__(256) vfe_kernel(const float* __restrict__ img, int H, int W, int sw, int n_slices,
                                                  const float* __restrict__ conv, const float* __restrict__ bn,
                                                  int n_layers, TY* __restrict__ out) {
  __shared__ float buf[2][(VFE_MAXH + 2) * (VFE_MAXW + 2)];
  const int P = sw + 2;  // pitch with a 1-px zero border on each side
  const int slice = blockIdx.x;
  const int b = slice / n_slices, i = slice - b * n_slices;
  const float* src = img + (int64_t)b * H * W + (int64_t)i * sw;
  const int tid = threadIdx.x;
  for (int v = tid; v < (H + 2) * P; v += 256) {
    const int r = v / P, c = v - r * P;
    float val = 0.f;
    if (r >= 1 && r <= H && c >= 1 && c <= sw) val = src[(int64_t)(r - 1) * W + (c - 1)];
    buf[0][v] = val;
    buf[1][v] = 0.f;
  }
  __syncthreads();
  int cur = 0;
  for (int l = 0; l < n_layers; ++l) {
    const float* k = conv + l * 10;
    const float sc = bn[2 * l], sh = bn[2 * l + 1];
    for (int v = tid; v < H * sw; v += 256) {
      const int r = v / sw + 1, c = v - (r - 1) * sw + 1;
      const float* s = buf[cur];
      float acc = k[9];
#pragma unroll
      for (int dr = -1; dr <= 1; ++dr)
#pragma unroll
        for (int dc = -1; dc <= 1; ++dc) acc += k[(dr + 1) * 3 + (dc + 1)] * s[(r + dr) * P + (c + dc)];
      const float y = acc * sc + sh;
      buf[cur ^ 1][r * P + c] = y > 0.f ? y : 0.f;
    }
    __syncthreads();
    cur ^= 1;
  }
  TY* o = out + (int64_t)slice * H * sw;
  for (int v = tid; v < H * sw; v += 256) {
    const int r = v / sw, c = v - r * sw;
    o[v] = from_f32<TY>(buf[cur][(r + 1) * P + (c + 1)]);
  }
}

// ---- the general form (vo_vfe_stencil_ex): context windows of `stride` character cells, kh x kw taps
//
// One workgroup per window (b, i) = image columns [i sw, i sw + ww), ww = sw * stride.  The whole window with
// its zero border ((kh-1)/2 rows, (KW-1)/2 columns, the columns rounded up to whole 16-byte chunks on both
// sides) sits twice in dynamic LDS; the layers ping-pong between the two copies and only ever write the
// interior, so every layer sees zeros past the WINDOW's edge -- never a neighbouring window's pixels.
// A thread produces 4 adjacent columns: per kernel row it reads the 4 + 2 PWA columns around them as
// 16-byte chunks (consecutive lanes, consecutive chunks) and reuses them across the KW taps in registers.
// KW is a template parameter so that this register window is indexed by constants; kh, the layers and
// the tap values (uniform: scalar loads) are runtime.  Per output: acc = bias, one fma per tap in
// row-major tap order, acc * scale + shift, ReLU -- vfe_kernel's arithmetic.
constexpr int VFE_MAXK = 9;
constexpr int64_t VFE_LDS_MAX = 160 * 1024;
constexpr int VFE_EX_THREADS = 1024;  // per window; DESIGN.md section 3 has the 256 / 512 / 1024 times

// floats per bordered LDS row
static inline int64_t vfe_ex_pitch(int win_w, int kw) {
  const int pwa = ((kw - 1) / 2 + 3) / 4 * 4;
  return 2 * (int64_t)pwa + ((int64_t)win_w + 3) / 4 * 4;
}

template <typename TY, int KW>
__global__ void __launch_bounds__(1024) vfe_ex_kernel(const float* __restrict__ img, int H, int W, int sw, int ww,
                                                      int n_slices, int kh, const float* __restrict__ conv,
                                                      const float* __restrict__ bn, int n_layers,
                                                      TY* __restrict__ out) {
  extern __shared__ __align__(16) float vfe_lds[];
  constexpr int PW = (KW - 1) / 2, PWA = (PW + 3) / 4 * 4, NX = 4 + 2 * PWA;
  const int ph = (kh - 1) / 2;
  const int nq = (ww + 3) >> 2;    // 4-column chunks of a window row
  const int P = 2 * PWA + 4 * nq;  // LDS pitch (floats), PQ chunks
  const int PQ = P >> 2;
  const int rows = H + 2 * ph;
  float* buf0 = vfe_lds;
  float* buf1 = vfe_lds + rows * P;
  const int slice = blockIdx.x;
  const int b = slice / n_slices, i = slice - b * n_slices;
  const float* src = img + (int64_t)b * H * W + (int64_t)i * sw;
  const int tid = threadIdx.x, nt = blockDim.x;

  // stage: every load unconditional (row and column clamped into the window), zeroed at the LDS write
  for (int v = tid; v < rows * PQ; v += nt) {
    const int r = v / PQ, q = v - r * PQ;
    const int h = r - ph, c0 = 4 * q - PWA;
    const bool rin = h >= 0 && h < H;
    const float* sr = src + (int64_t)min(max(h, 0), H - 1) * W;
    f32x4 val;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = c0 + e;
      const float x = sr[min(max(c, 0), ww - 1)];
      val[e] = (rin && c >= 0 && c < ww) ? x : 0.f;
    }
    *reinterpret_cast<f32x4*>(buf0 + 4 * v) = val;
    *reinterpret_cast<f32x4*>(buf1 + 4 * v) = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  __syncthreads();

  const int ntap = kh * KW;
  int cur = 0;
  for (int l = 0; l < n_layers; ++l) {
    const float* k = conv + (int64_t)l * (ntap + 1);
    const float bias = k[ntap], sc = bn[2 * l], sh = bn[2 * l + 1];
    const float* s = cur ? buf1 : buf0;
    float* d = cur ? buf0 : buf1;
    for (int v = tid; v < H * nq; v += nt) {
      const int h = v / nq, q = v - h * nq;
      float acc[4] = {bias, bias, bias, bias};
      // LDS row h + di is window row h + di - ph; LDS column 4 q + j is window column 4 q + j - PWA
      const float* rp = s + h * P + 4 * q;
      for (int di = 0; di < kh; ++di, rp += P) {
        float x[NX];
#pragma unroll
        for (int c = 0; c < NX / 4; ++c) {
          const f32x4 t = *reinterpret_cast<const f32x4*>(rp + 4 * c);
          x[4 * c] = t[0]; x[4 * c + 1] = t[1]; x[4 * c + 2] = t[2]; x[4 * c + 3] = t[3];
        }
        const float* kr = k + di * KW;
#pragma unroll
        for (int dj = 0; dj < KW; ++dj) {
          const float kv = kr[dj];
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[e] = fmaf(kv, x[PWA - PW + dj + e], acc[e]);
        }
      }
      f32x4 y;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float t = fmaf(acc[e], sc, sh);
        y[e] = (4 * q + e < ww && t > 0.f) ? t : 0.f;  // the chunk's columns past ww stay zero: they are border
      }
      *reinterpret_cast<f32x4*>(d + (h + ph) * P + PWA + 4 * q) = y;
    }
    __syncthreads();
    cur ^= 1;
  }
  const float* s = (cur ? buf1 : buf0) + ph * P + PWA;
  TY* o = out + (int64_t)slice * H * ww;
  for (int v = tid; v < H * ww; v += nt) {
    const int h = v / ww, c = v - h * ww;
    o[v] = from_f32<TY>(s[h * P + c]);
  }
}

template <typename TX>
__global__ void add_pos_class_kernel(TX* __restrict__ x, const float* __restrict__ pe, const float* __restrict__ cls,
                                     const int64_t* __restrict__ cls_idx, int per_token, int B, int T, int D) {
  const int64_t n4 = (int64_t)B * T * D / 4;
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < n4; v += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = v * 4;
    const int c = (int)(e % D);
    const int64_t bt = e / D;
    const int t = (int)(bt % T), b = (int)(bt / T);
    float q[4];
    load4(x + e, q);
    if (pe) {
      float p[4];
      load4(pe + (int64_t)t * D + c, p);
#pragma unroll
      for (int k = 0; k < 4; ++k) q[k] += p[k];
    }
    if (cls) {
      float p[4];
      load4(cls + cls_idx[per_token ? bt : b] * D + c, p);
#pragma unroll
      for (int k = 0; k < 4; ++k) q[k] += p[k];
    }
    store4(x + e, q);
  }
}

// mask[b, t] = t >= len[b] (True = padding), len given as int64, int32 or float
template <typename TL>
__global__ void mask_kernel(const TL* __restrict__ lens, int B, int L, bool* __restrict__ mask,
                            int32_t* __restrict__ lens32) {
  const int64_t n = (int64_t)B * L;
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < n; v += (int64_t)gridDim.x * blockDim.x) {
    const int b = (int)(v / L), t = (int)(v - (int64_t)b * L);
    if (mask) mask[v] = (double)t >= (double)lens[b];
    if (lens32 && t == 0) lens32[b] = (int32_t)lens[b];
  }
  if (L == 0 && lens32) {
    for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < B; b += gridDim.x * blockDim.x) lens32[b] = (int32_t)lens[b];
  }
}

}  // namespace vo

using namespace vo;

extern "C" int vo_mask_from_lengths(const void* lens, int lens_dtype, int B, int L, bool* mask, int32_t* lens32,
                                    void* stream) {
  VO_CHECK_ARG(lens && (mask || lens32), "mask_from_lengths: null pointer");
  if (B == 0) return VO_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t n = std::max<int64_t>((int64_t)B * L, B);
  dim3 grid((unsigned)std::min<int64_t>((n + 255) / 256, 1024));
  if (lens_dtype == 0)
    hipLaunchKernelGGL(mask_kernel<float>, grid, dim3(256), 0, st, (const float*)lens, B, L, mask, lens32);
  else if (lens_dtype == 2)
    hipLaunchKernelGGL(mask_kernel<int64_t>, grid, dim3(256), 0, st, (const int64_t*)lens, B, L, mask, lens32);
  else if (lens_dtype == 3)
    hipLaunchKernelGGL(mask_kernel<int32_t>, grid, dim3(256), 0, st, (const int32_t*)lens, B, L, mask, lens32);
  else {
    vo_set_error("mask_from_lengths: lens dtype must be 0 (f32), 2 (int64) or 3 (int32)");
    return VO_ERR_INVALID;
  }
  VO_RETURN_LAUNCH();
}

extern "C" int vo_vfe_stencil(const float* images, int B, int H, int W, int slice_w, int n_slices, const float* conv,
                              const float* bn, int n_layers, void* out, int out_dtype, void* stream) {
  VO_CHECK_ARG(images && conv && bn && out, "vfe_stencil: null pointer");
  VO_CHECK_ARG(H <= VFE_MAXH && slice_w <= VFE_MAXW && H > 0 && slice_w > 0,
               "vfe_stencil: slice %dx%d exceeds %dx%d", H, slice_w, VFE_MAXH, VFE_MAXW);
  VO_CHECK_ARG(n_slices >= 0 && (int64_t)n_slices * slice_w <= W, "vfe_stencil: %d slices of %d px > width %d",
               n_slices, slice_w, W);
  if (B == 0 || n_slices == 0) return VO_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  dim3 grid((unsigned)(B * n_slices));
  if (out_dtype == VO_BF16)
    hipLaunchKernelGGL(vfe_kernel<bf16_t>, grid, dim3(256), 0, st, images, H, W, slice_w, n_slices, conv, bn,
                       n_layers, (bf16_t*)out);
  else
    hipLaunchKernelGGL(vfe_kernel<float>, grid, dim3(256), 0, st, images, H, W, slice_w, n_slices, conv, bn,
                       n_layers, (float*)out);
  VO_RETURN_LAUNCH();
}

extern "C" int64_t vo_vfe_stencil_lds_bytes(int H, int win_w, int kh, int kw) {
  if (H < 1 || win_w < 1 || kh < 1 || kw < 1) return -1;
  return 2 * ((int64_t)H + kh - 1) * vfe_ex_pitch(win_w, kw) * (int64_t)sizeof(float);
}

template <typename TY>
static void vfe_ex_launch(int kw, dim3 grid, int threads, size_t lds, hipStream_t st, const float* images, int H, int W,
                          int slice_w, int ww, int n_slices, int kh, const float* conv, const float* bn, int n_layers,
                          TY* out) {
#define VO_VFE_EX(KW)                                                                                              \
  hipLaunchKernelGGL((vfe_ex_kernel<TY, KW>), grid, dim3(threads), lds, st, images, H, W, slice_w, ww, n_slices, kh, \
                     conv, bn, n_layers, out)
  switch (kw) {
    case 1: VO_VFE_EX(1); break;
    case 3: VO_VFE_EX(3); break;
    case 5: VO_VFE_EX(5); break;
    case 7: VO_VFE_EX(7); break;
    default: VO_VFE_EX(9); break;
  }
#undef VO_VFE_EX
}

extern "C" int vo_vfe_stencil_ex(const float* images, int B, int H, int W, int slice_w, int stride, int n_slices, int kh,
                                 int kw, const float* conv, const float* bn, int n_layers, void* out, int out_dtype,
                                 void* stream) {
  VO_CHECK_ARG(images && conv && bn && out, "vfe_stencil_ex: null pointer");
  VO_CHECK_ARG(kh >= 1 && kw >= 1 && kh % 2 == 1 && kw % 2 == 1 && kh <= VFE_MAXK && kw <= VFE_MAXK,
               "vfe_stencil_ex: kernel %dx%d unsupported (odd sizes up to %d)", kh, kw, VFE_MAXK);
  VO_CHECK_ARG(H > 0 && H <= VFE_MAXH && slice_w > 0 && B >= 0 && W > 0 && n_layers >= 0,
               "vfe_stencil_ex: H=%d (1..%d), slice_w=%d, B=%d, W=%d, n_layers=%d", H, VFE_MAXH, slice_w, B, W, n_layers);
  VO_CHECK_ARG(stride >= 1, "vfe_stencil_ex: stride %d < 1", stride);
  const int64_t ww = (int64_t)slice_w * stride;
  VO_CHECK_ARG(n_slices >= 0 && ((int64_t)n_slices - 1) * slice_w + ww <= W,
               "vfe_stencil_ex: %d windows of %d x %d px at a step of %d px > width %d", n_slices, stride, slice_w, slice_w, W);
  // ww <= W < 2^31 from here on
  const int64_t lds = vo_vfe_stencil_lds_bytes(H, (int)ww, kh, kw);
  if (lds > VFE_LDS_MAX) {
    vo_set_error("vfe_stencil_ex: a %d x %lld window with %dx%d taps needs %lld B of LDS, over 160 KiB", H, (long long)ww,
                 kh, kw, (long long)lds);
    return VO_ERR_INVALID;
  }
  if (B == 0 || n_slices == 0) return VO_OK;
  VO_CHECK_ARG((int64_t)B * n_slices <= INT32_MAX, "vfe_stencil_ex: %d x %d windows", B, n_slices);
  // The ICASSP point is vfe_kernel itself, so the two entries agree to the bit there whatever the compiler makes
  // of either kernel.  (As built today vfe_kernel is no pure fma chain: its first tap is fused, the other eight
  // are packed multiplies followed by adds; vfe_ex_kernel fuses every tap, so the two differ in the last bits.)
  if (stride == 1 && kh == 3 && kw == 3 && slice_w <= VFE_MAXW)
    return vo_vfe_stencil(images, B, H, W, slice_w, n_slices, conv, bn, n_layers, out, out_dtype, stream);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  // threads: VFE_EX_THREADS, but no more than the window has 4-column items (whole waves)
  const int64_t items = (int64_t)H * ((ww + 3) / 4);
  const int threads = (int)std::min<int64_t>(VFE_EX_THREADS, (items + 63) / 64 * 64);
  dim3 grid((unsigned)(B * n_slices));
  if (out_dtype == VO_BF16)
    vfe_ex_launch<bf16_t>(kw, grid, threads, (size_t)lds, st, images, H, W, slice_w, (int)ww, n_slices, kh, conv, bn,
                          n_layers, (bf16_t*)out);
  else
    vfe_ex_launch<float>(kw, grid, threads, (size_t)lds, st, images, H, W, slice_w, (int)ww, n_slices, kh, conv, bn,
                         n_layers, (float*)out);
  VO_RETURN_LAUNCH();
}

extern "C" int vo_add_pos_class(void* x, int x_dtype, const float* pe, const float* cls, const int64_t* cls_idx,
                                int idx_per_token, int B, int T, int D, void* stream) {
  VO_CHECK_ARG(x && (!cls || cls_idx), "add_pos_class: null pointer");
  VO_CHECK_ARG(D % 4 == 0, "add_pos_class: D=%d must be a multiple of 4", D);
  if (B == 0 || T == 0) return VO_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int64_t n4 = (int64_t)B * T * D / 4;
  dim3 grid((unsigned)std::min<int64_t>((n4 + 255) / 256, 2048));
  if (x_dtype == VO_BF16)
    hipLaunchKernelGGL(add_pos_class_kernel<bf16_t>, grid, dim3(256), 0, st, (bf16_t*)x, pe, cls, cls_idx, idx_per_token, B, T, D);
  else
    hipLaunchKernelGGL(add_pos_class_kernel<float>, grid, dim3(256), 0, st, (float*)x, pe, cls, cls_idx, idx_per_token, B, T, D);
  VO_RETURN_LAUNCH();
}
