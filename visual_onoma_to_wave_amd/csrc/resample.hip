// Sample-rate conversion on the device: band-limited interpolation with a Kaiser-windowed
// sinc, the step in front of the mel front end (the reference's librosa.load(path, sr=22050),
// scripts/preprocessor/preprocessor.py:385) and the step behind the vocoder (delivery at another rate).
//
// include/vonoma.h states the rule.  With O / M the reduced input / output rates, output n of a row reads the
// T = 2 W + 1 input samples around q = (n O) div M through row r = (n O) mod M of an (M, T) fp32 table:
//   res[n] = sum_j h[r][j] x[q - W + j],  x = 0 outside the row's n_b samples.
//
// resample_kernel: blockIdx.y = row, blockIdx.x = a tile of RS_TILE consecutive outputs, one output per lane.  The
// tile's input window (at most RS_WIN samples: 8 RS_TILE + 2 W + 2 at the decimation limit) is staged once in LDS,
// converted from int16 and zeroed outside [0, n_b), so the tap loop has no bounds and no type.  Every lane walks its
// own table row from L2 (the 48000 -> 22050 table is 170 KiB: more than LDS holds) four taps to a load, and sums
// j = 0 .. T - 1 in that order in one fmaf chain: an output's bits depend on its row's samples, n and the table
// alone -- not on the batch, the tile, skip, N, N_out or the element types.  Plain fp32 VALU work: 2 T flops per
// output against a few bytes of traffic.

#include <cmath>

#include "vo_common.h"

namespace vo {

constexpr int RS_TILE = 256;      // outputs of one workgroup, one per lane
constexpr int RS_Z = 64;          // zero crossings of the sinc on either side
constexpr double RS_ROLLOFF = 0.9475937167399596;
constexpr double RS_BETA = 14.769656459379492;
constexpr int RS_MAX_RATE = 1024; // O, M of a reduced pair
constexpr int RS_MAX_DECIM = 8;   // O / M
constexpr int RS_W_MAX = 541;     // ceil(RS_Z RS_MAX_DECIM / RS_ROLLOFF)
constexpr int RS_WIN = RS_MAX_DECIM * RS_TILE + 2 * RS_W_MAX + 2;  // 3132 samples, 12.2 KiB
static_assert(RS_W_MAX >= RS_Z * RS_MAX_DECIM / RS_ROLLOFF, "the half width at the decimation limit");

// The half width W of a reduced pair the library runs, 0 of any other: 1 <= O, M <= RS_MAX_RATE, O != M, coprime,
// O <= RS_MAX_DECIM M.
static int resample_half_width(int64_t O, int64_t M) {
  if (O < 1 || M < 1 || O > RS_MAX_RATE || M > RS_MAX_RATE || O == M || O > RS_MAX_DECIM * M) return 0;
  int64_t a = O, b = M;
  while (b) {
    const int64_t t = a % b;
    a = b;
    b = t;
  }
  if (a != 1) return 0;
  const double c = (double)(O < M ? O : M) * RS_ROLLOFF / (double)O;
  return (int)std::ceil((double)RS_Z / c);
}

// I0 by its power series sum_k ((x / 2)^k / k!)^2: every term positive, so double loses nothing to cancellation
static double bessel_i0(double x) {
  const double h = 0.5 * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 500; ++k) {
    term *= (h / k) * (h / k);
    sum += term;
    if (term < 1e-18 * sum) break;
  }
  return sum;
}

__device__ __forceinline__ float rs_sample(const int16_t* p, float mwv) { return __fdiv_rn((float)*p, mwv); }
__device__ __forceinline__ float rs_sample(const float* p, float) { return *p; }

// four consecutive coefficients of a table row: rows are T = 2 W + 1 floats apart, so only 4-byte aligned
struct __attribute__((packed, aligned(4))) RsTaps4 {
  float v[4];
};

template <typename TX, typename TY>
__global__ void __launch_bounds__(RS_TILE) resample_kernel(const TX* __restrict__ x, float mwv, int N,
                                                           const int32_t* __restrict__ lens,
                                                           const int32_t* __restrict__ skip,
                                                           const float* __restrict__ table, int O, int M, int W,
                                                           TY* __restrict__ y, PostStore<TY> store, int N_out,
                                                           int32_t* __restrict__ out_lens) {
  __shared__ float win[RS_WIN];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int64_t n_b = lens ? min(max(lens[b], 0), N) : N;
  const int64_t L = (n_b * M + O - 1) / O;
  const int64_t s = skip ? min((int64_t)max(skip[b], 0), L) : 0;
  const int m = (int)min(L - s, (int64_t)N_out);
  const int i0 = blockIdx.x * RS_TILE, i = i0 + tid;  // i < N_out + RS_TILE <= 2^31 - 1 (launcher)
  TY* yrow = y + (int64_t)b * N_out;
  if (blockIdx.x == 0 && tid == 0 && out_lens) out_lens[b] = m;
  if (i0 >= m) {  // uniform: the whole tile is padding
    if (i < N_out) yrow[i] = store(0.f);
    return;
  }
  // the tile's outputs n0 .. n0 + cnt - 1 read the input samples base .. base + wl - 1:
  // wl <= (RS_TILE - 1) RS_MAX_DECIM + 1 + 2 RS_W_MAX + 1 <= RS_WIN
  const int cnt = min(RS_TILE, m - i0);
  const int64_t n0 = s + i0, q0 = n0 * O / M;
  const int r0 = (int)(n0 * O - q0 * M);
  const int64_t base = q0 - W;
  const int wl = (r0 + (cnt - 1) * O) / M + 2 * W + 1;
  const TX* xrow = x + (int64_t)b * N;
  for (int k = tid; k < wl; k += RS_TILE) {
    const int64_t p = base + k;
    win[k] = (p >= 0 && p < n_b) ? rs_sample(xrow + p, mwv) : 0.f;
  }
  __syncthreads();
  if (i < m) {
    // n O = q0 M + r0 + tid O: the lane's q and r in 32 bits (r0 < M and tid O are below 2^18)
    const int e = r0 + tid * O, dq = e / M, r = e - dq * M;
    const int T = 2 * W + 1;
    const float* h = table + (int64_t)r * T;
    const float* w = win + dq;  // x[q - W + j] = win[q - W + j - base] = win[dq + j]
    float acc = 0.f;
    int j = 0;
#pragma unroll 4
    for (; j + 4 <= T; j += 4) {
      const RsTaps4 c = *reinterpret_cast<const RsTaps4*>(h + j);
      acc = __fmaf_rn(c.v[0], w[j], acc);
      acc = __fmaf_rn(c.v[1], w[j + 1], acc);
      acc = __fmaf_rn(c.v[2], w[j + 2], acc);
      acc = __fmaf_rn(c.v[3], w[j + 3], acc);
    }
    for (; j < T; ++j) acc = __fmaf_rn(h[j], w[j], acc);
    yrow[i] = store(acc);
  } else if (i < N_out) {
    yrow[i] = store(0.f);
  }
}

}  // namespace vo

using namespace vo;

extern "C" int vo_resample_geometry(int64_t sr_in, int64_t sr_out, int32_t* O, int32_t* M, int32_t* W) {
  VO_CHECK_ARG(O && M && W, "resample_geometry: null pointer");
  VO_CHECK_ARG(sr_in >= 1 && sr_out >= 1, "resample_geometry: the rates %lld and %lld must be >= 1", (long long)sr_in,
               (long long)sr_out);
  VO_CHECK_ARG(sr_in != sr_out, "resample_geometry: the rates are equal (%lld): nothing to convert",
               (long long)sr_in);
  int64_t a = sr_in, b = sr_out;
  while (b) {
    const int64_t t = a % b;
    a = b;
    b = t;
  }
  const int64_t o = sr_in / a, m = sr_out / a;
  const int w = resample_half_width(o, m);
  VO_CHECK_ARG(w > 0,
               "resample_geometry: %lld -> %lld reduces to %lld / %lld: both must be <= %d and their quotient <= %d",
               (long long)sr_in, (long long)sr_out, (long long)o, (long long)m, RS_MAX_RATE, RS_MAX_DECIM);
  *O = (int32_t)o;
  *M = (int32_t)m;
  *W = (int32_t)w;
  return VO_OK;
}

extern "C" int64_t vo_resample_len(int64_t n, int O, int M) {
  if (n <= 0 || O < 1 || M < 1) return 0;
  return (int64_t)(((__int128)n * M + O - 1) / O);
}

extern "C" int vo_resample_table(int O, int M, float* host_out) {
  VO_CHECK_ARG(host_out, "resample_table: null pointer");
  const int W = resample_half_width(O, M);
  VO_CHECK_ARG(W > 0, "resample_table: (%d, %d) is not a reduced pair with both <= %d and O / M <= %d", O, M,
               RS_MAX_RATE, RS_MAX_DECIM);
  const int T = 2 * W + 1;
  const double pi = 3.14159265358979323846;
  const double c = (double)(O < M ? O : M) * RS_ROLLOFF / (double)O, i0b = bessel_i0(RS_BETA);
  for (int r = 0; r < M; ++r)
    for (int j = 0; j < T; ++j) {
      const double t = c * ((double)(j - W) - (double)r / (double)M);
      double h = 0.0;
      if (std::fabs(t) < RS_Z) {
        const double u = t / RS_Z, a = pi * t;
        const double sinc = t == 0.0 ? 1.0 : std::sin(a) / a;
        h = c * sinc * bessel_i0(RS_BETA * std::sqrt(1.0 - u * u)) / i0b;
      }
      host_out[(int64_t)r * T + j] = (float)h;
    }
  return VO_OK;
}

extern "C" int vo_resample(const void* x, int x_is_int16, float max_wav_value, int B, int N, const int32_t* lens,
                           const int32_t* skip, const float* table, int O, int M, void* y, int y_is_int16,
                           float pcm_scale, int N_out, int32_t* out_lens, void* stream) {
  VO_CHECK_ARG(x && y && table, "resample: null pointer");
  VO_CHECK_ARG(B >= 1 && B <= 65535, "resample: B %d is outside [1, 65535]", B);
  VO_CHECK_ARG(N >= 1 && N_out >= 1, "resample: N %d and N_out %d must be >= 1", N, N_out);
  VO_CHECK_ARG(N_out <= INT32_MAX - RS_TILE, "resample: N_out %d is above 2^31 - 1 - %d", N_out, RS_TILE);
  const int W = resample_half_width(O, M);
  VO_CHECK_ARG(W > 0, "resample: (%d, %d) is not a reduced pair with both <= %d and O / M <= %d", O, M, RS_MAX_RATE,
               RS_MAX_DECIM);
  VO_CHECK_ARG(!x_is_int16 || (std::isfinite(max_wav_value) && max_wav_value > 0.f),
               "resample: max_wav_value %g is not finite and positive", max_wav_value);
  VO_CHECK_ARG(!y_is_int16 || (std::isfinite(pcm_scale) && pcm_scale > 0.f),
               "resample: pcm_scale %g is not finite and positive", pcm_scale);
  const dim3 grid((unsigned)((N_out + RS_TILE - 1) / RS_TILE), (unsigned)B);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  with_bool(x_is_int16 != 0, [&](auto xi) {
    return with_bool(y_is_int16 != 0, [&](auto yi) {
      using TX = std::conditional_t<decltype(xi)::value, int16_t, float>;
      using TY = std::conditional_t<decltype(yi)::value, int16_t, float>;
      PostStore<TY> store{};
      if constexpr (decltype(yi)::value) store.scale = pcm_scale;
      hipLaunchKernelGGL((resample_kernel<TX, TY>), grid, dim3(RS_TILE), 0, st, static_cast<const TX*>(x),
                         max_wav_value, N, lens, skip, table, O, M, W, static_cast<TY*>(y), store, N_out, out_lens);
      return 0;
    });
  });
  VO_RETURN_LAUNCH();
}
