// Shared device helpers for the gfx950 (CDNA4) kernels of the synthesis path.
// Wave = 64 lanes; MFMA 16x16x32 bf16 (or 8 x 16x16x4 f32 in the fp32 parity mode).
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/vonoma.h"

typedef unsigned short bf16_t;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace vo {

// ---------------------------------------------------------------- scalar conversion
__device__ __forceinline__ float to_f32(float x) { return x; }
__device__ __forceinline__ float to_f32(bf16_t x) { return __uint_as_float(((uint32_t)x) << 16); }

template <typename T> __device__ __forceinline__ T from_f32(float x);
template <> __device__ __forceinline__ float from_f32<float>(float x) { return x; }
template <> __device__ __forceinline__ bf16_t from_f32<bf16_t>(float x) {
  __hip_bfloat16 b = __float2bfloat16(x);  // round-to-nearest-even, NaN stays NaN
  return *reinterpret_cast<bf16_t*>(&b);
}

// Two floats -> one packed bf16 pair in ONE v_cvt_pk_bf16_f32 (round to nearest even, NaN stays
// NaN).  The pair of scalar conversions compiled to two v_cvt_pk_bf16_f32 and a v_or_b32_sdwa.
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pk_bf16(float lo, float hi) {
  return __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2_t){lo, hi}, bf16x2_t));
}
// leaky ReLU max(v, s v) for 0 <= s <= 1.  IEEE maximum: unlike fmaxf it needs no operand
// canonicalisation (fmaxf of a value bit-cast from bf16 compiled to two v_max_f32); the results
// are identical (a NaN input gives a NaN either way).
__device__ __forceinline__ float lrelu_max(float v, float s) { return __builtin_elementwise_maximum(v, v * s); }

// The conv epilogue of 8 consecutive channels, q = (post(acc + bias) + x1) * scale + x2 in this order of roundings
// (post = tanh, or leaky ReLU with slope ps in [0, 1]: 1 = none, 0 = ReLU; x1 / x2 only where r1 / r2).  One
// definition for conv_epilogue_vec (conv1d.hip) and the plane conv (conv_plane.hip): both compile the same
// expression, so the two kernels round alike.
__device__ __forceinline__ void conv_epilogue8(const float (&acc)[8], const float (&bias)[8], bool tanh_act, float ps,
                                               bool r1, const float (&x1)[8], float scale, bool r2,
                                               const float (&x2)[8], float (&q)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float v = acc[e] + bias[e];
    v = tanh_act ? tanhf(v) : lrelu_max(v, ps);  // ps in [0, 1]
    if (r1) v += x1[e];
    v *= scale;
    if (r2) v += x2[e];
    q[e] = v;
  }
}

// Index of the table entry owning item x: the last i < n with start[i] <= x (start ascending,
// start[0] = 0) -- a binary search over a table in the kernel arguments, so a workgroup near the
// end of a 32-entry table pays 5 dependent scalar loads instead of 32.
__device__ __forceinline__ int table_find(const int* start, int n, int x) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (start[mid] <= x) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// Ragged batches (vonoma.h, "per-utterance lengths"): the valid rows of utterance b of a (B, T, C) tensor,
// clamp(lens[b] * scale, 0, T).  b is uniform where the kernels call it: a scalar load.
__device__ __forceinline__ int rag_rows(const int32_t* lens, int scale, int b, int T) {
  const int64_t r = (int64_t)max(lens[b], 0) * scale;
  return (int)min(r, (int64_t)T);
}

// Workgroups are dispatched round-robin over the 8 XCDs by linear id (w -> XCD w % 8), and each
// XCD has its own L2.  xcd_grouped_id(w, n) maps linear id w of an n-workgroup grid to a logical id
// in [0, n) such that consecutive logical ids run on one XCD: workgroups that read the same bytes
// (the query tiles of one attention head, ...) take logical ids next to each other and share that
// XCD's L2 instead of every XCD fetching them.
__device__ __forceinline__ int xcd_grouped_id(int w, int n) {
  const int x = w & 7, k = w >> 3, q = n >> 3, r = n & 7;
  return x * q + (x < r ? x : r) + k;
}

// Workgroup barrier for LDS hand-offs: this wave's LDS operations drained, then s_barrier.
// __syncthreads() adds a workgroup-scope release fence, and on gfx950 that fence waits vmcnt(0):
// every outstanding global load or store of the wave (an epilogue's y stores, a prefetch meant to
// stay in flight across the barrier) is drained at each barrier.  LDS-DMA destinations still
// need their own vmcnt wait before this barrier; no global memory is handed between waves.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ---------------------------------------------------------------- counter-based dropout mask
// Element i of a dropout site is kept iff drop_hash(s0, s1, i) >= p 2^32 (vo_dropout, and the LayerNorm kernels
// that apply a sublayer's dropout in-pass): (s0, s1) from the step's device seed and the site's salt.
__device__ __forceinline__ uint32_t drop_mix(uint32_t h) {  // murmur3 finaliser
  h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
  return h;
}
__device__ __forceinline__ uint32_t drop_hash(uint32_t s0, uint32_t s1, uint32_t i) {
  return drop_mix(drop_mix(i * 0x9E3779B9u ^ s0) + s1);
}
__device__ __forceinline__ void drop_keys(const int64_t* seed, uint32_t salt, uint32_t& s0, uint32_t& s1) {
  const uint64_t sd = (uint64_t)seed[0];
  s0 = (uint32_t)sd ^ drop_mix(salt + 0x3C6EF372u);
  s1 = (uint32_t)(sd >> 32);
}

// ---------------------------------------------------------------- 8-element vectors
// Load 8 consecutive elements (16 B for bf16, 32 B for f32) as floats.
__device__ __forceinline__ void load8(const bf16_t* p, float (&v)[8]) {
  uint4 u = *reinterpret_cast<const uint4*>(p);
  uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[2 * i] = __uint_as_float(w[i] << 16);
    v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}
__device__ __forceinline__ void load8(const float* p, float (&v)[8]) {
  float4 a = *reinterpret_cast<const float4*>(p);
  float4 b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void store8(bf16_t* p, const float (&v)[8]) {
  uint32_t w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    w[i] = pk_bf16(v[2 * i], v[2 * i + 1]);
  *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
}
__device__ __forceinline__ void store8(float* p, const float (&v)[8]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}
__device__ __forceinline__ void store4(bf16_t* p, const float (&v)[4]) {
  uint32_t a = pk_bf16(v[0], v[1]);
  uint32_t b = pk_bf16(v[2], v[3]);
  *reinterpret_cast<uint2*>(p) = make_uint2(a, b);
}
__device__ __forceinline__ void store4(float* p, const float (&v)[4]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void load4(const bf16_t* p, float (&v)[4]) {
  uint2 u = *reinterpret_cast<const uint2*>(p);
  v[0] = __uint_as_float(u.x << 16); v[1] = __uint_as_float(u.x & 0xffff0000u);
  v[2] = __uint_as_float(u.y << 16); v[3] = __uint_as_float(u.y & 0xffff0000u);
}
__device__ __forceinline__ void load4(const float* p, float (&v)[4]) {
  float4 a = *reinterpret_cast<const float4*>(p);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
}

// One 16-byte vector of a lane, V = 8 bf16 / 4 fp32 elements (the vectorised BatchNorm kernels, vo_dropout)
template <typename TX> struct BnVec;
template <> struct BnVec<float> {
  static constexpr int V = 4;
  __device__ static __forceinline__ void load(const float* p, float (&v)[4]) {
    const float4 u = *reinterpret_cast<const float4*>(p);
    v[0] = u.x; v[1] = u.y; v[2] = u.z; v[3] = u.w;
  }
  __device__ static __forceinline__ void store(float* p, const float (&v)[4]) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  }
};
template <> struct BnVec<bf16_t> {
  static constexpr int V = 8;
  __device__ static __forceinline__ void load(const bf16_t* p, float (&v)[8]) {
    const uint4 u = *reinterpret_cast<const uint4*>(p);
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[2 * i] = __uint_as_float(w[i] << 16);
      v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
    }
  }
  __device__ static __forceinline__ void store(bf16_t* p, const float (&v)[8]) {
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = pk_bf16(v[2 * i], v[2 * i + 1]);
    *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
  }
};

// ---------------------------------------------------------------- MFMA fragments
// A fragment holds A[row = lane&15][k = 8*(lane>>4) + j], B holds B[k = 8*(lane>>4)+j][col = lane&15]
// (j = 0..7).  For bf16 that is exactly one v_mfma_f32_16x16x32_bf16.  For f32 the same
// 32-deep k-slice is split into 8 v_mfma_f32_16x16x4_f32 whose k index (lane>>4) maps to
// k = 8*(lane>>4) + j -- any consistent k permutation of A and B gives the same sum.
template <typename TC> struct Frag;
template <> struct Frag<bf16_t> {
  bf16x8 v;
  __device__ __forceinline__ void load(const bf16_t* p) { v = *reinterpret_cast<const bf16x8*>(p); }
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (__bf16)0.0f;
  }
};
// Fragment by two transposed LDS reads (ds_read_b64_tr_b16, gfx950): each read delivers 4 rows of one channel per
// lane, so a row-major (channels-last) LDS tile feeds the fragment's k = row index without a transpose pass.  Lane
// 4 q + p of a 16-lane group names row q, channels 4 p .. 4 p + 3 of a 4-row block (8-byte aligned; every lane
// active); lo fills elements 0..3, hi 4..7.  The callers differ only in where the two blocks lie.
__device__ __forceinline__ Frag<bf16_t> tr_frag(const bf16_t* lo_p, const bf16_t* hi_p) {
  typedef short v4s __attribute__((ext_vector_type(4)));
  typedef short v8s __attribute__((ext_vector_type(8)));
  typedef __attribute__((address_space(3))) v4s lds_v4s;
  const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)lo_p);
  const v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)hi_p);
  // whole-vector bit cast: per-element __bf16 inserts were mis-lowered by hipcc (only the low dword of each read
  // survived)
  Frag<bf16_t> f;
  f.v = __builtin_bit_cast(bf16x8, (v8s)__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
  return f;
}
template <> struct Frag<float> {
  float v[8];
  __device__ __forceinline__ void load(const float* p) {
    float4 a = *reinterpret_cast<const float4*>(p);
    float4 b = *reinterpret_cast<const float4*>(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  }
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = 0.f;
  }
};

__device__ __forceinline__ f32x4 mfma(const Frag<bf16_t>& a, const Frag<bf16_t>& b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.v, b.v, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma(const Frag<float>& a, const Frag<float>& b, f32x4 c) {
#pragma unroll
  for (int j = 0; j < 8; ++j) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.v[j], b.v[j], c, 0, 0, 0);
  return c;
}

// ---------------------------------------------------------------- split-bf16 fp32 contractions (VO_F32X3)
// An fp32 operand v is held as hi = bf16(v), lo = bf16(v - hi) (v - hi is exact in fp32), and a product
// as hi a * hi b + hi a * lo b + lo a * hi b: three 16x16x32 bf16 MFMAs with fp32 accumulation in place
// of eight 16x16x4 f32 ones (5.3x fewer MFMA cycles).  Per product the dropped lo a * lo b and the
// rounding of the lo parts leave <= 3 * 2^-18 of |a b| (~1e-5) -- fp32-class accuracy, not bit-exact
// fp32.  bx3_t is the LDS element of such a tile: 8 channels = 32 bytes = [hi x 8 | lo x 8], so an
// 8-element vector sits where an fp32 tile would put it (same offsets, same 4-byte element).
struct bx3_t { uint32_t u; };
__device__ __forceinline__ void split8(const float (&v)[8], uint4& hi, uint4& lo) {
  uint32_t h[4], l[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    h[i] = pk_bf16(v[2 * i], v[2 * i + 1]);
    const float r0 = v[2 * i] - __uint_as_float(h[i] << 16);
    const float r1 = v[2 * i + 1] - __uint_as_float(h[i] & 0xffff0000u);
    l[i] = pk_bf16(r0, r1);
  }
  hi = make_uint4(h[0], h[1], h[2], h[3]);
  lo = make_uint4(l[0], l[1], l[2], l[3]);
}
__device__ __forceinline__ void store8(bx3_t* p, const float (&v)[8]) {
  uint4 hi, lo;
  split8(v, hi, lo);
  reinterpret_cast<uint4*>(p)[0] = hi;
  reinterpret_cast<uint4*>(p)[1] = lo;
}
template <> struct Frag<bx3_t> {
  bf16x8 hi, lo;
  __device__ __forceinline__ void load(const bx3_t* p) {
    hi = reinterpret_cast<const bf16x8*>(p)[0];
    lo = reinterpret_cast<const bf16x8*>(p)[1];
  }
};
__device__ __forceinline__ f32x4 mfma(const Frag<bx3_t>& a, const Frag<bx3_t>& b, f32x4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.lo, b.hi, c, 0, 0, 0);  // small terms first
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.hi, b.lo, c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.hi, b.hi, c, 0, 0, 0);
}

// ---------------------------------------------------------------- activations
__device__ __forceinline__ float act(int kind, float x, float slope) {
  switch (kind) {
    case VO_ACT_RELU: return x > 0.f ? x : 0.f;
    case VO_ACT_LRELU: return x > 0.f ? x : x * slope;
    case VO_ACT_TANH: return tanhf(x);
    default: return x;
  }
}

// ---------------------------------------------------------------- waveform stores
// How a kernel that ends in a waveform (conv_post, resample) stores a sample, by the output element type TY.  float: the value itself (the struct is
// empty, so the fp32 instantiations are the kernels they were).  int16_t: q = (int16) clamp(trunc(v * scale), -32768,
// 32767), the product in fp32 -- the host's (wav * max_wav_value).astype("int16") for values in range.  Deliberate
// deviation: tanhf gives exactly +-1.0f for large inputs and 1.0f * 32768 is outside int16, where the host cast is
// undefined (it wraps to -32768, a click); this stores 32767.  NaN stores 0.  Element stores only: a row of y is
// 2-byte aligned when T is odd.
template <typename TY>
struct PostStore;
template <>
struct PostStore<float> {
  __device__ float operator()(float v) const { return v; }
};
template <>
struct PostStore<int16_t> {
  float scale;
  __device__ int16_t operator()(float v) const {
    const float p = v * scale;
    // fminf / fmaxf return the non-NaN operand, so a NaN is caught first; both bounds are exact in fp32
    return (p != p) ? (int16_t)0 : (int16_t)(int)truncf(fminf(fmaxf(p, -32768.f), 32767.f));
  }
};

// ---------------------------------------------------------------- wave reductions (64 lanes)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// ---------------------------------------------------------------- host: device query
// compute units of the current device, queried once (256, the MI355X's, when the query fails):
// what the persistent launchers size their grids by
inline int cu_count() {
  static int n = 0;
  if (!n) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      n = 256;
  }
  return n;
}

}  // namespace vo

// error plumbing shared by the launchers (vo_runtime.cpp)
extern "C" void vo_set_error(const char* fmt, ...);
extern "C" int vo_tune_get(const char* key);

#define VO_CHECK_ARG(cond, ...)                \
  do {                                         \
    if (!(cond)) {                             \
      vo_set_error(__VA_ARGS__);               \
      return VO_ERR_INVALID;                   \
    }                                          \
  } while (0)

#define VO_RETURN_LAUNCH()                                       \
  do {                                                           \
    hipError_t e_ = hipGetLastError();                           \
    if (e_ != hipSuccess) {                                      \
      vo_set_error("launch failed: %s", hipGetErrorString(e_));  \
      return (int)e_;                                            \
    }                                                            \
    return VO_OK;                                                \
  } while (0)

// ---------------------------------------------------------------- host: runtime dtype / flag -> template argument
// A launcher names its instantiations once, inside a generic lambda: with_dtype(dtype, who, f) calls f(tag) with
// decltype(tag)::type = float / bf16_t and ::id = VO_F32 / VO_BF16, with_dtypes the same for a pair, with_bool
// f(std::true_type / std::false_type).  Any other dtype value: VO_ERR_INVALID, the error naming `who`.  The caller
// leaves the combinations it does not ship out with `if constexpr`, so nothing else is instantiated.
namespace vo {

template <typename T, int ID>
struct DtypeTag {
  using type = T;
  static constexpr int id = ID;
};

template <class F>
int with_dtype(int dtype, const char* who, F f) {
  if (dtype == VO_F32) return f(DtypeTag<float, VO_F32>{});
  if (dtype == VO_BF16) return f(DtypeTag<bf16_t, VO_BF16>{});
  vo_set_error("%s: unsupported dtype %d", who, dtype);
  return VO_ERR_INVALID;
}

template <class F>
int with_dtypes(int dtype_a, int dtype_b, const char* who, F f) {
  return with_dtype(dtype_a, who, [&](auto a) { return with_dtype(dtype_b, who, [&](auto b) { return f(a, b); }); });
}

template <class F>
int with_bool(bool v, F f) {
  return v ? f(std::true_type{}) : f(std::false_type{});
}

}  // namespace vo
