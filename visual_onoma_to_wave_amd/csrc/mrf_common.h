// Shared by the fused MRF kernels (resblock*.hip): device helpers (16-byte staging vectors, the
// conflict-free LDS row swizzle, packed-bf16 leaky ReLU) and the one copy of their host side (the
// persistent launch, the call structs and the prototypes of the vo_*_try dispatch).
#pragma once

#include <algorithm>
#include <cmath>
#include <type_traits>

#include "vo_common.h"

namespace vo {

// staging registers use a clang vector type: HIP's uint4 struct is copied with memcpy, which
// kept the streamed-weight registers in scratch memory
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// LDS rows of 64 B (32 bf16 of one 32-channel plane); 16-byte chunk q of row r sits at chunk
// q ^ ((r >> (sh - 1)) & 2): the fragment reads of 16 consecutive rows hit distinct banks
__device__ __forceinline__ int rb_off(int r, int q, int sh) { return r * 32 + 8 * (q ^ ((r >> (sh - 1)) & 2)); }

__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
  return pk_bf16(lo, hi);
}

// leaky ReLU of 8 packed bf16 (0 <= slope <= 1: lrelu(v) = max(v, slope * v))
__device__ __forceinline__ u32x4 lrelu8(u32x4 u, float s) {
  uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float lo = __uint_as_float(w[i] << 16), hi = __uint_as_float(w[i] & 0xffff0000u);
    w[i] = pk_bf16(lrelu_max(lo, s), lrelu_max(hi, s));
  }
  return u32x4{w[0], w[1], w[2], w[3]};
}

// packed-fp32 forms (v_pk_mul_f32 / v_pk_add_f32: two values per VALU instruction) for the
// epilogues, whose VALU work -- not the MFMAs -- bound the narrow MRF kernels (round-3 counters:
// 6-9 VALU instructions per MFMA in the k = 3 blocks)
typedef float f32x2v __attribute__((ext_vector_type(2)));

// bf16 pair of leaky-ReLU(a), leaky-ReLU(b): one packed multiply, two maxima, one packed convert
__device__ __forceinline__ uint32_t lrelu_pk(float a, float b, float s) {
  const f32x2v m = f32x2v{a, b} * s;
  return pk_bf16(__builtin_elementwise_maximum(a, m.x), __builtin_elementwise_maximum(b, m.y));
}

// lrelu8 with the packed multiply: 8 packed bf16 -> 8 packed bf16
__device__ __forceinline__ u32x4 lrelu8_pk(u32x4 u, float s) {
  uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = lrelu_pk(__uint_as_float(w[i] << 16), __uint_as_float(w[i] & 0xffff0000u), s);
  return u32x4{w[0], w[1], w[2], w[3]};
}

__device__ __forceinline__ void unpack8(u32x4 u, float (&f)[8]) {
  const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __uint_as_float(w[i] << 16);
    f[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}

// ---------------------------------------------------------------- the persistent kernels' tile walk
// Ragged batches: utterance b of the (B, T, C) tensors has R_b = clamp(lens[b] * scale, 0, T) valid rows; rows
// outside [0, R_b) read as zero and rows >= R_b are not written.  lens == nullptr: dense (R_b = T).
struct MrfLens {
  const int32_t* lens;  // [B] on the device
  int scale, B;
};
struct MrfTile { int b, t0, R; };  // utterance, first row of the tile, valid rows of the utterance

// tile -> (b, t0, R_b) of a kernel whose tiles are BT rows.  Dense: b = tile / tiles_per_b.  RAG: the tiles past an
// utterance's end do not exist -- utterance b owns ceil((R_b + EX) / BT) consecutive tile ids (none when R_b = 0;
// EX = rows a kernel computes past R_b: the upsamplers' last phase row), total() of them in the launch, so a
// workgroup's share of total() is all work.  The prefix sums are never stored: a kernel walks its tile ids upwards,
// so at() keeps a cursor (utterance, its first tile id, its tile count) and steps it forward, a scalar load of
// lens[b] per utterance passed; total() and the first at() cost one pass over lens each (B scalar loads).
// at() wants non-decreasing tile ids below total().  No LDS, no scratch buffer, nothing on the host.
template <bool RAG, int EX = 0>
struct MrfWalk {
  int tiles_per_b, ntiles, T, BT;
  MrfLens rg;
  int cb, cbase, cn, cR;
  __device__ __forceinline__ MrfWalk(int tiles_per_b_, int ntiles_, int T_, int BT_, const MrfLens& rg_)
      : tiles_per_b(tiles_per_b_), ntiles(ntiles_), T(T_), BT(BT_), rg(rg_), cb(0), cbase(0), cn(0), cR(0) {
    if constexpr (RAG) {
      cR = rag_rows(rg.lens, rg.scale, 0, T);
      cn = count(cR);
    }
  }
  __device__ __forceinline__ int count(int R) const { return R > 0 ? (R + EX + BT - 1) / BT : 0; }
  __device__ __forceinline__ int total() const {
    if constexpr (!RAG) return ntiles;
    int n = 0;
    for (int b = 0; b < rg.B; ++b) n += count(rag_rows(rg.lens, rg.scale, b, T));
    return n;
  }
  __device__ __forceinline__ MrfTile at(int tile) {
    if constexpr (!RAG) {
      const int b = tile / tiles_per_b;
      return MrfTile{b, (tile - b * tiles_per_b) * BT, T};
    } else {
      while (tile >= cbase + cn && cb + 1 < rg.B) {
        cbase += cn;
        ++cb;
        cR = rag_rows(rg.lens, rg.scale, cb, T);
        cn = count(cR);
      }
      return MrfTile{cb, (tile - cbase) * BT, cR};
    }
  }
};

// A workgroup's tile run: its contiguous share [tile, tile_end) of the walk's total() tiles (all work: see MrfWalk),
// for the kernels that stage the next tile's window while they compute the current one.
//   MrfRun<RAG, BT> run(a.tiles_per_b, a.ntiles, T, a.rg);
//   if (run.empty()) return;  // uniform per workgroup: the early exit is safe
//   run.start();              // ... run.at(run.tile): stage the first window ...
//   for (; run.more(); run.advance()) {
//     const MrfTile ti = run.enter();  // this tile; run.at(run.succ()): its successor, whose window is prefetched
//   }                                  // (the last tile's is itself: the prefetch loads unconditionally)
// RAG: the walk's cursor only moves forward, so the run keeps one tile (nx) and at() answers with it whatever it is
// asked: the first tile after start(), each tile's successor after enter().
// The constructor's arguments are bound by reference and the dense tiles are computed from the kernel argument
// tiles_per_b itself (tpb): with copies the same code came out in another order, and the plane kernels, at 496-510
// of 512 registers, gained registers and instructions.
template <bool RAG, int BT>
struct MrfRun {
  MrfWalk<RAG> walk;
  int tile, tile_end;
  MrfTile nx;
  const int& tpb;
  __device__ __forceinline__ MrfRun(const int& tiles_per_b, const int& ntiles, const int& T, const MrfLens& rg)
      : walk(tiles_per_b, ntiles, T, BT, rg), tpb(tiles_per_b) {
    const int ntl = RAG ? walk.total() : ntiles;
    const int G = gridDim.x;
    tile = (int)(((int64_t)blockIdx.x * ntl) / G);
    tile_end = (int)(((int64_t)(blockIdx.x + 1) * ntl) / G);
  }
  __device__ __forceinline__ bool empty() const { return tile >= tile_end; }
  __device__ __forceinline__ void start() { if constexpr (RAG) nx = walk.at(tile); }
  __device__ __forceinline__ bool more() const { return tile < tile_end; }
  __device__ __forceinline__ void advance() { ++tile; }
  __device__ __forceinline__ int succ() const { return tile + 1 < tile_end ? tile + 1 : tile; }
  __device__ __forceinline__ MrfTile dense(int tl) const { const int b = tl / tpb; return MrfTile{b, (tl - b * tpb) * BT, walk.T}; }
  __device__ __forceinline__ MrfTile at(int tl) { if constexpr (RAG) return nx; else return dense(tl); }
  __device__ __forceinline__ MrfTile enter() {
    const MrfTile ti = RAG ? nx : dense(tile);
    if constexpr (RAG) nx = walk.at(succ());
    return ti;
  }
};

// ---------------------------------------------------------------- host side: launch and dispatch
// Every MRF kernel is persistent: a workgroup walks its share of `work` items (tiles, or groups of NWV tiles in
// the kernels whose waves take a tile each).  The grid is min(CUs * per_cu, work) with per_cu = 1, or, with
// `by_occupancy`, the resident workgroups per CU the runtime reports for (threads, lds).
template <class Args>
static int mrf_launch(void (*kern)(Args), const Args& a, int64_t work, int threads, size_t lds, bool by_occupancy,
                      hipStream_t st) {
  int per_cu = 1;
  if (by_occupancy &&
      (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, threads, lds) != hipSuccess || per_cu < 1))
    per_cu = 1;
  const int grid = (int)std::min<int64_t>((int64_t)cu_count() * per_cu, work);
  hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(threads), lds, st, a);
  VO_RETURN_LAUNCH();
}

// How the plane kernels add the MRF accumulator: 0 = none; 2 = acc_in / out_scale through an identity MFMA, when
// 1 / out_scale is a bf16 value (the MRF's 1/3 -> 3); 1 = added in the epilogue
inline int mrf_acc_mode(const void* acc, float out_scale) {
  if (!acc) return 0;
  const float inv = 1.0f / out_scale;
  const float invb = __bfloat162float(__float2bfloat16(inv));
  return (invb == inv && std::isfinite(inv) && inv * out_scale == 1.0f) ? 2 : 1;
}

// Where a launch function sends its kernel: a stream -- or, for the host-only tile-rows queries
// (vo_resblock_pair_tile_rows, vo_resblock3_tile_rows, vo_resblockk_tile_rows), nowhere: with `rows` set, the launch function the dispatch
// reaches writes its output rows per tile there and returns before any HIP call (mrf_tile_rows_query).  The queries
// run the entries' own dispatch this way, so what they report is the constant the launch computes its grid from.
struct MrfTo {
  hipStream_t st;
  int* rows;
  MrfTo(hipStream_t s = nullptr, int* r = nullptr) : st(s), rows(r) {}
  operator hipStream_t() const { return st; }
};
// first statement of a launch function once it knows its tile: true = a query, answered
inline bool mrf_tile_rows_query(const MrfTo& to, int rows) {
  if (to.rows) *to.rows = rows;
  return to.rows != nullptr;
}

// One vo_resblock_pair / vo_resblock3 / vo_resblockk call, as the entry points hand it to the kernels' vo_*_try functions
struct MrfPairCall {
  const void* x; const void* w1; const float* b1; const void* w2; const float* b2;
  void* y; const void* acc;
  int B, T, C, K, dil;
  float slope, out_scale;
  MrfTo st;
  const int32_t* lens; int lens_scale;  // ragged batch (vo_*_lens entries); nullptr: dense
};
struct MrfBlockCall {  // a whole block of three (c1, c2) stages: vo_resblock3 (K = 3), vo_resblockk (K = 7 / 11)
  const void* x; const void* const* w1; const float* const* b1; const void* const* w2; const float* const* b2;
  const int* dil;
  void* y; const void* acc;
  int B, T, C, K;
  float slope, out_scale;
  MrfTo st;
  const int32_t* lens; int lens_scale;
};

// the fields every pair kernel's argument struct has, from the call
template <class A>
static void mrf_pair_args(A& a, const MrfPairCall& c) {
  a.x = (const bf16_t*)c.x; a.w1 = (const bf16_t*)c.w1; a.b1 = c.b1; a.w2 = (const bf16_t*)c.w2; a.b2 = c.b2;
  a.y = (bf16_t*)c.y; a.acc = (const bf16_t*)c.acc;
  a.T = c.T; a.dil = c.dil; a.slope = c.slope; a.out_scale = c.out_scale;
  a.tiles_per_b = a.ntiles = 0;
}
// the fields every plane block kernel's argument struct has (conv v = 2 s + ph: c1 / c2 of stage s), from the call
template <class A>
static void mrf_block_args(A& a, const MrfBlockCall& c) {
  a.x = (const bf16_t*)c.x;
  for (int s = 0; s < 3; ++s) {
    a.w[2 * s] = (const bf16_t*)c.w1[s]; a.b[2 * s] = c.b1[s];
    a.w[2 * s + 1] = (const bf16_t*)c.w2[s]; a.b[2 * s + 1] = c.b2[s];
  }
  a.y = (bf16_t*)c.y; a.acc = (const bf16_t*)c.acc;
  a.T = c.T; a.slope = c.slope; a.out_scale = c.out_scale;
  a.tiles_per_b = a.ntiles = 0;
  a.rg = MrfLens{c.lens, c.lens_scale, c.B};
}

// f(std::integral_constant<int, ACC>) for the call's accumulator mode (mrf_acc_mode): the kernels take it as a
// template argument
template <class F>
static int mrf_with_acc(int accm, F f) {
  if (accm == 2) return f(std::integral_constant<int, 2>{});
  if (accm == 1) return f(std::integral_constant<int, 1>{});
  return f(std::integral_constant<int, 0>{});
}

}  // namespace vo

// The argument checks of vo_resblock_pair and (frag) vo_resblock_pair_frag (resblock.hip); the error names the entry
int vo_pair_check(const vo::MrfPairCall& c, bool frag);
// vo_resblock_pair_frag's check and dispatch (resblock_rw.hip)
int vo_pair_frag_entry(const vo::MrfPairCall& c);
// The argument checks vo_resblock3 and vo_resblockk share (resblock3.hip); the error names the entry
int vo_block_check(const vo::MrfBlockCall& c, const char* entry);

// The kernels behind vo_resblock_pair / vo_resblock3: each launches and sets *handled = 1 when it covers the shape
// (and the knob value `cfg`), else leaves *handled = 0 for the next one.
int vo_pair_rw_try(const vo::MrfPairCall& c, int cfg, int frag, int* handled);  // resblock_rw.hip
int vo_rb3_pb_try(const vo::MrfBlockCall& c, int* handled);                      // resblock_pb3.hip
int vo_rb3_rr_try(const vo::MrfBlockCall& c, int cfg, int* handled);             // resblock_rr.hip
int vo_rbk_pb_try(const vo::MrfBlockCall& c, int* handled);                      // resblock_pbk.hip (vo_resblockk)
