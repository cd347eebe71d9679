// Channels-last implicit-GEMM Conv1d on gfx950 MFMA.
//
// GEMM view of one launch:  C[co][pos] = sum_{tap k, ci} W[k][co][ci] * X[pos + k*dil - pad][ci]
//   M = output channels (A operand = packed weights, rows read from LDS),
//   N = output positions of one batch element (B operand = the input window in LDS),
//   reduction = (input-channel chunk of 32) x (tap).
// One workgroup owns a BCO x BT output tile.  For every 32-channel chunk it stages the
// input WINDOW (BT + (K-1)*dil rows) once and reuses it for all K taps by shifting the
// row index -- a dilated conv costs no extra HBM/L2 traffic over a 1x1 conv.  The weight
// tile of the next (chunk, tap) step and the next chunk's window are fetched into
// registers before the current step's MFMAs and written to the other LDS buffer after
// them (issue-early / write-late), so there is one barrier per step.
//
// Accumulator -> output mapping: MFMA row m of co-tile i is channel NI*4*(m>>2) + 4*i +
// (m&3), so lane (g = lane>>4, n = lane&15) ends up holding 4*NI CONTIGUOUS channels of
// ONE position -> vector stores of whole channel runs (channels-last).
//
// The lrelu/relu prologue is applied while staging (replaces F.leaky_relu before every
// HiFi-GAN conv), and the epilogue fuses bias, post-activation (relu/tanh), residual add,
// scale and MRF accumulate (y = (post(acc + b) + res1) * scale + res2).
//
// References: PositionwiseFeedForward (scripts/transformer/SubLayers.py:85-93), PostNet
// (scripts/transformer/Layers.py:129-137), VariancePredictor.Conv (scripts/model/
// modules.py:216-259), ResBlock (scripts/hifigan/models.py:96-103), Generator conv_pre /
// ups (models.py:149-160).

#include <string.h>

#include <algorithm>
#include <type_traits>

#include "vo_common.h"

namespace vo {

constexpr int KC = 32;        // reduction chunk = one bf16 MFMA k-depth
constexpr int HALO_MAX = 64;  // (K-1)*dil supported by the register staging arrays

struct ConvArgs {
  const void* x; int64_t xbs; int ldx;
  const void* w; const float* bias;
  void* y; int64_t ybs; int ldy;
  const void* res1; const void* res2;
  int T_in, T_out, Ci, Co, K, dil, pad;
  int pre_act; float pre_slope; int post_act; float post_slope; float out_scale;
  int transposed, up_stride, up_pad, up_cout, up_tout;
  int tiles_per_b, co_tiles, B;
  int cig, cog;  // channels per group (in / out): grouped conv = block-diagonal packed weights
  float* partial;  // split reduction: fp32 partials [splits][B][T_out][Co] (null = off)
  int kcs;         // 32-channel chunks per split (grid z = split)
  const void* ymask;  // outputs stored as round(round(v) * (ymask > 0 ? 1 : ymask_slope)) (y's layout)
  float ymask_slope;
  const int32_t* lens;  // ragged batch (vonoma.h): utterance b has clamp(lens[b] * lens_scale, 0, T_in) input rows
  int lens_scale;
};

template <typename T> struct Raw8;  // 8 elements of T held in registers
template <> struct Raw8<bf16_t> {
  uint4 u;
  __device__ __forceinline__ void load(const bf16_t* p) { u = *reinterpret_cast<const uint4*>(p); }
  __device__ __forceinline__ void zero() { u = make_uint4(0, 0, 0, 0); }
  __device__ __forceinline__ void to_f32(float (&v)[8]) const {
    uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[2 * i] = __uint_as_float(w[i] << 16);
      v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
    }
  }
};
template <> struct Raw8<float> {
  float4 a, b;
  __device__ __forceinline__ void load(const float* p) {
    a = *reinterpret_cast<const float4*>(p);
    b = *reinterpret_cast<const float4*>(p + 4);
  }
  __device__ __forceinline__ void zero() { a = b = make_float4(0.f, 0.f, 0.f, 0.f); }
  __device__ __forceinline__ void to_f32(float (&v)[8]) const {
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  }
};

// VO_F32X3: the packed weights are fp32 ([K][Co][Ci], the VO_F32 packing), staged as fp32 and split
// into hi / lo bf16 on their way into LDS (store8 / lds_put below)
template <> struct Raw8<bx3_t> : Raw8<float> {
  __device__ __forceinline__ void load(const bx3_t* p) { Raw8<float>::load(reinterpret_cast<const float*>(p)); }
};

// ---------------------------------------------------------------- LDS tile layout
// bf16: 32 elements (64 B) per row; 16-byte chunk q of row r lives at chunk
//   q ^ ((r >> (SH - 1)) & 2).  With SH = 2 the B-fragment reads (16 consecutive rows from
//   ANY starting row -- taps shift the window by k*dil -- x 4 chunks) are free of
//   ds_read_b128 bank conflicts; with SH = log2(4*NI) so are the A-fragment reads of the
//   weight rows NI*4*(m>>2) + 4*i + (m&3) (checked exhaustively against the gfx950 lane
//   groups; the first version's unswizzled 80-byte pitch was 2-way (B) / 4-way (A)).
//   Adding 16*j rows never changes the swizzle bit, so one offset serves all NJ tiles.
// f32 (parity mode): 40-float padded rows, no swizzle.
template <typename TC> struct Lds;
template <> struct Lds<bf16_t> {
  static constexpr int PITCH = 32;
  template <int SH> __device__ static __forceinline__ int off(int r, int q) {
    return r * 32 + 8 * (q ^ ((r >> (SH - 1)) & 2));
  }
};
template <> struct Lds<float> {
  static constexpr int PITCH = 40;
  template <int SH> __device__ static __forceinline__ int off(int r, int q) { return r * 40 + 8 * q; }
};
// split-bf16 (VO_F32X3): the fp32 tile's geometry, each 32-byte vector slot holding [hi x 8 | lo x 8]
template <> struct Lds<bx3_t> {
  static constexpr int PITCH = 40;
  template <int SH> __device__ static __forceinline__ int off(int r, int q) { return r * 40 + 8 * q; }
};

__device__ __forceinline__ void lds_put(bf16_t* p, const Raw8<bf16_t>& v) { *reinterpret_cast<uint4*>(p) = v.u; }
__device__ __forceinline__ void lds_put(float* p, const Raw8<float>& v) {
  *reinterpret_cast<float4*>(p) = v.a;
  *reinterpret_cast<float4*>(p + 4) = v.b;
}
__device__ __forceinline__ void lds_put(bx3_t* p, const Raw8<bx3_t>& v) {
  float f[8];
  v.to_f32(f);
  store8(p, f);
}

constexpr int ilog2(int v) { return v <= 1 ? 0 : 1 + ilog2(v / 2); }

// vo_conv1d_last_launch: the tile of this thread's last vo_conv1d call (zeroed at its entry, filled
// from its plan before the launch; host stores only)
static thread_local int32_t g_last_launch[VO_CONV1D_LAUNCH_FIELDS] = {};

// epilogue: lane (g = lane>>4, lr = lane&15) holds channels [n0, n0 + 4*NI) of position
// pos for each of its NJ position tiles
// bf16 output, plain conv, whole 8-channel runs (vec_ok: ldy / y_bstride multiples of 8):
// every residual / accumulator row of JG positions is requested before any is used (one memory
// round trip per JG positions instead of one per position: the scalar form waited for each row's
// load before its store, 8 times per 128-row wave tile), 16-byte loads and stores; the same
// arithmetic in the same order as the scalar form (bit-identical)
template <int NI, int NJ, int EJ = 2>
__device__ __forceinline__ void conv_epilogue_vec(const ConvArgs& a, f32x4 (&acc)[NI][NJ], int b, int t0, int n0,
                                                  int wave_t0, int lr) {
  static_assert(NI % 2 == 0, "8-channel runs");
  constexpr int NH = NI / 2;
  constexpr int JG = NJ < EJ ? NJ : EJ;  // position tiles whose rows are requested together
  bf16_t* Y = reinterpret_cast<bf16_t*>(a.y) + (int64_t)b * a.ybs;
  const bf16_t* R1 = reinterpret_cast<const bf16_t*>(a.res1 ? a.res1 : a.y) + (int64_t)b * a.ybs;
  const bf16_t* R2 = reinterpret_cast<const bf16_t*>(a.res2 ? a.res2 : a.y) + (int64_t)b * a.ybs;
  const bool r1 = a.res1 != nullptr, r2 = a.res2 != nullptr, om = a.ymask != nullptr;
  const bf16_t* YM = reinterpret_cast<const bf16_t*>(om ? a.ymask : a.y) + (int64_t)b * a.ybs;
  float bias[4 * NI];
#pragma unroll
  for (int e = 0; e < 4 * NI; ++e) bias[e] = a.bias ? a.bias[n0 + e] : 0.f;
  const float ps = a.post_act == VO_ACT_RELU ? 0.f : (a.post_act == VO_ACT_LRELU ? a.post_slope : 1.f);
  const bool tanh_act = a.post_act == VO_ACT_TANH;
#pragma unroll
  for (int j0 = 0; j0 < NJ; j0 += JG) {
    uint4 rv1[JG][NH], rv2[JG][NH], rvm[JG][NH];
#pragma unroll
    for (int jj = 0; jj < JG; ++jj) {  // rows past T_out re-read the last row (not stored)
      const int pos = min(t0 + wave_t0 + 16 * (j0 + jj) + lr, a.T_out - 1);
      const int64_t off = (int64_t)pos * a.ldy + n0;
#pragma unroll
      for (int h = 0; h < NH; ++h) {
        if (r1) rv1[jj][h] = *reinterpret_cast<const uint4*>(R1 + off + 8 * h);
        if (r2) rv2[jj][h] = *reinterpret_cast<const uint4*>(R2 + off + 8 * h);
        if (om) rvm[jj][h] = *reinterpret_cast<const uint4*>(YM + off + 8 * h);
      }
    }
#pragma unroll
    for (int jj = 0; jj < JG; ++jj) {
      const int j = j0 + jj;
      const int pos = t0 + wave_t0 + 16 * j + lr;
      const int64_t off = (int64_t)min(pos, a.T_out - 1) * a.ldy + n0;
#pragma unroll
      for (int h = 0; h < NH; ++h) {
        float q[8], x1[8], x2[8];
        if (r1) {
          const uint32_t w[4] = {rv1[jj][h].x, rv1[jj][h].y, rv1[jj][h].z, rv1[jj][h].w};
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            x1[2 * u] = __uint_as_float(w[u] << 16);
            x1[2 * u + 1] = __uint_as_float(w[u] & 0xffff0000u);
          }
        }
        if (r2) {
          const uint32_t w[4] = {rv2[jj][h].x, rv2[jj][h].y, rv2[jj][h].z, rv2[jj][h].w};
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            x2[2 * u] = __uint_as_float(w[u] << 16);
            x2[2 * u + 1] = __uint_as_float(w[u] & 0xffff0000u);
          }
        }
        float av[8], bv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          av[e] = acc[2 * h + e / 4][j][e & 3];
          bv[e] = bias[8 * h + e];
        }
        conv_epilogue8(av, bv, tanh_act, ps, r1, x1, a.out_scale, r2, x2, q);
        if (om) {  // the leaky-ReLU backward of the layer whose output ymask is, on the stored value
          const uint32_t w[4] = {rvm[jj][h].x, rvm[jj][h].y, rvm[jj][h].z, rvm[jj][h].w};
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float m = __uint_as_float((e & 1) ? (w[e >> 1] & 0xffff0000u) : (w[e >> 1] << 16));
            const float r = to_f32(from_f32<bf16_t>(q[e]));
            q[e] = m > 0.f ? r : r * a.ymask_slope;
          }
        }
        if (pos < a.T_out) store8(Y + off + 8 * h, q);
      }
    }
  }
}

template <typename TOUT, int NI, int NJ, int EJ = 2>
__device__ __forceinline__ void conv_epilogue(const ConvArgs& a, f32x4 (&acc)[NI][NJ], int b, int t0, int co_blk,
                                              int wave_co0, int wave_t0, int lane) {
  const int lr = lane & 15;
  const int g = lane >> 4;
  const int n0 = co_blk + wave_co0 + NI * 4 * g;
  if (n0 >= a.Co) return;
  if constexpr (std::is_same<TOUT, bf16_t>::value && NI % 2 == 0) {
    // uniform per launch: plain conv, 8-element aligned rows, the lane's whole run inside Co
    if (!a.transposed && (a.ldy & 7) == 0 && (a.ybs & 7) == 0 && a.Co % (4 * NI) == 0) {
      conv_epilogue_vec<NI, NJ, EJ>(a, acc, b, t0, n0, wave_t0, lr);
      return;
    }
  }
  TOUT* Y = reinterpret_cast<TOUT*>(a.y) + (int64_t)b * a.ybs;
  const TOUT* R1 = a.res1 ? reinterpret_cast<const TOUT*>(a.res1) + (int64_t)b * a.ybs : nullptr;
  const TOUT* R2 = a.res2 ? reinterpret_cast<const TOUT*>(a.res2) + (int64_t)b * a.ybs : nullptr;

  int col = n0, trow_shift = 0;
  if (a.transposed) {
    const int phase = n0 / a.up_cout;
    col = n0 - phase * a.up_cout;
    trow_shift = phase - a.up_pad;
  }
  // Co % (4 * NI) != 0: the run of the lane that crosses the end is clamped into the bias (those channels are
  // not stored); unclamped, it read up to 4 * NI - 4 floats past a bias of Co floats
  const int bmax = (a.transposed ? a.up_cout : a.Co) - 1;
  float bias[4 * NI];
#pragma unroll
  for (int e = 0; e < 4 * NI; ++e) bias[e] = a.bias ? a.bias[min((a.transposed ? col : n0) + e, bmax)] : 0.f;

#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int pos = t0 + wave_t0 + 16 * j + lr;
    if (pos >= a.T_out) continue;
    int trow = pos;
    if (a.transposed) {
      trow = pos * a.up_stride + trow_shift;
      if (trow < 0 || trow >= a.up_tout) continue;
    }
    const int64_t off = (int64_t)trow * a.ldy + col;
    float v[4 * NI];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) v[4 * i + r] = acc[i][j][r] + bias[4 * i + r];
    if (a.post_act == VO_ACT_TANH) {
#pragma unroll
      for (int e = 0; e < 4 * NI; ++e) v[e] = tanhf(v[e]);
    } else {
      const float ps = a.post_act == VO_ACT_RELU ? 0.f : (a.post_act == VO_ACT_LRELU ? a.post_slope : 1.f);
#pragma unroll
      for (int e = 0; e < 4 * NI; ++e) v[e] = lrelu_max(v[e], ps);  // ps in [0, 1]
    }
#pragma unroll
    for (int h = 0; h < NI; ++h) {
      if (n0 + 4 * h >= a.Co) break;  // Co % (4 * NI) != 0: the lane's run crosses the end
      float q[4] = {v[4 * h], v[4 * h + 1], v[4 * h + 2], v[4 * h + 3]};
      if (R1) {
        float rr[4];
        load4(R1 + off + 4 * h, rr);
#pragma unroll
        for (int e = 0; e < 4; ++e) q[e] += rr[e];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) q[e] *= a.out_scale;
      if (R2) {
        float rr[4];
        load4(R2 + off + 4 * h, rr);
#pragma unroll
        for (int e = 0; e < 4; ++e) q[e] += rr[e];
      }
      if (a.ymask) {
        float mm[4];
        load4(reinterpret_cast<const TOUT*>(a.ymask) + (int64_t)b * a.ybs + off + 4 * h, mm);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float r = to_f32(from_f32<TOUT>(q[e]));
          q[e] = mm[e] > 0.f ? r : r * a.ymask_slope;
        }
      }
      store4(Y + off + 4 * h, q);
    }
  }
}

// split reduction, first pass: raw fp32 accumulators of this split's chunks (lane layout of
// conv_epilogue: channels [n0, n0 + 4 NI) of each of its NJ positions)
template <int NI, int NJ>
__device__ __forceinline__ void conv_partial_store(const ConvArgs& a, f32x4 (&acc)[NI][NJ], int b, int t0,
                                                   int co_blk, int wave_co0, int wave_t0, int lane) {
  const int lr = lane & 15;
  const int n0 = co_blk + wave_co0 + NI * 4 * (lane >> 4);
  if (n0 >= a.Co) return;
  float* P = a.partial + ((int64_t)blockIdx.z * a.B + b) * (int64_t)a.T_out * a.Co;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int pos = t0 + wave_t0 + 16 * j + lr;
    if (pos >= a.T_out) continue;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      if (n0 + 4 * i >= a.Co) break;
      *reinterpret_cast<float4*>(P + (int64_t)pos * a.Co + n0 + 4 * i) =
          make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
    }
  }
}

// ROLE only names the instantiation (0 = generic, 1..4 = HiFi-GAN MRF stage 0..3), so a
// profiler attributes the vocoder's stages to distinct kernels; the code is identical.
// TPS = taps per pipeline step: the weight tiles of TPS taps are staged together so one
// barrier covers TPS x NI x NJ MFMAs per wave.  NICE = (Ci % 32 == 0 && Co % BCO == 0):
// no channel bounds checks in the staging loops.
// Instruction budget: every staging / fragment address is precomputed once per thread;
// the loop body is LDS reads + MFMAs + a few global loads / LDS stores per step (the
// first version spent ~15 VALU+SALU instructions per MFMA on address math).
// PRIO: s_setprio(1) around each MFMA cluster (keeps hipcc from moving the cluster across
// the barriers; guide T5): the MRF stage-0 tiles.
// GL (bf16, NICE, stride 1): the weight taps are copied HBM / L2 -> LDS by LDS-DMA
// (global_load_lds_dwordx4, 1 KiB per wave instruction, the XOR swizzle moved to the source
// address as in the fused ResBlock kernels): no staging VGPRs and no ds_write for them.  The
// next chunk's window is then fetched after the first step's DMA (so a step's vmcnt wait does not
// drain it), which leaves it two steps instead of a whole chunk to arrive.
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N <= 8, "wait_vmcnt: 0..8");
  if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if constexpr (N == 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
  if constexpr (N == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
  if constexpr (N == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
  if constexpr (N == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  if constexpr (N == 5) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
  if constexpr (N == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  if constexpr (N == 7) asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
  if constexpr (N == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
}

// RS (with GL): the waves split the staging by role -- the first half issue every weight DMA piece,
// the second half load and store every window chunk.  vmcnt is per wave and retires in issue order,
// so a wave that waits for its weight DMA each step no longer drains the next chunk's window loads
// (issued one chunk ahead, they got one step to land); and the step barriers are bare s_barrier
// (LDS writes drained by lgkmcnt): __syncthreads' workgroup release fence waits vmcnt(0) too.
// SEG (4-byte TC, stride 1, T_out <= 16): utterance-segment tiles -- each 16-row position tile j of a
// wave is one whole utterance (b0 + its index), staged as its own window of 16 + (K-1) dil rows (rows
// outside [0, T_in) zeroed), so the BT / 16 utterances of a workgroup share every staged weight tap.
// The short-sequence convs (glyph encoder, variance predictors: T ~ 12) otherwise ran one utterance
// per workgroup and re-read the whole weight once per utterance (FFN w_1 at B = 32: 302 MB of L2
// reads for 9.4 MB of weights).  Halo <= SEG_HALO.
constexpr int SEG_HALO = 8;
template <typename TIN, typename TC, typename TOUT, int NI, int NJ, int WCO, int WT, int TPS, bool NICE, int ROLE,
          int PRIO = 0, int S = 1, bool GL = false, bool RS = false, int EJ = 2, bool SEG = false,
          bool RAG = false>
__global__ void __launch_bounds__(WCO * WT * 64)
conv1d_kernel(ConvArgs a) {
  static_assert(!RAG || (!SEG && S == 1), "conv1d RAG: whole-utterance tiles, stride 1");
  static_assert(!SEG || (sizeof(TC) == 4 && S == 1 && !GL), "conv1d SEG: 4-byte compute, stride 1");
  constexpr int NT = WCO * WT * 64;
  constexpr int BCO = 16 * NI * WCO;
  constexpr int BT = 16 * NJ * WT;
  constexpr int P = Lds<TC>::PITCH;
  constexpr int VPR = KC / 8;                 // 8-element vectors per row (4)
  constexpr bool DMA = GL && NICE && S == 1 && sizeof(TC) == 2 && sizeof(TIN) == 2;
  constexpr bool SPLIT = RS && DMA && (NT / 64) % 2 == 0;
  constexpr int MAXV = SPLIT ? 1 : SEG ? ((BT / 16) * (16 + SEG_HALO) * VPR + NT - 1) / NT
                                      : (((BT - 1) * S + 1 + HALO_MAX) * VPR + NT - 1) / NT;
  // SPLIT: the window waves copy each chunk's window by LDS-DMA (XPW 1-KiB pieces per wave,
  // lane-linear) into a raw staging area; at the chunk's end each lane applies the prologue
  // activation to the 16 bytes it fetched and stores them into the swizzled window buffer
  constexpr int XPW = SPLIT ? (((BT - 1) * S + 1 + HALO_MAX) * VPR + 64 * (NT / 128) - 1) / (64 * (NT / 128)) : 1;
  constexpr int WV = (TPS * BCO * VPR + NT - 1) / NT;
  constexpr int SHW = ilog2(4 * NI);

  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  TC* smem = reinterpret_cast<TC*>(smem_raw);

  const int seg_rows = 16 + (a.K - 1) * a.dil;  // SEG: window rows per utterance
  const int win_rows = SEG ? (BT / 16) * seg_rows : (BT - 1) * S + 1 + (a.K - 1) * a.dil;  // S: conv stride
  TC* const win0 = smem;
  TC* const wt0 = smem + 2 * win_rows * P;
  const int win_stride = win_rows * P;      // elements between the two window buffers
  constexpr int WSTRIDE = TPS * BCO * P;    // elements between the two weight buffers
  TC* const dummy = wt0 + 2 * WSTRIDE;      // one row that absorbs the stores of idle staging slots

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wave_co0 = (wave % WCO) * 16 * NI;
  const int wave_t0 = (wave / WCO) * 16 * NJ;

  const int b = SEG ? blockIdx.x * (BT / 16) : blockIdx.x / a.tiles_per_b;  // SEG: the tile's first utterance
  const int t0 = SEG ? 0 : (blockIdx.x - b * a.tiles_per_b) * BT;
  const int co_blk = blockIdx.y * BCO;
  if constexpr (RAG) {
    // ragged batch (a.lens; never SEG / strided / split: vo_conv1d rejects those): utterance b is a tensor of R rows -- its
    // bounds replace the batch's in this workgroup's copy of the arguments (the batch strides stay), and a tile that
    // starts past its output rows has nothing to do.  Polyphase form: R + 1 phase rows, (R + 1) s - 2 p output rows.
    const int R = rag_rows(a.lens, a.lens_scale, b, a.T_in);
    const int rows = a.transposed ? R + 1 : R;
    if (R == 0 || t0 >= rows) return;
    a.T_in = R;
    a.T_out = rows;
    a.up_tout = min(a.up_tout, (R + 1) * a.up_stride - 2 * a.up_pad);
  }

  const TIN* __restrict__ X = reinterpret_cast<const TIN*>(a.x) + (int64_t)b * a.xbs;
  const TC* __restrict__ Wp = reinterpret_cast<const TC*>(a.w);
  // grouped conv: this block's output channels [co_blk, co_blk + BCO) read only input
  // channels [ci_lo, ci_hi) of their groups (32-aligned; the packed weights are
  // block-diagonal, so the extra channels of a partial chunk multiply zeros)
  const int co_last = min(co_blk + BCO, a.Co) - 1;
  int ci_lo = (co_blk / a.cog) * a.cig / KC * KC;
  const int ci_hi = min(a.Ci, (co_last / a.cog + 1) * a.cig);
  int n_chunks = (ci_hi - ci_lo + KC - 1) / KC;
  if (a.partial) {  // split reduction: this workgroup's run of chunks
    const int z0 = blockIdx.z * a.kcs;
    ci_lo += z0 * KC;
    n_chunks = min(a.kcs, n_chunks - z0);
  }
  const int tsteps = (a.K + TPS - 1) / TPS;
  const bool raw_window = std::is_same<TIN, TC>::value && a.pre_act == VO_ACT_NONE;
  // prologue activation as one select: none -> slope 1, relu -> 0, lrelu -> slope
  const float pre_s = a.pre_act == VO_ACT_RELU ? 0.f : (a.pre_act == VO_ACT_LRELU ? a.pre_slope : 1.f);
  const int64_t tap_stride = (int64_t)a.Co * a.Ci;

  // ---- per-thread staging geometry, computed once
  // Every global load below is UNCONDITIONAL (addresses clamped into the tensor) and the
  // out-of-range vectors are zeroed when they are written to LDS: a load under a divergent
  // branch gets an immediate s_waitcnt vmcnt(0) from the compiler, which serialised the
  // prefetch against HBM latency (seen in the ISA of the first version).
  constexpr int MAXVA = MAXV;
  int xg[MAXVA], xl[MAXVA], xr[MAXVA], xc[MAXVA];  // xr: row-in-range flag
#pragma unroll
  for (int s = 0; s < MAXVA; ++s) {
    const int v = tid + s * NT;
    const int r = v / VPR, q = v % VPR;
    xc[s] = q * 8;
    if constexpr (SEG) {
      const int seg = r / seg_rows, row = r - seg * seg_rows - a.pad;
      xr[s] = r < win_rows && b + seg < a.B && row >= 0 && row < a.T_in;
      xg[s] = (int)(min(seg, a.B - 1 - b) * a.xbs) + min(max(row, 0), a.T_in - 1) * a.ldx + q * 8;
    } else {
      const int row = t0 * S - a.pad + r;
      xr[s] = r < win_rows && row >= 0 && row < a.T_in;  // row in range
      xg[s] = min(max(row, 0), a.T_in - 1) * a.ldx + q * 8;
    }
    xl[s] = r < win_rows ? Lds<TC>::template off<2>(r, q) : -1;
  }
  int wg[WV], wl[WV], wk[WV], wq[WV];
  bool wok[WV];
#pragma unroll
  for (int s = 0; s < WV; ++s) {
    const int v = tid + s * NT;
    const int r = v / VPR, q = v % VPR;   // r = tap_in_step * BCO + co_local
    const int t = r / BCO, col = r - t * BCO;
    wk[s] = t;
    wq[s] = q * 8;
    wok[s] = r < TPS * BCO && (NICE || co_blk + col < a.Co);
    wg[s] = min(co_blk + col, a.Co - 1) * a.Ci + q * 8;
    wl[s] = t * BCO * P + Lds<TC>::template off<SHW>(col, q);
  }

  Raw8<TIN> win_r[MAXV];
  // SEG: second register sets -- weights fetched two steps ahead, and (one-tap convs) windows two chunks ahead
  Raw8<TIN> win_r2[SEG ? MAXV : 1];
  bool win_ok2[SEG ? MAXV : 1];
  Raw8<TC> w_r2[SEG ? WV : 1];
  bool w_ok2[SEG ? WV : 1];
  constexpr int NW = NT / 64;
  constexpr int NWW = SPLIT ? NW / 2 : NW;  // waves issuing the weight DMA
  constexpr int GLN = DMA ? (TPS * BCO * VPR) / (64 * NWW) : 1;  // DMA instructions per wave per step
  static_assert(!DMA || (TPS * BCO * VPR) % (64 * NWW) == 0, "conv1d GL: a step's weights must split into whole wave-KiB");
  Raw8<TC> w_r[DMA ? 1 : WV];
  bool win_ok[MAXVA], w_ok[DMA ? 1 : WV];
  constexpr int GLNA = SPLIT ? 1 : GLN;
  int gl_t[GLNA], gl_src[GLNA];
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const int wave_w = wave_u % NWW;
  // wave roles (uniform): SPLIT -> waves [0, NW/2) weights, [NW/2, NW) window; else every wave both
  const bool wwave = !SPLIT || wave_u < NWW, xwave = !SPLIT || wave_u >= NWW;
  const int wave_x = wave_u - NWW;  // SPLIT: window wave index
  TC* const xraw = dummy + P;       // SPLIT: raw window pieces [NW - NWW][XPW][64 lanes][8]
  if constexpr (DMA && !SPLIT) {
#pragma unroll
    for (int s = 0; s < GLN; ++s) {
      const int p = (s * NWW + wave_w) * 64 + lane;  // LDS slot (16 B): tap t, row col, chunk q'
      const int t = p / (BCO * VPR), rem = p - t * BCO * VPR;
      const int col = rem / VPR, qs = rem - col * VPR;
      const int q = qs ^ ((col >> (SHW - 1)) & 2);  // the swizzle of Lds<bf16_t>::off, on the source
      gl_t[s] = t;
      gl_src[s] = (co_blk + col) * a.Ci + q * 8;
    }
  }
  auto load_w_dma = [&](int c, int k0, int buf) {
    if constexpr (DMA) {
      typedef __attribute__((address_space(3))) void lds_void;
      typedef const __attribute__((address_space(1))) void g_void;
      const int c0 = ci_lo + c * KC;
      if constexpr (SPLIT) {
        // piece s = tap s / PPT, rows (s % PPT) * CSTEP + (wave_w * 64 + lane) / VPR; its swizzle
        // bit does not depend on s, so one per-lane offset (opaque: not hoisted as GLN 64-bit
        // addresses, which spilled) plus a scalar offset per piece
        constexpr int PPT = BCO * VPR / (64 * NWW), CSTEP = 64 * NWW / VPR;
        static_assert(GLN % PPT == 0 && CSTEP % (1 << SHW) == 0, "conv1d RS: whole taps per step, swizzle kept");
        const int p0 = wave_w * 64 + lane, col0 = p0 / VPR;
        int lane_off = (co_blk + col0) * a.Ci + ((p0 % VPR) ^ ((col0 >> (SHW - 1)) & 2)) * 8;
        asm volatile("" : "+v"(lane_off));
#pragma unroll
        for (int s = 0; s < GLN; ++s) {
          const int k = min(k0 + s / PPT, a.K - 1);  // taps >= K are skipped by the MFMA loop
          const TC* src = Wp + (k * tap_stride + (s % PPT) * CSTEP * a.Ci + c0) + lane_off;
          TC* dst = wt0 + buf * WSTRIDE + (s * NWW + wave_w) * 64 * 8;
          __builtin_amdgcn_global_load_lds((g_void*)src, (lds_void*)dst, 16, 0, 0);
        }
        return;
      }
#pragma unroll
      for (int s = 0; s < GLN; ++s) {
        int gt, gsrc;
        {
          gt = gl_t[s];
          gsrc = gl_src[s];
        }
        const int k = min(k0 + gt, a.K - 1);  // taps >= K are skipped by the MFMA loop
        const TC* src = Wp + k * tap_stride + gsrc + c0;
        TC* dst = wt0 + buf * WSTRIDE + (s * NWW + wave_w) * 64 * 8;
        __builtin_amdgcn_global_load_lds((g_void*)src, (lds_void*)dst, 16, 0, 0);
      }
    }
  };

  // SPLIT: two raw areas -- chunk c + 2's window is fetched while chunk c computes and chunk c + 1's
  // lands; the pass at chunk c's end waits only for chunk c + 1 (vmcnt(XPW): the younger pieces of
  // chunk c + 2 stay in flight), so each window DMA has a whole chunk or more to land
  constexpr int XRAW = (NT / 128) * XPW * 64 * 8;  // elements per raw area
  static_assert(!SPLIT || XPW <= 8, "conv1d RS: wait_vmcnt<XPW>");
  auto load_window_to = [&](auto& wr, auto& wo, int c) {
    const int c0 = ci_lo + c * KC;
#pragma unroll
    for (int s = 0; s < MAXVA; ++s) {
      wo[s] = xr[s] && (NICE || c0 + xc[s] < a.Ci);
      wr[s].load(X + xg[s] + (NICE ? c0 : min(c0, a.Ci - 8 - xc[s])));
    }
  };
  auto load_window = [&](int c, int rb = 0) {
    const int c0 = ci_lo + c * KC;
    if constexpr (SPLIT) {  // NICE: no channel bounds; rows clamped (zeroed by the LDS pass)
      typedef __attribute__((address_space(3))) void lds_void;
      typedef const __attribute__((address_space(1))) void g_void;
      int lrow = lane / VPR;  // opaque per call (see load_w_dma)
      asm volatile("" : "+v"(lrow));
      const TIN* xq = X + (lane % VPR) * 8 + c0;
#pragma unroll
      for (int s = 0; s < XPW; ++s) {
        const int row = min(max(t0 * S - a.pad + (wave_x * XPW + s) * (64 / VPR) + lrow, 0), a.T_in - 1);
        __builtin_amdgcn_global_load_lds((g_void*)(xq + (int64_t)row * a.ldx),
                                         (lds_void*)(xraw + rb * XRAW + (wave_x * XPW + s) * 64 * 8), 16, 0, 0);
      }
      return;
    }
    load_window_to(win_r, win_ok, c);
  };
  auto store_window_from = [&](auto& wr, auto& wo, int buf) {
    TC* base = win0 + buf * win_stride;
#pragma unroll
    for (int s = 0; s < MAXV; ++s) {  // branch-free: idle slots store to the dummy row
      TC* dst;
      {
        dst = xl[s] >= 0 ? base + xl[s] : dummy;
        if (!wo[s]) wr[s].zero();
      }
      if constexpr (std::is_same<TIN, TC>::value) {
        if (raw_window) {
          lds_put(dst, wr[s]);
          continue;
        }
      }
      float f[8];
      wr[s].to_f32(f);
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = lrelu_max(f[e], pre_s);  // pre_s in [0, 1]
      store8(dst, f);
    }
  };
  auto store_window = [&](int buf, int rb = 0, bool young = false) {
    TC* base = win0 + buf * win_stride;
    if constexpr (SPLIT) {  // this wave's own DMA pieces (same lanes): no barrier needed first
      if (young)
        wait_vmcnt<XPW>();  // the next chunk's pieces (issued after these) may stay in flight
      else
        wait_vmcnt<0>();
#pragma unroll
      for (int s = 0; s < XPW; ++s) {
        const int v = (wave_x * XPW + s) * 64 + lane, r = v / VPR, row = t0 * S - a.pad + r;
        Raw8<TIN> u;
        u.load(reinterpret_cast<const TIN*>(xraw + rb * XRAW + v * 8));
        if (!(row >= 0 && row < a.T_in)) u.zero();
        float f[8];
        u.to_f32(f);
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = lrelu_max(f[e], pre_s);  // pre_s in [0, 1]
        store8(r < win_rows ? base + Lds<TC>::template off<2>(r, v % VPR) : dummy, f);
      }
      return;
    }
    store_window_from(win_r, win_ok, buf);
  };
  auto load_w_to = [&](auto& wr, auto& wo, int c, int k0) {
    if constexpr (DMA) return;
    const int c0 = ci_lo + c * KC;
#pragma unroll
    for (int s = 0; s < WV; ++s) {
      const int k = min(k0 + wk[s], a.K - 1);  // taps >= K are skipped by the MFMA loop
      wo[s] = wok[s] && (NICE || c0 + wq[s] < a.Ci);
      wr[s].load(Wp + k * tap_stride + wg[s] + (NICE ? c0 : min(c0, a.Ci - 8 - wq[s])));
    }
  };
  auto store_w_from = [&](auto& wr, auto& wo, int buf) {
    if constexpr (DMA) return;
    TC* base = wt0 + buf * WSTRIDE;
#pragma unroll
    for (int s = 0; s < WV; ++s) {
      if (!wo[s]) wr[s].zero();
      lds_put((tid + s * NT) / VPR < TPS * BCO ? base + wl[s] : dummy, wr[s]);
    }
  };
  auto load_w = [&](int c, int k0) { load_w_to(w_r, w_ok, c, k0); };
  auto store_w = [&](int buf) { store_w_from(w_r, w_ok, buf); };

  f32x4 acc[NI][NJ];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // fragment read offsets (elements)
  const int lr = lane & 15;
  const int lq = lane >> 4;
  int a_off[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i)
    a_off[i] = Lds<TC>::template off<SHW>(wave_co0 + NI * 4 * (lr >> 2) + 4 * i + (lr & 3), lq);
  const int brow0 = SEG ? (wave_t0 / 16) * seg_rows + lr : wave_t0 + lr;
  const int jst = SEG ? seg_rows * P : 16 * S * P;  // rows between position tiles j (SEG: one utterance window)

  // prologue
  if (xwave) load_window(0);
  load_w(0, 0);
  if (wwave) load_w_dma(0, 0, 0);
  if (xwave) store_window(0);
  store_w(0);
  if constexpr (DMA) wait_vmcnt<0>();
  __syncthreads();

  // One pipeline step = TPS taps of one 32-channel chunk c (weights in buffer s & 1).  The
  // next chunk's window is fetched when a chunk starts and written to LDS in its last step.
  // Loads are issued on every path (re-fetching the last chunk instead of branching): a
  // conditional load makes the compiler's wait counts conservative on every path.
  auto mfma_step = [&](int c, int tg, int s) {
    const TC* xb = win0 + (c & 1) * win_stride;
    const TC* wb = wt0 + (s & 1) * WSTRIDE;
    const int k0 = tg * TPS;
#pragma unroll
    for (int t = 0; t < TPS; ++t) {
      if (k0 + t < a.K) {
        Frag<TC> af[NI], bfr[NJ];
#pragma unroll
        for (int i = 0; i < NI; ++i) af[i].load(wb + t * BCO * P + a_off[i]);
        const int br = brow0 * S + (k0 + t) * a.dil;
        const int boff = Lds<TC>::template off<2>(br, lq);
#pragma unroll
        for (int j = 0; j < NJ; ++j) bfr[j].load(xb + boff + (SEG ? j * jst : 16 * S * j * P));  // +16S rows keeps the swizzle
        if constexpr (PRIO) __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
          for (int j = 0; j < NJ; ++j) acc[i][j] = mfma(af[i], bfr[j], acc[i][j]);
        if constexpr (PRIO) __builtin_amdgcn_s_setprio(0);
      }
    }
  };

  if constexpr (SEG) {
    // Short chains (9..72 steps of 2..8 MFMAs per wave): every step of the generic loop below waited a
    // whole load round trip (its weights are fetched at the step's start, and __syncthreads drains
    // vmcnt).  Here step q's weights are fetched two steps ahead (register sets A / B alternate),
    // written to LDS one step ahead, and the barriers are bare (lds_barrier): loads stay in flight
    // across them.  One-tap convs (a step per chunk) fetch windows two chunks ahead the same way.
    // Step q = chunk q / tsteps, tap group q % tsteps: the generic loop's order (bit-identical).
    const int nq = n_chunks * tsteps;
    auto wload = [&](auto& wr, auto& wo, int q) {
      q = min(q, nq - 1);  // clamped re-fetch past the end: loads stay unconditional
      const int c = q / tsteps;
      load_w_to(wr, wo, c, (q - c * tsteps) * TPS);
    };
    if (tsteps == 1) {
      load_window_to(win_r, win_ok, min(1, n_chunks - 1));
      wload(w_r, w_ok, 1);
      auto body1 = [&](int c, auto& cw, auto& cwo, auto& cx, auto& cxo, auto& nw, auto& nwo, auto& nx, auto& nxo) {
        load_window_to(nx, nxo, min(c + 2, n_chunks - 1));
        wload(nw, nwo, c + 2);
        mfma_step(c, 0, c);
        if (c + 1 < n_chunks) {
          store_window_from(cx, cxo, (c + 1) & 1);
          store_w_from(cw, cwo, (c + 1) & 1);
        }
        lds_barrier();
      };
      for (int c = 0; c < n_chunks; c += 2) {
        body1(c, w_r, w_ok, win_r, win_ok, w_r2, w_ok2, win_r2, win_ok2);
        if (c + 1 < n_chunks) body1(c + 1, w_r2, w_ok2, win_r2, win_ok2, w_r, w_ok, win_r, win_ok);
      }
    } else {
      wload(w_r, w_ok, 1);
      auto body = [&](int q, auto& cw, auto& cwo, auto& nw, auto& nwo) {
        const int c = q / tsteps, tg = q - c * tsteps;
        if (tg == 0) load_window(min(c + 1, n_chunks - 1));
        wload(nw, nwo, q + 2);
        mfma_step(c, tg, q);
        store_w_from(cw, cwo, (q + 1) & 1);  // past the last step: a buffer no step reads
        if (tg == tsteps - 1 && c + 1 < n_chunks) store_window((c + 1) & 1);
        lds_barrier();
      };
      for (int q = 0; q < nq; q += 2) {
        body(q, w_r, w_ok, w_r2, w_ok2);
        if (q + 1 < nq) body(q + 1, w_r2, w_ok2, w_r, w_ok);
      }
    }
    wait_vmcnt<0>();  // the clamped re-fetches land before the registers are reused by the epilogue
  }
  int s = 0;
  if constexpr (SPLIT) {
    for (int c = 0; c < n_chunks; ++c) {
      const bool more_chunks = c + 1 < n_chunks;
      if (xwave) {  // chunk c's raw area was consumed at chunk c - 1's end
        if (c == 0) load_window(min(1, n_chunks - 1), 1);
        load_window(min(c + 2, n_chunks - 1), c & 1);
      }
      for (int tg = 0; tg < tsteps - 1; ++tg, ++s) {
        if (wwave) load_w_dma(c, (tg + 1) * TPS, (s + 1) & 1);
        mfma_step(c, tg, s);
        if (wwave) wait_vmcnt<0>();  // this wave's DMA pieces landed
        lds_barrier();
      }
      if (wwave) load_w_dma(min(c + 1, n_chunks - 1), 0, (s + 1) & 1);
      mfma_step(c, tsteps - 1, s);
      if (xwave && more_chunks) store_window((c + 1) & 1, (c + 1) & 1, true);
      if (wwave) wait_vmcnt<0>();
      lds_barrier();
      ++s;
    }
    if (xwave) wait_vmcnt<0>();  // the clamped re-fetches of the last chunks land before the epilogue
  }
  for (int c = 0; c < (SPLIT || SEG ? 0 : n_chunks); ++c) {
    const bool more_chunks = c + 1 < n_chunks;
    if constexpr (!DMA) load_window(min(c + 1, n_chunks - 1));  // a whole chunk of MFMAs ahead of its use
    for (int tg = 0; tg < tsteps - 1; ++tg, ++s) {
      load_w(c, (tg + 1) * TPS);
      if constexpr (DMA) {
        load_w_dma(c, (tg + 1) * TPS, (s + 1) & 1);
        if (tg == 0) load_window(min(c + 1, n_chunks - 1));  // issued after the DMA: in-order vmcnt
      }
      mfma_step(c, tg, s);
      store_w((s + 1) & 1);
      if constexpr (DMA) {  // this wave's DMA pieces landed (the window loads after them may not)
        if (tg == 0)
          wait_vmcnt<MAXV>();
        else
          wait_vmcnt<0>();
      }
      __syncthreads();
    }
    load_w(min(c + 1, n_chunks - 1), 0);
    if constexpr (DMA) {
      load_w_dma(min(c + 1, n_chunks - 1), 0, (s + 1) & 1);
      if (tsteps == 1) load_window(min(c + 1, n_chunks - 1));
    }
    mfma_step(c, tsteps - 1, s);
    if (more_chunks) {
      store_w((s + 1) & 1);
      store_window((c + 1) & 1);
    }
    if constexpr (DMA) wait_vmcnt<0>();
    __syncthreads();
    ++s;
  }
  if constexpr (SEG) {  // position tile j = utterance b + wave_t0 / 16 + j, positions 0..15
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int bj = b + wave_t0 / 16 + j;
      if (bj >= a.B) continue;
      f32x4 a1[NI][1];
#pragma unroll
      for (int i = 0; i < NI; ++i) a1[i][0] = acc[i][j];
      if (a.partial)
        conv_partial_store<NI, 1>(a, a1, bj, 0, co_blk, wave_co0, 0, lane);
      else
        conv_epilogue<TOUT, NI, 1, EJ>(a, a1, bj, 0, co_blk, wave_co0, 0, lane);
    }
    return;
  }
  if (a.partial) {
    conv_partial_store<NI, NJ>(a, acc, b, t0, co_blk, wave_co0, wave_t0, lane);
    return;
  }
  conv_epilogue<TOUT, NI, NJ, EJ>(a, acc, b, t0, co_blk, wave_co0, wave_t0, lane);
}

// split reduction, second pass: y = epilogue(sum_z partial[z] + bias) with the partials added
// in split order; the epilogue (activation, residual, scale, accumulate) is conv_epilogue's
template <typename TOUT>
__global__ void __launch_bounds__(256) conv_splitk_reduce_kernel(ConvArgs a, int splits) {
  const int cg = a.Co / 4;
  const int64_t rows = (int64_t)a.B * a.T_out;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * cg) return;
  const int64_t row = idx / cg;
  const int c = (int)(idx - row * cg) * 4;
  const int b = (int)(row / a.T_out), t = (int)(row - (int64_t)b * a.T_out);
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  for (int z = 0; z < splits; ++z) {
    const float4 p = *reinterpret_cast<const float4*>(a.partial + ((int64_t)z * rows + row) * a.Co + c);
    v[0] += p.x; v[1] += p.y; v[2] += p.z; v[3] += p.w;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] += a.bias ? a.bias[c + e] : 0.f;
  if (a.post_act == VO_ACT_TANH) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = tanhf(v[e]);
  } else {
    const float ps = a.post_act == VO_ACT_RELU ? 0.f : (a.post_act == VO_ACT_LRELU ? a.post_slope : 1.f);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = lrelu_max(v[e], ps);  // ps in [0, 1]
  }
  const int64_t off = (int64_t)b * a.ybs + (int64_t)t * a.ldy + c;
  if (a.res1) {
    float rr[4];
    load4(reinterpret_cast<const TOUT*>(a.res1) + off, rr);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] += rr[e];
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] *= a.out_scale;
  if (a.res2) {
    float rr[4];
    load4(reinterpret_cast<const TOUT*>(a.res2) + off, rr);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] += rr[e];
  }
  store4(reinterpret_cast<TOUT*>(a.y) + off, v);
}

// fp32 convs over short sequences (T_out <= 16 rows: glyph encoder, variance predictors at
// T_src ~ 12) are a serial chain of (Ci / 32) * K pipeline steps per workgroup, each bound by
// a load round trip (FFN w_1: 72 steps, 51 us for 1.8 GFLOP).  Split the chunks so a workgroup
// runs about 4 steps; the partials are added by conv_splitk_reduce_kernel.  splitk_cfg 1 = off.
// bf16 deep reductions into narrow outputs (the C4 decoder's FFN w_1 input gradient: 1024 -> 256, k = 9,
// 16 k rows: a 9216-deep reduction, 106 us on 64 x 128 tiles): the 256 x 256 tile with its chunks split
// over ~256 workgroups, the fp32 partials added in split order by conv_splitk_reduce_kernel.  Plain convs
// only (no bias, activation, residual, scale or mask).  splitk_cfg 3 = off (A/B).
static bool splitk_bf16_ok(const vo_conv1d_desc* d) {
  return d->compute_dtype == VO_BF16 && d->x_dtype == VO_BF16 && !d->transposed && d->stride <= 1 && d->groups <= 1 &&
         d->variant == 0 && !d->bias && !d->res1 && !d->res2 && !d->ymask && d->pre_act == VO_ACT_NONE &&
         d->post_act == VO_ACT_NONE && d->out_scale == 1.f && d->Co <= 256 && d->Co % 64 == 0 && d->Ci % KC == 0 &&
         (int64_t)(d->Ci / KC) * d->K >= 64 && (int64_t)d->B * d->T_out >= 8192 && d->ldy == d->Co &&
         vo_tune_get("splitk_cfg") != 3 && vo_tune_get("splitk_cfg") != 1;
}

static bool splitk_plan(const vo_conv1d_desc* d, int* splits, int* kcs) {
  *splits = 1;
  *kcs = 0;
  if (vo_tune_get("splitk_cfg") == 1) return false;
  if (d->compute_dtype == VO_BF16) {
    if (!splitk_bf16_ok(d)) return false;
    const int n_chunks = d->Ci / KC;
    const int64_t tiles = (int64_t)d->B * ((d->T_out + 255) / 256) * ((d->Co + 255) / 256);
    int s = (int)std::min<int64_t>(n_chunks / 4, std::max<int64_t>(2, (256 + tiles - 1) / tiles));
    if (s < 2) return false;
    const int k = (n_chunks + s - 1) / s;
    *splits = (n_chunks + k - 1) / k;
    *kcs = k;
    return *splits >= 2;
  }
  if ((d->compute_dtype != VO_F32 && d->compute_dtype != VO_F32X3) || d->x_dtype != VO_F32 || d->y_dtype != VO_F32)
    return false;
  if (d->transposed || d->stride > 1 || d->groups > 1 || d->variant != 0) return false;
  if (d->T_out > 16 || d->Co < 64 || d->Co % 4 || d->ldy % 4) return false;
  const int n_chunks = (d->Ci + KC - 1) / KC;
  if (n_chunks * d->K < 16) return false;
  // ~4 steps per split (bench step 13.78 ms vs 13.85 with ~8 and 13.93 unsplit,
  // tools/bench_splitk_ab.sh); splitk_cfg 2 = ~8, 4 = ~16
  const int target = vo_tune_get("splitk_cfg") == 2 ? 8 : vo_tune_get("splitk_cfg") == 4 ? 16 : 4;
  const int k = std::max(1, target / d->K);
  const int s = (n_chunks + k - 1) / k;
  if (s < 2) return false;
  *splits = s;
  *kcs = k;
  return true;
}

// ------------------------------------------------------------------ host dispatch
// vo_conv1d = conv1d_check (arguments -> type triple), a select_* rule (descriptor, compute width, vo_tune knobs -> tile),
// plan_tile (nice, LDS bytes, reduction splits), launch_plan (tile -> instantiation).  All but the last are plain host
// code without a HIP call: vo_conv1d_plan runs them and stops there.
//
// A tile, written once: a wave holds NI x NJ MFMA tiles of 16 channels x 16 rows, a workgroup is WCO x WT waves, so
// BCO = 16 NI WCO output channels x BT = 16 NJ WT rows.  TPS = taps per pipeline step in bf16 compute (4-byte compute
// steps one tap); ROLE .. SEG are conv1d_kernel's parameters of the same names.  The conv stride
// is the descriptor's, not the tile's: launch_tile takes it beside the tile.
struct Tile {
  int NI, NJ, WCO, WT, TPS, ROLE = 0, PRIO = 0;
  bool GL = false, RS = false;
  int EJ = 2;
  bool SEG = false;
  constexpr int bco() const { return 16 * NI * WCO; }
  constexpr int bt() const { return 16 * NJ * WT; }
  constexpr Tile role(int r, int prio = 0) const { Tile t = *this; t.ROLE = r; t.PRIO = prio; return t; }
  constexpr Tile dma(bool rs = false) const { Tile t = *this; t.GL = true; t.RS = rs; return t; }  // weights by LDS-DMA; role split
  constexpr Tile seg() const { Tile t = *this; t.SEG = true; return t; }
};
// T<BCO>x<BT> {NI, NJ, WCO, WT, TPS}; _n<NI>w<WCO> names the twin of equal BCO x BT (128 x 32 and 64 x 64: the strided /
// grouped convs' tiles; 64 x 128: the Co = 80 tile); _seg = utterance-segment tile (BT / 16
// utterances); _mrf<s> = MRF stage s in its own ROLE (stage 0: s_setprio, weights by LDS-DMA, _rs = role-split staging)
constexpr Tile T32x16{1, 1, 2, 1, 4}, T128x16{2, 1, 4, 1, 4}, T128x32{2, 2, 4, 1, 4},
    T128x32_n4w2{4, 1, 2, 2, 2}, T32x64{2, 1, 1, 4, 4}, T64x64{2, 2, 2, 2, 2}, T64x64_n4w1{4, 1, 1, 4, 4},
    T128x64{4, 2, 2, 2, 2}, T64x128{2, 4, 2, 2, 2}, T64x128_n4w1{4, 2, 1, 4, 4}, T128x128{4, 4, 2, 2, 2},
    T32x256{2, 4, 1, 4, 4}, T64x256{4, 4, 1, 4, 4}, T128x256{4, 4, 2, 4, 2}, T256x256{4, 8, 4, 2, 2};
constexpr Tile T32x64_seg = Tile{1, 2, 2, 2, 1}.seg(), T64x64_seg = Tile{2, 2, 2, 2, 1}.seg(),
               T32x128_seg = Tile{1, 4, 2, 2, 1}.seg(), T64x128_seg = Tile{2, 4, 2, 2, 1}.seg();
constexpr Tile T256x256_mrf0 = T256x256.role(1, 1).dma(), T256x256_mrf0_rs = T256x256.role(1, 1).dma(true),
               T128x128_mrf1 = T128x128.role(2), T64x256_mrf2 = T64x256.role(3), T32x256_mrf3 = T32x256.role(4);

// (TIN, TC, TOUT) of an instantiation: F = float, B = bf16_t, X = bx3_t (split-bf16, VO_F32X3)
enum ConvTypes { FFF, FXF, BBB, BBF, FBB, FBF };
constexpr int kTypeBytes[][3] = {{4, 4, 4}, {4, 4, 4}, {2, 2, 2}, {2, 2, 4}, {4, 2, 2}, {4, 2, 4}};

// What one vo_conv1d call launches: all the launch record holds, and what launch_tile needs beyond the tile.
struct ConvPlan {
  bool ups;          // the streaming upsampler (upsample.hip) takes the descriptor: no tile, an all-zero record
  bool plane;        // the plane conv (conv_plane.hip) takes the descriptor: the 256 x 256 stage-0 record, its own launch
  int types, role;   // ConvTypes; d->variant where it selects an MRF stage's own tiles (bf16 in, compute and out)
  const Tile* tile;  // null = refused by the selector
  int S;             // conv stride
  bool nice;         // Ci % 32 == 0 and Co % BCO == 0: the instantiation without channel bounds checks
  int splits, kcs;   // split reduction: grid z, 32-channel chunks per split (1, 0 = off)
  size_t lds;
};

static ConvArgs conv_args(const vo_conv1d_desc* d, int BCO, int BT) {
  ConvArgs a;
  memset(&a, 0, sizeof(a));
  a.x = d->x; a.xbs = d->x_bstride; a.ldx = d->ldx; a.w = d->w; a.bias = d->bias;
  a.y = d->y; a.ybs = d->y_bstride; a.ldy = d->ldy; a.res1 = d->res1; a.res2 = d->res2;
  a.T_in = d->T_in; a.T_out = d->T_out; a.Ci = d->Ci; a.Co = d->Co; a.K = d->K; a.dil = d->dil; a.pad = d->pad;
  a.pre_act = d->pre_act; a.pre_slope = d->pre_slope;
  a.post_act = d->post_act; a.post_slope = d->post_slope; a.out_scale = d->out_scale;
  a.transposed = d->transposed; a.up_stride = d->up_stride; a.up_pad = d->up_pad; a.up_cout = d->up_cout; a.up_tout = d->up_tout;
  a.tiles_per_b = (d->T_out + BT - 1) / BT;
  a.co_tiles = (d->Co + BCO - 1) / BCO;
  a.B = d->B;
  a.ymask = d->ymask; a.ymask_slope = d->ymask_slope;
  a.lens = d->lens; a.lens_scale = d->lens_scale;
  const int groups = d->groups > 1 ? d->groups : 1;
  a.cig = d->Ci / groups;
  a.cog = d->Co / groups;
  return a;
}

template <const Tile& T, typename TIN, typename TC, typename TOUT, bool RAG = false, int S = 1>
static int launch_tile(const vo_conv1d_desc* d, const ConvPlan& p, hipStream_t st) {
  constexpr int BT = T.bt(), TPS = sizeof(TC) == 2 ? T.TPS : 1;
  ConvArgs a = conv_args(d, T.bco(), BT);
  if (T.SEG) a.tiles_per_b = 1;
  a.partial = p.splits > 1 ? reinterpret_cast<float*>(d->workspace) : nullptr;
  a.kcs = p.kcs;
  auto kern = p.nice ? conv1d_kernel<TIN, TC, TOUT, T.NI, T.NJ, T.WCO, T.WT, TPS, true, T.ROLE, T.PRIO, S, T.GL, T.RS, T.EJ, T.SEG, RAG>
                     : conv1d_kernel<TIN, TC, TOUT, T.NI, T.NJ, T.WCO, T.WT, TPS, false, T.ROLE, T.PRIO, S, false, false, 2, T.SEG, RAG>;
  const unsigned gx = T.SEG ? (unsigned)((d->B + BT / 16 - 1) / (BT / 16)) : (unsigned)(a.tiles_per_b * d->B);
  dim3 grid(gx, (unsigned)a.co_tiles, (unsigned)p.splits);
  hipLaunchKernelGGL(kern, grid, dim3(T.WCO * T.WT * 64), p.lds, st, a);
  if (a.partial) {
    const int64_t n = (int64_t)d->B * d->T_out * (d->Co / 4);
    hipLaunchKernelGGL(conv_splitk_reduce_kernel<TOUT>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, p.splits);
  }
  VO_RETURN_LAUNCH();
}

// The rest of the plan once the tile is chosen: nice, the LDS request, the reduction splits.
static int plan_tile(const vo_conv1d_desc* d, ConvPlan* p) {
  const Tile& t = *p->tile;
  p->nice = false; p->splits = 1; p->kcs = 0; p->lds = 0;
  const int S = p->S, tin = kTypeBytes[p->types][0], tc = kTypeBytes[p->types][1];
  const int BCO = t.bco(), BT = t.bt(), tps = tc == 2 ? t.TPS : 1, halo = (d->K - 1) * d->dil;
  // the ragged instantiations exist for the tiles select_types picks and the MRF stage-0 role (strided / grouped
  // convs and variants 2-4 with lens never pass conv1d_check): a call with lens is refused, never run dense
  VO_CHECK_ARG(!(d->lens && t.SEG), "conv1d: no ragged (lens) form of this tile (utterance-segment tiles: T_out <= 16 in fp32)");
  const int win_rows = t.SEG ? (BT / 16) * (16 + halo) : (BT - 1) * S + 1 + halo;
  p->nice = d->Ci % KC == 0 && d->Co % BCO == 0;
  // role-split kernels (RS): + the raw window staging area of conv1d_kernel (XPW pieces per window wave)
  const bool spl = t.RS && t.GL && S == 1 && tc == 2 && tin == 2 && (t.WCO * t.WT) % 2 == 0;
  const int nwx = t.WCO * t.WT / 2;
  const size_t raw = spl ? 2 * (size_t)((((BT - 1) * S + 1 + HALO_MAX) * (KC / 8) + 64 * nwx - 1) / (64 * nwx)) * nwx * 1024 : 0;
  p->lds = (size_t)(2 * win_rows + 2 * tps * BCO + 1) * (tc == 2 ? Lds<bf16_t>::PITCH : Lds<float>::PITCH) * tc + (p->nice ? raw : 0);
  if (p->lds > 160 * 1024) {
    vo_set_error("conv1d: LDS request %zu B exceeds 160 KiB", p->lds);
    return VO_ERR_INVALID;
  }
  int splits = 1, kcs = 0;
  if (S == 1 && d->workspace && !d->lens && splitk_plan(d, &splits, &kcs) &&
      d->workspace_bytes >= (int64_t)splits * d->B * d->T_out * d->Co * (int64_t)sizeof(float)) {
    p->splits = splits;
    p->kcs = kcs;
  }
  return VO_OK;
}

// the VO_CONV1D_LAUNCH_FIELDS record of a plan (rec zeroed by the caller: it stays so for the upsampler)
static void plan_record(const vo_conv1d_desc* d, const ConvPlan& p, int32_t* rec) {
  if (p.ups) return;
  const Tile& t = *p.tile;
  const int32_t r[VO_CONV1D_LAUNCH_FIELDS] = {t.bco(), t.bt(), p.S, t.SEG, p.nice, p.splits, kTypeBytes[p.types][0],
                                              kTypeBytes[p.types][1], kTypeBytes[p.types][2], t.ROLE, d->compute_dtype, t.NI, t.WCO};
  memcpy(rec, r, sizeof(r));
}

// HiFi-GAN discriminator layers (strided and/or grouped, C5): 64-row tiles so that a stride-4 window ((64 - 1) * 4 + 1
// + 40 rows) still double-buffers in LDS; output-channel tiles no wider than a group where groups are narrow
// (block-diagonal weights: a tile spanning g groups reduces over g groups' input channels).
static const Tile* select_disc(const vo_conv1d_desc* d) {
  const int groups = d->groups > 1 ? d->groups : 1;
  const int cog = d->Co / groups;
  if (d->stride > 4 && d->stride != 8) vo_set_error("conv1d: stride %d unsupported (1..4, 8)", d->stride);
  if (d->stride > 4) return d->stride == 8 ? &T128x32_n4w2 : nullptr;  // ConvTranspose1d(k 16, s 8) input gradient
  if (d->Co <= 32 || cog <= 32) return &T32x64;
  if (d->Co <= 64 || cog <= 64) return &T64x64_n4w1;
  // 64 x 64 where 128 x 64 tiles would leave fewer than 256 workgroups (the MPD's stride-3 layers over joined
  // period columns): C5 23.63 -> 23.57 ms in one process
  const int64_t t64 = (int64_t)d->B * ((d->T_out + 63) / 64) * ((d->Co + 127) / 128);
  if (t64 < 256) return &T64x64_n4w1;
  return &T128x64;
}

// The MRF stages' own instantiations (variant 1..4 with bf16 in, compute and out; same tiles as generic)
static const Tile* select_role(const vo_conv1d_desc* d, int role) {
  if (role != 1) return role == 2 ? &T128x128_mrf1 : role == 3 ? &T64x256_mrf2 : &T32x256_mrf3;
  // C = 256: 256 x 256 tile, 8 waves of 64 co x 128 rows (each weight tap feeds twice the rows of the 128 x 128 tile:
  // 0.095/0.151/0.208 -> 0.077/0.125/0.172 ms for k = 3/7/11 at B = 32, bit-identical).
  // s_setprio(1) around each MFMA cluster: +1-3 % (0.1667 -> 0.1654 ms at k = 11).
  // Round 2: weights by LDS-DMA (GL): 0.084 / 0.134 / 0.171 -> 0.083 / 0.126 / 0.163 ms for k = 3 / 7 / 11 alone
  // (bit-identical), within noise in the bench step; GL with 3-tap steps spilled
  const int cc = vo_tune_get("conv_cfg");
  if (d->lens && cc != 0) {
    vo_set_error("conv1d: conv_cfg=%d selects a kernel without a ragged (lens) form", cc);
    return nullptr;
  }
  // Round 2: role-split staging (RS: half the waves issue the weight DMA, half copy the window by LDS-DMA two chunks
  // ahead; bare step barriers): k = 7 / 11 0.137 / 0.175 -> 0.130 / 0.168 ms, k = 3 0.084 -> 0.096 (two-step chunks: the
  // weight waves' 8 DMA pieces per step, not the window, bind) -- k >= 5 only; conv_cfg 5 forces it, 6 disables it
  // (tools/probes/s0_probe.py, bit-identical)
  // Round 3, measured and dropped (tools/mrf_bench.py --stages 0, conv pairs): 4-wave tiles, two workgroups per CU
  // (256 co x 128 rows, 1 tap per step, with and without RS; 128 co x 256 rows) -- 27-45 % slower than the 8-wave
  // 256 x 256 tile at k = 3 / 7 / 11
  // (EJ, the epilogue's position tiles whose residual / accumulator rows are requested together: 4 measured within
  // 1 % of 2, 8 spills and runs 10-20 % slower -- kept at 2)
  // conv_cfg 9 = this rule as shipped, for the calls the plane conv (conv_plane.hip) takes at conv_cfg 0: A/B in one process
  return cc == 5 || (cc != 6 && d->K >= 5) ? &T256x256_mrf0_rs : &T256x256_mrf0;
}

// Every other conv; tc = sizeof the LDS compute element
static const Tile* select_types(const vo_conv1d_desc* d, int tc) {
  const int64_t rows = (int64_t)d->B * d->T_out;
  // short sequences (the glyph encoder / phoneme-level predictors run at T_src ~ 12): one
  // 16- or 32-row time tile, waves spread over output channels
  if (tc == 4) {
    // fp32 / split-bf16 at T_out <= 16: utterance-segment tiles (SEG, see conv1d_kernel), 4 utterances
    // x 64 output channels (32 below Co = 512); seg_cfg 3 = 8 utterances, 4 = off (the tiles below)
    const int gc = vo_tune_get("seg_cfg");
    if (d->T_out <= 16 && !d->transposed && d->stride <= 1 && (d->K - 1) * d->dil <= SEG_HALO && d->Co >= 32 &&
        gc != 4 && (int64_t)d->B * d->x_bstride < ((int64_t)1 << 31)) {
      if (gc == 3) return d->Co >= 512 ? &T64x128_seg : &T32x128_seg;
      return d->Co >= 512 ? &T64x64_seg : &T32x64_seg;
    }
  }
  if (d->T_out <= 16 && d->Co >= 64) {
    // fp32 (glyph encoder, variance predictors at B = 32, T = 12): 32 x 16 tiles, 4x the
    // workgroups of 128 x 16: FFN w_1 66 -> 51 us, w_2 28 -> 20, predictor k3 20 -> 13
    return tc == 4 ? &T32x16 : &T128x16;
  }
  if (d->T_out <= 32 && d->Co >= 64) return &T128x32;
  if (d->Co <= 32) return &T32x256;
  if (d->Co <= 64 || d->Co == 80) {
    // Co = 80 (PostNet output conv, mel_linear at B*T = 16384 rows): 64 x 128 tiles, twice the
    // workgroups of 64 x 256 (512 -> 80 k5 36.7 -> 29.7 us; tools/probes/small_convs.py)
    return d->Co == 80 ? &T64x128_n4w1 : &T64x256;
  }
  if (rows <= 2048) return &T64x64;
  if (tc == 2) {
    if (d->workspace && splitk_bf16_ok(d)) return &T256x256;  // split reduction
    // decoder shapes at B*T = 16384 rows: wide outputs (FFN w_1 k9 1024,
    // fused q/k/v 768) -> 256 x 256 tiles (-18 %); 1x1 convs to 256 channels -> 64 x 128
    // (twice the workgroups, -12 %).
    // 256 x 256 for the wide convs.  In isolation (profiles/r01j/wide_convs.txt) 256 co x 128 rows looked
    // 11 % faster on FFN w_1, but in the bench step its 12 decoder launches took 818 us against 584 (profiles/r01k/): kept out.
    // ups0 (polyphase 512 -> 8 x 256, K = 2) on the role-split staging was 11-20 % slower (its
    // one-step chunks: 8 weight-DMA pieces per weight wave per 2-tap step; tools/probes/ups0_probe.py)
    // (unless that leaves fewer than 128 workgroups: the MPD's joined period columns, ~4-5k rows x
    // 1024 channels, got 68-80 -- there the tiles below)
    const int64_t t256 = (int64_t)d->B * ((d->T_out + 255) / 256) * (d->Co / 256);
    // (utterances of >= 256 rows: at T_out = 128 -- the MSD's 1024-channel layers -- half of every 256-row
    // tile was padding: C5 23.68 -> 23.43 ms with them on the tiles below)
    if (d->T_out >= 256 && d->Co >= 768 && d->Co % 256 == 0 && t256 >= 128) return &T256x256;
    if (d->K == 1 && d->Co <= 256) return &T64x128;
    // Co <= 256 k > 1 with fewer than 512 128 x 128 tiles (the C4 decoder's FFN w_1 input gradient, 1024 ->
    // 256 k9 at 16384 rows: 125 -> 106 us): 64 x 128, twice the workgroups
    const int64_t t128 = (int64_t)d->B * ((d->T_out + 127) / 128) * ((d->Co + 127) / 128);
    if (d->Co <= 256 && d->Co % 64 == 0 && t128 < 512) return &T64x128;
    // wide convs with fewer than 256 128 x 128 tiles (C5's MPD over joined period columns, 1024 -> 1024
    // k = 5 at 2-5 k rows: 136-312 workgroups) on 64 x 128 tiles too: C5 24.07 -> 23.75 ms
    if (d->Co % 64 == 0 && t128 < 256) return &T64x128;
    // mid-width convs (PostNet 512 -> 512 k5, conv_pre 80 -> 512 k7 at 16384 rows): 128 x 256
    // tiles (twice the rows per staged weight tap): 512 k5 67.9 -> 63.4 us, 80 k7 27.6 -> 27.0,
    // bit-identical; the Co = 128 polyphase upsampler is slower with it (210 -> 234 us); 256 x 128: no gain
    if (d->Co >= 512 && d->Co < 768 && d->Co % 128 == 0 && !d->transposed) return &T128x256;
    // bf16: 64 x 128 in place of the 128 x 128 tile of 4-byte compute (C5 23.68 -> 23.52 ms, C4 and inference
    // shapes unaffected)
    return &T64x128;
  }
  return &T128x128;  // 4-byte compute
}

// ---- tile -> instantiation: the one place that says which (tile, types, RAG, S) combinations are compiled
constexpr int kNoTile = -1000;  // launch_among: p.tile is none of TS
template <typename TIN, typename TC, typename TOUT, bool RAG, int S, const Tile&... TS>
static int launch_among(const vo_conv1d_desc* d, const ConvPlan& p, hipStream_t st) {
  int rc = kNoTile;
  (void)((p.tile == &TS && ((rc = launch_tile<TS, TIN, TC, TOUT, RAG, S>(d, p, st)), true)) || ...);
  return rc;
}

// RAG: the ragged instantiations of the same tiles (vo_conv1d with lens); SEG tiles: 4-byte compute only, no ragged form
template <typename TIN, typename TC, typename TOUT, bool RAG = false>
static int launch_types(const vo_conv1d_desc* d, const ConvPlan& p, hipStream_t st) {
  // the tiles select_types returns at one compute width only, then those of both
  int rc = kNoTile;
  if constexpr (sizeof(TC) == 4) {
    rc = launch_among<TIN, TC, TOUT, false, 1, T32x64_seg, T64x64_seg, T32x128_seg, T64x128_seg>(d, p, st);
    if (rc == kNoTile) rc = launch_among<TIN, TC, TOUT, RAG, 1, T32x16, T128x128>(d, p, st);
  } else {
    rc = launch_among<TIN, TC, TOUT, RAG, 1, T128x16, T64x128, T128x256, T256x256>(d, p, st);
  }
  if (rc != kNoTile) return rc;
  return launch_among<TIN, TC, TOUT, RAG, 1, T128x32, T32x256, T64x256, T64x128_n4w1, T64x64>(d, p, st);
}

// strided / grouped: stride 8 has the one tile select_disc returns for it, the other strides three
template <typename TIN, typename TC, typename TOUT, int S>
static int launch_disc_s(const vo_conv1d_desc* d, const ConvPlan& p, hipStream_t st) {
  if constexpr (S >= 8)
    return launch_among<TIN, TC, TOUT, false, S, T128x32_n4w2>(d, p, st);
  else
    return launch_among<TIN, TC, TOUT, false, S, T32x64, T64x64_n4w1, T128x64>(d, p, st);
}
template <typename TIN, typename TC, typename TOUT>
static int launch_disc(const vo_conv1d_desc* d, const ConvPlan& p, hipStream_t st) {
  switch (p.S) {
    case 1: return launch_disc_s<TIN, TC, TOUT, 1>(d, p, st);
    case 2: return launch_disc_s<TIN, TC, TOUT, 2>(d, p, st);
    case 3: return launch_disc_s<TIN, TC, TOUT, 3>(d, p, st);
    case 4: return launch_disc_s<TIN, TC, TOUT, 4>(d, p, st);
    default: return launch_disc_s<TIN, TC, TOUT, 8>(d, p, st);
  }
}

int vo_conv_plane_launch(const vo_conv1d_desc* d, hipStream_t st);  // conv_plane.hip

static int launch_plan(const vo_conv1d_desc* d, const ConvPlan& p, hipStream_t st) {
  if (p.plane) return vo_conv_plane_launch(d, st);
  const bool rag = d->lens != nullptr;
  int rc = kNoTile;
  if (d->stride > 1 || d->groups > 1)  // discriminator layers: three type triples, no ragged form
    rc = p.types == FFF ? launch_disc<float, float, float>(d, p, st)
                        : p.types == BBB ? launch_disc<bf16_t, bf16_t, bf16_t>(d, p, st) : launch_disc<bf16_t, bf16_t, float>(d, p, st);
  else if (p.role && rag)  // MRF stages: bf16 only, ragged for stage 0 alone
    rc = launch_among<bf16_t, bf16_t, bf16_t, true, 1, T256x256_mrf0, T256x256_mrf0_rs>(d, p, st);
  else if (p.role)
    rc = launch_among<bf16_t, bf16_t, bf16_t, false, 1, T256x256_mrf0, T256x256_mrf0_rs, T128x128_mrf1, T64x256_mrf2, T32x256_mrf3>(d, p, st);
  else switch (p.types) {  // ragged: fp32, and bf16 compute with a bf16 output
    case FXF: rc = launch_types<float, bx3_t, float>(d, p, st); break;
    case FFF: rc = rag ? launch_types<float, float, float, true>(d, p, st) : launch_types<float, float, float>(d, p, st); break;
    case BBB: rc = rag ? launch_types<bf16_t, bf16_t, bf16_t, true>(d, p, st) : launch_types<bf16_t, bf16_t, bf16_t>(d, p, st); break;
    case FBB: rc = rag ? launch_types<float, bf16_t, bf16_t, true>(d, p, st) : launch_types<float, bf16_t, bf16_t>(d, p, st); break;
    case BBF: rc = launch_types<bf16_t, bf16_t, float>(d, p, st); break;
    default: rc = launch_types<float, bf16_t, float>(d, p, st);
  }
  if (rc == kNoTile) vo_set_error("conv1d: the selected tile is not compiled for type triple %d", p.types);
  return rc == kNoTile ? VO_ERR_INVALID : rc;
}

bool vo_ups_takes(const vo_conv1d_desc* d);                  // upsample.hip
int vo_ups_launch(const vo_conv1d_desc* d, hipStream_t st);  // upsample.hip

// The argument checks of vo_conv1d and vo_conv1d_plan; sets p->ups, and p->types and p->role unless p->ups
static int conv1d_check(const vo_conv1d_desc* d, ConvPlan* p) {
  VO_CHECK_ARG(d != nullptr, "conv1d: null descriptor");
  VO_CHECK_ARG(d->x && d->w && d->y, "conv1d: null tensor pointer");
  VO_CHECK_ARG((d->pre_act != VO_ACT_LRELU || (d->pre_slope >= 0.f && d->pre_slope <= 1.f)) &&
                   (d->post_act != VO_ACT_LRELU || (d->post_slope >= 0.f && d->post_slope <= 1.f)),
               "conv1d: leaky-ReLU slope outside [0, 1]");
  VO_CHECK_ARG(d->B > 0 && d->T_in > 0 && d->T_out > 0 && d->Ci > 0 && d->Co > 0 && d->K > 0,
               "conv1d: non-positive size (B=%d T_in=%d T_out=%d Ci=%d Co=%d K=%d)", d->B, d->T_in, d->T_out, d->Ci, d->Co, d->K);
  VO_CHECK_ARG(d->Ci % 8 == 0 && d->ldx % 8 == 0 && d->ldx >= d->Ci,
               "conv1d: Ci (%d) and ldx (%d) must be multiples of 8, ldx >= Ci", d->Ci, d->ldx);
  VO_CHECK_ARG(d->Co % 4 == 0 && d->ldy % 4 == 0, "conv1d: Co (%d) and ldy (%d) must be multiples of 4", d->Co, d->ldy);
  VO_CHECK_ARG(d->dil >= 1 && (d->K - 1) * d->dil <= HALO_MAX,
               "conv1d: (K-1)*dil = %d exceeds the supported halo %d", (d->K - 1) * d->dil, HALO_MAX);
  VO_CHECK_ARG(d->variant == 0 || (d->variant == 1 && d->Co >= 128) || (d->variant == 2 && d->Co >= 128) ||
                   (d->variant == 3 && d->Co <= 64 && d->Co % 16 == 0) || (d->variant == 4 && d->Co <= 32),
               "conv1d: variant %d does not fit Co=%d", d->variant, d->Co);
  if (d->transposed) {
    VO_CHECK_ARG(d->up_stride >= 1 && d->up_cout > 0 && d->Co == d->up_stride * d->up_cout &&
                     d->up_cout % 16 == 0 && d->K == 2 && d->pad == 1,
                 "conv1d: bad polyphase ConvTranspose1d descriptor");
  } else {
    VO_CHECK_ARG(d->Co % 16 == 0 || d->Co == 80 || d->Co <= 32, "conv1d: unsupported Co %d", d->Co);
  }
  VO_CHECK_ARG(!d->ymask || (d->y_dtype == VO_BF16 && !d->transposed && !d->bias && !d->res1 && !d->res2 &&
                             d->post_act == VO_ACT_NONE && d->out_scale == 1.f && d->variant == 0 &&
                             d->ymask_slope >= 0.f && d->ymask_slope <= 1.f),
               "conv1d: ymask needs a bf16 output without bias, residuals, activation or scale, slope in [0, 1]");
  // split-bf16 compute has no polyphase form: refused before the streaming upsampler can take the call
  VO_CHECK_ARG(!(d->compute_dtype == VO_F32X3 && d->transposed), "conv1d: VO_F32X3 compute excludes transposed");
  if (d->lens) {
    // Ragged batch: the forms the vocoder reaches (conv_pre, the polyphase upsamplers, the ResBlock convs).  Anything
    // else is refused, not run dense.
    VO_CHECK_ARG(d->lens_scale >= 1, "conv1d: lens_scale %d < 1", d->lens_scale);
    VO_CHECK_ARG(d->stride <= 1 && d->groups <= 1, "conv1d: lens excludes stride > 1 and groups > 1");
    VO_CHECK_ARG(!d->workspace, "conv1d: lens excludes a split-reduction workspace");
    VO_CHECK_ARG(!d->ymask, "conv1d: lens excludes ymask");
    VO_CHECK_ARG(d->compute_dtype != VO_F32X3, "conv1d: lens excludes VO_F32X3 compute");
    VO_CHECK_ARG(d->transposed ? d->T_out == d->T_in + 1 : (d->T_out == d->T_in && (d->K - 1) * d->dil == 2 * d->pad),
                 "conv1d: lens needs a same-length conv (T_out = T_in, 2 pad = (K - 1) dil; polyphase: T_out = T_in + 1)");
    const int uc = vo_tune_get("ups_cfg");
    VO_CHECK_ARG(!d->transposed || uc == 0 || uc == 1 || uc == 4,
                 "conv1d: ups_cfg=%d selects a kernel without a ragged (lens) form", uc);
  }
  p->ups = d->transposed && vo_ups_takes(d);  // narrow upsamplers: the persistent streaming kernel (upsample.hip)
  if (p->ups) return VO_OK;
  const int xi = d->x_dtype, yo = d->y_dtype;
  p->role = 0;
  if (d->compute_dtype == VO_F32X3) {  // split-bf16 fp32 contractions (vonoma.h)
    VO_CHECK_ARG(xi == VO_F32 && yo == VO_F32 && d->stride <= 1 && d->groups <= 1 && d->variant == 0,
                 "conv1d: VO_F32X3 compute needs fp32 I/O, stride 1, no groups");
    p->types = FXF;
    return VO_OK;
  }
  if (d->stride > 1 || d->groups > 1) {  // discriminator layers
    const int g = d->groups > 1 ? d->groups : 1;
    VO_CHECK_ARG(!d->transposed && d->variant == 0, "conv1d: stride/groups exclude transposed and variants");
    VO_CHECK_ARG(d->Ci % g == 0 && d->Co % g == 0, "conv1d: Ci %d / Co %d not divisible by groups %d", d->Ci, d->Co, g);
    if (d->compute_dtype != VO_F32) {
      VO_CHECK_ARG(d->compute_dtype == VO_BF16 && xi == VO_BF16, "conv1d: strided/grouped bf16 needs bf16 input");
      p->types = yo == VO_BF16 ? BBB : BBF;
      return VO_OK;
    }
  }
  if (d->compute_dtype == VO_F32) {
    VO_CHECK_ARG(xi == VO_F32 && yo == VO_F32, "conv1d: fp32 compute needs fp32 I/O");
    p->types = FFF;
    return VO_OK;
  }
  VO_CHECK_ARG(d->compute_dtype == VO_BF16, "conv1d: bad compute dtype");
  if (d->lens) {  // the vocoder's forms: bf16 activations (MRF stage 0 in its own role), conv_pre reading an fp32 mel
    VO_CHECK_ARG(yo == VO_BF16 && d->variant <= 1, "conv1d: lens with bf16 compute needs a bf16 output, variant 0 / 1");
    p->types = xi == VO_F32 ? FBB : BBB;
  } else if ((xi != VO_BF16 && xi != VO_F32) || (yo != VO_BF16 && yo != VO_F32)) {
    vo_set_error("conv1d: bad dtypes");
    return VO_ERR_INVALID;
  } else {
    p->types = xi == VO_BF16 ? (yo == VO_BF16 ? BBB : BBF) : (yo == VO_BF16 ? FBB : FBF);
  }
  p->role = p->types == BBB ? d->variant : 0;  // HiFi-GAN MRF stages: own instantiations (same tiles as generic)
  return VO_OK;
}

// check, select, plan: on VO_OK *p is what vo_conv1d launches
static int conv1d_plan(const vo_conv1d_desc* d, ConvPlan* p) {
  p->plane = false;
  const int rc = conv1d_check(d, p);
  if (rc != VO_OK || p->ups) return rc;
  // MRF stage 0, dense: wave-owned output planes (conv_plane.hip).  The tile selected below is its true geometry
  // (256 x 256, NI 4, WCO 4) and stays the launch record
  p->plane = p->role == 1 && vo_conv1d_plane_takes(d) != 0;
  p->S = d->stride > 1 ? d->stride : 1;
  p->tile = d->stride > 1 || d->groups > 1 ? select_disc(d) : p->role ? select_role(d, p->role)
                                           : select_types(d, kTypeBytes[p->types][1]);
  return p->tile ? plan_tile(d, p) : VO_ERR_INVALID;
}

}  // namespace vo

using namespace vo;

extern "C" int64_t vo_conv1d_workspace_size(const vo_conv1d_desc* d) {
  int splits = 1, kcs = 0;
  if (!d || !splitk_plan(d, &splits, &kcs)) return 0;
  return (int64_t)splits * d->B * d->T_out * d->Co * (int64_t)sizeof(float);
}

static int copy_record(const int32_t* src, int32_t* rec, int n) {
  const int m = rec ? std::max(0, std::min(n, (int)VO_CONV1D_LAUNCH_FIELDS)) : 0;
  if (m > 0) memcpy(rec, src, m * sizeof(int32_t));
  return m;
}

extern "C" int vo_conv1d_last_launch(int32_t* rec, int n) { return copy_record(g_last_launch, rec, n); }

extern "C" int vo_conv1d_plan(const vo_conv1d_desc* d, int32_t* rec, int n) {
  int32_t r[VO_CONV1D_LAUNCH_FIELDS] = {};
  ConvPlan p;
  const int rc = conv1d_plan(d, &p);
  if (rc == VO_OK) plan_record(d, p, r);
  copy_record(r, rec, n);
  return rc;
}

extern "C" int vo_conv1d(const vo_conv1d_desc* d, void* stream) {
  memset(g_last_launch, 0, sizeof(g_last_launch));
  ConvPlan p;
  const int rc = conv1d_plan(d, &p);
  if (rc != VO_OK) return rc;
  hipStream_t st = reinterpret_cast<hipStream_t>(const_cast<void*>(stream));
  if (p.ups) return vo_ups_launch(d, st);
  plan_record(d, p, g_last_launch);
  return launch_plan(d, p, st);
}
