// MRF stage-0 conv (HiFi-GAN ResBlock1 convs at C = 256, k = 3 / 7 / 11) in the "wave-owned output planes" form of
// resblock_rw.hip:
//   y = (post(conv_dil(lrelu x) + b) + res1) * scale + res2
// (scripts/hifigan/models.py:96-103, one conv of a (c1, c2) iteration; the residual, the MRF sum and its 1 / 3 ride
// in the epilogue; Generator's c1 applies c2's leaky ReLU as its post-activation, so its c2 comes without a prologue).  vo_conv1d sends it the dense variant-1 calls vo_conv1d_plane_takes accepts (conv1d.hip); the
// tiled conv1d_kernel keeps everything else.
//
// The tiled kernel (256 x 256 tile, 8 waves at 256 registers) shares every weight tap between its waves through
// LDS, so each 2-tap step ends in a workgroup barrier with the weight-DMA wait in front of it (34-45 % of wave
// cycles), and it has no register left to prefetch the epilogue's residual rows.  Here the workgroup is 4 waves, one
// per SIMD at 512 registers, and wave w owns output channels [64 w, 64 w + 64) of all 256 rows of the tile:
//   * 4 co tiles x 16 row tiles of v_mfma_f32_16x16x32_bf16 = 256 accumulator registers;
//   * its weights go straight from L2 into its own registers: one A piece = 64 co x 32 ci of one tap (four 16-byte
//     loads per lane, 64 MFMAs), streamed through a ring DA pieces ahead -- no wave reads another wave's weights,
//     no tap ends in a barrier;
//   * only the activations are shared through LDS: the lrelu'd input window as 32-channel planes of 320 rows (256 +
//     the 64-row halo limit) in the plane_off swizzle, a ring of CPL_NPB planes.  Plane c + 3 is requested (global ->
//     registers) during chunk c, plane c + 1 written (lrelu8 -> ds_write_b128, five slots per thread) in chunk c's
//     first tap, and ONE barrier per chunk, after that tap, publishes it: 8 per tile;
//   * vmcnt retires in issue order, so in every step the A pieces are requested before window or residual rows;
//   * the tile's last TG taps run row-tile-major (all TG taps x 4 co tiles of row tile j, then j + 1): row tile j is
//     final after its 4 TG MFMAs and its epilogue issues under row tile j + 1's; its res1 / res2 rows are requested
//     RD row tiles ahead.  At k = 3 that is the whole last chunk.
// Arithmetic: accumulators start at zero, the reduction runs chunk-major with the taps ascending inside a chunk and
// ci = 32 c + 8 (lane >> 4) + e, the epilogue is conv_epilogue8 (vo_common.h) -- every accumulator sees the (c, k)
// sequence and the roundings of conv1d_kernel, so the two kernels agree bit for bit.
// Output channels: A row m of co tile i is channel 64 w + 16 (m >> 2) + 4 i + (m & 3) (conv1d_kernel's permutation), so
// lane (g = lane >> 4, lr = lane & 15) holds the 16 consecutive channels 64 w + 16 g .. + 15 of row 16 j + lr: two
// 16-byte residual loads and y stores per row tile.
// Weights: the ordinary [K][C_out][C_in] bf16 pack; bias fp32.

#include "mrf_plane.h"

namespace vo {

struct CplArgs {
  const bf16_t* x; const bf16_t* w; const float* bias; bf16_t* y; const bf16_t* res1; const bf16_t* res2;
  int64_t xbs, ybs;  // elements between utterances (x; y, res1, res2)
  int T, dil, pad, tiles_per_b;
  float pre_slope, ps, out_scale;  // ps: post leaky-ReLU slope, 1 = none
  unsigned long long* stamps;      // diagnostic builds only (-DVO_CPL_STAMPS, tools/probes/cpl_stamps.py)
};

constexpr int CPL_C = 256, CPL_R = 256;        // channels, rows per tile
constexpr int CPL_WR = CPL_R + 64;             // window rows per plane (halo <= 64)
constexpr int CPL_PL = CPL_WR * 32;            // plane stride (elements)
constexpr int CPL_NPB = 4;                     // LDS plane ring
constexpr size_t CPL_LDS = (size_t)CPL_NPB * CPL_PL * sizeof(bf16_t) + CPL_C * sizeof(float);
constexpr int CPL_NSTW = 16, CPL_NPT = 16;     // stamp geometry (diagnostic builds): workgroups, stamps per wave

template <int K, bool ST = false>
__global__ void __launch_bounds__(256, 1) mrf_conv_plane_kernel(CplArgs a) {
  constexpr int C = CPL_C, NC = C / 32, NJ = 16, NS = CPL_WR / 64;  // chunks, row tiles, staging slots per thread and plane
  constexpr int PL = CPL_PL, NPB = CPL_NPB;
  // A ring: piece p (chunk p / K, tap p % K) in slot p % NA, requested over the first four steps of piece p - DA.
  // A piece is 1,024 MFMA cycles (0.43 us): five pieces ahead is an L2 round trip with room for an HBM one, which
  // the in-order vmcnt charges to the A piece requested after a window row
  constexpr int NA = 6, DA = NA - 1;
  constexpr int TG = K < DA ? K : DA;          // taps of the last chunk run row-tile-major (their pieces all resident)
  constexpr int NPC = NC * K, P0 = NPC - TG;   // pieces; the first row-tile-major one
  constexpr int NQ = NPC * NJ;                 // steps (one B fragment, four MFMAs)
  constexpr int NB = 6, DB = 4;                // B-fragment ring / prefetch distance (steps)
  constexpr int NR = 4, RD = 3;                // residual-row ring / request distance (row tiles)
  static_assert(K >= 3 && TG >= 3 && NA > DA && NR > RD && DB <= NJ, "conv plane: schedule");

  const int T = a.T, dil = a.dil;

  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  bf16_t* win = reinterpret_cast<bf16_t*>(smem_raw);              // [NPB][CPL_WR][32]
  float* sbias = reinterpret_cast<float*>(win + NPB * PL);        // [C]

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, lg = lane >> 4;
  const int b = blockIdx.x / a.tiles_per_b;
  const int t0 = (blockIdx.x - b * a.tiles_per_b) * CPL_R;
  // ST (diagnostic builds): s_memtime at fixed points, written by lane 0 of each wave of workgroups 0 .. CPL_NSTW-1
  // to a buffer nothing else reads
  auto stamp = [&](int idx) {
    if constexpr (ST) {
      if (blockIdx.x < CPL_NSTW && lane == 0)
        a.stamps[(blockIdx.x * 4 + w) * CPL_NPT + idx] = __builtin_amdgcn_s_memtime();
    }
  };
  stamp(0);

  sbias[tid] = a.bias[tid];

  // ---- A fragments: lane l holds W[tap][co][ci] for co = 64 w + 16 (lr >> 2) + 4 i + (lr & 3) (co tile i) and
  // ci = 32 c + 8 lg .. + 7, through a buffer resource
  const int aoff = ((64 * w + 16 * (lr >> 2) + (lr & 3)) * C + 8 * lg) * (int)sizeof(bf16_t);
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)a.w, (short)0, K * C * C * 2, 0x00020000);
  bf16x8 A[NA][4];
  auto loadA = [&](int p, int i) {
    const int c = p / K, k = p % K;
    A[p % NA][i] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rw, aoff + i * 4 * C * 2 + c * 64,
                                                                                     k * (C * C * 2), 0));
  };

  // ---- window staging: slot s of a thread is (row tid / 4 + 64 s, 16-byte column tid % 4) of the plane.  Rows
  // before 0 / past T are out of the utterance's buffer range and read 0 (the conv's zero padding); so are the rows
  // past the 256 + (K - 1) dil the taps read, without touching memory
  const int srow = tid >> 2, sq = tid & 3;
  const int xl = plane_off(srow, sq);  // + 64 s rows (swizzle unchanged)
  const __amdgpu_buffer_rsrc_t rsx = plane_utt<C>(a.x + b * a.xbs, 0, T, T);
  const int wneed = CPL_R + (K - 1) * dil;
  int xo[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s)
    xo[s] = srow + 64 * s < wneed ? ((t0 - a.pad + srow + 64 * s) * C + 8 * sq) * 2 : 0x7ffffff0;
  u32x4 xw[2][NS];  // plane c in set c & 1
  const float pre_slope = a.pre_slope;
  auto load_win = [&](int c, int s) { xw[c & 1][s] = __builtin_amdgcn_raw_buffer_load_b128(rsx, xo[s] + c * 64, 0, 0); };
  auto store_win = [&](int c, int s) {
    *reinterpret_cast<u32x4*>(win + (c % NPB) * PL + xl + s * 64 * 32) = lrelu8(xw[c & 1][s], pre_slope);
  };

  // ---- epilogue operands: rows [t0, t0 + valid) of y / res1 / res2 (loads past them read 0, stores are dropped;
  // an absent residual is an empty range: its loads touch no memory and conv_epilogue8 skips the add)
  const int valid = min(CPL_R, T - t0);
  const int64_t ybase = b * a.ybs + (int64_t)t0 * C;
  const bool r1 = a.res1 != nullptr, r2 = a.res2 != nullptr;
  const __amdgpu_buffer_rsrc_t yrs =
      __builtin_amdgcn_make_buffer_rsrc((void*)(a.y + ybase), (short)0, valid * C * 2, 0x00020000);
  const __amdgpu_buffer_rsrc_t r1s =
      __builtin_amdgcn_make_buffer_rsrc((void*)((r1 ? a.res1 : a.y) + ybase), (short)0, r1 ? valid * C * 2 : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t r2s =
      __builtin_amdgcn_make_buffer_rsrc((void*)((r2 ? a.res2 : a.y) + ybase), (short)0, r2 ? valid * C * 2 : 0, 0x00020000);
  const int eoff = (lr * C + 64 * w + 16 * lg) * 2;  // + row tile j: 16 rows; + half h: 16 bytes
  u32x4 rv1[NR][2], rv2[NR][2];
  auto load_res = [&](int j) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      rv1[j % NR][h] = __builtin_amdgcn_raw_buffer_load_b128(r1s, eoff + j * 16 * C * 2 + 16 * h, 0, 0);
      rv2[j % NR][h] = __builtin_amdgcn_raw_buffer_load_b128(r2s, eoff + j * 16 * C * 2 + 16 * h, 0, 0);
    }
  };

  // ---- prologue: A pieces first (in-order vmcnt), planes 0 and 1, plane 0 written, plane 2 into its registers
#pragma unroll
  for (int p = 0; p < DA; ++p)
#pragma unroll
    for (int i = 0; i < 4; ++i) loadA(p, i);
#pragma unroll
  for (int s = 0; s < NS; ++s) load_win(0, s);
#pragma unroll
  for (int s = 0; s < NS; ++s) load_win(1, s);
#pragma unroll
  for (int s = 0; s < NS; ++s) store_win(0, s);
#pragma unroll
  for (int s = 0; s < NS; ++s) load_win(2, s);

  f32x4 acc[4][NJ];
  bf16x8 Bq[NB];
  int tb[K];  // B-fragment offset of tap k: row k dil + lr, chunk lg (+ 16 j rows: swizzle unchanged)
#pragma unroll
  for (int k = 0; k < K; ++k) tb[k] = plane_off(k * dil + lr, lg);

  // step q -> (chunk, tap, row tile): piece-major with the 16 row tiles inside a piece, then from piece P0 on
  // row-tile-major over the last TG taps
  auto chunk_of = [&](int q) { return q < P0 * NJ ? q / NJ / K : NC - 1; };
  auto tap_of = [&](int q) { return q < P0 * NJ ? (q / NJ) % K : K - TG + (q - P0 * NJ) % TG; };
  auto rt_of = [&](int q) { return q < P0 * NJ ? q % NJ : (q - P0 * NJ) / TG; };
  auto readB = [&](int q) {
    Bq[q % NB] = *reinterpret_cast<const bf16x8*>(win + (chunk_of(q) % NPB) * PL + tb[tap_of(q)] + rt_of(q) * 512);
  };

  const float ps = a.ps, osc = a.out_scale;
  auto post = [&](int j, int h) {  // half h of row tile j: channels 64 w + 16 lg + 8 h .. + 7
    float av[8], bv[8], x1[8], x2[8], q[8];
    const f32x4 b0 = *reinterpret_cast<const f32x4*>(sbias + 64 * w + 16 * lg + 8 * h);
    const f32x4 b1 = *reinterpret_cast<const f32x4*>(sbias + 64 * w + 16 * lg + 8 * h + 4);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      av[e] = acc[2 * h + e / 4][j][e & 3];
      bv[e] = e < 4 ? b0[e & 3] : b1[e & 3];
    }
    unpack8(rv1[j % NR][h], x1);
    unpack8(rv2[j % NR][h], x2);
    conv_epilogue8(av, bv, false, ps, r1, x1, osc, r2, x2, q);
    const u32x4 v = u32x4{pk_bf16(q[0], q[1]), pk_bf16(q[2], q[3]), pk_bf16(q[4], q[5]), pk_bf16(q[6], q[7])};
    __builtin_amdgcn_raw_buffer_store_b128(v, yrs, eoff + j * 16 * C * 2 + 16 * h, 0, 0);
  };

  lds_barrier();  // plane 0 and the bias staged
  stamp(1);
#pragma unroll
  for (int q = 0; q < DB; ++q) readB(q);

  // Every step is one B-fragment read (DB steps ahead) and four MFMAs; the other work is spread over the steps so that
  // it issues in the MFMAs' free issue cycles: the A pieces of DA pieces ahead (steps 0-3 of a piece), in a chunk's
  // first tap the next plane's LDS writes, then the chunk's barrier, in its second tap the requests of the plane three
  // chunks ahead; in the row-tile-major part the epilogue of row tile j - 1 and the residual requests of row tile j + RD.
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int c = chunk_of(q), k = tap_of(q), j = rt_of(q);
    const bool tail = q >= P0 * NJ;
    const int p = tail ? NPC : q / NJ;  // piece-major part: the piece
    if (q % (K * NJ) == 0) stamp(2 + c);
    if (q == P0 * NJ) stamp(2 + NC);
    if (q + DB < NQ) readB(q + DB);
    if (!tail) {
      if (j < 4 && p + DA < NPC) loadA(p + DA, j);
      if (k == 0 && c + 1 < NC && j >= 5 && j % 2 == 1 && (j - 5) / 2 < NS) store_win(c + 1, (j - 5) / 2);
      if (k == 1 && c + 3 < NC && j >= 4 && j % 2 == 0 && (j - 4) / 2 < NS) load_win(c + 3, (j - 4) / 2);
      if (p == P0 - 1 && j >= 10 && j - 10 < RD) load_res(j - 10);
    }
    __builtin_amdgcn_sched_barrier(0);
    const bf16x8 bq = Bq[q % NB];
    const bf16x8(&Ak)[4] = A[(c * K + k) % NA];
    if (c == 0 && k == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ak[i], bq, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ak[i], bq, acc[i][j], 0, 0, 0);
    }
    if (tail) {
      const int kk = (q - P0 * NJ) % TG;
      if (j > 0 && kk == 1) post(j - 1, 0);
      if (j > 0 && kk == 2) post(j - 1, 1);
      if (kk == 2 && j + RD < NJ) load_res(j + RD);  // after the epilogue that read the ring slot it takes
    }
    __builtin_amdgcn_sched_barrier(0);
    // the chunk's barrier, after its first tap: plane c + 1 is written (read from the chunk's end on, DB steps
    // ahead); the slot it took was last read in chunk c - 3, before the barrier of chunk c - 1
    if (!tail && k == 0 && j == NJ - 1 && c + 1 < NC) lds_barrier();
  }
  stamp(3 + NC);
  post(NJ - 1, 0);
  post(NJ - 1, 1);
  stamp(4 + NC);
}

template <int K>
static int cpl_launch(const CplArgs& a, int B, hipStream_t st) {
  hipLaunchKernelGGL(mrf_conv_plane_kernel<K>, dim3((unsigned)(a.tiles_per_b * B)), dim3(256), CPL_LDS, st, a);
  VO_RETURN_LAUNCH();
}

static CplArgs cpl_args(const vo_conv1d_desc* d) {
  CplArgs a;
  a.x = (const bf16_t*)d->x; a.w = (const bf16_t*)d->w; a.bias = d->bias; a.y = (bf16_t*)d->y;
  a.res1 = (const bf16_t*)d->res1; a.res2 = (const bf16_t*)d->res2;
  a.xbs = d->x_bstride; a.ybs = d->y_bstride;
  a.T = d->T_out; a.dil = d->dil; a.pad = d->pad;
  a.tiles_per_b = (d->T_out + CPL_R - 1) / CPL_R;
  // no prologue activation (c2 reads c1's output, which c1's epilogue already put through the leaky ReLU) is slope 1:
  // max(v, 1 v) = v and bf16 -> fp32 -> bf16 is exact, so the window is the copy the tiled kernel stages
  a.pre_slope = d->pre_act == VO_ACT_LRELU ? d->pre_slope : 1.f;
  a.ps = d->post_act == VO_ACT_LRELU ? d->post_slope : 1.f;
  a.out_scale = d->out_scale;
  a.stamps = nullptr;
  return a;
}

// vo_conv1d's launch of a descriptor vo_conv1d_plane_takes accepted (conv1d.hip, launch_plan)
int vo_conv_plane_launch(const vo_conv1d_desc* d, hipStream_t st) {
  const CplArgs a = cpl_args(d);
  return d->K == 3 ? cpl_launch<3>(a, d->B, st) : d->K == 7 ? cpl_launch<7>(a, d->B, st) : cpl_launch<11>(a, d->B, st);
}

}  // namespace vo

using namespace vo;

extern "C" int vo_conv1d_plane_takes(const vo_conv1d_desc* d) {
  if (!d || !d->x || !d->w || !d->y || !d->bias) return 0;
  if (d->variant != 1 || d->x_dtype != VO_BF16 || d->y_dtype != VO_BF16 || d->compute_dtype != VO_BF16) return 0;
  if (d->Ci != CPL_C || d->Co != CPL_C || d->ldx != CPL_C || d->ldy != CPL_C) return 0;
  if (!(d->K == 3 || d->K == 7 || d->K == 11) || d->dil < 1 || (d->K - 1) * d->dil > 64) return 0;
  if (2 * d->pad != (d->K - 1) * d->dil || d->T_out != d->T_in || d->T_in < 1 || d->B < 1) return 0;
  if (d->stride > 1 || d->groups > 1 || d->transposed || d->ymask || d->workspace || d->lens) return 0;
  // the prologue of c1 (leaky ReLU) or of c2 (none: Generator's c1 applies c2's leaky ReLU in its own epilogue)
  if (!(d->pre_act == VO_ACT_NONE || d->pre_act == VO_ACT_LRELU)) return 0;
  if (!(d->post_act == VO_ACT_NONE || d->post_act == VO_ACT_LRELU)) return 0;
  if (vo_tune_get("conv_cfg") != 0) return 0;
  // 16-byte rows, and every byte offset of an utterance (the window's rows past its end included) within 31 bits
  if (d->x_bstride % 8 != 0 || d->y_bstride % 8 != 0) return 0;
  if (((int64_t)d->T_in + CPL_WR) * CPL_C * 2 >= ((int64_t)1 << 31)) return 0;
  if ((int64_t)d->B * ((d->T_out + CPL_R - 1) / CPL_R) >= ((int64_t)1 << 31)) return 0;
  return 1;
}

#ifdef VO_CPL_STAMPS
// Diagnostic entry (tools/probes/cpl_stamps.py builds its own library with -DVO_CPL_STAMPS): one stamped launch of
// the descriptor; host_out receives CPL_NSTW workgroups x 4 waves x CPL_NPT stamps (0 start, 1 prologue done,
// 2 .. 9 chunk starts, 10 row-tile-major part, 11 loop end, 12 last epilogue done).
extern "C" int vo_cpl_stamps(const vo_conv1d_desc* d, unsigned long long* host_out) {
  if (!vo_conv1d_plane_takes(d)) return -1;
  const size_t n = (size_t)CPL_NSTW * 4 * CPL_NPT;
  unsigned long long* dev = nullptr;
  if (hipMalloc(&dev, n * 8) != hipSuccess) return -1;
  (void)hipMemset(dev, 0, n * 8);
  CplArgs a = cpl_args(d);
  a.stamps = dev;
  const dim3 grid((unsigned)(a.tiles_per_b * d->B));
  if (d->K == 3) hipLaunchKernelGGL((mrf_conv_plane_kernel<3, true>), grid, dim3(256), CPL_LDS, 0, a);
  else if (d->K == 7) hipLaunchKernelGGL((mrf_conv_plane_kernel<7, true>), grid, dim3(256), CPL_LDS, 0, a);
  else hipLaunchKernelGGL((mrf_conv_plane_kernel<11, true>), grid, dim3(256), CPL_LDS, 0, a);
  (void)hipDeviceSynchronize();
  (void)hipMemcpy(host_out, dev, n * 8, hipMemcpyDeviceToHost);
  (void)hipFree(dev);
  return 0;
}
#endif
