// HiFi-GAN ResBlock1 with kernel size 7 / 11 at C = 32 (MRF stage 3) -- the whole block (three (c1_d, c2)
// iterations, dilations (1, 3, 5)) in one launch, the k = 3 plane block of resblock_pb3.hip with a general tap loop:
//   x1 = x  + c2_0(lrelu(c1_1(lrelu x )))        (x1, x2 rounded to bf16 as between per-pair launches)
//   x2 = x1 + c2_1(lrelu(c1_3(lrelu x1)))
//   y  = (x2 + c2_2(lrelu(c1_5(lrelu x2)))) * out_scale (+ acc)
// (scripts/hifigan/models.py:96-103; the MRF sum and 1/num_kernels scale of models.py:155-160 ride in the
// last epilogue).
//
// Why.  As three vo_resblock_pair launches the block makes three passes over HBM (x -> x1 -> x2 -> y, 268 MB each
// way at B = 32) where the result needs one, and the C = 32 pairs are HBM-bound.  Here x1, x2 and the c1 outputs
// never leave the chip:
//   * one 32-channel plane; 4 waves, one per SIMD, wave w owns frame rows [256 w, 256 w + 256) in all six convs.
//     Its weights (2 KiB per tap) stream from L2 straight into its registers, R - 1 taps ahead (a ring of R = L + 2
//     tap slots): no weight goes through LDS, no tap needs a barrier;
//   * the activations are shared through LDS: the lrelu'd window (lrelu x, then lrelu x1, lrelu x2 written over
//     it) and c1's output T1.  6 barriers per tile (one per conv);
//   * a wave's P2 accumulators ARE the x_{s+1} rows of its row group, kept as bf16 in registers (the next P2's
//     residual, entered by identity MFMAs: exact) and written lrelu'd into the window for the next c1;
//   * every conv runs on the whole F = 1024-row frame; the valid rows shrink by the halos ((K-1)/2 (1+1+3+1+5+1) =
//     36 / 60 per side), so a tile yields 952 (k = 7) / 904 (k = 11) output rows;
//   * a conv's first K - L taps run tap by tap over the 16 row tiles (phase A); its last L taps run interleaved in
//     blocks of two row tiles (phase B), so that a block's accumulators are final after its 2 L steps and its
//     epilogue issues under the next block's MFMAs (the epilogues, not the MFMAs, bound the k = 3 block);
//   * LDS rows [row][32 ch] in the swizzle of plane_off (mrf_plane.h): the B-fragment reads at any row shift and
//     the T1 / window stores of the epilogues are bank-conflict free.
// Weights: [K][C_out][C_in] bf16 packs (vo_pack_weight); biases fp32.

#include <algorithm>
#include <cmath>
#include <type_traits>

#include "mrf_plane.h"

namespace vo {

struct PbkArgs {
  const bf16_t* x;
  const bf16_t* w[6];  // conv v = 2 s + ph: c1 of stage s (ph 0), c2 of stage s (ph 1)
  const float* b[6];
  bf16_t* y; const bf16_t* acc;
  int T, tiles_per_b, ntiles;
  float slope, out_scale;
  MrfLens rg;  // RAG instantiations: per-utterance lengths (mrf_common.h)
};

constexpr int PBK_C = 32, PBK_F = 1024, PBK_NJ = 16;  // channels, frame rows per tile, row tiles (16 rows) per wave
constexpr int pbk_h2(int K) { return (K - 1) / 2; }
constexpr int pbk_hp(int K) { return (pbk_h2(K) * 5 + 7) / 8 * 8; }  // LDS pad rows per side: the farthest tap (d = 5), a multiple of 8
constexpr int pbk_halo(int K) { return pbk_h2(K) * (1 + 1 + 3 + 1 + 5 + 1); }  // valid rows lost per side
constexpr int pbk_bt(int K) { return PBK_F - 2 * pbk_halo(K); }               // output rows per tile
constexpr int pbk_rp(int K) { return PBK_F + 2 * pbk_hp(K) + 1; }             // LDS rows per buffer
constexpr size_t pbk_lds(int K) { return (size_t)2 * pbk_rp(K) * 32 * sizeof(bf16_t) + 6 * PBK_C * sizeof(float); }

// RAG: ragged batch -- the workgroup walks the compacted tile list of MrfWalk, and utterance b's R_b rows stand where
// T does in the dense form (buffer ranges, zeroed frame rows, stored rows); T stays the row stride between utterances
template <int K, int ACC, bool RAG = false>
__global__ void __launch_bounds__(256, 1) mrf_pbk_kernel(PbkArgs a) {
  constexpr int C = PBK_C, F = PBK_F, NJ = PBK_NJ, H2 = pbk_h2(K), HP = pbk_hp(K), HALO = pbk_halo(K);
  constexpr int RP = pbk_rp(K), PL = RP * 32, BT = pbk_bt(K);
  constexpr int RPS = 64, NWV = F / RPS;       // window staging: rows per slot (256 threads x 16 B), slots
  constexpr int L = 4, KA = K - L;             // phase-B taps (interleaved with the epilogues), phase-A taps
  constexpr int R = L + 2;                     // A-fragment ring: tap u of the tile's 6 K in slot u % R
  constexpr int NU = 6 * K;                    // taps per tile
  constexpr int NB = 10, DB = 8;               // B-fragment ring / prefetch distance (steps)
  constexpr int BS = 2 * L;                    // phase-B block: L taps x 2 row tiles
  constexpr int NQ = K * NJ;                   // steps per conv
  constexpr int WT = KA - 2;                   // phase-A tap that carries the residual / next-window requests
  static_assert(NU % R == 0 && KA >= 3 && 2 * L <= NJ && NJ % 2 == 0 && HP >= 5 * H2 && HP % 8 == 0 && NWV == NJ, "geometry");

  const int T = a.T;
  const float slope = a.slope;

  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  bf16_t* win = reinterpret_cast<bf16_t*>(smem_raw);    // [RP][32]: lrelu x_s
  bf16_t* t1 = win + PL;                                 // [RP][32]: c1's output
  float* sbias = reinterpret_cast<float*>(t1 + PL);      // [6][C]

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int row0 = w * 16 * NJ;  // the wave's first frame row
  const int lr = lane & 15, lg = lane >> 4;

  MrfRun<RAG, BT> run(a.tiles_per_b, a.ntiles, T, a.rg);
  if (run.empty()) return;  // uniform per workgroup: the early exit is safe
  run.start();

  for (int i = tid; i < 6 * C; i += 256) sbias[i] = a.b[i / C][i % C];
  plane_zero_pads<2, HP, F, PL>(win, tid);

  // ---- A fragments (as resblock_rw.hip): lane l holds W[tap][co][ci], co = 8(lr>>2) + 4t + (lr&3), ci = 8lg .. +7;
  // accumulator register i of co tile t is then channel 8lg + 4t + i
  const int aoff = ((8 * (lr >> 2) + (lr & 3)) * C + 8 * lg) * (int)sizeof(bf16_t);
  __amdgpu_buffer_rsrc_t rw[6];
#pragma unroll
  for (int v = 0; v < 6; ++v) rw[v] = __builtin_amdgcn_make_buffer_rsrc((void*)a.w[v], (short)0, K * C * C * 2, 0x00020000);
  bf16x8 A[R][2];
  auto loadA_piece = [&](int u, int t) __attribute__((always_inline)) {
    const int uu = u % NU, v = uu / K, k = uu % K;
    A[uu % R][t] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rw[v], aoff + t * 4 * C * 2, k * (C * C * 2), 0));
  };

  auto utt = [&](const bf16_t* p, int b, int Tv) __attribute__((always_inline)) { return plane_utt<C>(p, b, T, Tv); };

  // ---- window staging: vector v = tid + 256 slot = (frame row xr + RPS slot, 16-byte column xc)
  const int xr = tid >> 2, xc = tid & 3;
  const int xl = plane_off(xr + HP, xc);  // + slot * RPS rows (swizzle unchanged)
  u32x4 xw[NWV];
  // the lane's byte offset of slot 0 in the window of tile nt (rswin: its utterance), opaque per tile: hoisted out of the
  // tile loop, the sixteen slot offsets (and those of the residual, accumulator and y rows below) stayed live
  // throughout, spilled, and every reload waited for vmcnt(0)
  __amdgpu_buffer_rsrc_t rswin;
  int wbase;
  auto win_tile = [&](int tl) __attribute__((always_inline)) {
    const MrfTile nt = run.at(tl);
    const int b = nt.b, p0 = nt.t0 - HALO;
    rswin = utt(a.x, b, nt.R);
    wbase = ((p0 + xr) * C + xc * 8) * 2;
    asm volatile("" : "+v"(wbase));
  };
  // positions before 0 wrap to huge offsets and past T exceed the range: both read 0 (zero padding)
  auto load_win = [&](int sl) __attribute__((always_inline)) {
    xw[sl] = __builtin_amdgcn_raw_buffer_load_b128(rswin, wbase + sl * (RPS * C * 2), 0, 0);
  };
  auto store_win = [&](int sl) __attribute__((always_inline)) { *reinterpret_cast<u32x4*>(win + xl + sl * RPS * 32) = lrelu8(xw[sl], slope); };

#pragma unroll
  for (int u = 0; u < R - L; ++u)
#pragma unroll
    for (int t = 0; t < 2; ++t) loadA_piece(u, t);
  win_tile(run.tile);
#pragma unroll
  for (int sl = 0; sl < NWV; ++sl) load_win(sl);
#pragma unroll
  for (int sl = 0; sl < NWV; ++sl) store_win(sl);

  f32x4 acc[2][NJ];
  bf16x8 Bq[NB];
  u32x4 xres[NJ];  // the wave's residual rows (x from HBM for stage 0, then x1, x2 from its own epilogues)
  u32x4 ares[NJ];
  bf16x8 aid[2], ais[2];  // identity A fragments (co tile t); ais scaled by 1 / out_scale (ACC == 2)
  plane_identity(aid, ais, lr, lg, a.out_scale);

  // One conv of the block over the frame.  Step q of the conv -> (tap, row tile): phase A (q < KA NJ) tap-major;
  // phase B in blocks of two row tiles, tap-major inside the block with the two row tiles alternating, so no MFMA
  // depends on the one just issued.  Each step: one B-fragment read (DB steps ahead), two MFMAs, and the side work:
  // A pieces (the ring is kept R - 1 taps ahead of the first unfinished tap: L taps' worth at a conv's tap 0, whose
  // predecessors -- the previous conv's phase B -- finished together, one tap's worth elsewhere), hook(k, jj) (k = KA:
  // phase B), and in phase B the previous block's epilogue in 8 parts.
  auto conv = [&](auto vc, auto hook, auto post, auto extra) __attribute__((always_inline)) {
    constexpr int V = decltype(vc)::value, PH = V & 1, S = V >> 1;
    constexpr int step = PH ? 1 : 2 * S + 1;
    const bf16_t* src = PH ? t1 : win;
    int lro = lr, lgo = lg;
    asm volatile("" : "+v"(lro), "+v"(lgo));
    auto dk = [&](int q) __attribute__((always_inline)) { return q < KA * NJ ? q / NJ : KA + ((q - KA * NJ) % BS) / 2; };
    auto dj = [&](int q) __attribute__((always_inline)) { return q < KA * NJ ? q % NJ : 2 * ((q - KA * NJ) / BS) + (q - KA * NJ) % 2; };
    auto readB = [&](int q) __attribute__((always_inline)) {
      const int k = dk(q), j = dj(q);
      Bq[q % NB] = *reinterpret_cast<const bf16x8*>(src + plane_off(HP + (k - H2) * step + row0 + lro, lgo) + j * 512);
    };
    const f32x4* bz = reinterpret_cast<const f32x4*>(sbias + V * C + 8 * lg);
    const f32x4 bz0 = bz[0], bz1 = bz[1];
#pragma unroll
    for (int q = 0; q < DB; ++q) readB(q);
    auto body = [&](int q, int k, int j) __attribute__((always_inline)) {
      const bf16x8 b = Bq[q % NB];
      const bf16x8(&Ak)[2] = A[(V * K + k) % R];
      if (k == 0) {
        acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ak[0], b, bz0, 0, 0, 0);
        acc[1][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ak[1], b, bz1, 0, 0, 0);
      } else {
        acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ak[0], b, acc[0][j], 0, 0, 0);
        acc[1][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ak[1], b, acc[1][j], 0, 0, 0);
      }
      extra(k, j);
    };
#pragma unroll
    for (int k = 0; k < KA; ++k) {
      const int first = V * K + k, lo = k == 0 ? first + R - L : first + R - 1, np = 2 * (first + R - lo);
#pragma unroll
      for (int jj = 0; jj < NJ; ++jj) {
        const int q = k * NJ + jj;
        if (q + DB < NQ) readB(q + DB);
        if (jj < np) loadA_piece(lo + jj / 2, jj % 2);
        hook(k, jj);
        __builtin_amdgcn_sched_barrier(0);
        body(q, k, jj);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
#pragma unroll
    for (int jj = 0; jj < L * NJ; ++jj) {
      const int q = KA * NJ + jj;
      const int k = dk(q), j = dj(q);
      if (q + DB < NQ) readB(q + DB);
      if (jj < 2) loadA_piece(V * K + KA + R - 1, jj);
      hook(KA, jj);
      __builtin_amdgcn_sched_barrier(0);
      body(q, k, j);
      if (jj >= BS) {  // the previous block's epilogue: 8 parts over this block's BS steps
        const int bb = jj / BS - 1, r = jj % BS;
#pragma unroll
        for (int p = 0; p < 8; ++p)
          if (r == p * BS / 8) post(2 * bb + p / 4, p % 4);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int p = 0; p < 8; ++p) post(NJ - 2 + p / 4, p % 4);
  };

  const int cofs = 8 * lg;
  for (; run.more(); run.advance()) {
    const MrfTile ti = run.enter();
    const int b = ti.b, t0 = ti.t0, Tv = ti.R;  // utterance, first output row, the utterance's valid rows
    const int ntile = run.succ();
    const int p0 = t0 - HALO;  // position of frame row 0
    const PlaneEdge edge(p0, F, Tv);  // the rows outside [0, Tv) of the wave's own row group are zeroed after each epilogue
    auto zero_rows = [&](bf16_t* buf) __attribute__((always_inline)) { edge.zero_rows<HP>(buf, row0, 16 * NJ, lane); };
    const __amdgpu_buffer_rsrc_t rsx = utt(a.x, b, Tv);
    const __amdgpu_buffer_rsrc_t rsa = utt(ACC ? a.acc : a.x, b, Tv);
    // byte offsets of the lane's 8 channels of row tile 0: in x / acc (frame row row0 + lr) and in y's tile range
    int rbase = ((p0 + row0 + lr) * C + cofs) * 2, ybase = ((row0 + lr - HALO) * C + cofs) * 2;
    asm volatile("" : "+v"(rbase), "+v"(ybase));

    lds_barrier();  // window staged; the previous tile's T1 reads are done

    uint32_t pv[4];
    // P1 epilogue: T1 = lrelu(acc) (bias in acc)
    auto p1_post = [&](int j, int p) __attribute__((always_inline)) {
      const int t = p >> 1, e = 2 * (p & 1);
      pv[p] = pk_bf16(lrelu_max(acc[t][j][e], slope), lrelu_max(acc[t][j][e + 1], slope));
      if (p == 3) {
        const int f = row0 + 16 * j + lr;
        *reinterpret_cast<u32x4*>(t1 + plane_off(f + HP, lg)) = u32x4{pv[0], pv[1], pv[2], pv[3]};
      }
    };
    // P2 epilogue of stages 0 / 1: x_{s+1} = bf16(acc) kept in xres; lrelu(x_{s+1}) into the window, taken from
    // the fp32 sum (as resblock3.hip's epilogues)
    uint32_t lv[4];
    auto p2_mid_post = [&](int j, int p) __attribute__((always_inline)) {
      const int e = 2 * p;
      const float a0 = acc[e >> 2][j][e & 3], a1 = acc[e >> 2][j][(e & 3) + 1];
      pv[p] = pk_bf16(a0, a1);
      lv[p] = pk_bf16(lrelu_max(a0, slope), lrelu_max(a1, slope));
      if (p == 3) {
        const int f = row0 + 16 * j + lr;
        xres[j] = u32x4{pv[0], pv[1], pv[2], pv[3]};
        *reinterpret_cast<u32x4*>(win + plane_off(f + HP, lg)) = u32x4{lv[0], lv[1], lv[2], lv[3]};
      }
    };
    // the residual through identity MFMAs at tap 0: the lane's residual vector of row tile j IS a B fragment
    auto res_extra = [&](int k, int j) __attribute__((always_inline)) {
      if (k != 0) return;
#pragma unroll
      for (int t = 0; t < 2; ++t)
        acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aid[t], __builtin_bit_cast(bf16x8, xres[j]), acc[t][j], 0, 0, 0);
    };
    auto no_hook = [&](int, int) __attribute__((always_inline)) {};
    auto no_extra = [&](int, int) __attribute__((always_inline)) {};

    // ---- stage 0, c1 over lrelu x; x's rows of this wave requested in phase-A tap WT after its A pieces (L2 hits:
    // the window staging just read them).  vmcnt retires in issue order: the A pieces requested in the next tap are
    // not needed before the conv after this one, so nothing waits on these loads before then
    auto s0_hook = [&](int k, int jj) __attribute__((always_inline)) {
      if (k != WT) return;
#pragma unroll
      for (int j = 0; j < NJ; ++j)
        if (plane_at(jj, 2, NJ - 2, NJ, j))
          xres[j] = __builtin_amdgcn_raw_buffer_load_b128(rsx, rbase + j * (16 * C * 2), 0, 0);
    };
    conv(std::integral_constant<int, 0>{}, s0_hook, p1_post, no_extra);
    zero_rows(t1);
    lds_barrier();
    conv(std::integral_constant<int, 1>{}, no_hook, p2_mid_post, res_extra);
    zero_rows(win);
    lds_barrier();
    conv(std::integral_constant<int, 2>{}, no_hook, p1_post, no_extra);
    zero_rows(t1);
    lds_barrier();
    conv(std::integral_constant<int, 3>{}, no_hook, p2_mid_post, res_extra);
    zero_rows(win);
    lds_barrier();

    // ---- stage 2: c1 requests the next tile's window (HBM misses) in phase-A tap WT, as the residual above
    auto s2a_hook = [&](int k, int jj) __attribute__((always_inline)) {
      if (k != WT) return;
#pragma unroll
      for (int sl = 0; sl < NWV; ++sl)
        if (plane_at(jj, 2, NJ - 2, NWV, sl)) load_win(sl);
    };
    win_tile(ntile);
    conv(std::integral_constant<int, 4>{}, s2a_hook, p1_post, no_extra);
    zero_rows(t1);
    lds_barrier();  // T1 complete; the window is dead until the next tile

    // ---- stage 2, c2: y = (x2 + c2) * out_scale (+ acc) -> HBM.  Phase A: the next window written lrelu'd, slot by
    // slot, and after each slot one row tile's MRF accumulator rows requested (NWV = NJ); the accumulator enters
    // at the last tap (identity MFMA, ACC == 2)
    const int valid = min(BT, Tv - t0);
    const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(a.y + ((int64_t)b * T + t0) * C), (short)0, valid * C * (int)sizeof(bf16_t), 0x00020000);
    auto s2b_hook = [&](int k, int jj) __attribute__((always_inline)) {
      if (k >= KA) return;
      const int g = k * NJ + jj;
#pragma unroll
      for (int sl = 0; sl < NWV; ++sl)
        if (plane_at(g, NJ / 2, KA * NJ - NJ / 2, NWV, sl)) {
          store_win(sl);
          if constexpr (ACC != 0)  // into the registers the window slot just left
            ares[sl] = __builtin_amdgcn_raw_buffer_load_b128(rsa, rbase + sl * (16 * C * 2), 0, 0);
        }
    };
    auto s2b_extra = [&](int k, int j) __attribute__((always_inline)) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        if (k == 0)
          acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aid[t], __builtin_bit_cast(bf16x8, xres[j]), acc[t][j], 0, 0, 0);
        if constexpr (ACC == 2)
          if (k == K - 1)
            acc[t][j] =__builtin_amdgcn_mfma_f32_16x16x32_bf16(ais[t], __builtin_bit_cast(bf16x8, ares[j]), acc[t][j], 0, 0, 0);
      }
    };
    const float osc = a.out_scale;
    auto s2b_post = [&](int j, int p) __attribute__((always_inline)) {
      const int e = 2 * p;
      pv[p] = pk_bf16(acc[e >> 2][j][e & 3] * osc, acc[e >> 2][j][(e & 3) + 1] * osc);
      if (p == 3)  // frame rows before the halo wrap to huge offsets, rows past `valid` exceed the range
        __builtin_amdgcn_raw_buffer_store_b128(u32x4{pv[0], pv[1], pv[2], pv[3]}, yrs, ybase + j * (16 * C * 2), 0, 0);
    };
    conv(std::integral_constant<int, 5>{}, s2b_hook, s2b_post, s2b_extra);
  }
}

template <int K, int ACC>
static int pbk_launch(PbkArgs a, int B, MrfTo st) {
  if (mrf_tile_rows_query(st, pbk_bt(K))) return VO_OK;
  a.tiles_per_b = (a.T + pbk_bt(K) - 1) / pbk_bt(K);
  a.ntiles = a.tiles_per_b * B;
  if (a.rg.lens) return mrf_launch(mrf_pbk_kernel<K, ACC, true>, a, a.ntiles, 256, pbk_lds(K), false, st);
  return mrf_launch(mrf_pbk_kernel<K, ACC, false>, a, a.ntiles, 256, pbk_lds(K), false, st);
}

}  // namespace vo

using namespace vo;

// Entry from vo_resblockk / vo_resblockk_lens: *handled = 1 when this kernel covers the call -- C = 32, K = 7 / 11,
// dilations (1, 3, 5), and an MRF accumulator only with 1 / out_scale a bf16 value (it enters through an identity MFMA)
int vo_rbk_pb_try(const MrfBlockCall& c, int* handled) {
  *handled = 0;
  if (c.C != PBK_C || !(c.K == 7 || c.K == 11)) return VO_OK;
  if (c.dil[0] != 1 || c.dil[1] != 3 || c.dil[2] != 5) return VO_OK;
  const int accm = mrf_acc_mode(c.acc, c.out_scale);
  if (accm == 1) return VO_OK;
  if ((int64_t)c.T * PBK_C * 2 > 0x7fffffff) return VO_OK;  // an utterance is one buffer range
  PbkArgs a;
  mrf_block_args(a, c);
  *handled = 1;
  if (c.K == 7) return accm == 2 ? pbk_launch<7, 2>(a, c.B, c.st) : pbk_launch<7, 0>(a, c.B, c.st);
  return accm == 2 ? pbk_launch<11, 2>(a, c.B, c.st) : pbk_launch<11, 0>(a, c.B, c.st);
}

// vo_resblockk (lens == nullptr) and vo_resblockk_lens
static int resblockk_entry(const void* x, const void* const* w1, const float* const* b1, const void* const* w2,
                           const float* const* b2, int K, const int* dil, void* y, const void* acc, int B, int T, int C,
                           float slope, float out_scale, MrfTo st, const int32_t* lens, int lens_scale) {
  const MrfBlockCall c{x, w1, b1, w2, b2, dil, y, acc, B, T, C, K, slope, out_scale, st, lens, lens_scale};
  if (const int rc = vo_block_check(c, "resblockk")) return rc;
  VO_CHECK_ARG(K % 2 == 1 && K >= 1 && K <= 15, "resblockk: K=%d unsupported (odd K <= 15)", K);
  for (int s = 0; s < 3; ++s)
    VO_CHECK_ARG(dil[s] >= 1 && dil[s] * (K - 1) <= 64, "resblockk: dilation %d unsupported ((K-1)*dil <= 64)", dil[s]);
  int handled = 0;
  const int rc = vo_rbk_pb_try(c, &handled);
  return handled ? rc : VO_NOT_HANDLED;
}

extern "C" int vo_resblockk(const void* x, const void* const* w1, const float* const* b1, const void* const* w2,
                            const float* const* b2, int K, const int* dil, void* y, const void* acc, int B, int T, int C,
                            float slope, float out_scale, void* stream) {
  return resblockk_entry(x, w1, b1, w2, b2, K, dil, y, acc, B, T, C, slope, out_scale,
                         reinterpret_cast<hipStream_t>(stream), nullptr, 0);
}

extern "C" int vo_resblockk_lens(const void* x, const void* const* w1, const float* const* b1, const void* const* w2,
                                 const float* const* b2, int K, const int* dil, void* y, const void* acc, int B, int T,
                                 int C, float slope, float out_scale, void* stream, const int32_t* lens, int lens_scale) {
  VO_CHECK_ARG(lens && lens_scale >= 1, "resblockk_lens: lens is null or lens_scale %d < 1", lens_scale);
  return resblockk_entry(x, w1, b1, w2, b2, K, dil, y, acc, B, T, C, slope, out_scale,
                         reinterpret_cast<hipStream_t>(stream), lens, lens_scale);
}

// Host-only: output rows per tile of the kernel that vo_resblockk launches for K (0: none) -- its dispatch run as a
// tile-rows query, as vo_resblock3_tile_rows (resblock3.hip): placeholder operands that are compared and copied, never
// read through
extern "C" int vo_resblockk_tile_rows(int K) {
  static const char in = 0;
  static char out = 0;
  const float* const fb = reinterpret_cast<const float*>(&in);
  const void* const w[3] = {&in, &in, &in};
  const float* const b[3] = {fb, fb, fb};
  const int dil[3] = {1, 3, 5};
  int rows = 0;
  if (resblockk_entry(&in, w, b, w, b, K, dil, &out, nullptr, 1, 1, 32, 0.1f, 1.0f, MrfTo(nullptr, &rows), nullptr, 0) != VO_OK)
    return 0;
  return rows;
}
