// The scaffold of the "wave-owned output planes" MRF kernels (resblock_rw.hip, resblock_pb3.hip, resblock_pbk.hip):
// the layouts and algorithms the three must agree on, each defined once -- the LDS row swizzle, the identity MFMA
// fragments, an utterance's buffer range, the pad rows and the zeroed edge rows of a frame, the step spreader.  (The
// workgroup's tile run, MrfRun, is beside MrfWalk in mrf_common.h.)  The conv() step schedules are each kernel's own.
#pragma once

#include "mrf_common.h"

namespace vo {

// LDS rows of 64 B, [plane][row][32 ch]: 16-byte chunk q of row r sits at chunk q ^ ((r >> 1) & 3).  The B-fragment
// reads (16 rows x 4 chunks at ANY row offset -- the taps shift rows by k * dil), the 16-byte stores of the epilogues
// (T1, the window) and the window staging stores (odd plane stride in rows) are all bank-conflict free: checked
// exhaustively over the lane groups of ds_read_b128 / ds_write_b128 (MI355X_MICROARCH.md section LDS).  The swizzle
// has period 8 in r: a row offset that is a multiple of 8 (the pad rows, a staging slot) leaves it unchanged.
__device__ __forceinline__ int plane_off(int r, int q) { return r * 32 + 8 * (q ^ ((r >> 1) & 3)); }

// Identity A fragments (co tile t) of lane (lr = lane & 15, lg = lane >> 4): 1 at k = 4t + (lr & 3) of the lane's 8
// when lr / 4 == lg, so that an MFMA with a lane's own 8-channel row vector as B adds it to the accumulator rows that
// hold those channels (exact: products of 1 and bf16, fp32 accumulation).  ais carries 1 / out_scale instead of 1
// (ACC == 2: exact by the launcher's check, mrf_acc_mode)
__device__ __forceinline__ void plane_identity(bf16x8 (&aid)[2], bf16x8 (&ais)[2], int lr, int lg, float out_scale) {
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const bool one = (lr >> 2) == lg && e == 4 * t + (lr & 3);
      aid[t][e] = (__bf16)(one ? 1.0f : 0.0f);
      ais[t][e] = (__bf16)(one ? 1.0f / out_scale : 0.0f);
    }
}

// Buffer resource of rows [0, Tv) of utterance b of a (B, T, C) bf16 tensor: loads of rows outside read 0 (the convs'
// zero padding; positions before 0 wrap to huge offsets) with no clamp, and 32-bit lane offsets address it (a 64-bit
// address per load kept 2 VGPRs live each and spilled).  The kernels call it through a local lambda that binds T.
template <int C>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t plane_utt(const bf16_t* p, int b, int T, int Tv) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)(p + (int64_t)b * T * C), (short)0, Tv * C * 2, 0x00020000);
}

// op i of n spread over the steps [lo, lo + span) of a tap or phase: does step jj carry it?
__device__ __forceinline__ constexpr bool plane_at(int jj, int lo, int span, int n, int i) { return jj == lo + i * span / n; }

// Frames of the whole-block kernels: NBUF plane buffers of PL elements, each HP pad rows, F frame rows, HP + 1 pad rows.
// The pad rows are read only by taps of frame rows whose outputs the halo discards: zeros, never NaN (once per kernel)
template <int NBUF, int HP, int F, int PL>
__device__ __forceinline__ void plane_zero_pads(bf16_t* bufs, int tid) {
  for (int i = tid; i < NBUF * (2 * HP + 1) * 4; i += 256) {
    const int q = i & 3, r0 = (i >> 2) % (2 * HP + 1), pb = (i >> 2) / (2 * HP + 1);
    const int r = r0 < HP ? r0 : F + r0;
    *reinterpret_cast<u32x4*>(bufs + pb * PL + plane_off(r, q)) = u32x4{0u, 0u, 0u, 0u};
  }
}

// Zero padding at an utterance's ends in the whole-block kernels: the epilogues write every frame row unmasked (a mask
// per row tile cost 5 of its ~38 vector instructions, in the VALU-bound epilogue phase; a branch around it made hipcc
// copy eight accumulators out of the AGPRs at every join); in the tiles whose frame (F rows from position p0) crosses
// an end of the utterance's Tv rows, a wave zeroes the rows outside [0, Tv) of what it owns after the epilogue, before
// the barrier that publishes them.  (Parameters by reference, as the kernels' lambdas capture: by value the plane
// kernels came out with more registers and instructions.)
struct PlaneEdge {
  bool edge;
  int zlo, zhi;  // frame rows [zlo, zhi) are inside the utterance
  __device__ __forceinline__ PlaneEdge(const int& p0, const int& F, const int& Tv)
      : edge(p0 < 0 || p0 + F > Tv), zlo(p0 < 0 ? -p0 : 0), zhi(Tv - p0) {}
  // the wave's frame rows [row0, row0 + n) of one plane buffer (HP pad rows before frame row 0)
  template <int HP>
  __device__ __forceinline__ void zero_rows(bf16_t* plane, const int& row0, const int& n, const int& lane) const {
    if (!edge) return;
    for (int f = row0 + lane; f < row0 + n; f += 64)
      if (f < zlo || f >= zhi)
#pragma unroll
        for (int q = 0; q < 4; ++q) *reinterpret_cast<u32x4*>(plane + plane_off(f + HP, q)) = u32x4{0u, 0u, 0u, 0u};
  }
};

}  // namespace vo
