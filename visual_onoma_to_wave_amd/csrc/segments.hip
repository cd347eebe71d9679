// HiFi-GAN training batches on the device: aligned (mel, audio) segments cut from the packed
// corpus (vo_corpus) and the waveforms beside it (vo_wave_corpus) by a plan of two integers per row, and the draw of
// that plan from a counter in device memory, so that a captured training step replays with its batch.
//
// The reference trains no vocoder; the host code this replaces is HiFi-GAN's MelDataset (fine-tuning branch: the mel
// from file, the audio cropped at mel_start * hop, both zero-padded to the segment), random.randint per item and one
// host-to-device copy per step.  include/vonoma.h states the rules.  Nothing is summed: every output is a copy or one
// IEEE division, so the numpy model of the tests is matched bit for bit.
//
// vo_segment_batch is one grid for the whole batch as augment_batch_kernel, blockIdx.y = plan row.  Along x: the
// row's samples in groups of SEG_SAMPLES, then its frames in groups of SEG_FRAMES.  Every workgroup decodes its plan
// row itself (six uniform loads).  A segment is one contiguous run of the corpus in both tensors, so a workgroup's
// part is a prefix that is copied and a suffix that is padding.

#include "vo_common.h"

namespace vo {

constexpr int SEG_SAMPLES = 2048;  // samples of one workgroup: 8 to a lane, 8 KB of y
constexpr int SEG_FRAMES = 64;     // mel frames of one workgroup: 20 KB of an 80-bin mel
constexpr int SEG_UNROLL = 4;      // 16-byte mel vectors a lane has in flight

// A decoded plan row.  Refused rows have ns = nf = 0: every consumer then writes padding and reads nothing.
struct SegRow {
  int status, nf;   // frames to copy: min(fps, F - start)
  int64_t ns;       // samples to copy: min(fps hop, max(N - start hop, 0))
  int64_t so, fo;   // first sample of the segment in wav, first frame in mel
};

// The plan is device data nobody has checked: src and start are bounded before anything is indexed with them, and an
// accepted row has start <= F, so start hop < 2^62 and every product is formed in 64 bits.
__device__ __forceinline__ SegRow seg_row(const vo_corpus& c, const vo_wave_corpus& w, const int32_t* __restrict__ plan,
                                          int b, int fps, int hop) {
  SegRow r = {};
  r.status = VO_SEG_BAD_ROW;
  const int src = plan[(int64_t)b * 2], start = plan[(int64_t)b * 2 + 1];
  if (src < 0 || src >= c.U || start < 0) return r;
  const int64_t fo = c.frame_off[src], F = c.frame_off[src + 1] - fo;
  if (start > (F > fps ? F - fps : 0)) return r;
  const int64_t s0 = (int64_t)start * hop, left = w.n_samples[src] - s0, L = (int64_t)fps * hop;
  r.status = VO_SEG_OK;
  r.nf = (int)(F - start < fps ? F - start : fps);
  r.ns = left < 0 ? 0 : (left < L ? left : L);
  r.so = w.sample_off[src] + s0;
  r.fo = fo + start;
  return r;
}

__device__ __forceinline__ float seg_sample(const int16_t* p, float mwv) { return __fdiv_rn((float)*p, mwv); }
__device__ __forceinline__ float seg_sample(const float* p, float) { return *p; }

// the eight samples of a lane whose source is 16-byte (int16) or 32-byte (fp32) aligned and wholly inside the utterance
__device__ __forceinline__ void seg_load8(const int16_t* p, float mwv, float4& a, float4& b) {
  const uint4 v = *reinterpret_cast<const uint4*>(p);
  const uint32_t q[4] = {v.x, v.y, v.z, v.w};
  float f[8];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    f[2 * k] = __fdiv_rn((float)(int16_t)(q[k] & 0xffffu), mwv);
    f[2 * k + 1] = __fdiv_rn((float)(int16_t)(q[k] >> 16), mwv);
  }
  a = make_float4(f[0], f[1], f[2], f[3]);
  b = make_float4(f[4], f[5], f[6], f[7]);
}
__device__ __forceinline__ void seg_load8(const float* p, float, float4& a, float4& b) {
  a = reinterpret_cast<const float4*>(p)[0];
  b = reinterpret_cast<const float4*>(p)[1];
}

// T: the corpus's sample type.  VECY: hop % 8 == 0 and wav, y 16-byte aligned; VECX: n_mels % 4 == 0 and mel, x
// 16-byte aligned (the launcher).
template <typename T, bool VECY, bool VECX>
__global__ void __launch_bounds__(256) segment_batch_kernel(vo_corpus c, vo_wave_corpus w,
                                                            const int32_t* __restrict__ plan, int fps, int hop,
                                                            float mel_pad, int wave_blocks, float* __restrict__ y,
                                                            float* __restrict__ x, int32_t* __restrict__ frames,
                                                            int32_t* __restrict__ status) {
  const int b = blockIdx.y, tid = threadIdx.x;
  int blk = blockIdx.x;
  const SegRow r = seg_row(c, w, plan, b, fps, hop);

  if (blk < wave_blocks) {
    const int64_t L = (int64_t)fps * hop;  // < 2^31 (launcher)
    const T* src = static_cast<const T*>(w.wav) + r.so;
    float* dst = y + (int64_t)b * L;
    const float mwv = w.max_wav_value;
    if (VECY) {
      // L, r.so and b L are multiples of 8: a lane's eight samples are wholly inside the row or wholly past it, and
      // its vectors are aligned.  Only the group that straddles the utterance's end goes sample by sample.
      const int64_t i = (int64_t)blk * SEG_SAMPLES + tid * 8;
      if (i < L) {
        float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;
        if (i + 8 <= r.ns) {
          seg_load8(src + i, mwv, lo, hi);
        } else if (i < r.ns) {
          float f[8];
#pragma unroll
          for (int k = 0; k < 8; ++k) f[k] = i + k < r.ns ? seg_sample(src + i + k, mwv) : 0.f;
          lo = make_float4(f[0], f[1], f[2], f[3]);
          hi = make_float4(f[4], f[5], f[6], f[7]);
        }
        reinterpret_cast<float4*>(dst + i)[0] = lo;
        reinterpret_cast<float4*>(dst + i)[1] = hi;
      }
    } else {
      float f[SEG_SAMPLES / 256];
#pragma unroll
      for (int k = 0; k < SEG_SAMPLES / 256; ++k) {
        const int64_t i = (int64_t)blk * SEG_SAMPLES + k * 256 + tid;
        f[k] = i < r.ns ? seg_sample(src + i, mwv) : 0.f;
      }
#pragma unroll
      for (int k = 0; k < SEG_SAMPLES / 256; ++k) {
        const int64_t i = (int64_t)blk * SEG_SAMPLES + k * 256 + tid;
        if (i < L) dst[i] = f[k];
      }
    }
    if (blk == 0 && tid == 0) {
      frames[b] = r.nf;
      status[b] = r.status;
    }
    return;
  }
  blk -= wave_blocks;

  // the frames f0 .. f0 + nf of the row, as one run of nf n_mels floats of which the first nc are the corpus's
  const int n_mels = c.n_mels;
  const int f0 = blk * SEG_FRAMES, nf = min(SEG_FRAMES, fps - f0);
  const int n = nf * n_mels, nc = min(max(r.nf - f0, 0), nf) * n_mels;  // fps n_mels < 2^31 (launcher)
  const float* src = c.mel + (r.fo + f0) * n_mels;
  float* dst = x + ((int64_t)b * fps + f0) * n_mels;
  if (VECX) {
    // SEG_UNROLL vectors of a lane are loaded before the first is stored, as augment_batch_kernel does
    const int nv = n >> 2, ncv = nc >> 2;
    for (int i0 = tid; i0 < nv; i0 += SEG_UNROLL * 256) {
      float4 v[SEG_UNROLL];
#pragma unroll
      for (int k = 0; k < SEG_UNROLL; ++k) {
        const int i = i0 + k * 256;
        v[k] = make_float4(mel_pad, mel_pad, mel_pad, mel_pad);
        if (i < ncv) v[k] = reinterpret_cast<const float4*>(src)[i];
      }
#pragma unroll
      for (int k = 0; k < SEG_UNROLL; ++k)
        if (i0 + k * 256 < nv) reinterpret_cast<float4*>(dst)[i0 + k * 256] = v[k];
    }
  } else {
    for (int i = tid; i < n; i += 256) dst[i] = i < nc ? src[i] : mel_pad;
  }
}

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC 2011), word 0 of the
// output.  The key is bumped before every round but the first.
__device__ __forceinline__ uint32_t philox4x32_10_w0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                     uint32_t k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c0;
}

// One workgroup.  Every lane reads the counter, the barrier orders those reads before the one store that advances it.
__global__ void __launch_bounds__(256) segment_plan_kernel(vo_corpus c, const int32_t* __restrict__ order, int n_order,
                                                           int64_t* counter, uint64_t seed, int B, int fps,
                                                           int32_t* __restrict__ plan) {
  const uint64_t k0 = (uint64_t)*counter;
  __syncthreads();
  for (int b = threadIdx.x; b < B; b += 256) {
    const uint64_t k = k0 + (uint64_t)b;
    const int src = order[k % (uint64_t)n_order];
    int start = 0;
    if (src >= 0 && src < c.U) {
      const int64_t F = c.frame_off[src + 1] - c.frame_off[src];
      int64_t span = F > fps ? F - fps + 1 : 1;
      if (span > ((int64_t)1 << 31)) span = (int64_t)1 << 31;  // start is an int32
      const uint32_t w = philox4x32_10_w0((uint32_t)k, (uint32_t)(k >> 32), 0u, 0u, (uint32_t)seed,
                                          (uint32_t)(seed >> 32));
      start = (int)(((uint64_t)w * (uint64_t)span) >> 32);
    }
    plan[2 * b] = src;
    plan[2 * b + 1] = start;
  }
  if (threadIdx.x == 0) *counter = (int64_t)(k0 + (uint64_t)B);
}

template <typename T>
static void launch_segment_batch(bool vecy, bool vecx, dim3 grid, hipStream_t st, const vo_corpus& c,
                                 const vo_wave_corpus& w, const int32_t* plan, int fps, int hop, float mel_pad,
                                 int wave_blocks, float* y, float* x, int32_t* frames, int32_t* status) {
  with_bool(vecy, [&](auto vy) {
    return with_bool(vecx, [&](auto vx) {
      hipLaunchKernelGGL((segment_batch_kernel<T, decltype(vy)::value, decltype(vx)::value>), grid, dim3(256), 0, st, c,
                         w, plan, fps, hop, mel_pad, wave_blocks, y, x, frames, status);
      return 0;
    });
  });
}

}  // namespace vo

using namespace vo;

extern "C" int vo_segment_batch(const vo_corpus* c, const vo_wave_corpus* w, const int32_t* plan, int B, int fps,
                                int hop, float mel_pad, float* y, float* x, int32_t* frames, int32_t* status,
                                void* stream) {
  VO_CHECK_ARG(c && w && plan && y && x && frames && status, "segment_batch: null pointer");
  VO_CHECK_ARG(c->frame_off && c->mel, "segment_batch: null pointer in the corpus");
  VO_CHECK_ARG(w->sample_off && w->n_samples && w->wav, "segment_batch: null pointer in the wave corpus");
  VO_CHECK_ARG(c->U > 0 && c->n_mels > 0, "segment_batch: empty corpus");
  VO_CHECK_ARG(w->U == c->U, "segment_batch: the wave corpus has %d utterances, the corpus %d", (int)w->U, (int)c->U);
  VO_CHECK_ARG(B >= 1 && B <= 65535, "segment_batch: B %d is outside [1, 65535]", B);
  VO_CHECK_ARG(fps >= 1 && hop >= 1, "segment_batch: fps %d and hop %d must be >= 1", fps, hop);
  VO_CHECK_ARG((int64_t)fps * hop < ((int64_t)1 << 31) && (int64_t)fps * c->n_mels < ((int64_t)1 << 31),
               "segment_batch: a row of fps hop = %lld samples or fps n_mels = %lld values is at or above 2^31",
               (long long)fps * hop, (long long)fps * c->n_mels);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int wave_blocks = (int)(((int64_t)fps * hop + SEG_SAMPLES - 1) / SEG_SAMPLES);
  const int mel_blocks = (fps + SEG_FRAMES - 1) / SEG_FRAMES;
  const dim3 grid((unsigned)(wave_blocks + mel_blocks), (unsigned)B);
  const bool vecy = hop % 8 == 0 && (reinterpret_cast<uintptr_t>(w->wav) | reinterpret_cast<uintptr_t>(y)) % 16 == 0;
  const bool vecx =
      c->n_mels % 4 == 0 && (reinterpret_cast<uintptr_t>(c->mel) | reinterpret_cast<uintptr_t>(x)) % 16 == 0;
  if (w->is_int16)
    launch_segment_batch<int16_t>(vecy, vecx, grid, st, *c, *w, plan, fps, hop, mel_pad, wave_blocks, y, x, frames,
                                  status);
  else
    launch_segment_batch<float>(vecy, vecx, grid, st, *c, *w, plan, fps, hop, mel_pad, wave_blocks, y, x, frames,
                                status);
  VO_RETURN_LAUNCH();
}

extern "C" int vo_segment_plan(const vo_corpus* c, const int32_t* order, int n_order, int64_t* counter, uint64_t seed,
                               int B, int fps, int32_t* plan, void* stream) {
  VO_CHECK_ARG(c && order && counter && plan, "segment_plan: null pointer");
  VO_CHECK_ARG(c->frame_off, "segment_plan: null pointer in the corpus");
  VO_CHECK_ARG(c->U > 0, "segment_plan: empty corpus");
  VO_CHECK_ARG(n_order >= 1, "segment_plan: n_order %d must be >= 1", n_order);
  VO_CHECK_ARG(B >= 1 && B <= 65535, "segment_plan: B %d is outside [1, 65535]", B);
  VO_CHECK_ARG(fps >= 1, "segment_plan: fps %d must be >= 1", fps);
  hipLaunchKernelGGL(segment_plan_kernel, dim3(1), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), *c, order,
                     n_order, counter, seed, B, fps, plan);
  VO_RETURN_LAUNCH();
}
