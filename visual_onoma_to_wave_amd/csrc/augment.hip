// Repeat and consecutive augmentation on the device: the padded training batch written in
// one launch from a base corpus packed once (vo_corpus) and a plan of five integers per utterance.
//
// Reference (host, per variant, through files):
//   Preprocessor._augmentation / _repeataug / _consecutiveaug (scripts/preprocessor/preprocessor.py:468-622): np.tile
//     and np.insert over text, duration, energy, kurtosis, widths and mel, PIL crops and pastes of the strip, one
//     .npy per array and a PNG per variant;
//   Dataset.__getitem__ + reprocess (scripts/dataset.py): np.load of each, pad_1D / pad_2D, and the glyph layout
//     of glyph.hip.
// Both augmentations are index maps (include/vonoma.h states them): an output character is a base character, an
// output frame a base frame, an output pixel a base pixel or white.  Nothing is summed or rounded, so every output
// equals the reference's files bit for bit.
//
// One grid for the whole batch, blockIdx.y = plan row.  Along x: the row's mel in groups of AUG_FRAMES frames, then
// its image in groups of AUG_PIX pixels, then one workgroup for the per-character tensors and the row's scalars.
// Every workgroup decodes its plan row itself (a dozen uniform loads): no scan, no second launch.

#include "vo_common.h"

namespace vo {

constexpr int AUG_FRAMES = 64;  // mel frames of one workgroup: 20 KB of an 80-bin mel
constexpr int AUG_PIX = 1024;   // image pixels of one workgroup, 4 to a lane at a stride of 256
constexpr int AUG_UNROLL = 4;   // 16-byte mel vectors a lane has in flight

struct AugOut {
  int64_t *audiotypes, *texts, *src_lens;
  float *mels, *mel_lens, *energies, *kurtosises, *durations, *images;
  int32_t* status;
};

// A decoded plan row.  Refused rows have L = FL = 0: every consumer then writes padding and reads nothing.
struct AugRow {
  int status, src;
  int co, n1, L, pos, m;     // first character of src, n', characters out
  int spos, d, md, F1, FL;   // s_pos, d[pos], m_mel d[pos], F', frames out
  float rn1;                 // 1 / n'
  int64_t fo, po;            // first frame of src, first pixel of its strip
  int sw;
};

// The refusal rules of vonoma.h, in their order.  The plan is device data nobody has checked: the products are
// formed in 64 bits and each factor is bounded before the next product, so no value of a row overflows, and an
// accepted row indexes inside the corpus (sigma < n, phi < F).
__device__ __forceinline__ AugRow aug_row(const vo_corpus& c, const int32_t* __restrict__ plan, int b, int T_src,
                                          int T_mel) {
  AugRow r = {};
  const int32_t* p = plan + (int64_t)b * 5;
  const int src = p[0], pos = p[1], m = p[2], mm = p[3], rep = p[4];
  r.status = VO_AUG_BAD_ROW;
  if (src < 0 || src >= c.U || m < 0 || mm < 0 || rep < 1) return r;
  const int co = c.char_off[src], n = c.char_off[src + 1] - co;
  if (pos < 0 || pos >= n) return r;
  const int64_t n1 = (int64_t)n + m;  // >= 1
  r.status = VO_AUG_CHARS_OVER;
  if (n1 > T_src || n1 * rep > T_src) return r;  // rep <= T_src from here
  const int64_t fo = c.frame_off[src];
  const int64_t F = c.frame_off[src + 1] - fo;
  const int d = c.ch_dur[co + pos];
  const int64_t F1 = F + (int64_t)mm * d;
  r.status = VO_AUG_FRAMES_OVER;
  if (F1 > T_mel || F1 * rep > T_mel) return r;  // m_mel d <= T_mel from here
  r.status = VO_AUG_OK;
  r.src = src;
  r.co = co, r.n1 = (int)n1, r.L = (int)(n1 * rep), r.pos = pos, r.m = m;
  r.rn1 = 1.0f / (float)r.n1;
  r.spos = c.ch_dstart[co + pos], r.d = d, r.md = (int)((int64_t)mm * d), r.F1 = (int)F1, r.FL = (int)(F1 * rep);
  r.fo = fo, r.po = c.px_off[src], r.sw = c.strip_w[src];
  return r;
}

// base character of output character j < L, from j' = j mod n'
__device__ __forceinline__ int aug_sigma(const AugRow& r, int jp) {
  return r.co + (jp < r.pos ? jp : (jp <= r.pos + r.m ? r.pos : jp - r.m));
}

// a / d, and a % d in rem, for 0 <= a < 2^22, 1 <= d < 2^22 and rd = 1.0f / d.  a is exact in a float, rd and the
// product are each within 2^-24 of theirs, so the estimate is within 2^22 * 2^-22.9 < 1 of a / d: truncated it is the
// quotient or a neighbour, and one step either way settles it (an rd the device divided itself may be an ulp off: the
// dividends it meets, character indices, are below 2^21).  An integer division by a value the compiler does not
// know is some thirty instructions and the image pass did three per pixel: 10.9 -> 10.2 us per 48-row batch (DESIGN.md
// section 14).
__device__ __forceinline__ int div22(int a, int d, float rd, int& rem) {
  int q = (int)((float)a * rd);
  int r = a - q * d;
  if (r < 0) {
    --q;
    r += d;
  } else if (r >= d) {
    ++q;
    r -= d;
  }
  rem = r;
  return q;
}

// base frame of output frame f < FL.  d = 0 leaves the middle range empty (q < md + d is q < 0): no division.
__device__ __forceinline__ int aug_phi(const AugRow& r, int f) {
  int fp = f % r.F1;
  if (fp >= r.spos) {
    const int q = fp - r.spos;
    fp = q < r.md + r.d ? r.spos + q % r.d : fp - r.md;
  }
  return fp;
}

template <bool VEC>
__global__ void __launch_bounds__(256) augment_batch_kernel(vo_corpus c, const int32_t* __restrict__ plan, int T_src,
                                                            int T_mel, int H, int cell, int margin, int W_out,
                                                            float rcell, float rW, int mel_blocks, int img_blocks,
                                                            AugOut o) {
  __shared__ int srcf[AUG_FRAMES];
  const int b = blockIdx.y, tid = threadIdx.x;
  int blk = blockIdx.x;
  const AugRow r = aug_row(c, plan, b, T_src, T_mel);

  if (blk < mel_blocks) {
    // phi once per frame, by the first lanes; then the frames move as rows of n_mels floats, the workgroup's
    // output one contiguous run
    const int f0 = blk * AUG_FRAMES, nf = min(AUG_FRAMES, T_mel - f0);
    if (tid < nf) srcf[tid] = f0 + tid < r.FL ? aug_phi(r, f0 + tid) : -1;
    __syncthreads();
    const int n_mels = c.n_mels;
    float* dst = o.mels + ((int64_t)b * T_mel + f0) * n_mels;
    const float* src = c.mel + r.fo * n_mels;
    if (VEC) {
      // AUG_UNROLL vectors of a lane are loaded before the first is stored: the output may alias the corpus as
      // far as the compiler knows, and a rolled loop waits for each load before the next is issued
      const int V = n_mels >> 2, nv = nf * V;
      for (int i0 = tid; i0 < nv; i0 += AUG_UNROLL * 256) {
        float4 x[AUG_UNROLL];
#pragma unroll
        for (int k = 0; k < AUG_UNROLL; ++k) {
          const int i = i0 + k * 256;
          x[k] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (i < nv) {
            const int fr = i / V, s = srcf[fr];
            if (s >= 0) x[k] = reinterpret_cast<const float4*>(src + (int64_t)s * n_mels)[i - fr * V];
          }
        }
#pragma unroll
        for (int k = 0; k < AUG_UNROLL; ++k)
          if (i0 + k * 256 < nv) reinterpret_cast<float4*>(dst)[i0 + k * 256] = x[k];
      }
    } else {
      for (int i = tid; i < nf * n_mels; i += 256) {
        const int fr = i / n_mels, v = i - fr * n_mels, s = srcf[fr];
        dst[i] = s >= 0 ? src[(int64_t)s * n_mels + v] : 0.f;
      }
    }
    return;
  }
  blk -= mel_blocks;

  if (blk < img_blocks) {
    // per output pixel as glyph_batch_kernel, over the row's H x W_out pixels as one run
    const int npx = H * W_out;
    float* img = o.images + (int64_t)b * npx;
    const uint8_t* strip = c.px + r.po;
    // in three passes over the lane's pixels, so that their loads are in flight together: the characters' widths
    // and columns, then the pixels' bytes, then the stores
    constexpr int K = AUG_PIX / 256;
    const int i0 = blk * AUG_PIX, y0 = i0 / W_out, x0 = i0 - y0 * W_out;  // uniform: one division a workgroup
    int y[K], cc[K], ch[K], len[K], col[K], v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      int x, jp;
      y[k] = y0 + div22(x0 + k * 256 + tid, W_out, rW, x);  // x0 + 1023 < 2^22 (launcher)
      ch[k] = -1;
      len[k] = col[k] = cc[k] = 0;
      if (i0 + k * 256 + tid < npx && x >= margin) {
        const int j = div22(x - margin, cell, rcell, cc[k]);
        if (j < r.L) {
          div22(j, r.n1, r.rn1, jp);
          ch[k] = aug_sigma(r, jp);
          len[k] = c.ch_width[ch[k]];
          col[k] = c.ch_col[ch[k]];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int pleft = (cell - len[k]) / 2 + (cell - len[k]) % 2;
      const int sc = cc[k] - pleft;
      v[k] = 255;
      if (ch[k] >= 0 && sc >= 0 && sc < len[k]) v[k] = strip[(int64_t)y[k] * r.sw + col[k] + sc];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int i = blk * AUG_PIX + k * 256 + tid;
      if (i < npx) img[i] = __fdiv_rn((float)v[k], 255.f);
    }
    return;
  }

  for (int j = tid; j < T_src; j += 256) {
    int64_t id = 0;
    float du = 0.f, en = 0.f, ku = 0.f;
    if (j < r.L) {
      const int ch = aug_sigma(r, j % r.n1);
      id = c.ch_id[ch];
      du = (float)c.ch_dur[ch];
      if (o.energies) en = c.ch_energy[ch];
      if (o.kurtosises) ku = c.ch_kurtosis[ch];
    }
    const int64_t at = (int64_t)b * T_src + j;
    o.texts[at] = id;
    o.durations[at] = du;
    if (o.energies) o.energies[at] = en;
    if (o.kurtosises) o.kurtosises[at] = ku;
  }
  if (tid == 0) {
    o.audiotypes[b] = r.status == VO_AUG_OK ? c.audiotype[r.src] : 0;
    o.src_lens[b] = r.L;
    o.mel_lens[b] = (float)r.FL;
    o.status[b] = r.status;
  }
}

}  // namespace vo

using namespace vo;

extern "C" int vo_augment_batch(const vo_corpus* c, const int32_t* plan, int B, int T_src, int T_mel, int H, int cell,
                                int margin, int W_out, int64_t* audiotypes, int64_t* texts, int64_t* src_lens,
                                float* mels, float* mel_lens, float* energies, float* kurtosises, float* durations,
                                float* images, int32_t* status, void* stream) {
  VO_CHECK_ARG(c && plan && audiotypes && texts && src_lens && mels && mel_lens && durations && images && status,
               "augment_batch: null pointer");
  VO_CHECK_ARG(c->char_off && c->frame_off && c->px_off && c->strip_w && c->audiotype && c->ch_id && c->ch_dur &&
                   c->ch_dstart && c->ch_width && c->ch_col && c->mel && c->px,
               "augment_batch: null pointer in the corpus");
  VO_CHECK_ARG((!energies || c->ch_energy) && (!kurtosises || c->ch_kurtosis),
               "augment_batch: energies or kurtosises asked of a corpus packed without them");
  VO_CHECK_ARG(c->U > 0 && c->n_mels > 0 && c->strip_h > 0, "augment_batch: empty corpus");
  VO_CHECK_ARG(B > 0 && B <= 65535 && T_src > 0 && T_mel > 0 && cell > 0 && margin >= 0, "augment_batch: bad sizes");
  VO_CHECK_ARG(H == c->strip_h, "augment_batch: H %d is not the corpus's strip height %d", H, (int)c->strip_h);
  VO_CHECK_ARG(W_out < (1 << 21), "augment_batch: W_out %d is 2^21 columns or more", W_out);
  VO_CHECK_ARG((int64_t)T_src * cell + 2 * (int64_t)margin <= W_out,
               "augment_batch: W_out %d below T_src cell + 2 margin = %lld", W_out,
               (long long)T_src * cell + 2 * (long long)margin);
  // a workgroup's pixel and vector indices run up to one group past the end before they are compared with it
  VO_CHECK_ARG((int64_t)H * W_out < ((int64_t)1 << 31) - AUG_PIX && (int64_t)T_mel * c->n_mels < ((int64_t)1 << 30),
               "augment_batch: an image of one row past 2^31 or its mel past 2^30 elements");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int mel_blocks = (T_mel + AUG_FRAMES - 1) / AUG_FRAMES;
  const int img_blocks = (int)(((int64_t)H * W_out + AUG_PIX - 1) / AUG_PIX);
  const AugOut o = {audiotypes, texts, src_lens, mels, mel_lens, energies, kurtosises, durations, images, status};
  const dim3 grid((unsigned)(mel_blocks + img_blocks + 1), (unsigned)B);
  const bool vec = c->n_mels % 4 == 0 && (reinterpret_cast<uintptr_t>(c->mel) | reinterpret_cast<uintptr_t>(mels)) % 16 == 0;
  if (vec)
    hipLaunchKernelGGL(augment_batch_kernel<true>, grid, dim3(256), 0, st, *c, plan, T_src, T_mel, H, cell, margin,
                       W_out, 1.0f / (float)cell, 1.0f / (float)W_out, mel_blocks, img_blocks, o);
  else
    hipLaunchKernelGGL(augment_batch_kernel<false>, grid, dim3(256), 0, st, *c, plan, T_src, T_mel, H, cell, margin,
                       W_out, 1.0f / (float)cell, 1.0f / (float)W_out, mel_blocks, img_blocks, o);
  VO_RETURN_LAUNCH();
}
