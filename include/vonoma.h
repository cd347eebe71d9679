/* vonoma.h -- C ABI of the MI355X (gfx950) synthesis-path kernels.
 *
 * Drop-in boundary for the reference's visual-onomatopoeia -> mel -> waveform path
 * (sarulab-speech/visual-onoma-to-wave).  The reference is pure PyTorch: every op on
 * its path is an implicit ATen kernel launched from the nn.Modules cited below.  Each
 * entry point here replaces those ATen calls for one reference function; the Python
 * host layer (visual_onoma_to_wave_amd/, same module/class names as the reference)
 * binds them through ctypes (INTEGRATION.md shows the binding).
 *
 * Conventions
 *  - plain device pointers and sizes; all buffers are caller-owned (no allocation
 *    inside, no host synchronisation: every call is stream-ordered and graph-capturable);
 *  - `stream` is a hipStream_t passed as void*; NULL = the default stream;
 *  - return 0 (VO_OK) on success, VO_ERR_INVALID on a rejected argument, or the
 *    hipError_t of a failed launch; vo_last_error() describes the last failure;
 *  - activations are channels-last ("(B, T, C)", C contiguous) -- the layout the
 *    reference's transformer side already uses (scripts/transformer/SubLayers.py:85-93
 *    transposes to (B, C, T) only to call Conv1d) and the one whose 8 consecutive
 *    channels form one MFMA operand fragment;
 *  - element types: VO_F32 or VO_BF16 for tensor I/O; VO_BF16 compute = bf16 MFMA with
 *    fp32 accumulation, VO_F32 compute = exact-f32 MFMA (the parity mode), VO_F32X3 compute
 *    (fp32 I/O and fp32 packed weights, stride 1, no groups) = split-bf16 contractions: each
 *    fp32 operand as hi + lo bf16, three bf16 MFMAs per product (<= 3 * 2^-18 relative error
 *    per product: fp32-class, not bit-exact fp32; the mixed-precision training step's fp32 side).
 */
#ifndef VONOMA_H_
#define VONOMA_H_

#include <stdint.h>
#ifndef __cplusplus
#include <stdbool.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define VO_OK 0
#define VO_ERR_INVALID (-1)
/* vo_resblockk / vo_resblockk_lens only: the arguments are valid but no whole-block kernel covers them; nothing was launched, no
 * error text is set, and the caller runs the block as three vo_resblock_pair launches */
#define VO_NOT_HANDLED (-2)

enum vo_dtype { VO_F32 = 0, VO_BF16 = 1, VO_F32X3 = 2 /* compute only */ };
enum vo_act { VO_ACT_NONE = 0, VO_ACT_RELU = 1, VO_ACT_LRELU = 2, VO_ACT_TANH = 3 };

/* ------------------------------------------------------------------ runtime */
const char* vo_last_error(void);
/* ABI version of this header; vo_version() returns the library's.  A binding checks they are equal
 * at load time.  2 (round 4): vo_bucket_embed gained n_table (before n), vo_conv1d_desc gained
 * ymask / ymask_slope at its end -- a version-1 binding would pass shifted arguments or leave the
 * new fields uninitialised.  3: vo_conv1d_desc gained lens / lens_scale at its end (a version-2 binding would
 * leave them uninitialised), and the vo_*_lens entries below.  4: vo_conv1d_wgrad and vo_conv1d_wgrad_grouped,
 * forwarding wrappers of vo_conv1d_wgrad_bias without a caller, are gone (a version-3 binding would look them
 * up). */
#define VO_ABI_VERSION 4
int vo_version(void);
/* number of entry points and their names (used by the loader test) */
int vo_num_symbols(void);
const char* vo_symbol_name(int i);
/* kernel-variant knobs for A/B experiments ("pair_cfg", "conv_cfg"; default 0 = shipped
 * configuration); returns VO_OK or VO_ERR_INVALID for an unknown key */
int vo_tune(const char* key, int value);

/* ------------------------------------------------------------------ conv1d (implicit GEMM)
 * y[b, t, co] = post( sum_{k, ci} W[k][co][ci] * pre(x[b, t*1 + k*dil - pad, ci]) + bias[co] )
 *               (+ res1) * out_scale (+ res2)
 * Replaces: nn.Conv1d in PositionwiseFeedForward (scripts/transformer/SubLayers.py:60-93),
 *   PostNet ConvNorm+BatchNorm1d (scripts/transformer/Layers.py:33-137, BN folded),
 *   VariancePredictor Conv (scripts/model/modules.py:216-259), nn.Linear as K=1
 *   (SubLayers.py:18-26, vtts.py:23-26, visual_feature_extractor.py:49-55),
 *   HiFi-GAN conv_pre / ResBlock convs with the lrelu prologue and residual epilogue
 *   (scripts/hifigan/models.py:96-103,150,155-160).
 * transposed != 0: ConvTranspose1d(stride=s, padding=p, K_t = 2s) in its polyphase form
 *   (scripts/hifigan/models.py:124-135,153): W holds the 2-tap phase weights packed by
 *   vo_pack_weight(..., VO_PACK_CONVT, ...), co spans s*C_out phase-major columns and output
 *   row m lands at time m*s - p + phase.
 */
typedef struct vo_conv1d_desc {
  const void* x;      /* input (B, T_in, ldx) channels-last, dtype x_dtype            */
  int x_dtype;
  int64_t x_bstride;  /* elements between batches (usually T_in * ldx)               */
  int ldx;            /* elements between rows (>= Ci, multiple of 8)                */
  const void* w;      /* packed weights [K][Co][Ci], dtype = compute dtype            */
  const float* bias;  /* [Co] or NULL                                                 */
  void* y;            /* output, dtype y_dtype                                        */
  int y_dtype;
  int64_t y_bstride;
  int ldy;
  const void* res1;   /* optional, same layout and dtype as y                        */
  const void* res2;   /* optional, same layout and dtype as y (may alias y)          */
  int B, T_in, T_out; /* T_out = output rows (for transposed: T_in + 1 phase rows)   */
  int Ci, Co;         /* Co = GEMM columns (transposed: s * C_out)                    */
  int K, dil, pad;
  int pre_act;  float pre_slope;
  int post_act; float post_slope;
  float out_scale;
  int compute_dtype;  /* VO_BF16, VO_F32 or VO_F32X3 */
  int transposed, up_stride, up_pad, up_cout, up_tout; /* polyphase ConvTranspose1d */
  int variant;        /* 0 = generic; 1..4 = HiFi-GAN MRF stage 0..3 (bf16 I/O): a kernel
                         instantiation of its own, so profiles attribute the stages   */
  int stride;         /* 0/1 = 1; 2..4: output row o reads input rows o*stride + k*dil - pad
                         (HiFi-GAN MPD Conv2d (k,1)/(s,1) per period column, MSD Conv1d)  */
  int groups;         /* 0/1 = dense; g: grouped conv, w packed dense [K][Co][Ci] with zeros
                         outside the g diagonal blocks (MSD grouped Conv1d)              */
  void* workspace;    /* optional caller-owned device scratch (NULL = none): when it holds
                         vo_conv1d_workspace_size(d) bytes, fp32 convs over short sequences
                         (T_out <= 16: glyph encoder, variance predictors) split their
                         reduction over workgroups and add the fp32 partials in a fixed
                         order (deterministic)                                           */
  int64_t workspace_bytes;
  const void* ymask;  /* optional, y's layout and dtype (bf16 y, no bias / residual / activation):
                         each output is stored as round(round(v) * (ymask > 0 ? 1 : ymask_slope))
                         -- an input gradient masked by the leaky-ReLU output it flows into, as
                         vo_lrelu_mask would mask it (HiFi-GAN discriminators, D step)          */
  float ymask_slope;
  const int32_t* lens; /* optional (NULL = dense): ragged batch, see "per-utterance lengths" below.  Same-length
                         convs only (T_out = T_in, 2 pad = (K - 1) dil; polyphase: T_out = T_in + 1); refused
                         with stride > 1, groups > 1, a workspace, ymask, VO_F32X3 and T_out <= 16 in fp32     */
  int lens_scale;      /* rows of x per unit of lens (>= 1 when lens is given)                              */
} vo_conv1d_desc;
int vo_conv1d(const vo_conv1d_desc* d, void* stream);
/* Per-utterance lengths (ragged batches; the HiFi-GAN vocoder path: vo_conv1d with lens, vo_resblock_pair_lens,
 * vo_resblock_pair_frag_lens, vo_resblock3_lens, vo_resblockk_lens, vo_conv_post_lens).  lens: B device int32; utterance b of a
 * (B, T, C) tensor has R_b = clamp(lens[b] * lens_scale, 0, T) valid rows (lens in mel frames, lens_scale the rows
 * per frame at that layer: 1, 8, 64, 128, 256 in HiFi-GAN V1).  The call computes what the dense call computes on the
 * tensor x[b, :R_b] alone: every read of a row outside [0, R_b) -- input, residuals, the MRF accumulator and the
 * fused kernels' on-chip intermediates -- yields zero, and rows >= R_b of the output are neither read nor written
 * (vo_conv_post_lens stores 0.0f there).  For the polyphase upsampler R_b counts input rows; its output has
 * R_b * up_stride rows.  The lengths are read on the device only: no host synchronisation, graph-capturable, and a
 * replay follows lengths changed in place.  The persistent kernels walk a compacted tile list (no tile past an
 * utterance's end), so the work is proportional to sum_b R_b.  A vo_tune knob that selects a kernel without a
 * ragged form is refused with an error naming the knob. */
/* scratch bytes the split-reduction path of vo_conv1d wants for d (0 = it does not split d) */
int64_t vo_conv1d_workspace_size(const vo_conv1d_desc* d);
/* The tile the last vo_conv1d call of the calling thread launched (host bookkeeping only: the tests
 * assert which dispatcher branch a shape took).  Copies min(n, VO_CONV1D_LAUNCH_FIELDS) fields into
 * rec, in this order: output channels per tile (BCO), output rows per tile (BT), conv stride of the
 * instantiation (S), utterance-segment tile (SEG, 0 / 1), nice (1 = the instantiation without
 * channel bounds checks: Ci % 32 == 0 and Co % BCO == 0), reduction splits, sizeof the input, LDS
 * compute and output element, ROLE (0 = generic, 1..4 = MRF stage), compute dtype (enum vo_dtype),
 * then the wave tiling that tells apart instantiations of equal BCO x BT: 16-channel MFMA tiles per
 * wave (NI) and waves across the output channels (WCO); BCO = 16 NI WCO.
 * All zeros: the call was rejected, or handled outside conv1d_kernel (the streaming upsampler).
 * Returns the number of fields copied. */
#define VO_CONV1D_LAUNCH_FIELDS 13
int vo_conv1d_last_launch(int32_t* rec, int n);
/* The record vo_conv1d(d, stream) would leave, without launching: the same argument checks and the same tile
 * rule, on the host alone (no tensor pointer of d is dereferenced, no HIP call, no GPU needed; the pointers
 * only have to be null or not as in the real call).  Writes min(n, VO_CONV1D_LAUNCH_FIELDS) fields into rec
 * (all zeros: refused, or a descriptor the streaming upsampler takes) and returns what vo_conv1d would return
 * before its launch: VO_OK, or VO_ERR_INVALID with the same vo_last_error text.  The calling thread's
 * last-launch record is left as it was. */
int vo_conv1d_plan(const vo_conv1d_desc* d, int32_t* rec, int n);
/* 1 when vo_conv1d runs d on the plane conv (csrc/conv_plane.hip: MRF stage 0 in the wave-owned output-plane form)
 * instead of the tiled kernel, else 0; host only, like vo_conv1d_plan.  It takes the dense variant-1 call with bf16
 * in, compute and out, Ci = Co = ldx = ldy = 256, K = 3 / 7 / 11, (K - 1) dil <= 64 = 2 pad, T_out = T_in, a bias, the
 * leaky-ReLU prologue or none (the ResBlock's c1 and c2), no or a leaky-ReLU post-activation, no stride / groups / transposed / ymask / workspace / lens,
 * every byte offset of an utterance within 31 bits, and "conv_cfg" 0 (5, 6, 9 = the tiled kernels: forced role split,
 * none, the shipped rule).  The launch record of such a call is the 256 x 256 stage-0 tile's: the plane tile's own
 * geometry.  Results equal the tiled kernel's bit for bit. */
int vo_conv1d_plane_takes(const vo_conv1d_desc* d);

/* Weight preparation (load time).  Replaces the weight-norm fold (remove_weight_norm,
 * scripts/hifigan/models.py:105-109,167-174: w = g * v / ||v||, norm over all dims but 0)
 * and the eval-mode BatchNorm fold of PostNet / VFE (Layers.py:129-137), and writes the
 * [K][Co][Ci] compute layout.
 *   mode VO_PACK_CONV : src (Co, Ci, K) -> dst [K][Co][Ci]
 *   mode VO_PACK_CONVT: src (Ci, Co, 2s) (ConvTranspose1d) -> dst [2][s*Co][Ci],
 *                       dst[kk][r*Co + co][ci] = src[ci][co][r + s*(1-kk)]
 *   mode VO_PACK_DGRAD: src (Co, Ci, K) -> dst [K][Ci][Co], dst[K-1-k][ci][co] = src[co][ci][k]
 *                       (the input-gradient of a conv is the conv of dY with these weights,
 *                       padding (K-1)*dil - pad)
 * g (nullable): weight-norm gains, one per src dim-0 slice; row_scale (nullable): per-Co
 * multiplier (BatchNorm gamma / sqrt(var + eps)). */
enum vo_pack_mode { VO_PACK_CONV = 0, VO_PACK_CONVT = 1, VO_PACK_DGRAD = 2 };
int vo_pack_weight(const float* src, const float* g, const float* row_scale, int mode, int Co,
                   int Ci, int K, int stride, void* dst, int dst_dtype, void* stream);

/* ------------------------------------------------------------------ layer norm
 * y[r, :] = LayerNorm(x[r, :] + res[r, :]) * gamma + beta, then zeroed where row r is padding
 * (t >= lens[b], r = b*T + t; lens may be NULL).  eps 1e-5.
 * Replaces: MultiHeadAttention/PositionwiseFeedForward post-LN + residual
 * (scripts/transformer/SubLayers.py:55,91) and FFTBlock.masked_fill (Layers.py:25,28);
 * VariancePredictor LN (modules.py:197-206) with res = NULL, lens = NULL. */
int vo_layernorm(const void* x, int x_dtype, const void* res, int res_dtype, const float* gamma,
                 const float* beta, const int32_t* lens, int B, int T, int D, float eps, void* y,
                 int y_dtype, void* stream);

/* vo_layernorm with an fp32 y and, in the same pass, its bf16 copy y16 (round to nearest even;
 * pad rows 0 in both).  The mixed-precision decoder keeps its residual stream (y) in fp32, as the
 * reference's bf16 autocast does, while the next conv reads y16 -- the same bits that conv's own
 * fp32 -> bf16 staging would make, at half the bytes.  x / res: both fp32, both bf16, or (round 6,
 * the training decoder: bf16 sublayer output + fp32 residual stream) bf16 x with fp32 res. */
int vo_layernorm_dual(const void* x, int x_dtype, const void* res, int res_dtype, const float* gamma,
                      const float* beta, const int32_t* lens, int B, int T, int D, float eps, void* y,
                      void* y16, void* stream);

/* Backward of vo_layernorm (training, config C4): gh = dL/d(x + res) (the gradient of both x
 * and res; 0 on pad rows), dgamma / dbeta (fp32, D) summed over the unmasked rows.  x / res /
 * gh share x_dtype.  workspace: vo_layernorm_bwd_workspace_size(B, T, D) bytes (per-workgroup
 * partial column sums, added in a fixed order: deterministic).
 * Replaces: the autograd of nn.LayerNorm + masked_fill (scripts/transformer/SubLayers.py:55,91,
 * scripts/transformer/Layers.py:25,28) under scripts/04_train.py:128-141. */
int64_t vo_layernorm_bwd_workspace_size(int B, int T, int D);
int vo_layernorm_bwd(const void* x, const void* res, int x_dtype, const void* gy, int gy_dtype,
                     const float* gamma, const int32_t* lens, int B, int T, int D, float eps, void* gh,
                     float* dgamma, float* dbeta, void* workspace, void* stream);

/* vo_layernorm_bwd for the backward of vo_layernorm_dual (round 6, mixed-precision training): res may be
 * fp32 beside a bf16 x (res_dtype), gy2 (bf16, may be NULL) is a second incoming gradient -- that of
 * y16 -- added to gy, and gh32 (may be NULL) receives the fp32 gradient of res beside gh (x_dtype).
 * Combinations: bf16 x + fp32 res with fp32 or bf16 gy; or x_dtype == res_dtype with gy2 = gh32 = NULL
 * (then exactly vo_layernorm_bwd).  Same workspace. */
int vo_layernorm_bwd_ex(const void* x, int x_dtype, const void* res, int res_dtype, const void* gy, int gy_dtype,
                        const void* gy2, const float* gamma, const int32_t* lens, int B, int T, int D, float eps,
                        void* gh, float* gh32, float* dgamma, float* dbeta, void* workspace, void* stream);

/* Training FFT blocks (round 6): the sublayer output's dropout (scripts/transformer/SubLayers.py:51,88) fused
 * into the LayerNorm that follows it.  Forward: y = LN(dropout(x) + res) * gamma + beta (pad rows 0), element i
 * of x kept iff it is kept by vo_dropout(p, seed, salt) on the same tensor, scaled by 1 / (1 - p); y16 (may be
 * NULL; fp32 y only) its bf16 copy.  x / res / y: fp32 / fp32 / fp32, bf16 / fp32 / fp32, bf16 / bf16 / bf16.
 * Backward: gh = dL/dx (through the mask, x_dtype), gres = dL/dres (res_dtype), gy2 (bf16, may be NULL) the
 * gradient of y16 added to gy; dgamma / dbeta as vo_layernorm_bwd (same workspace).  B*T*D < 2^32. */
int vo_layernorm_drop(const void* x, int x_dtype, const void* res, int res_dtype, const float* gamma,
                      const float* beta, const int32_t* lens, int B, int T, int D, float eps, void* y, int y_dtype,
                      void* y16, float p, const int64_t* seed, unsigned salt, void* stream);
int vo_layernorm_bwd_drop(const void* x, int x_dtype, const void* res, int res_dtype, const void* gy, int gy_dtype,
                          const void* gy2, const float* gamma, const int32_t* lens, int B, int T, int D, float eps,
                          float p, const int64_t* seed, unsigned salt, void* gh, void* gres, float* dgamma,
                          float* dbeta, void* workspace, void* stream);

/* ------------------------------------------------------------------ attention
 * Scaled dot-product attention with key padding, H heads of d_k = D/H, over the fused
 * qkv activations (B, L, 3D) (columns [q | k | v], head h at h*d_k) -> out (B, L, D)
 * (head-concat columns h*d_k + d).  Keys t >= lens[b] are masked (-inf before softmax).
 * Head sizes: d_k in {32, 64, 128} for any H >= 1, in VO_F32 and VO_BF16, on all four entry
 * points below (hidden 256 with 8 / 4 / 2 heads, hidden 512 with 16 / 8 / 4); any other dk is
 * VO_ERR_INVALID with a message naming the three sizes.
 * lens contract, for the forward, the backward and their _lse forms alike: utterance b has
 * clamp(lens[b], 0, L) keys (a length past L masks nothing inside [0, L)); lens = NULL means L
 * keys everywhere; an utterance with no key has zero output rows and lse = +inf, and its
 * gradients dQ / dK / dV are zero.
 * Replaces: MultiHeadAttention split/permute + ScaledDotProductAttention
 * (scripts/transformer/SubLayers.py:39-53, scripts/transformer/Modules.py:14-25).  The
 * probabilities are never materialised (the reference returns them but no caller uses
 * them: Models.py:119-124, 190-195). */
int vo_attention(const void* qkv, int dtype, const int32_t* lens, int B, int L, int H, int dk,
                 float scale, void* out, void* stream);

/* Backward of vo_attention (training, config C4): dqkv (B, L, 3D) = [dQ | dK | dV] in the
 * qkv layout, from qkv, the forward output out (B, L, D) and its gradient dout (B, L, D), all in
 * `dtype`.  Flash-style: the row log-sum-exp is rebuilt from qkv, no L x L tensor is stored.
 * workspace: vo_attention_bwd_workspace_size(B, L, H) bytes.  Masked keys get zero dK / dV.
 * Replaces: the autograd of SubLayers.py:39-53 / Modules.py:14-25 under
 * scripts/04_train.py:128-141. */
int64_t vo_attention_bwd_workspace_size(int B, int L, int H);
int vo_attention_bwd(const void* qkv, const void* out, const void* dout, int dtype, const int32_t* lens, int B,
                     int L, int H, int dk, float scale, void* dqkv, void* workspace, void* stream);
/* vo_attention that also writes the row log-sum-exp lse (B, H, L) fp32 (+inf for a row with no key),
 * and the backward that consumes it (bf16: no pass over the keys to rebuild it; every product formed
 * transposed so P / dS stay in registers; fp32: as vo_attention_bwd).  Same reference as above. */
int vo_attention_lse(const void* qkv, int dtype, const int32_t* lens, int B, int L, int H, int dk,
                     float scale, void* out, float* lse, void* stream);
int vo_attention_bwd_lse(const void* qkv, const void* out, const void* dout, int dtype, const int32_t* lens, int B,
                         int L, int H, int dk, float scale, const float* lse, void* dqkv, void* workspace,
                         void* stream);

/* ------------------------------------------------------------------ length regulator
 * out[b, t, :] = x[b, j, :] for cs[j-1] <= t < cs[j] (cs = inclusive cumsum of
 * max(trunc(d[b, j]), 0)), zero for t >= mel_len[b]; mel_len[b] = cs[T_src-1]; rows past
 * max_len are cropped.  index (nullable) receives j (or -1).
 * Replaces: LengthRegulator.LR/expand (scripts/model/modules.py:132-159) + pad
 * (scripts/utils/tools.py:669-687): no per-token device->host sync. */
int vo_length_regulate(const void* x, int x_dtype, const float* dur, int B, int T_src, int D,
                       int max_len, void* out, int out_dtype, int64_t* mel_len, int32_t* index,
                       void* stream);

/* Backward of vo_length_regulate (training, config C4): gx[b, j, :] = sum of go[b, t, :] over
 * the frames t in [cs[j-1], min(cs[j], max_len)) that token j was copied to (frames past the
 * crop get no gradient), summed in frame order (deterministic).  go (B, max_len, D), gx
 * (B, T_src, D); D % 8 == 0.  Replaces: the autograd of LengthRegulator.LR/expand + pad
 * (scripts/model/modules.py:132-159, scripts/utils/tools.py:669-687). */
int vo_length_regulate_bwd(const void* go, int go_dtype, const float* dur, int B, int T_src, int D, int max_len,
                           void* gx, int gx_dtype, void* stream);
/* mel_len only (int64 and int32 copies), so the host can size the output. */
int vo_lr_lengths(const float* dur, int B, int T_src, int64_t* mel_len, int32_t* mel_len32,
                  void* stream);

/* ------------------------------------------------------------------ variance heads
 * Linear(D -> 1) + masked_fill(pad, 0) over h (B*T, D)  (VariancePredictor.linear_layer,
 * scripts/model/modules.py:207-213), then per head:
 *  VO_HEAD_DURATION: pred -> log_d; if d_round != NULL: d_round = clamp(round(exp(log_d)-1)
 *                    * d_control, 0) (modules.py:110-113, round half to even)
 *  VO_HEAD_ENERGY:   pred -> e_pred; idx = bucketize(target or ((pred*std+mean)*control -
 *                    mean)/std, bins) (right=False); x[b, t, :] += table[idx] (modules.py:
 *                    53-64,101-104); e_pred receives the transformed prediction when no
 *                    target is given, as the reference returns it. */
enum vo_head_kind { VO_HEAD_DURATION = 0, VO_HEAD_ENERGY = 1 };
typedef struct vo_head_desc {
  int kind;
  const void* h; int h_dtype;     /* (B*T, D) after the second LayerNorm     */
  const float* w; float b;        /* Linear(D, 1) weight [D] and bias         */
  const int32_t* lens;            /* src lengths [B] (pad mask), nullable     */
  int B, T, D;
  float* pred;                    /* [B*T] log_d or energy prediction         */
  float* d_round; float d_control;/* duration head                            */
  const float* target;            /* energy target [B*T] or NULL              */
  const float* bins; int n_bins;  /* bucket boundaries (n_bins)               */
  float e_mean, e_std, e_control;
  const float* table;             /* embedding (n_bins + 1, D) fp32           */
  void* x; int x_dtype;           /* (B*T, D) hidden state, += table[idx]     */
  int32_t* idx_out;               /* optional bucket indices                  */
} vo_head_desc;
int vo_variance_head(const vo_head_desc* d, void* stream);
/* vo_variance_head with a per-token multiplier read on the device: the multiplier of token
 * (b, t) is control[b*stride_b + t*stride_t] (fp32, strides in floats, 0 = broadcast along that
 * dimension).  It replaces d->d_control for VO_HEAD_DURATION and d->e_control for VO_HEAD_ENERGY
 * (d's own field is ignored); with an energy target it is unused, as in the reference.  Every
 * token's multiplier is loaded, pad tokens included.  n_control = the number of floats
 * addressable from control: VO_ERR_INVALID, and nothing is launched, for a NULL control, a
 * negative stride, (B-1)*stride_b + (T-1)*stride_t >= n_control (a view that would read past
 * its storage) and whatever vo_variance_head refuses.  Control values are not validated: the
 * duration's fmaxf maps a NaN product to 0 where torch.clamp keeps the NaN.  The pointer is
 * read when the kernel runs, so a captured graph follows values changed in place.
 * Replaces: the (B, T) e_control / d_control of vTTS.forward (scripts/model/vtts.py:68-69),
 * broadcast in prediction * control (modules.py:53-64) and round(exp(log_d) - 1) * d_control
 * (modules.py:110-113). */
int vo_variance_head_ctl(const vo_head_desc* d, const float* control, int64_t n_control,
                         int64_t stride_b, int64_t stride_t, void* stream);

/* Training-side energy embedding (config C4, teacher-forced): idx = bucketize(target, bins)
 * (right=False; a NaN target -> n_bins, as torch.bucketize), out = x + table[idx] (out of place),
 * rows = B*T, table (n_table >= n_bins + 1, D) fp32 (VO_ERR_INVALID otherwise);
 * vo_embed_bwd: dtable[e] = sum of dy rows with idx == e, added in row order (deterministic).
 * Replaces: energy_embedding(torch.bucketize(e_target, energy_bins)) and its autograd
 * (scripts/model/modules.py:53-64,101-104). */
int vo_bucket_embed(const void* x, int x_dtype, const float* target, const float* bins, int n_bins,
                    const float* table, int n_table, int64_t rows, int D, void* out, int32_t* idx_out, void* stream);
int vo_embed_bwd(const void* dy, int dy_dtype, const int32_t* idx, int64_t rows, int D, int n_table, float* dtable,
                 void* stream);

/* ------------------------------------------------------------------ encoder glue
 * Visual feature extractor front: for every 24 x W_s slice (b, i) of images (B, 1, 24, W),
 * 3 x [Conv2d 3x3 pad 1 (1 -> 1 ch) -> BatchNorm2d(eval, folded scale/shift) -> ReLU],
 * flattened h*W_s + w into out (B*n, 24*W_s) (then the bridge Linear runs as vo_conv1d K=1).
 * Replaces: VisualFeatureExtractor.forward slicing loop + embedder
 * (scripts/model/visual_feature_extractor.py:60-80).  conv: [n_layers][10] = 9 weights +
 * bias; bn: [n_layers][2] = scale, shift. */
int vo_vfe_stencil(const float* images, int B, int H, int W, int slice_w, int n_slices,
                   const float* conv, const float* bn, int n_layers, void* out, int out_dtype,
                   void* stream);
/* The general glyph stencil (additive; vo_vfe_stencil stays the ICASSP path): context windows of `stride`
 * cells (preprocess.yaml visual_text.stride) and kh x kw taps (model.yaml conv_kernel_size), kh, kw odd <= 9.
 * host only: LDS bytes vo_vfe_stencil_ex needs for an H x win_w window (win_w = slice_w * stride);
 * makes no HIP call (as vo_resblock3_tile_rows); -1 for a size below 1 */
int64_t vo_vfe_stencil_lds_bytes(int H, int win_w, int kh, int kw);
/* for every window (b, i), columns [i*slice_w, i*slice_w + slice_w*stride) of images (B, 1, H, W):
 * n_layers x [Conv2d kh x kw, zero pad ((kh-1)/2, (kw-1)/2), 1 -> 1 ch -> y*scale + shift -> ReLU],
 * flattened h*win_w + w into out (B*n_slices, H*win_w).  Each window is convolved on its own: every
 * layer zero-pads at the window's edges, never reading a neighbouring window.
 * conv: [n_layers][kh*kw + 1] (row-major taps, then bias); bn: [n_layers][2] = scale, shift
 * (1, 0 when the module has no BatchNorm).  fp32: acc = bias, one fma per tap in row-major order,
 * fma(acc, scale, shift), ReLU -- at 3 x 3, stride 1 bit-identical to vo_vfe_stencil.
 * H <= 32; (n_slices - 1)*slice_w + slice_w*stride <= W; a window whose vo_vfe_stencil_lds_bytes
 * exceed 160 KiB is refused with VO_ERR_INVALID and nothing is launched.
 * Replaces: scripts/model/visual_feature_extractor.py:60-80 for any stride / kernel size. */
int vo_vfe_stencil_ex(const float* images, int B, int H, int W, int slice_w, int stride, int n_slices,
                      int kh, int kw, const float* conv, const float* bn, int n_layers,
                      void* out, int out_dtype, void* stream);
/* x[b, t, :] += pe[t, :] (pe nullable) + cls[idx, :] (cls nullable) with idx = cls_idx[b]
 * (idx_per_token = 0) or cls_idx[b*T + t] (idx_per_token = 1).
 * Replaces: position_enc add (Models.py:107-116, 184-186), audiotype_emb add (vtts.py:84-85)
 * and the src_word_emb lookup of the use_image=False branch (Models.py:114). */
int vo_add_pos_class(void* x, int x_dtype, const float* pe, const float* cls,
                     const int64_t* cls_idx, int idx_per_token, int B, int T, int D, void* stream);
/* mask[b, t] = t >= lens[b] (True = padding) and/or lens32[b] = (int32) lens[b];
 * lens_dtype: 0 = fp32, 2 = int64, 3 = int32.  Replaces get_mask_from_lengths
 * (scripts/utils/tools.py:164-171). */
int vo_mask_from_lengths(const void* lens, int lens_dtype, int B, int L, bool* mask,
                         int32_t* lens32, void* stream);

/* ------------------------------------------------------------------ vocoder glue
 * conv_post: y[b, t] = tanh(bias + sum_{k<7, c} w[k][c] * lrelu(x[b, t+k-3, c], 0.01))
 * over channels-last x (B, T, C) -> (B, T) fp32.  Replaces Generator.forward tail
 * (scripts/hifigan/models.py:161-163).  w packed [K][C] fp32. */
int vo_conv_post(const void* x, int x_dtype, const float* w, float bias, int B, int T, int C,
                 int K, float slope, float* y, void* stream);
/* vo_conv_post on a ragged batch (per-utterance lengths, above): y[b, t] = 0.0f for t >= R_b. */
int vo_conv_post_lens(const void* x, int x_dtype, const float* w, float bias, int B, int T, int C,
                      int K, float slope, float* y, void* stream, const int32_t* lens, int lens_scale);
/* vo_conv_post / vo_conv_post_lens with 16-bit PCM output: the same kernels (same dispatch, same fp32 order up to
 * and including tanhf) instantiated with an int16_t output element, y (B, T) int16.  Each sample is stored as
 *   q = (int16) clamp(trunc(v * scale), -32768, 32767)      v = tanhf(...), the product formed in fp32,
 * truncated toward zero: what the reference's host-side (wavs * max_wav_value).astype("int16")
 * (scripts/utils/model.py:73-98) gives for values in range.  A NaN v stores 0; the _lens form stores 0 at t >= R_b.
 * DELIBERATE DEVIATION (saturation): tanhf returns exactly +-1.0f for large inputs and 1.0f * 32768 lies outside
 * int16, where the host cast is undefined (in practice it wraps to -32768: an audible click).  These entries store
 * 32767 there (and -32768 at the negative end, which is in range).
 * scale must be finite and > 0; everything vo_conv_post refuses is refused here (VO_ERR_INVALID, nothing launched,
 * text in vo_last_error()).  Rows of y are T samples apart: no alignment beyond 2 bytes is assumed. */
int vo_conv_post_pcm16(const void* x, int x_dtype, const float* w, float bias, int B, int T, int C,
                       int K, float slope, float scale, int16_t* y, void* stream);
int vo_conv_post_pcm16_lens(const void* x, int x_dtype, const float* w, float bias, int B, int T, int C,
                            int K, float slope, float scale, int16_t* y, void* stream, const int32_t* lens,
                            int lens_scale);
/* Fused ResBlock1 pair for C = 32 / 64 / 128 (bf16, channels-last (B, T, C)):
 *   y = (x + c2(lrelu(c1_dil(lrelu(x, slope)), slope))) * out_scale (+ acc)
 * c1 / c2: K taps, packed [K][C][C] bf16 (vo_pack_weight VO_PACK_CONV), biases fp32;
 * c1 dilation dil, c2 dilation 1, both "same" padding.  The c1 output stays in LDS.
 * acc may alias y (MRF accumulate); y must not alias x.
 * Replaces one (c1, c2) iteration of ResBlock.forward (scripts/hifigan/models.py:96-103)
 * plus the MRF sum / 1/num_kernels of Generator.forward (models.py:155-160). */
int vo_resblock_pair(const void* x, const void* w1, const float* b1, const void* w2,
                     const float* b2, void* y, const void* acc, int B, int T, int C, int K,
                     int dil, float slope, float out_scale, void* stream);
/* vo_resblock_pair on a ragged batch (per-utterance lengths, above): K = 7 / 11 (the shapes the vocoder runs as
 * pairs), shipped dispatch only. */
int vo_resblock_pair_lens(const void* x, const void* w1, const float* b1, const void* w2,
                          const float* b2, void* y, const void* acc, int B, int T, int C, int K,
                          int dil, float slope, float out_scale, void* stream, const int32_t* lens, int lens_scale);
/* vo_resblock_pair for C = 64 / 128, K = 7 / 11 with w1 / w2 in the fragment order that the pair
 * kernel streams into registers (vo_pack_frag of the [K][C][C] pack): every weight load is one
 * contiguous KiB.  C = 128: results equal vo_resblock_pair's on the same weights bit for bit.  Same
 * reference (scripts/hifigan/models.py:96-103, 155-160). */
int vo_resblock_pair_frag(const void* x, const void* w1, const float* b1, const void* w2,
                          const float* b2, void* y, const void* acc, int B, int T, int C, int K,
                          int dil, float slope, float out_scale, void* stream);
/* vo_resblock_pair_frag on a ragged batch (per-utterance lengths, above). */
int vo_resblock_pair_frag_lens(const void* x, const void* w1, const float* b1, const void* w2,
                               const float* b2, void* y, const void* acc, int B, int T, int C, int K,
                               int dil, float slope, float out_scale, void* stream, const int32_t* lens,
                               int lens_scale);
/* [K][C][C] bf16 (vo_pack_weight VO_PACK_CONV), C = 64 / 128 -> [K][C/32][C/32][2][64][8] fragment order:
 * dst[k][p][s][t][l][e] = src[k][32p + 8((l & 15) >> 2) + 4t + (l & 3)][32s + 8(l >> 4) + e]. */
int vo_pack_frag(const void* src, void* dst, int C, int K, void* stream);

/* Fused ResBlock1 with K = 3 (bf16, channels-last (B, T, C), C = 32 / 64 / 128): all three
 * (c1_dil[s], c2) iterations in one launch,
 *   x_{s+1} = x_s + c2_s(lrelu(c1_s(lrelu(x_s, slope)), slope))   (s = 0, 1; bf16-rounded)
 *   y = (x_2 + c2_2(lrelu(c1_2(lrelu(x_2))))) * out_scale (+ acc)
 * w1[s] / w2[s]: packed [3][C][C] bf16, b1[s] / b2[s] fp32, dil[s] in [1, 8] with
 * sum_s (dil[s] + 1) <= 12 (HiFi-GAN V1: 1, 3, 5).  x_1, x_2 never leave the chip.  acc may
 * alias y; y must not alias x.  Replaces a whole ResBlock.forward (scripts/hifigan/
 * models.py:96-103) with the MRF sum of Generator.forward (models.py:155-160); results equal
 * three vo_resblock_pair launches up to the fp32 summation order. */
int vo_resblock3(const void* x, const void* const* w1, const float* const* b1, const void* const* w2,
                 const float* const* b2, const int* dil, void* y, const void* acc, int B, int T, int C,
                 float slope, float out_scale, void* stream);
/* vo_resblock3 on a ragged batch (per-utterance lengths, above): C = 64 / 128, or C = 32 with dilations (1, 3, 5);
 * shipped dispatch only. */
int vo_resblock3_lens(const void* x, const void* const* w1, const float* const* b1, const void* const* w2,
                      const float* const* b2, const int* dil, void* y, const void* acc, int B, int T, int C,
                      float slope, float out_scale, void* stream, const int32_t* lens, int lens_scale);
/* Fused ResBlock1 with K = 7 / 11 (bf16, channels-last (B, T, C)): vo_resblock3's computation with K-tap convs,
 * all three (c1_dil[s], c2) iterations in one launch; x_1, x_2 (bf16-rounded) and the c1 outputs never leave the
 * chip.  w1[s] / w2[s]: packed [K][C][C] bf16, b1[s] / b2[s] fp32.  acc may alias y; y must not alias x.
 * A whole-block kernel exists for C = 32, K = 7 / 11, dil = (1, 3, 5), and with acc only when 1 / out_scale is a
 * bf16 value (the MRF's 1/3); every other valid call returns VO_NOT_HANDLED and launches nothing -- the caller
 * then runs three vo_resblock_pair launches, whose result this one equals up to the fp32 summation order.
 * Additive: VO_ABI_VERSION unchanged. */
int vo_resblockk(const void* x, const void* const* w1, const float* const* b1, const void* const* w2,
                 const float* const* b2, int K, const int* dil, void* y, const void* acc, int B, int T, int C,
                 float slope, float out_scale, void* stream);
/* vo_resblockk on a ragged batch (per-utterance lengths, above); covers what vo_resblockk covers. */
int vo_resblockk_lens(const void* x, const void* const* w1, const float* const* b1, const void* const* w2,
                      const float* const* b2, int K, const int* dil, void* y, const void* acc, int B, int T, int C,
                      float slope, float out_scale, void* stream, const int32_t* lens, int lens_scale);
/* output rows per tile of vo_resblockk's kernel for K (952 / 904 for K = 7 / 11; 0: no kernel) -- the edge shapes
 * of its tests */
int vo_resblockk_tile_rows(int K);
/* output rows per tile of the kernel that vo_resblock_pair (frag != 0: vo_resblock_pair_frag) / vo_resblock3 would
 * launch now for a dense call of that shape, the current vo_tune knobs included; 0 for a shape the entry refuses.
 * Host only: they run the entry's dispatch without a launch, make no HIP call and read no memory but dil[0..2].
 * C = 32 pair: 512 - (K - 1); vo_resblock3: 200 / 488 at C = 128 / 64, 104 at C = 32 with dilations (1, 3, 5), else
 * 232.  The edge shapes of the entries' tests.  Additive: VO_ABI_VERSION unchanged. */
int vo_resblock_pair_tile_rows(int C, int K, int dil, int frag);
int vo_resblock3_tile_rows(int C, const int* dil);

/* (B, C, T) -> (B, T, ldy) with channels C..ldy-1 zero-filled; fp32 in, dtype out. */
int vo_transpose_bct(const float* x, int B, int C, int T, void* y, int y_dtype, int ldy,
                     void* stream);

/* ------------------------------------------------------------------ mel / STFT front-end
 * log-mel (B, n_mels, F) and energy (B, F), F = 1 + N / hop, of wav (B, N) fp32 with
 * torchaudio Spectrogram(n_fft, win=n_fft, hop, power=1, center=True, reflect) +
 * MelScale(fb) + log(clamp_min(., 1e-5)) semantics (scripts/preprocessor/preprocessor.py:
 * 22-36,323-337).  window: (n_fft) fp32; fb: (n_fft/2+1, n_mels) fp32. */
int vo_stft_mel(const float* wav, int B, int N, const float* window, const float* fb, int n_fft,
                int hop, int n_mels, float log_floor, float* mel, float* energy, void* stream);
/* General framing: frame f covers reflect-padded samples [f*hop - pad, f*hop - pad + n_fft),
 * F = 1 + (N + 2*pad - n_fft) / hop; |X| = sqrt(re^2 + im^2 + mag_eps); clip != 0 clamps the
 * input to [-1, 1].  HiFi-GAN's training mel (pad (n_fft - hop)/2, center=False, mag_eps 1e-9,
 * no clip, slaney fb) and vo_stft_mel (pad n_fft/2, eps 0, clip). */
int vo_stft_mel_ex(const float* wav, int B, int N, const float* window, const float* fb, int n_fft,
                   int hop, int n_mels, int pad, float mag_eps, int clip, float log_floor, float* mel,
                   float* energy, float* fstats, void* stream);
/* fstats (nullable, (B, F, 2)): per frame sum_k |X_k|^2 and sum_k log(|X_k|^2 + 1e-8), the
 * power-spectrum statistics of Preprocessor._get_kurtosis. */

/* vo_stft_mel_ex with one length per signal (INTEGRATION.md "Ragged batches in the mel front end").  lens
 * (nullable = every row is N): B device int32 sample counts, clamped to n_b in [0, N] by the kernel and never read on
 * the host.  Row b has F_b = vo_stft_mel_frames(n_b, n_fft, hop, pad) frames; frames f < F_b are, operation for
 * operation, those vo_stft_mel_ex gives on wav[b, :n_b] alone (reflect padding against n_b; no sample at index
 * >= n_b is read); frames F_b <= f < F = vo_stft_mel_frames(N, ...) of mel, energy and fstats are 0.0f, so a finished
 * call leaves no output element unwritten.  frames (nullable): B device int32, frames[b] = F_b.  mel_layout 0:
 * mel (B, n_mels, F); 1: channels-last (B, F, n_mels), the vocoder's input layout.  Stream-ordered, no allocation,
 * no host read: a captured graph follows lengths changed in place.  VO_ERR_INVALID (nothing launched) for whatever
 * vo_stft_mel_ex refuses at the capacity N, and for another mel_layout.  Additive: VO_ABI_VERSION unchanged. */
int vo_stft_mel_lens(const float* wav, int B, int N, const float* window, const float* fb, int n_fft, int hop,
                     int n_mels, int pad, float mag_eps, int clip, float log_floor, float* mel, float* energy,
                     float* fstats, const int32_t* lens, int32_t* frames, int mel_layout, void* stream);
/* Frames of an n-sample signal: 1 + (n + 2*pad - n_fft) / hop when n > pad and n + 2*pad >= n_fft, else 0 (a signal
 * too short to reflect-pad, or shorter than one frame, has none).  Host only, like vo_conv1d_plan: no HIP call. */
int vo_stft_mel_frames(int n, int n_fft, int hop, int pad);

/* Character-level acoustic features (Preprocessor._process energy
 * averaging and _get_kurtosis, scripts/preprocessor/preprocessor.py:339-357,395-403): for
 * utterance b with characters j in [char_off[b], char_off[b+1]) of dur[j] frames (consecutive,
 * from frame 0): e_char[j] = mean(energy[b, span]) (0 if dur 0); k_char[j] = (eta+2)(eta+3)/
 * (eta(eta+1)+1e-8), eta = (3 - g + sqrt((g-3)^2 + 24 g)) / (12 g),
 * g = log(mean p + 1e-8) - mean log(p + 1e-8) over the span's n_bins x dur[j] power values. */
int vo_char_features(const float* energy, const float* fstats, int F, const int32_t* dur,
                     const int32_t* char_off, int B, int n_bins, float* e_char, float* k_char,
                     void* stream);

/* ------------------------------------------------------------------ HiFi-GAN training (C5)
 * Discriminator glue (the reference ships no discriminator code, only
 * the training hyper-parameters of scripts/hifigan/config.json):
 *  vo_pack_grouped: (Co, Ci/groups, K) fp32 -> dense [K][Co][Ci_pad] block-diagonal (zeros
 *    outside the groups and for ci >= Ci) for vo_conv1d's groups mode; vo_pack_grouped_blocks
 *    writes the diagonal blocks only (an in-place update of a buffer whose other entries are
 *    already zero);
 *  vo_period_fold: wav (B, T) -> (B*P, ceil(T/P), 8) channels-last, the MPD's reflect pad to a
 *    multiple of P and (T/P, P) view with each period column a separate sequence;
 *  vo_wav_cl8: (B, T) -> (B, T, 8) (channel 0); vo_avgpool_wav: AvgPool1d(4, 2, padding 2),
 *    (B, T) -> (B, T/2 + 1);
 *  vo_gan_reduce: *out += sum over a (rows x width) view of |a-b| (kind 0), (1-a)^2 (kind 1)
 *    or a^2 (kind 2), deterministic (block partials in workspace, >= 512 floats, added in order);
 *    vo_gan_reduce_grad: ga = *scale * d(sum)/da. */
int vo_pack_grouped(const float* src, int Co, int Ci, int K, int groups, int Ci_pad, void* dst,
                    int dst_dtype, void* stream);
int vo_pack_grouped_blocks(const float* src, int Co, int Ci, int K, int groups, int Ci_pad, void* dst,
                           int dst_dtype, void* stream);
/* Input-gradient weights of one stride phase r of a strided / grouped conv: w (Co, Ci/groups, K) fp32
 * -> dst [J][ci_out][co_in], dst[t][ci][co] = w[co][ci mod cig][k_r + S (J - 1 - t)] within a group,
 * 0 elsewhere (blocks_only: the diagonal blocks only, other entries left as they are).  Replaces
 * the transpose / flip / pack chain of the HiFi-GAN discriminators' backward (C5). */
int vo_pack_dgrad_phase(const float* w, int Co, int cig, int K, int groups, int S, int k_r, int J, int ci_out,
                        int co_in, int blocks_only, void* dst, int dst_dtype, void* stream);
/* Many weight packs in one call (hifigan/gan_ops.prepack: the ~270 re-packs after each C5 optimizer
 * step).  Job: for r < rows, j < width, t < T, with cbase(r) = (r / rpg) * cpg,
 *   dst[(t * dst_rows + r) * ld + cbase(r) + j] =
 *     GATHER swap 0: src[r][j][tap0 + tstep t]                    (vo_pack_weight CONV, grouped blocks)
 *     GATHER swap 1: src[cbase(r) + j][r mod rpg][tap0 + tstep t] (DGRAD, vo_pack_dgrad_phase blocks)
 *     CONVT:         src[j][r mod cig][r / cig + tap0 (1 - t)]    (vo_pack_weight CONVT, tap0 = s, K = 2s, T = 2)
 * src (src_rows, cig, K) fp32 contiguous (CONVT: (Ci, Co = cig, K)); other dst entries untouched;
 * a job's tap range (|tstep| (T - 1) + 1, CONVT: K) is at most 48. */
enum vo_pack_job_mode { VO_PJ_GATHER = 0, VO_PJ_CONVT = 1 };
typedef struct vo_pack_job {
  const float* src;
  void* dst;
  int mode, swap, T, rows, width, dst_rows, ld, rpg, cpg, cig, K, tap0, tstep, src_rows;
} VoPackJob;
int vo_pack_batch(int n, const VoPackJob* jobs, int dst_dtype, void* stream);
/* Row remap of channels-last rows (row_bytes, a multiple of 4): dst row r (r < dst_rows; n = r / Td,
 * t = r mod Td) = src row n Ss + t + shift if lo <= t < hi, else zeros.  The joined-sequence layout of
 * the discriminators' short period columns (hifigan/gan_ops._conv_joined) and its adjoint. */
int vo_seq_remap(const void* src, int64_t src_rows, void* dst, int64_t dst_rows, int row_bytes, int Td,
                 int64_t Ss, int lo, int hi, int shift, void* stream);
/* One or two remaps in one launch (rows of whole 16-byte units).  Job: dst row r (n = r / Td, t =
 * r mod Td) = src row n Ss + t + shift [+ src2 row n Ss2 + t + shift2, added in dtype (bf16 / fp32)
 * when src2 is non-NULL] for lo <= t < hi, else zeros; src_rows / src2_rows bound the reads.  One
 * joined discriminator conv feeding the next: the split output and the next joined input from one
 * read, and the backward's two gathers plus autograd's add of them (hifigan/gan_ops.RejoinFn). */
typedef struct vo_remap_job {
  const void* src; const void* src2; void* dst;
  int64_t src_rows, src2_rows, dst_rows, Ss, Ss2;
  int Td, lo, hi, shift, shift2;
} VoRemapJob;
int vo_seq_remap2(int n, const VoRemapJob* jobs, int row_bytes, int dtype, void* stream);
int vo_period_fold(const float* wav, int B, int T, int P, void* out, int dtype, void* stream);
int vo_wav_cl8(const float* wav, int64_t n, void* out, int dtype, void* stream);
int vo_avgpool_wav(const float* x, int B, int T, float* y, void* stream);
/* Their adjoints (dL/dwav, fp32, written): g in the forward's output layout and dtype; the period
 * fold adds the gradient of each right-pad row to the sample it mirrored. */
int vo_period_fold_bwd(const void* g, int dtype, int B, int T, int P, float* gwav, void* stream);
int vo_wav_cl8_bwd(const void* g, int dtype, int64_t n, float* gwav, void* stream);
int vo_avgpool_wav_bwd(const float* g, int B, int T, float* gx, void* stream);

/* Weight normalisation over n layers per call (torch.nn.utils.weight_norm, dim = 0; the HiFi-GAN
 * generator's and discriminators' weight-normed convs in C5 training -- replaces PyTorch's
 * per-layer torch._weight_norm forward / backward kernels, hifigan/models.py:96-103,124-132 and
 * the HiFi-GAN V1 discriminators).  Layer k: fp32 v[k] (rows[k] x len[k], contiguous), g[k]
 * (rows[k]); forward w[k] = v * g / ||v_row||; backward from dw[k]: dv[k], dg[k].  The pointer
 * and size tables are host arrays (copied into the kernel arguments, 24 layers per launch). */
int vo_weight_norm(int n, const void* const* v, const void* const* g, void* const* w, const int* rows,
                   const int* len, void* stream);
int vo_weight_norm_bwd(int n, const void* const* v, const void* const* g, const void* const* dw, void* const* dv,
                       void* const* dg, const int* rows, const int* len, void* stream);
/* Spectral normalisation (torch.nn.utils.spectral_norm: dim 0, one power iteration per training
 * forward; the HiFi-GAN V1 MSD's first scale in C5) for n layers per call.  Layer: W = weight_orig
 * (rows x L fp32), buffers u (rows) / v (L) updated in place when power != 0 (v = normalize(W^T u),
 * u = normalize(W v), normalize(x) = x / max(|x|, eps)), copies of the u / v used written to
 * u_out / v_out, sigma = u . W v, w = W / sigma; vraw (L) and s (rows) are scratch, and so is w
 * until it is written (it must not alias W).  Replaces the
 * per-layer PyTorch hook (two gemv, norms, clamps, divides, clones and a dot per layer). */
typedef struct vo_sn_layer {
  const float* W;
  float *u, *v, *u_out, *v_out, *vraw, *s, *sigma, *w;
  int rows, L;
} VoSnLayer;
int vo_spectral_norm(int n, const VoSnLayer* layers, int power, float eps, void* stream);
/* Its backward (u, v, sigma as the forward used them, held constant, as torch's autograd of the
 * hook does): gW = g / sigma - (sum(g * W) / sigma^2) u v^T for n layers in three launches; the sum
 * in a fixed order (deterministic).  workspace: vo_spectral_norm_bwd_workspace_size bytes. */
typedef struct vo_sn_bwd_layer {
  const float *g, *W, *u, *v, *sigma;
  float* gW;
  int rows, L;
} VoSnBwdLayer;
int64_t vo_spectral_norm_bwd_workspace_size(int n, const VoSnBwdLayer* layers);
int vo_spectral_norm_bwd(int n, const VoSnBwdLayer* layers, float* workspace, void* stream);
int vo_gan_reduce(int kind, const void* a, int lda, const void* b, int ldb, int64_t rows, int width,
                  int dtype, float* out, float* workspace, void* stream);
int vo_gan_reduce_grad(int kind, const void* a, int lda, const void* b, int ldb, int64_t rows,
                       int width, int dtype, const float* scale, void* ga, int ldg, void* stream);
/* Many terms per launch (the C5 G step's feature-matching / adversarial terms, the D step's halves):
 * vo_gan_reduce_multi writes out[i] = sum_i * scale[i] (scale NULL: 1; workspace:
 * vo_gan_reduce_multi_workspace_size(n) bytes); vo_gan_reduce_grad_multi writes term i's gradient
 * ga_i = scale[i] * d(sum_i)/da_i (ga, ldg per term).  scale: n device floats.  vo_gan_reduce and
 * vo_gan_reduce_grad run the same two kernels with a table of one term, and a term's blocks do not
 * depend on the terms around it: sum_i and ga_i are the single-term results bit for bit. */
typedef struct vo_gan_term {
  int kind; const void* a; int lda; const void* b; int ldb; int64_t rows; int width; void* ga; int ldg;
} VoGanTerm;
int64_t vo_gan_reduce_multi_workspace_size(int n);
int vo_gan_reduce_multi(int n, const VoGanTerm* terms, int dtype, const float* scale, float* out, float* workspace,
                        void* stream);
int vo_gan_reduce_grad_multi(int n, const VoGanTerm* terms, int dtype, const float* scale, void* stream);

/* ------------------------------------------------------------------ training backward
 * Weight gradient of a channels-last conv on MFMA (replaces the MIOpen weight pass of the
 * training backward):
 *   dw[(m*N + n)*K + k] = sum_{b, t < T_A} A[b, t, m] * B[b, t*S + k*dil - pad, n]
 * (written in the conv weight's own (M, N, K) order; B rows outside [0, T_B) read as 0;
 * pre_a / pre_b: leaky-ReLU(slope) applied to that operand).
 * Conv1d (Co, Ci, K): A = dY (T_out rows, M = Co), B = pre(x) (T_in rows, N = Ci).
 * ConvTranspose1d (Ci, Co, 2s): A = pre(x) (T_in, M = Ci), B = dY (T_up, N = Co), S = s, pad p.
 * dw fp32.  Deterministic: each row split stores its partial tile into ``workspace``
 * (vo_conv1d_wgrad_workspace_size bytes for the same B, T_A, M, N, K, groups) and a second
 * kernel adds the splits in a fixed order.  dtype: VO_BF16 or VO_F32 for both operands, or VO_F32X3
 * (fp32 operands contracted as split-bf16, see the header note; stride 1, ungrouped).
 * vo_colsum: out[c] = sum_r x[r*ld + c] (bias gradient; block partials in workspace,
 * vo_colsum_workspace_size bytes, added in order). */
int64_t vo_conv1d_wgrad_workspace_size(int B, int T_A, int M, int N, int K, int groups);
/* The one entry (ABI 4 dropped the forwarding wrappers vo_conv1d_wgrad and vo_conv1d_wgrad_grouped: groups = 1
 * and db = NULL here).  Grouped conv (groups > 1): M = C_out / groups and N = C_in / groups per group,
 * lda >= groups*M, ldb >= groups*N; group g reads A columns [g*M, (g+1)*M), B columns [g*N, (g+1)*N) and writes
 * rows [g*M, (g+1)*M) of dw laid out (groups*M, N, K).  Replaces MIOpen's grouped weight pass of
 * the multi-scale discriminator (HiFi-GAN V1 MSD).
 * db non-NULL: the bias gradient in the same launch, db[g*M + m] = sum over all
 * A rows of A[.., g*M + m] (the conv form, A = dY; pre_a must be 0), summed by the tap-0
 * workgroups as they stage A (saves the separate vo_colsum launch). */
int vo_conv1d_wgrad_bias(const void* a, int lda, int T_A, const void* b, int ldb, int T_B, int B,
                         int M, int N, int K, int S, int dil, int pad, int groups, int pre_a,
                         int pre_b, float slope, int dtype, float* dw, float* db, float* workspace,
                         void* stream);
/* Which kernel this thread's last vo_conv1d_wgrad_bias call launched (host bookkeeping, zeroed at the
 * call's entry: a rejected call reads as zeros).  Copies min(n, VO_CONV1D_WGRAD_LAUNCH_FIELDS) fields into rec
 * and returns that count (0 for a null rec).  Fields, in order: ROUTE (1 per-tap kernel, 2 multi-tap kernel,
 * 3 K = 1 kernel), TM (output tile: 64 / 32 or 64 / 128), KG (taps per run; 0 off the multi-tap route), SW (its
 * window template 1 / 2 / 4; 0 off the multi-tap route), ntg (tap runs; 0 off the multi-tap route), gpt (groups
 * per tile), splits (row splits), rows_per_split (multi-tap: 64 x chunks per split), direct (1: the kernel wrote
 * dw / db in their final layout, no reduce ran), reduce_W (waves per output of the reduce: 16 or 1; 0 when
 * direct), compute_dtype, bias.
 * vo_conv1d_wgrad_plan launches nothing: the record vo_conv1d_wgrad_bias with the same sizes, flags and
 * vo_tune knobs would leave (with_bias = a non-null db), from the routing code the launch itself runs.  Returns
 * 0, or -1 with a zero record and vo_last_error for sizes the launch refuses; it leaves the last-launch
 * record alone. */
#define VO_CONV1D_WGRAD_LAUNCH_FIELDS 12
int vo_conv1d_wgrad_last_launch(int32_t* rec, int n);
int vo_conv1d_wgrad_plan(int B, int T_A, int T_B, int M, int N, int K, int S, int dil, int pad, int groups,
                         int pre_a, int pre_b, int dtype, int with_bias, int32_t* rec, int n);
int64_t vo_colsum_workspace_size(int64_t rows, int C);
int vo_colsum(const void* x, int64_t rows, int C, int ld, int dtype, float* out, float* workspace, void* stream);

/* Leaky-ReLU / ReLU backward mask: out[r, c] = g[r, c] * (ref[r, c] > 0 ? 1 : slope) over a
 * (rows x width) view with leading dimensions (out may alias g; ref = the activation's input, or
 * its output when slope > 0).  Replaces the elementwise autograd of F.leaky_relu / F.relu
 * (hifigan/models.py:96-103,155-163, SubLayers.py:85-93) in the training backward. */
int vo_lrelu_mask(const void* g, int ldg, int g_dtype, const void* ref, int ldr, int ref_dtype, int64_t rows,
                  int width, float slope, void* out, int ldo, void* stream);
/* out = round(g * (ref > 0 ? 1 : slope)) + add (the masked gradient plus a residual branch's gradient
 * in one pass; add has g's dtype; rows of 8-element vectors, 16-byte aligned). */
int vo_lrelu_mask_add(const void* g, int ldg, int g_dtype, const void* ref, int ldr, int ref_dtype, const void* add,
                      int lda, int64_t rows, int width, float slope, void* out, int ldo, void* stream);
/* out = round(round(g + add) * (ref > 0 ? 1 : slope)): two gradients of a leaky-ReLU output (the next
 * conv's input gradient and a feature-matching loss's, HiFi-GAN discriminators) summed as autograd
 * sums them and masked in one pass (same layout rules as vo_lrelu_mask_add). */
int vo_lrelu_mask_sum(const void* g, int ldg, int g_dtype, const void* ref, int ldr, int ref_dtype, const void* add,
                      int lda, int64_t rows, int width, float slope, void* out, int ldo, void* stream);

/* ------------------------------------------------------------------ training glue (round 2)
 * BatchNorm with batch statistics over channels-last x (M rows x C channels, VO_F32 / VO_BF16):
 * y = (x - mean) rstd * gamma + beta (gamma / beta may both be NULL), mean_rstd[0..C) = mean,
 * [C..2C) = 1/sqrt(var_biased + eps); running stats (both or neither): r = (1-m) r + m stat with
 * the unbiased variance, *nbt += 1 (NULL: skipped).  workspace: vo_bn_workspace_size bytes.
 * Replaces nn.BatchNorm1d/2d in training mode -- PostNet (scripts/transformer/Layers.py:129-137)
 * and the glyph encoder's single-channel BatchNorm2d (C = 1; scripts/model/
 * visual_feature_extractor.py:40-47).  vo_bn_bwd: dgamma = sum dy xhat, dbeta = sum dy,
 * dx = gamma rstd (dy - dbeta / M - xhat dgamma / M) (dx in x's dtype).  Deterministic.  At C = 1
 * with M a multiple of the 16-byte vector the backward's sums and dx are formed in double (the workspace,
 * 8-byte aligned, holds them as doubles) and rounded once.
 *
 * vo_bn_route is the one place that decides which kernels the two calls launch, and with what geometry;
 * both take their dispatch from it.  It launches nothing and makes no GPU call (a plan, like
 * vo_conv1d_wgrad_plan).  dy_dtype < 0: the forward.  x, dy, out (y or dx): the call's pointers, NULL in
 * a plan call meaning "aligned".  Copies min(n, VO_BN_ROUTE_FIELDS) fields into rec (NULL: none) and
 * returns that count, or -1 with a zero record and vo_last_error for sizes / dtypes the calls refuse.
 * Fields, in order: route (0 scalar kernels, 1 vectorised: C a multiple of the 16-byte vector V with
 * C / V <= 256, 2 FLAT: C = 1 with M a multiple of V), V (elements per vector; 0 on the scalar route),
 * CV (vector columns C / V; FLAT 1; scalar 0), RL (row lanes 256 / CV of a block; scalar 256 / CT), RB
 * (rows -- FLAT: vectors -- per block), nb (row blocks = partials per channel), apply_blocks (grid of the
 * apply kernel; vectorised: its thread count a multiple of CV), CT (channels per block of the scalar
 * stats kernels, 1 or 64; 0 off the scalar route).
 * Alignment rule: the vectorised and FLAT kernels issue 16-byte loads and stores, so they need x, dy and
 * the output 16-byte aligned (a bf16 dy beside an fp32 x is read 8 bytes at a time: 8-byte aligned);
 * a call whose pointers are not (a contiguous slice that starts inside an allocation) takes the scalar
 * kernels, as does a bf16 x with an fp32 dy. */
#define VO_BN_ROUTE_FIELDS 8
int vo_bn_route(int M, int C, int x_dtype, int dy_dtype, const void* x, const void* dy, const void* out,
                int32_t* rec, int n);
int64_t vo_bn_workspace_size(int M, int C);
int vo_bn_train_fwd(const void* x, int dtype, int M, int C, const float* gamma, const float* beta, float eps,
                    float momentum, float* run_mean, float* run_var, int64_t* nbt, float* mean_rstd,
                    float* workspace, void* y, void* stream);
int vo_bn_bwd(const void* x, int x_dtype, const void* dy, int dy_dtype, int M, int C, const float* gamma,
              const float* mean_rstd, float* workspace, float* dgamma, float* dbeta, void* dx, void* stream);

/* Dropout in training (nn.Dropout / F.dropout: scripts/transformer/SubLayers.py:38,87,
 * scripts/transformer/Layers.py:129-131, scripts/model/modules.py:52-56): y[i] = x[i] / (1 - p) when
 * hash(*seed, salt, i) >= p 2^32, else 0 (x, y fp32 / bf16, 16-byte aligned, n < 2^32; y may alias x).
 * The mask depends only on (*seed, salt, i): the backward is the same call on dy.  One device seed per
 * training step, a distinct salt per dropout site of the step. */
int vo_dropout(const void* x, int dtype, int64_t n, float p, const int64_t* seed, unsigned salt, void* y,
               void* stream);

/* Glyph-encoder Conv2d(1, 1, 3, padding=1) on N single-channel H x W maps (fp32), w[0..9) the
 * row-major kernel, w[9] the bias (scripts/model/visual_feature_extractor.py:40-47,60-72):
 * forward, and the backward -> dx and dw[10] (weight + bias gradient; per-block partials summed in
 * a fixed order, workspace: vo_vfe_conv_workspace_size bytes). */
int64_t vo_vfe_conv_workspace_size(int N, int H, int W);
int vo_vfe_conv_fwd(const float* x, int N, int H, int W, const float* w, float* y, void* stream);
int vo_vfe_conv_bwd(const float* x, const float* dy, int N, int H, int W, const float* w, float* dx, float* dw,
                    float* workspace, void* stream);
/* The same for Conv2d(1, 1, (kh, kw), padding ((kh-1)/2, (kw-1)/2)), kh, kw odd <= 9 (additive; the 3 x 3
 * entries above stay the ICASSP path): w[kh*kw + 1] = row-major kernel, then the bias; dw[kh*kw + 1] alike.
 * Per-block partials in the workspace, summed in a fixed order (bit-reproducible).  The size query
 * returns -1 for arguments the entries refuse. */
int64_t vo_vfe_conv_workspace_size_ex(int N, int H, int W, int kh, int kw);
int vo_vfe_conv_fwd_ex(const float* x, int N, int H, int W, int kh, int kw, const float* w, float* y, void* stream);
int vo_vfe_conv_bwd_ex(const float* x, const float* dy, int N, int H, int W, int kh, int kw, const float* w,
                       float* dx, float* dw, float* workspace, void* stream);

/* Backward of vo_stft_mel_ex (clip off; the HiFi-GAN V1 training mel-loss front end):
 * gmel (B, n_mels, F) = dL/dlogmel -> dwav (B, N) fp32 (written, not accumulated).  Per frame the
 * spectrum is recomputed; the frame gradients (workspace: vo_stft_mel_bwd_workspace_size bytes)
 * are gathered per sample over the overlapping frames and the reflect-padding mirrors in a
 * fixed order.  n_mels <= 256. */
int64_t vo_stft_mel_bwd_workspace_size(int B, int N, int n_fft, int hop, int pad);
int vo_stft_mel_bwd(const float* wav, int B, int N, const float* window, const float* fb, int n_fft, int hop,
                    int n_mels, int pad, float mag_eps, float log_floor, const float* gmel, float* dwav,
                    float* workspace, void* stream);

/* Multi-resolution STFT loss (the auxiliary spectral loss of BASELINE.json config C5; Parallel
 * WaveGAN's formulation: per resolution spectral convergence ||Y - X||_F / ||Y||_F and mean
 * |log Y - log X| over STFT magnitudes).  vo_stft_mag: torch.stft(center=True, reflect padding
 * n_fft / 2, onesided) of wav (B, N) fp32 with `window` (n_fft samples: the win_len window zero-
 * padded to n_fft, centred, as torch.stft pads it) -> mag (B, 1 + N / hop, n_fft / 2 + 1) =
 * sqrt(max(|X|^2, eps)); vo_stft_mag_bwd: gmag -> dwav (written; workspace
 * vo_stft_mag_bwd_workspace_size bytes; deterministic gather as vo_stft_mel_bwd).
 * vo_stft_loss: out[3] = (sum (y - x)^2, sum y^2, sum |log y - log x|) over n magnitudes
 * (workspace >= 1536 floats); vo_stft_loss_grad: gx = d(w[0] sqrt(out0 / out1) + w[1] out2 / n)/dx with
 * the weights w[2] (the incoming loss gradients) read on the device. */
int vo_stft_mag(const float* wav, int B, int N, const float* window, int n_fft, int hop, float eps, float* mag,
                void* stream);
int64_t vo_stft_mag_bwd_workspace_size(int B, int N, int n_fft, int hop);
int vo_stft_mag_bwd(const float* wav, int B, int N, const float* window, int n_fft, int hop, float eps,
                    const float* gmag, float* dwav, float* workspace, void* stream);
int vo_stft_loss(const float* xm, const float* ym, int64_t n, float* out, float* workspace, void* stream);
int vo_stft_loss_grad(const float* xm, const float* ym, int64_t n, const float* sums, const float* w, float* gx,
                      void* stream);

/* ------------------------------------------------------------------ training input pipeline
 * Glyph batch: B grayscale strips packed in px (strip b at img_off[b],
 * H rows of img_w[b] uint8 columns) -> out (B, 1, H, W_out) fp32 = pixel / 255 with each
 * character j of sample b (char_off[b] <= j < char_off[b+1]: columns [char_start[j],
 * char_start[j] + char_len[j]) of its strip) centred in a `cell`-wide white cell
 * (pleft = (cell-len)/2 + (cell-len)%2), white right-padding to W_out and `margin` white
 * columns on the left.  char_off == NULL: strips copied as they are (already centred).
 * Replaces Dataset.character_padding_forinput (scripts/dataset.py:71-92), pad_2D_gray_image
 * (scripts/utils/tools.py:616-635) and to_device's ToTensor (tools.py:18-20,50-51). */
int vo_glyph_batch(const uint8_t* px, const int64_t* img_off, const int32_t* img_w,
                   const int32_t* char_off, const int32_t* char_start, const int32_t* char_len,
                   int B, int H, int cell, int margin, int W_out, float* out, void* stream);

/* Glyph stretching (additive): the per-character resize of the reference's renderers
 * (scripts/preprocessor/visualtext_generator.py:23-46 `c_im.resize((width, fontsize))`; prediction.ipynb
 * `c_im.resize((int(new_w), fs))`) with the layout above, from an atlas of unstretched glyphs and device tensors
 * of ids and pixel widths.  The resize is PIL's bicubic resample, horizontal pass only, bit for bit on gray
 * glyphs (8-bit fixed point: coefficients of 22 fractional bits, int32 sums).
 *
 * vo_glyph_stretch_table (host only, no HIP call): the coefficients of every target width w in 1 .. cell for
 * source width src_w.  Record w (w - 1) / 2 + c (column c of width w) is 2 + src_w int32: xmin, n, K[0 .. src_w)
 * with zeros past n; output pixel = clamp((2^21 + sum_x src[y][xmin + x] K[x]) >> 22, 0, 255).  w == src_w is the
 * identity.  vo_glyph_stretch_table_size: its bytes (546 312 for 24 / 102), -1 for sizes out of range.
 * VO_ERR_INVALID unless 1 <= src_w <= 64, 1 <= cell <= 256 and table_bytes is enough.
 *
 * vo_glyph_stretch: atlas (n_glyphs, H, src_w) uint8, ids (B, T) int64 (the model's `texts`), src_lens (B) int64,
 * widths (B, T) int32 pixels (NULL: every width is src_w), table as above for (src_w, cell), all device memory ->
 * out (B, 1, H, W_out) fp32, W_out >= T cell + 2 margin.  Cell t of row b, columns margin + t cell ... + cell - 1,
 * holds atlas[ids[b, t]] resized to w = min(widths[b, t], cell) columns, centred as vo_glyph_batch centres it
 * (pleft = (cell - w) / 2 + (cell - w) % 2), white elsewhere, as pixel / 255.  A cell is white when t >= src_lens[b],
 * widths[b, t] <= 0 or ids[b, t] is outside [0, n_glyphs); the margins and the columns past margin + T cell are
 * white.  Every element of out is written, and no value of ids, widths or src_lens makes the kernel read outside
 * atlas or table.  Allocates nothing, never synchronises, reads nothing on the host: graph-capturable.
 * H <= 65535. */
int64_t vo_glyph_stretch_table_size(int src_w, int cell);
int vo_glyph_stretch_table(int src_w, int cell, int32_t* table, int64_t table_bytes);
int vo_glyph_stretch(const uint8_t* atlas, int n_glyphs, int H, int src_w, const int64_t* ids,
                     const int64_t* src_lens, const int32_t* widths, int B, int T, int cell, int margin, int W_out,
                     const int32_t* table, float* out, void* stream);

/* Repeat and consecutive augmentation (additive): a padded training batch assembled on the
 * device from a base corpus packed once and a plan, one row per utterance.  Replaces the file-writing loop of
 * scripts/preprocessor/preprocessor.py:468-622 (_augmentation, _repeataug, _consecutiveaug) together with the
 * collate padding (pad_1D / pad_2D, scripts/utils/tools.py:585-614) and the layout of vo_glyph_batch.
 *
 * vo_corpus: U base utterances in device memory.  Utterance u has n = char_off[u + 1] - char_off[u] >= 1
 * characters at char_off[u] of the flat per-character arrays, F = frame_off[u + 1] - frame_off[u] mel frames at row
 * frame_off[u] of mel, and a strip of strip_h rows of strip_w[u] uint8 columns at px_off[u] of px.  Character c has
 * id ch_id, duration d = ch_dur >= 0, duration prefix s_c = ch_dstart = d[0] + ... + d[c - 1] (F = s_n), pixel
 * width w = ch_width >= 0 and first strip column ch_col = w[0] + ... + w[c - 1] (strip_w = their sum).  ch_energy
 * and ch_kurtosis may each be NULL (a model without that condition); the output of the same name is then NULL too.
 *
 * A plan is (B, 5) int32 in device memory, row b = src, pos, m, m_mel, r: utterance src with m more copies of
 * character pos, m_mel more copies of that character's frames, the whole repeated r times.  With n' = n + m and
 * F' = F + m_mel d[pos], row b has n' r characters and F' r frames:
 *   output character j is base character sigma(j mod n'):  sigma(j') = j' for j' < pos, pos for pos <= j' <= pos + m,
 *     j' - m above; text id, duration, energy, kurtosis, width and glyph cell are those of that character, the
 *     cell laid out as vo_glyph_batch lays it out (same pleft for widths above the cell too, same margin);
 *   output frame f is base frame phi(f mod F'):  phi(f') = f' for f' < s_pos, s_pos + (f' - s_pos) mod d[pos] for
 *     s_pos <= f' < s_pos + (m_mel + 1) d[pos] (empty when d[pos] = 0), f' - m_mel d[pos] above.
 * Past a row's length texts, durations, energies, kurtosises and mels are 0 and images 1.0 (white); every element of
 * every output is written.  The reference's consecutive augmentation of k copies is m = k - 1, m_mel = k (its mel
 * gains one copy more than its durations); its repeat augmentation is r.
 *
 * A row is refused on the device, never raised: it is written as an empty utterance (audiotype 0, src_len =
 * mel_len = 0, all padding) and status[b] says why, in this order: VO_AUG_BAD_ROW (src outside [0, U), pos outside
 * [0, n), m < 0, m_mel < 0 or r < 1), VO_AUG_CHARS_OVER (n' r > T_src), VO_AUG_FRAMES_OVER (F' r > T_mel);
 * VO_AUG_OK otherwise.
 *
 * vo_augment_batch: outputs audiotypes (B) int64, texts (B, T_src) int64, src_lens (B) int64, mels (B, T_mel,
 * n_mels) fp32, mel_lens (B) fp32, energies / kurtosises / durations (B, T_src) fp32, images (B, 1, H, W_out) fp32,
 * status (B) int32; H == strip_h, T_src cell + 2 margin <= W_out < 2^21, B <= 65535.  One launch; allocates nothing, never
 * synchronises, reads nothing on the host: graph-capturable, and a plan rewritten in place is what a replay reads.
 * Frames move as 16-byte vectors when n_mels % 4 == 0 and both mel pointers are 16-byte aligned. */
#define VO_AUG_OK 0
#define VO_AUG_BAD_ROW 1
#define VO_AUG_CHARS_OVER 2
#define VO_AUG_FRAMES_OVER 3
typedef struct vo_corpus {
  int32_t U, n_mels, strip_h;
  const int32_t* char_off;   /* (U + 1) */
  const int64_t* frame_off;  /* (U + 1), in frames */
  const int64_t* px_off;     /* (U), in pixels */
  const int32_t* strip_w;    /* (U) */
  const int64_t* audiotype;  /* (U) */
  const int32_t* ch_id;      /* flat per-character arrays, char_off[U] entries each */
  const int32_t* ch_dur;
  const int32_t* ch_dstart;
  const int32_t* ch_width;
  const int32_t* ch_col;
  const float* ch_energy;    /* or NULL */
  const float* ch_kurtosis;  /* or NULL */
  const float* mel;          /* (frame_off[U], n_mels) */
  const uint8_t* px;
} vo_corpus;
int vo_augment_batch(const vo_corpus* c, const int32_t* plan, int B, int T_src, int T_mel, int H, int cell, int margin,
                     int W_out, int64_t* audiotypes, int64_t* texts, int64_t* src_lens, float* mels, float* mel_lens,
                     float* energies, float* kurtosises, float* durations, float* images, int32_t* status,
                     void* stream);

/* Energy / kurtosis statistics over the augmented population and the normalisation of the packed corpus (additive;
 * DESIGN.md section 15).  Replaces the "feature normalization" pass of Preprocessor.build_from_path
 * (scripts/preprocessor/preprocessor.py:113-144) with its _remove_outlier (:647-660) and _normalize (:624-645), and
 * the energy pass of scripts/preprocessor/augmenter.py:330-398, none of which can run until every variant is a file.
 *
 * vo_corpus_stats: feature VO_STATS_ENERGY reads ch_energy, VO_STATS_KURTOSIS ch_kurtosis (VO_ERR_INVALID when the
 * corpus has no such array).  Row b of plan (n_rows, 5), as for vo_augment_batch, stands for the array
 * v[j] = x[sigma(j mod n')], j < L = n' r, in fp64 (m_mel plays no part beyond its sign).  Per row, as
 * _remove_outlier: p25, p75 = np.percentile(v, 25 / 75) (method "linear": h = (L - 1) q on the sorted array,
 * t = h - floor(h), a + (b - a) t for t < 0.5 and b - (b - a) (1 - t) otherwise, every operation rounded once),
 * lower = p25 - 1.5 (p75 - p25), upper = p75 + 1.5 (p75 - p25); v[j] is kept iff lower < v[j] < upper, both strict:
 * a row whose quartiles coincide (L = 1, all values equal) keeps nothing.  Then, as StandardScaler and _normalize,
 * out (6 doubles, device memory) =
 *   [0] the number of kept values of all rows, [1] their mean, [2] their population standard deviation (ddof 0;
 *   1.0 where it is zero, and mean 0, std 1 when nothing was kept at all), [3], [4] the smallest and largest raw
 *   value of the utterances that an accepted row names, kept or not (+inf, -inf when no row was accepted),
 *   [5] the number of rows that kept at least one value.
 * (x - mean) / std is monotone, so the min and max of stats.json are ([3] - [1]) / [2] and ([4] - [1]) / [2].
 * A row is refused on the device by vo_augment_batch's rules in their order, without its caps: VO_AUG_BAD_ROW, then
 * VO_STATS_CHARS_OVER for L > VO_STATS_MAX_CHARS (never truncated); a refused row contributes nothing, and its code
 * goes to status[b] (status (n_rows) int32, or NULL).  Non-finite values are the caller's responsibility: a row
 * that contains a NaN keeps nothing, as numpy's comparisons give, and nothing is promised about [3] and [4] then.
 * workspace: vo_corpus_stats_workspace_size(n_rows) bytes of device memory, 8-byte aligned, written in full.
 * Two launches (one workgroup per row, then one that folds the rows' (count, mean, M2) in a fixed order); no atomics,
 * so two calls give the same bits.  Allocates nothing, never synchronises, reads nothing on the host, plan included:
 * graph-capturable, and a plan rewritten in place is what a replay reads.
 *
 * vo_corpus_normalize: values[i] = (float)(((double)values[i] - stats[1]) / stats[2]) in place for i < n, stats
 * being the out of vo_corpus_stats in device memory, read on the device: stream-ordered behind that call with no
 * host round trip.  Equal to numpy's float64 (x - mean) / std followed by a cast to float32, bit for bit. */
#define VO_STATS_ENERGY 0
#define VO_STATS_KURTOSIS 1
#define VO_STATS_MAX_CHARS 4096
#define VO_STATS_CHARS_OVER 4
int64_t vo_corpus_stats_workspace_size(int n_rows);
int vo_corpus_stats(const vo_corpus* c, const int32_t* plan, int n_rows, int feature, void* workspace,
                    int64_t workspace_bytes, double* out, int32_t* status, void* stream);
int vo_corpus_normalize(float* values, int64_t n, const double* stats, void* stream);

/* HiFi-GAN training batches (additive): aligned (mel, audio) segments cut on the device from
 * the packed corpus and the base utterances' waveforms beside it, and the random draw of their rows.  The rules are
 * this project's own (the reference trains no vocoder); they follow the fine-tuning branch of HiFi-GAN's MelDataset:
 * the mel from the corpus, the audio cropped at mel_start * hop.
 *
 * vo_wave_corpus: the waveforms of the U utterances of a vo_corpus, in its order, packed flat in device memory.
 * Utterance u has N = n_samples[u] >= 1 samples at sample_off[u] of wav; every sample_off[u] is a multiple of 8 (the
 * gaps are padding nobody reads) and sample_off[U] is the packed length, so that with hop % 8 == 0 a segment starts
 * on a 16-byte boundary of int16 samples and a 32-byte one of fp32.  wav is int16 (is_int16 != 0; PCM as the files
 * hold it) or fp32.
 *
 * vo_segment_batch: plan (B, 2) int32 in device memory, row b = src, start (in frames).  With F frames and N samples
 * of utterance src, an accepted row writes
 *   y[b, i] = wav[sample_off[src] + start hop + i] for start hop + i < N, else 0.0f: an fp32 sample bit for bit (no
 *     clipping), an int16 sample s as (float)s / max_wav_value, one IEEE float32 division;
 *   x[b, f, :] = mel[frame_off[src] + start + f, :] for start + f < F, else mel_pad;
 *   frames[b] = min(fps, F - start), status[b] = VO_SEG_OK.
 * A row is refused on the device, never raised, when src is outside [0, U), start < 0 or start > max(F - fps, 0):
 * status[b] = VO_SEG_BAD_ROW, y all 0.0f, x all mel_pad, frames[b] = 0; the other rows are unaffected.  Outputs y
 * (B, fps hop) fp32, x (B, fps, n_mels) fp32 (channels-last: what the generator's training forward reads), frames (B)
 * int32, status (B) int32; every element of every output is written.  VO_ERR_INVALID, nothing launched: a null
 * pointer, w->U != c->U, B outside [1, 65535], fps < 1, hop < 1, fps hop or fps n_mels at or above 2^31.  start hop
 * and every offset are formed in 64 bits.  Samples move as 16-byte vectors when hop % 8 == 0 and wav and y are
 * 16-byte aligned, frames when n_mels % 4 == 0 and mel and x are; element by element otherwise.
 *
 * vo_segment_plan: the draw.  order (n_order) int32, an epoch's utterance order (the host shuffles it and rewrites it
 * in place); counter, one int64 in device memory >= 0, the number of rows drawn so far.  Row b of plan (B, 2) is drawn
 * from k = counter + b: src = order[k mod n_order]; (src, 0) when src is outside [0, U) (vo_segment_batch refuses it);
 * otherwise start = (uint64(w) span) >> 32 with span = F - fps + 1 for F > fps, else 1 (at most 2^31), and w word 0 of
 * Philox4x32-10 (Salmon et al. 2011: multipliers 0xD2511F53, 0xCD9E8D57, key increments 0x9E3779B9, 0xBB67AE85) of the
 * counter words (k lo, k hi, 0, 0) under the key (seed lo, seed hi).  Then counter <- counter + B: a replay of a
 * captured call draws the next B rows by itself.  One workgroup; no atomics.  VO_ERR_INVALID: a null pointer,
 * n_order < 1, B outside [1, 65535], fps < 1.
 *
 * Both are one launch each, allocate nothing, never synchronise and read nothing on the host: graph-capturable, and
 * a plan, an order or a counter rewritten in place is what a replay reads. */
#define VO_SEG_OK 0
#define VO_SEG_BAD_ROW 1
typedef struct vo_wave_corpus {
  int32_t U;
  const int64_t* sample_off;  /* (U + 1), in samples; multiples of 8 */
  const int64_t* n_samples;   /* (U) */
  const void* wav;            /* (sample_off[U]) int16 or fp32 */
  int32_t is_int16;
  float max_wav_value;
} vo_wave_corpus;
int vo_segment_batch(const vo_corpus* c, const vo_wave_corpus* w, const int32_t* plan, int B, int fps, int hop,
                     float mel_pad, float* y, float* x, int32_t* frames, int32_t* status, void* stream);
int vo_segment_plan(const vo_corpus* c, const int32_t* order, int n_order, int64_t* counter, uint64_t seed, int B,
                    int fps, int32_t* plan, void* stream);

/* Sample-rate conversion (additive): band-limited interpolation with a Kaiser-windowed sinc,
 * in front of the mel front end (the reference's librosa.load(path, sr=22050), scripts/preprocessor/preprocessor.py:385,
 * and its wav[int(sr * start):], :391) and behind the vocoder.  The rule is this project's own:
 *   constants   Z = 64 zero crossings, ROLLOFF = 0.9475937167399596, BETA = 14.769656459379492;
 *   geometry    g = gcd(sr_in, sr_out), O = sr_in / g, M = sr_out / g; c = min(O, M) ROLLOFF / O; W = ceil(Z / c) the
 *               half width in input samples; T = 2 W + 1 taps.  48000 -> 22050: O, M, W, T = 320, 147, 148, 297;
 *               22050 -> 48000: 147, 320, 68, 137;
 *   supported   O, M <= 1024, O / M <= 8, sr_in != sr_out.  Every other pair is refused with a message naming the
 *               reduced pair and the limits; no nearby ratio is ever run in its place;
 *   table       (M, T) fp32 row-major, computed in double and rounded once: with t = c (j - W - r / M),
 *               h[r][j] = c sinc(t) I0(BETA sqrt(1 - (t / Z)^2)) / I0(BETA) for |t| < Z, else 0; sinc(t) = sin(pi t) /
 *               (pi t), sinc(0) = 1;
 *   output n    of a row x of n_b samples (x[k] = 0 outside [0, n_b)): q = (n O) div M, r = (n O) mod M in 64 bits,
 *               res[n] = sum_j h[r][j] x[q - W + j] in fp32, j ascending in one fused multiply-add chain;
 *   length      L_b = ceil(n_b M / O), in 64 bits.
 *
 * Host only, like vo_conv1d_plan (no HIP call, no GPU needed): vo_resample_geometry gives O, M, W of two rates
 * (VO_ERR_INVALID for a refused pair or a rate < 1), vo_resample_len gives L of n samples (0 for n <= 0), and
 * vo_resample_table fills the M T coefficients of a reduced pair into host memory.
 *
 * vo_resample: x (B, N) with row stride N, fp32 or int16 (x_is_int16; a sample s is read as (float)s / max_wav_value,
 * one IEEE division, as vo_segment_batch reads it); lens (B) device int32 or NULL (every row is N): n_b =
 * clamp(lens[b], 0, N), and no sample at or past n_b is read; skip (B) device int32 or NULL (0): output samples
 * dropped from the front, clamped on the device to [0, L_b]; table: the device copy of vo_resample_table(O, M).  With
 * m_b = clamp(L_b - skip_b, 0, N_out): y[b, i] = res_b[i + skip_b] for i < m_b and 0.0f (int16 0) for m_b <= i <
 * N_out -- every element of y (B, N_out) is written -- and out_lens[b] = m_b (NULL: not wanted).  y is fp32, or int16
 * (y_is_int16) stored by the rule of vo_conv_post_pcm16: clamp(trunc(v pcm_scale)), NaN -> 0.  An output's bits
 * depend on its row's n_b samples, on n and on the table alone: not on the batch, the tile, skip, N, N_out or the
 * element types.  One launch, allocates nothing, never synchronises, reads nothing on the host: graph-capturable, and
 * a replay follows x, lens and skip rewritten in place.  VO_ERR_INVALID, nothing launched: a null x, y or table; B
 * outside [1, 65535]; N < 1 or N_out < 1 (or N_out within 256 of 2^31); an (O, M) the geometry refuses or that is not
 * reduced; max_wav_value (int16 input) or pcm_scale (int16 output) not finite and positive. */
int vo_resample_geometry(int64_t sr_in, int64_t sr_out, int32_t* O, int32_t* M, int32_t* W);
int64_t vo_resample_len(int64_t n, int O, int M);
int vo_resample_table(int O, int M, float* host_out);
int vo_resample(const void* x, int x_is_int16, float max_wav_value, int B, int N, const int32_t* lens,
                const int32_t* skip, const float* table, int O, int M, void* y, int y_is_int16, float pcm_scale,
                int N_out, int32_t* out_lens, void* stream);

/* ------------------------------------------------------------------ optimizer
 * Multi-tensor Adam (decoupled = 0: L2 weight decay on the gradient) / AdamW (decoupled = 1) step over
 * nt fp32 tensors (tables of device pointers and element counts, host memory), torch's
 * single-tensor update order; lr and step (the steps taken so far) are device scalars read by the
 * kernels, so the update is graph-capturable.  vo_opt_step_increment(step) advances the counter
 * (after every vo_adam_multi call of a step).  Replaces torch.optim.Adam behind ScheduledOptim
 * (scripts/model/optimizer.py:9-15) and the HiFi-GAN V1 recipe's AdamW. */
int vo_adam_multi(int nt, float* const* p, const float* const* g, float* const* m, float* const* v,
                  const int64_t* numel, const float* lr, const float* step, float beta1, float beta2, float eps,
                  float weight_decay, int decoupled, void* stream);
int vo_opt_step_increment(float* step, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VONOMA_H_ */
