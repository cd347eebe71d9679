// Glyph stretching on the device: every character's glyph resized to its own pixel
// width, centred in its cell, with the margins and ToTensor, in one launch that reads its ids, lengths and
// widths on the device -- a captured graph follows a width changed in place.
//
// Reference (host, PIL, per character):
//   Generator.draw (scripts/preprocessor/visualtext_generator.py:23-46): c_im.resize((width, fontsize)) of a
//     fontsize x fontsize render; prediction.ipynb: c_im.resize((int(new_w), fs)) with the user's rate;
//   then the layout of glyph.hip (character_padding_forinput, pad_2D_gray_image, ToTensor).
// Image.resize with its default filter on such an image is the bicubic resample, horizontal pass only, in PIL's
// 8-bit fixed point: double coefficients normalised per output column and rounded to 22 fractional bits, an int32
// sum started at 2^21, shifted down and clamped.  The coefficients depend on (source width, target width, column)
// alone: vo_glyph_stretch_table builds them once on the host, for every target width up to the cell, and the
// kernel does integer work only.

#include <math.h>

#include "vo_common.h"

// the host arithmetic below is PIL's, operation for operation in IEEE double: a product fused into a sum rounds
// once where PIL rounds twice
#pragma clang fp contract(off)

namespace vo {

constexpr int STRETCH_BITS = 22;       // PIL's PRECISION_BITS for 8-bit pixels: 32 - 8 - 2
constexpr int STRETCH_MAX_SRC = 64;    // source widths the table entries take
constexpr int STRETCH_MAX_CELL = 256;  // cell widths
constexpr int STRETCH_ROWS = 8;        // glyph rows of one workgroup

static double stretch_bicubic(double x) {  // PIL's bicubic_filter, a = -0.5
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

// record of column c at target width w: xmin, n, K[0 .. S), zeros past n (PIL's precompute_coeffs and
// normalize_coeffs_8bpc for a source box [0, S))
static void stretch_record(int S, int w, int c, int32_t* rec) {
  const double scale = (double)S / w;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = 2.0 * fs, ss = 1.0 / fs;
  const double center = (c + 0.5) * scale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > S) xmax = S;
  const int n = xmax - xmin;  // <= S
  double k[STRETCH_MAX_SRC];
  double ww = 0.0;
  for (int x = 0; x < n; ++x) {
    k[x] = stretch_bicubic((x + xmin - center + 0.5) * ss);
    ww += k[x];
  }
  rec[0] = xmin;
  rec[1] = n;
  for (int x = 0; x < S; ++x) rec[2 + x] = 0;
  for (int x = 0; x < n; ++x) {
    if (ww != 0.0) k[x] /= ww;
    rec[2 + x] = k[x] < 0 ? (int)(-0.5 + k[x] * (1 << STRETCH_BITS)) : (int)(0.5 + k[x] * (1 << STRETCH_BITS));
  }
}

// One workgroup per cell (b, t), t < T, and group of STRETCH_ROWS rows (blockIdx.z); workgroup t == T of a row
// writes what no cell covers: the left margin and the columns from margin + T cell to W_out.  A cell's workgroup
// stages its rows of the glyph and the w records of its width in LDS (record pitch odd: the lanes of a wave read
// one tap of consecutive records), then strides over its rows x cell pixels, x fastest.  The rows are split because
// the tap loop is a chain of LDS reads: at one workgroup per cell a CU holds one or two of them and nothing hides
// that latency (12.5 us at B = 32, T = 12).  ids, src_lens and widths are device data nobody
// has checked: a cell they put out of range is white, and w <= cell keeps every table index inside the (S, cell)
// table.
__global__ void __launch_bounds__(256) glyph_stretch_kernel(const uint8_t* __restrict__ atlas, int n_glyphs, int H, int S,
                                                            const int64_t* __restrict__ ids,
                                                            const int64_t* __restrict__ src_lens,
                                                            const int32_t* __restrict__ widths, int T, int cell,
                                                            int margin, int W_out, const int32_t* __restrict__ table,
                                                            float* __restrict__ out) {
  extern __shared__ __align__(16) int32_t stretch_lds[];
  const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
  const int y0 = blockIdx.z * STRETCH_ROWS, rows = min(STRETCH_ROWS, H - y0);  // rows >= 1 (launcher)
  float* orow = out + ((int64_t)b * H + y0) * W_out;
  if (t == T) {
    const int tail0 = margin + T * cell;  // <= W_out (launcher)
    const int nm = margin + (W_out - tail0);
    for (int i = tid; i < rows * nm; i += 256) {
      const int y = i / nm, j = i - y * nm;
      orow[(int64_t)y * W_out + (j < margin ? j : j - margin + tail0)] = 1.0f;
    }
    return;
  }
  const int64_t id = ids[(int64_t)b * T + t];
  const int wr = widths ? widths[(int64_t)b * T + t] : S;
  const bool white = t >= src_lens[b] || wr <= 0 || id < 0 || id >= n_glyphs;
  const int w = min(wr, cell);
  const int x0 = margin + t * cell;
  if (white) {  // uniform over the workgroup
    for (int i = tid; i < rows * cell; i += 256) {
      const int y = i / cell, c = i - y * cell;
      orow[(int64_t)y * W_out + x0 + c] = 1.0f;
    }
    return;
  }
  const int R = 2 + S, P = R | 1;
  int32_t* recs = stretch_lds;                                           // w records at a pitch of P
  uint8_t* glyph = reinterpret_cast<uint8_t*>(stretch_lds + cell * P);  // STRETCH_ROWS x S
  const int32_t* trec = table + (int64_t)(w * (w - 1) / 2) * R;
  for (int i = tid; i < w * R; i += 256) {
    const int r = i / R;
    recs[r * P + (i - r * R)] = trec[i];
  }
  const uint8_t* g = atlas + (id * H + y0) * S;
  for (int i = tid; i < rows * S; i += 256) glyph[i] = g[i];
  __syncthreads();
  const int pleft = (cell - w) / 2 + (cell - w) % 2;
  for (int i = tid; i < rows * cell; i += 256) {
    const int y = i / cell, c = i - y * cell;
    const int sc = c - pleft;
    int v = 255;
    if (sc >= 0 && sc < w) {
      const int32_t* rec = recs + sc * P;
      const int xmin = min(max(rec[0], 0), S);  // a table of another geometry still reads inside the glyph
      const int n = min(max(rec[1], 0), S - xmin);
      const uint8_t* src = glyph + y * S + xmin;
      int acc = 1 << (STRETCH_BITS - 1);
      for (int x = 0; x < n; ++x) acc += (int)src[x] * rec[2 + x];
      v = min(max(acc >> STRETCH_BITS, 0), 255);
    }
    orow[(int64_t)y * W_out + x0 + c] = __fdiv_rn((float)v, 255.f);
  }
}

}  // namespace vo

using namespace vo;

extern "C" int64_t vo_glyph_stretch_table_size(int src_w, int cell) {
  if (src_w < 1 || src_w > STRETCH_MAX_SRC || cell < 1 || cell > STRETCH_MAX_CELL) return -1;
  return (int64_t)cell * (cell + 1) / 2 * (2 + src_w) * (int64_t)sizeof(int32_t);
}

extern "C" int vo_glyph_stretch_table(int src_w, int cell, int32_t* table, int64_t table_bytes) {
  const int64_t need = vo_glyph_stretch_table_size(src_w, cell);
  VO_CHECK_ARG(need > 0, "glyph_stretch_table: src_w %d outside [1, %d] or cell %d outside [1, %d]", src_w,
               STRETCH_MAX_SRC, cell, STRETCH_MAX_CELL);
  VO_CHECK_ARG(table && table_bytes >= need, "glyph_stretch_table: the table needs %lld bytes, the buffer has %lld",
               (long long)need, (long long)(table ? table_bytes : 0));
  for (int w = 1; w <= cell; ++w)
    for (int c = 0; c < w; ++c) stretch_record(src_w, w, c, table + ((int64_t)w * (w - 1) / 2 + c) * (2 + src_w));
  return VO_OK;
}

extern "C" int vo_glyph_stretch(const uint8_t* atlas, int n_glyphs, int H, int src_w, const int64_t* ids,
                                const int64_t* src_lens, const int32_t* widths, int B, int T, int cell, int margin,
                                int W_out, const int32_t* table, float* out, void* stream) {
  VO_CHECK_ARG(atlas && ids && src_lens && table && out, "glyph_stretch: null pointer");
  VO_CHECK_ARG(src_w >= 1 && src_w <= STRETCH_MAX_SRC && cell >= 1 && cell <= STRETCH_MAX_CELL,
               "glyph_stretch: src_w %d outside [1, %d] or cell %d outside [1, %d]", src_w, STRETCH_MAX_SRC, cell,
               STRETCH_MAX_CELL);
  VO_CHECK_ARG(n_glyphs > 0 && H > 0 && H <= 65535 && B > 0 && B <= 65535 && T > 0 && margin >= 0,
               "glyph_stretch: bad sizes");
  VO_CHECK_ARG((int64_t)T * cell + 2 * (int64_t)margin <= W_out, "glyph_stretch: W_out %d below T cell + 2 margin = %lld",
               W_out, (long long)T * cell + 2 * (long long)margin);
  VO_CHECK_ARG((int64_t)n_glyphs * H * src_w < ((int64_t)1 << 31) && (int64_t)H * W_out < ((int64_t)1 << 31),
               "glyph_stretch: atlas or image rows past 2^31 elements");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  // 69 120 bytes at the most (cell 256, src_w 64); 11 208 for the packaged 24 / 102
  const size_t lds = (size_t)cell * ((2 + src_w) | 1) * sizeof(int32_t) + (size_t)STRETCH_ROWS * src_w;
  const dim3 grid((unsigned)T + 1, (unsigned)B, (unsigned)((H + STRETCH_ROWS - 1) / STRETCH_ROWS));
  hipLaunchKernelGGL(glyph_stretch_kernel, grid, dim3(256), lds, st, atlas, n_glyphs, H, src_w, ids, src_lens, widths, T,
                     cell, margin, W_out, table, out);
  VO_RETURN_LAUNCH();
}
