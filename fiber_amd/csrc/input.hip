// On-device input pipeline for the fused-backbone path (gfx950): what the reference does per sample on CPU dataloader
// workers, moved behind the H2D copy so that the loader only has to decode and ship raw bytes.
//
//   1. image transform  -- coarse_grained/fiber/transforms/transform.py:10-17 `albef_transform`:
//        torchvision Resize((S,S), interpolation=BICUBIC) on a PIL RGB image -> ToTensor -> Normalize(mean, std)
//      i.e. Pillow's ImagingResample (third party, src/libImaging/Resample.c; stable since Pillow 3.x; not in /root/reference):
//      separable two-pass CONVOLUTION resize (horizontal, then vertical) with an anti-aliasing bicubic kernel (a = -0.5,
//      support 2 x max(scale, 1)), per-output-pixel coefficient windows normalised in double precision and quantised to 22-bit
//      fixed point, 8-bit rounding after EACH pass.  Restated here operation by operation (integer and double arithmetic
//      in Pillow's order, no fused multiply-add) so that the result is bit-identical to PIL's, then x/255, (x - mean)/std in
//      fp32 as ToTensor / Normalize do.  Oracle: oracle/image_ref.py (numpy), pinned against PIL itself.
//   2. MLM masking      -- datamodule_base.py:52 `DataCollatorForLanguageModeling(mlm_probability=0.15)` (transformers 4.6.0
//      `mask_tokens`): 15 % of the non-special tokens become labels; of those 80 % -> <mask>, 10 % -> a random token, 10 % keep.
//      The collator's torch.bernoulli / randint streams cannot be reproduced off the CPU generator; the draws here come from
//      the counter-based hash of common.h (seed, token index), so a batch is a pure function of (ids, seed).
//
//   3. detection input -- fine_grained/maskrcnn_benchmark/data/transforms/build.py:5-43 `build_transforms` (Resize(min, max) ->
//      RandomHorizontalFlip -> ToTensor -> Normalize(format)), structures/image_list.py:30-72 `to_image_list` and
//      structures/bounding_box.py:101-171 `BoxList.resize` / `transpose`: the same Pillow resampler with the BILINEAR filter
//      (triangle, support 1 x max(scale, 1)) to a per-image (oh, ow); the second pass also flips (a read index), reorders and
//      rescales the channels ("bgr255"), normalises and zero-pads, writing the whole [B, 3, Hp, Wp] canvas exactly once.
//
// Layouts: source images are uint8 HWC (as PIL / a JPEG decoder leaves them), ragged sizes inside a batch, addressed through
// a descriptor table; the output is the [B, 3, S, S] fp32 tensor FIBERTransformerSS.infer consumes.  Byte / integer work,
// HBM-bound: one thread per output pixel (3 channels), taps read through L1/L2 (neighbouring threads share them), the
// intermediate is the uint8 image Pillow itself materialises between its passes.
#include "common.h"

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;      // Pillow: 22-bit fixed-point coefficients for 8-bit channels

struct ImgDesc {                                // one per image, built by the host (fiber_amd/data.py)
  long long src;                                // device pointer: uint8 [H][W][3] (row stride = src_stride bytes)
  int H, W, src_stride;
  int ksize_h, ksize_v;                         // coefficient window lengths (fiber_resample_ksize)
  int tmp_off;                                  // byte offset of this image's [H][S][3] intermediate in `tmp`
  int coef_h_off, coef_v_off;                   // int offsets of its [S][2 + ksize] tables (bounds + coefficients) in `coef`
};

#pragma clang fp contract(off)
// Pillow Resample.c filters, selected by their support: 2 = bicubic_filter (a = -0.5), 1 = bilinear_filter (the triangle)
template <int SUPPORT>
__device__ double resample_filter(double x) {
  if (x < 0.0) x = -x;
  if constexpr (SUPPORT == 2) {
    const double a = -0.5;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
  } else {
    static_assert(SUPPORT == 1, "bicubic (2) or bilinear (1)");
    if (x < 1.0) return 1.0 - x;
    return 0.0;
  }
}

// Pillow precompute_coeffs + normalize_coeffs_8bpc for output coordinate xx of an axis resized in_size -> out_size.
// table row: [xmin, xmax, k_0 .. k_{ksize-1}]
template <int SUPPORT>
__device__ void coeff_row(int in_size, int out_size, int ksize, int xx, int* row) {
#pragma clang fp contract(off)
  if (in_size == out_size) {                     // Pillow skips a pass whose size does not change (ImagingResample need_*)
    row[0] = xx; row[1] = 1; row[2] = 1 << PRECISION_BITS;
    for (int x = 1; x < ksize; ++x) row[2 + x] = 0;
    return;
  }
  const double scale = (double)in_size / out_size;
  double filterscale = scale;
  if (filterscale < 1.0) filterscale = 1.0;
  const double support = (double)SUPPORT * filterscale;
  const double center = (xx + 0.5) * scale;
  const double ss = 1.0 / filterscale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in_size) xmax = in_size;
  xmax -= xmin;
  double ww = 0.0;
  for (int x = 0; x < xmax; ++x) ww += resample_filter<SUPPORT>((x + xmin - center + 0.5) * ss);
  row[0] = xmin;
  row[1] = xmax;
  for (int x = 0; x < ksize; ++x) {
    double w = 0.0;
    if (x < xmax) {
      w = resample_filter<SUPPORT>((x + xmin - center + 0.5) * ss);
      if (ww != 0.0) w /= ww;
    }
    row[2 + x] = w < 0 ? (int)(-0.5 + w * (1 << PRECISION_BITS)) : (int)(0.5 + w * (1 << PRECISION_BITS));
  }
}

__global__ __launch_bounds__(128) void resample_coeffs_kernel(const ImgDesc* descs, int* coef, int S) {
  const ImgDesc d = descs[blockIdx.y];
  const int t = blockIdx.x * 128 + threadIdx.x;
  if (t < S) coeff_row<2>(d.W, S, d.ksize_h, t, coef + d.coef_h_off + (size_t)t * (2 + d.ksize_h));
  else if (t < 2 * S) coeff_row<2>(d.H, S, d.ksize_v, t - S, coef + d.coef_v_off + (size_t)(t - S) * (2 + d.ksize_v));
}

__device__ __forceinline__ int clip8(int ss) {
  const int v = ss >> PRECISION_BITS;            // arithmetic shift, as Pillow's lookup index
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// one pixel of pass 1: o[c] = clip8(2^21 + sum_x src_row[xmin + x][c] * k[x]), row = [xmin, xmax, k_0 ..]
__device__ __forceinline__ void resample_h_pixel(const unsigned char* src_row, const int* row, unsigned char* o) {
  const int xmin = row[0], xmax = row[1];
  const unsigned char* sp = src_row + (size_t)xmin * 3;
  int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
  for (int x = 0; x < xmax; ++x) {
    const int k = row[2 + x];
    s0 += sp[3 * x] * k; s1 += sp[3 * x + 1] * k; s2 += sp[3 * x + 2] * k;
  }
  o[0] = (unsigned char)clip8(s0); o[1] = (unsigned char)clip8(s1); o[2] = (unsigned char)clip8(s2);
}

// pass 1: tmp[y][xx][c] = clip8(2^21 + sum_x src[y][xmin + x][c] * k[x])
__global__ __launch_bounds__(256) void resample_h_kernel(const ImgDesc* descs, const int* coef, unsigned char* tmp, int S) {
  const ImgDesc d = descs[blockIdx.z];
  const int xx = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (y >= d.H || xx >= S) return;
  resample_h_pixel(reinterpret_cast<const unsigned char*>(d.src) + (size_t)y * d.src_stride,
                   coef + d.coef_h_off + (size_t)xx * (2 + d.ksize_h), tmp + d.tmp_off + ((size_t)y * S + xx) * 3);
}

// pass 2 + ToTensor + Normalize: out[b][c][yy][xx] = (clip8(...) / 255 - mean[c]) / std[c]   (fp32, each op rounded)
__global__ __launch_bounds__(256) void resample_v_norm_kernel(const ImgDesc* descs, const int* coef, const unsigned char* tmp,
                                                              float* out, int S, float m0, float m1, float m2, float d0, float d1,
                                                              float d2) {
#pragma clang fp contract(off)
  const ImgDesc d = descs[blockIdx.z];
  const int xx = blockIdx.x * 256 + threadIdx.x, yy = blockIdx.y;
  if (xx >= S) return;
  const int* row = coef + d.coef_v_off + (size_t)yy * (2 + d.ksize_v);
  const int ymin = row[0], ymax = row[1];
  const unsigned char* tp = tmp + d.tmp_off + ((size_t)ymin * S + xx) * 3;
  int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
  for (int y = 0; y < ymax; ++y) {
    const int k = row[2 + y];
    const unsigned char* p = tp + (size_t)y * S * 3;
    s0 += p[0] * k; s1 += p[1] * k; s2 += p[2] * k;
  }
  float* o = out + ((size_t)blockIdx.z * 3 * S + yy) * S + xx;
  const size_t plane = (size_t)S * S;
  o[0] = ((float)clip8(s0) / 255.0f - m0) / d0;
  o[plane] = ((float)clip8(s1) / 255.0f - m1) / d1;
  o[2 * plane] = ((float)clip8(s2) / 255.0f - m2) / d2;
}

// ---- detection input: bilinear resample to a per-image (oh, ow), flip, channel order / scale, normalise, zero-pad ----------------------
struct DetDesc {                                // one per image, built by the host (fiber_amd/data.py)
  long long src;                                // device pointer: uint8 [H][W][3] (row stride = src_stride bytes)
  int H, W, src_stride;
  int oh, ow;                                   // this image's size after Resize.get_size (oh <= Hp, ow <= Wp)
  int ksize_h, ksize_v;                         // fiber_resample_ksize_bilinear(W, ow), (H, oh)
  int tmp_off;                                  // byte offset (multiple of 16) of this image's [H][ow][3] intermediate in `tmp`
  int coef_h_off, coef_v_off;                   // int offsets of its [ow][2 + ksize_h] and [oh][2 + ksize_v] tables in `coef`
  int flip;                                     // RandomHorizontalFlip drawn on the host
  int tmp_pitch;                                // bytes per row of the intermediate: 3 * ow rounded up to a multiple of 4
};
static_assert(sizeof(DetDesc) == 56, "DetDesc is mirrored by fiber_amd/data.py");

struct BoxParam { float ratio_w, ratio_h; int flip; float new_w; int num_gt; };
static_assert(sizeof(BoxParam) == 20, "BoxParam is mirrored by fiber_amd/data.py");

__global__ __launch_bounds__(128) void det_coeffs_kernel(const DetDesc* descs, int* coef) {
  const DetDesc d = descs[blockIdx.y];
  const int t = blockIdx.x * 128 + threadIdx.x;
  if (t < d.ow) coeff_row<1>(d.W, d.ow, d.ksize_h, t, coef + d.coef_h_off + (size_t)t * (2 + d.ksize_h));
  else if (t - d.ow < d.oh) coeff_row<1>(d.H, d.oh, d.ksize_v, t - d.ow, coef + d.coef_v_off + (size_t)(t - d.ow) * (2 + d.ksize_v));
}

__global__ __launch_bounds__(256) void det_h_kernel(const DetDesc* descs, const int* coef, unsigned char* tmp) {
  const DetDesc d = descs[blockIdx.z];
  const int xx = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (y >= d.H || xx >= d.ow) return;
  resample_h_pixel(reinterpret_cast<const unsigned char*>(d.src) + (size_t)y * d.src_stride,
                   coef + d.coef_h_off + (size_t)xx * (2 + d.ksize_h), tmp + d.tmp_off + (size_t)y * d.tmp_pitch + (size_t)xx * 3);
}

// 12 consecutive bytes at p as three dwords, p at any byte offset from a 4-byte-aligned base: four aligned dword loads funnelled
// by the offset (v_alignbyte_b32) instead of twelve byte loads.  Reads up to 4 bytes past p + 12.
__device__ __forceinline__ void load12(const unsigned char* p, unsigned (&w)[3]) {
  const unsigned sh = (unsigned)(size_t)p & 3u;
  const unsigned* q = reinterpret_cast<const unsigned*>(p - sh);
  const unsigned w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3];
  w[0] = __builtin_amdgcn_alignbyte(w1, w0, sh);
  w[1] = __builtin_amdgcn_alignbyte(w2, w1, sh);
  w[2] = __builtin_amdgcn_alignbyte(w3, w2, sh);
}

// pass 2 + RandomHorizontalFlip + ToTensor + Normalize(format) + to_image_list: the whole padded canvas, written once.
// Block = 4 waves, one output row each; a lane owns 4 consecutive columns (one 16-byte store per plane, 1 KB per wave and plane).
// A wave whose row or column range lies in the padding neither reads a table nor the intermediate.
//   out[b][c][yy][xx] = lut[c][clip8(sum_y tmp[ymin + y][flip ? ow-1-xx : xx][bgr ? 2-c : c] * k[y])],
//   lut[c][v] = ((v / 255 [* 255]) - mean[c]) / std[c]
__global__ __launch_bounds__(256) void det_v_norm_pad_kernel(const DetDesc* descs, const int* coef, const unsigned char* tmp, float* out,
                                                             int Hp, int Wp, int bgr, int times255, float m0, float m1, float m2, float d0,
                                                             float d1, float d2) {
#pragma clang fp contract(off)
  // ToTensor + Normalize depend on (byte, output channel) only: 768 values, each by the reference's three or four correctly rounded fp32
  // operations, built once per block that lies inside its image (the divisions were 240 of the kernel's 550 VALU instructions per lane)
  __shared__ float lut[3][256];
  const DetDesc d = descs[blockIdx.z];
  if ((int)blockIdx.y * 4 < d.oh && (int)blockIdx.x * 256 < d.ow) {                  // block-uniform
    const int t = threadIdx.y * 64 + threadIdx.x;
    const float mean[3] = {m0, m1, m2}, sd[3] = {d0, d1, d2};
    float f = (float)t / 255.0f;                                                     // ToTensor
    if (times255) f = f * 255.0f;                                                    // Normalize: format "...255"
#pragma unroll
    for (int c = 0; c < 3; ++c) lut[c][t] = (f - mean[c]) / sd[c];
    __syncthreads();
  }
  const int x0 = (blockIdx.x * 64 + threadIdx.x) * 4;
  const int yy = __builtin_amdgcn_readfirstlane(blockIdx.y * 4 + threadIdx.y);       // wave-uniform: a wave is one threadIdx.y
  if (yy >= Hp || x0 >= Wp) return;
  float v[3][4] = {{0.0f, 0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f, 0.0f}};
  if (yy < d.oh && x0 < d.ow) {
    const int* row = coef + d.coef_v_off + (size_t)yy * (2 + d.ksize_v);
    const int ymin = row[0], ymax = row[1];
    const int nx = d.ow - x0 < 4 ? d.ow - x0 : 4;
    int s[4][3];                                  // s[j]: output column x0 + j
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j][0] = s[j][1] = s[j][2] = 1 << (PRECISION_BITS - 1);
    const size_t pitch = (size_t)d.tmp_pitch;
    const unsigned char* tp = tmp + d.tmp_off + (size_t)ymin * pitch;
    if (nx == 4) {                                // the 4 columns are 12 consecutive bytes of the intermediate, reversed when flipped
      const unsigned char* p = tp + (size_t)(d.flip ? d.ow - 4 - x0 : x0) * 3;
      int a[12];                                  // in memory order
#pragma unroll
      for (int i = 0; i < 12; ++i) a[i] = 1 << (PRECISION_BITS - 1);
      for (int y = 0; y < ymax; ++y) {
        const int k = row[2 + y];
        unsigned w[3];
        load12(p + (size_t)y * pitch, w);
#pragma unroll
        for (int i = 0; i < 12; ++i) a[i] += __mul24((int)((w[i >> 2] >> (8 * (i & 3))) & 0xffu), k);      // |k| <= 2^22
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) s[j][c] = d.flip ? a[3 * (3 - j) + c] : a[3 * j + c];
    } else {                                      // the image's last, partial group of columns: byte loads
      for (int y = 0; y < ymax; ++y) {
        const int k = row[2 + y];
        const unsigned char* p = tp + (size_t)y * pitch;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (j < nx) {
            const unsigned char* q = p + (size_t)(d.flip ? d.ow - 1 - x0 - j : x0 + j) * 3;
            s[j][0] += q[0] * k; s[j][1] += q[1] * k; s[j][2] += q[2] * k;
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < nx) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c][j] = lut[c][clip8(bgr ? s[j][2 - c] : s[j][c])];
      }
    }
  }
  const size_t plane = (size_t)Hp * Wp;
  float* o = out + ((size_t)blockIdx.z * 3 * Hp + yy) * Wp + x0;
  if ((Wp & 3) == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) *reinterpret_cast<f32x4*>(o + c * plane) = f32x4{v[c][0], v[c][1], v[c][2], v[c][3]};
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (x0 + j < Wp) o[c * plane + j] = v[c][j];
  }
}

// BoxList.resize then (flip) BoxList.transpose(FLIP_LEFT_RIGHT), in place on [B, G, 4] xyxy; rows g >= num_gt are zero.
__global__ __launch_bounds__(256) void det_boxes_kernel(float* boxes, const BoxParam* params, int B, int G) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * G) return;
  const BoxParam p = params[i / G];
  f32x4* bp = reinterpret_cast<f32x4*>(boxes) + i;
  f32x4 r = {0.0f, 0.0f, 0.0f, 0.0f};
  if (i % G < p.num_gt) {
    const f32x4 b = *bp;
    const float x0 = b[0] * p.ratio_w, y0 = b[1] * p.ratio_h, x1 = b[2] * p.ratio_w, y1 = b[3] * p.ratio_h;
    if (p.flip) r = f32x4{p.new_w - x1 - 1.0f, y0, p.new_w - x0 - 1.0f, y1};
    else r = f32x4{x0, y0, x1, y1};
  }
  *bp = r;
}

// MLM masking: one thread per token.  Draws: u_k = hash_u32(seed, 4 * index + k), k = 0 (select), 1 (replace with <mask>),
// 2 (replace with a random token), 3 (which token).  Thresholds are floor(p * 2^32).
__global__ __launch_bounds__(256) void mlm_mask_kernel(const long long* ids, long long* ids_mlm, long long* labels, long n,
                                                       unsigned long long seed, unsigned p_select, int mask_id, int vocab,
                                                       int special_lo, int special_hi) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long id = ids[i];
  const bool special = id >= special_lo && id <= special_hi;       // RoBERTa: <s> = 0, <pad> = 1, </s> = 2
  const bool masked = !special && hash_u32(seed, 4ull * i) < p_select;
  long long out = id;
  if (masked) {
    if (hash_u32(seed, 4ull * i + 1) < 3435973836u) out = mask_id;                       // 0.8 * 2^32
    else if (hash_u32(seed, 4ull * i + 2) < 2147483648u) out = hash_u32(seed, 4ull * i + 3) % (unsigned)vocab;   // 0.5
  }
  ids_mlm[i] = out;
  labels[i] = masked ? id : -100;
}

}  // namespace

// Coefficient window length Pillow allocates for an axis resized in_size -> out_size with a filter of the given support.
static int resample_ksize(int in_size, int out_size, double filter_support) {
  if (in_size <= 0 || out_size <= 0) return 0;
  double filterscale = (double)in_size / out_size;
  if (filterscale < 1.0) filterscale = 1.0;
  const double support = filter_support * filterscale;
  int c = (int)support;
  if ((double)c < support) ++c;                  // ceil
  return c * 2 + 1;
}
extern "C" int fiber_resample_ksize(int in_size, int out_size) { return resample_ksize(in_size, out_size, 2.0); }            // bicubic
extern "C" int fiber_resample_ksize_bilinear(int in_size, int out_size) { return resample_ksize(in_size, out_size, 1.0); }

// descs: device array of n ImgDesc (10 ints + 1 int64 each, see fiber_amd/data.py); coef / tmp: workspaces laid out by the
// host; out: fp32 [n, 3, S, S].  max_h: tallest source image of the batch (grid extent).  mean / std: 3 floats each (host).
extern "C" int fiber_resize_bicubic_norm_u8(const void* descs, int n, int* coef, void* tmp, float* out, int S, int max_h,
                                            const float* mean, const float* std, hipStream_t stream) {
  if (n <= 0) return FIBER_OK;
  if (S <= 0 || max_h <= 0 || !mean || !std) return FIBER_EINVAL;
  const ImgDesc* d = reinterpret_cast<const ImgDesc*>(descs);
  hipLaunchKernelGGL(resample_coeffs_kernel, dim3(cdiv(2 * S, 128), n), dim3(128), 0, stream, d, coef, S);
  hipLaunchKernelGGL(resample_h_kernel, dim3(cdiv(S, 256), max_h, n), dim3(256), 0, stream, d, coef,
                     reinterpret_cast<unsigned char*>(tmp), S);
  hipLaunchKernelGGL(resample_v_norm_kernel, dim3(cdiv(S, 256), S, n), dim3(256), 0, stream, d, coef,
                     reinterpret_cast<const unsigned char*>(tmp), out, S, mean[0], mean[1], mean[2], std[0], std[1], std[2]);
  FIBER_CHECK_LAUNCH();
  return FIBER_OK;
}

// descs: device array of n DetDesc (56 bytes each, see fiber_amd/data.py); coef / tmp: workspaces laid out by the host (tmp: 16-byte
// aligned, H * tmp_pitch bytes per image and 16 bytes of slack behind the last, which the dword reads of pass 2 may touch); out: fp32
// [n, 3, Hp, Wp], every element written.  max_h / max_oh / max_ow: grid extents (tallest source, largest resized size).  bgr: output
// channel c reads source channel 2 - c; times255: the "255" of Normalize's format.  mean / std: 3 floats each (host), by OUTPUT channel.
extern "C" int fiber_det_resize_norm_pad_u8(const void* descs, int n, int* coef, void* tmp, float* out, int Hp, int Wp, int max_h,
                                            int max_oh, int max_ow, int bgr, int times255, const float* mean, const float* std,
                                            hipStream_t stream) {
  if (n <= 0) return FIBER_OK;
  if (Hp <= 0 || Wp <= 0 || max_h <= 0 || max_oh <= 0 || max_ow <= 0 || max_oh > Hp || max_ow > Wp || !mean || !std) return FIBER_EINVAL;
  if (max_h > 65535 || cdiv(Hp, 4) > 65535 || n > 65535 || fiber_misaligned(16, out, tmp)) return FIBER_EINVAL;
  const DetDesc* d = reinterpret_cast<const DetDesc*>(descs);
  hipLaunchKernelGGL(det_coeffs_kernel, dim3(cdiv(max_oh + max_ow, 128), n), dim3(128), 0, stream, d, coef);
  hipLaunchKernelGGL(det_h_kernel, dim3(cdiv(max_ow, 256), max_h, n), dim3(256), 0, stream, d, coef, reinterpret_cast<unsigned char*>(tmp));
  hipLaunchKernelGGL(det_v_norm_pad_kernel, dim3(cdiv(Wp, 256), cdiv(Hp, 4), n), dim3(64, 4), 0, stream, d, coef,
                     reinterpret_cast<const unsigned char*>(tmp), out, Hp, Wp, bgr, times255, mean[0], mean[1], mean[2], std[0], std[1],
                     std[2]);
  FIBER_CHECK_LAUNCH();
  return FIBER_OK;
}

// boxes fp32 [B, G, 4] in place; params: device array of B records {float ratio_w, ratio_h; int32 flip; float new_w; int32 num_gt}.
extern "C" int fiber_det_boxes_f32(float* boxes, const void* params, int B, int G, hipStream_t stream) {
  if (B <= 0 || G <= 0) return FIBER_OK;
  if (!boxes || !params || fiber_misaligned(16, boxes) || (long long)B * G > 0x7fffffffLL) return FIBER_EINVAL;
  hipLaunchKernelGGL(det_boxes_kernel, dim3(cdiv(B * G, 256)), dim3(256), 0, stream, boxes, reinterpret_cast<const BoxParam*>(params), B, G);
  FIBER_CHECK_LAUNCH();
  return FIBER_OK;
}

// ids [n] int64 -> ids_mlm, labels (int64).  p_select = floor(mlm_probability * 2^32).
extern "C" int fiber_mlm_mask_i64(const long long* ids, long long* ids_mlm, long long* labels, long n, unsigned long long seed,
                                  unsigned p_select, int mask_id, int vocab, int special_lo, int special_hi, hipStream_t stream) {
  if (n <= 0) return FIBER_OK;
  if (vocab <= 0) return FIBER_EINVAL;
  hipLaunchKernelGGL(mlm_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, ids, ids_mlm, labels, n, seed,
                     p_select, mask_id, vocab, special_lo, special_hi);
  FIBER_CHECK_LAUNCH();
  return FIBER_OK;
}

// ---- training image transform: RandomResizedCrop + RandomHorizontalFlip + RandomAugment(N, M) + ToTensor + Normalize ------------------
// coarse_grained/fiber/transforms/transform.py:20-45 `albef_transform_randaug` with transforms/randaug.py.  Every random choice is made on
// the host (fiber_amd/data.py DeviceRandAugTransform.plan); the kernels below execute a plan:
//   crop + resize + flip : the bicubic resampler above on a sub-view (ImgDesc.src points at the crop's first pixel, the row stride is the
//                          source's), with a second pass that writes uint8 HWC and mirrors the output column;
//   per slot             : randaug_tables_kernel (one workgroup per image: histograms -> the slot's three 256-entry tables, only where the
//                          slot's op is AutoContrast / Equalize; Brightness needs no statistics) then one apply kernel that dispatches per
//                          image on the op code.  Table ops run in place; Sharpness and the affine gather read one uint8 image and write
//                          the other (RaSlot.src says which one holds the image when the slot starts: the host tracks the ping-pong).
//                          The last slot's apply writes ToTensor + Normalize in fp32 CHW instead of bytes.
// The statistics of slot k + 1 are those of slot k's OUTPUT: the launches are stream-ordered, one tables + one apply kernel per slot.
namespace {

enum RaOp : int { RA_IDENTITY = 0, RA_AUTOCONTRAST = 1, RA_EQUALIZE = 2, RA_BRIGHTNESS = 3, RA_SHARPNESS = 4, RA_SHEAR_X = 5,
                  RA_SHEAR_Y = 6, RA_TRANSLATE_X = 7, RA_TRANSLATE_Y = 8, RA_ROTATE = 9 };      // < 0: the slot was not applied

struct RaSlot {                                 // one per image and slot, built by the host (fiber_amd/data.py)
  int op;                                       // RaOp, or negative when the slot's coin said skip
  int src;                                      // which of the two uint8 images (0 / 1) holds this sample when the slot starts
  float factor;                                 // Brightness / Sharpness
  int pad;
  double m[6];                                  // the five geometric ops: the INVERSE affine map (dst -> src), as cv2.warpAffine inverts it
};
static_assert(sizeof(RaSlot) == 64, "RaSlot is mirrored by fiber_amd/data.py");

// pass 2 of the crop-resize, to bytes: out[b][yy][flip ? S-1-xx : xx][c] = clip8(sum_y tmp[ymin + y][xx][c] * k[y])
__global__ __launch_bounds__(256) void resample_v_u8_flip_kernel(const ImgDesc* descs, const int* flips, const int* coef,
                                                                 const unsigned char* tmp, unsigned char* out, int S, size_t pitch) {
  const ImgDesc d = descs[blockIdx.z];
  const int xx = blockIdx.x * 256 + threadIdx.x, yy = blockIdx.y;
  if (xx >= S) return;
  const int* row = coef + d.coef_v_off + (size_t)yy * (2 + d.ksize_v);
  const int ymin = row[0], ymax = row[1];
  const unsigned char* tp = tmp + d.tmp_off + ((size_t)ymin * S + xx) * 3;
  int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
  for (int y = 0; y < ymax; ++y) {
    const int k = row[2 + y];
    const unsigned char* p = tp + (size_t)y * S * 3;
    s0 += p[0] * k; s1 += p[1] * k; s2 += p[2] * k;
  }
  unsigned char* o = out + blockIdx.z * pitch + ((size_t)yy * S + (flips[blockIdx.z] ? S - 1 - xx : xx)) * 3;
  o[0] = (unsigned char)clip8(s0); o[1] = (unsigned char)clip8(s1); o[2] = (unsigned char)clip8(s2);
}

// One workgroup per image.  AutoContrast (randaug.py:13-43, cutoff 0) and Equalize (:46-67) need the three channel histograms of the
// image as it stands when the slot starts; Brightness (:119-125) only its factor.  luts: uint8 [n][3][256].
// Histograms: 16 waves, 16-byte loads (pitch is a multiple of 16; byte k of the image is channel k % 3 and 16 = 1 mod 3), LDS atomics on
// four copies (a wave uses copy wave % 4) so that a flat image does not serialise all 1024 lanes on one counter.
__global__ __launch_bounds__(1024) void randaug_tables_kernel(const RaSlot* slots, const unsigned char* buf0, const unsigned char* buf1,
                                                              size_t pitch, unsigned char* luts, int S) {
#pragma clang fp contract(off)
  const RaSlot sl = slots[blockIdx.x];
  if (sl.op < RA_AUTOCONTRAST || sl.op > RA_BRIGHTNESS) return;                          // block-uniform
  const int t = threadIdx.x;
  unsigned char* lut = luts + (size_t)blockIdx.x * 768;
  if (sl.op == RA_BRIGHTNESS) {
    if (t < 256) {
      float v = (float)t * sl.factor;
      v = v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v);
      const unsigned char b = (unsigned char)(int)v;
      lut[t] = b; lut[256 + t] = b; lut[512 + t] = b;
    }
    return;
  }
  __shared__ unsigned hist[4][768];
  __shared__ unsigned pre[768];                 // exclusive prefix sums of the histogram, per channel
  __shared__ int stat[3][3];                    // lo, hi, step
  for (int i = t; i < 4 * 768; i += 1024) (&hist[0][0])[i] = 0u;
  __syncthreads();
  const unsigned char* img = (sl.src ? buf1 : buf0) + blockIdx.x * pitch;
  const int nbytes = S * S * 3, nvec = nbytes >> 4;
  unsigned* h = hist[(t >> 6) & 3];
  const uint4* vp = reinterpret_cast<const uint4*>(img);
  for (int j = t; j < nvec; j += 1024) {
    const uint4 q = vp[j];
    const unsigned w[4] = {q.x, q.y, q.z, q.w};
    int c = j % 3;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      atomicAdd(&h[c * 256 + ((w[k >> 2] >> (8 * (k & 3))) & 0xffu)], 1u);
      c = c == 2 ? 0 : c + 1;
    }
  }
  for (int k = (nvec << 4) + t; k < nbytes; k += 1024) atomicAdd(&h[(k % 3) * 256 + img[k]], 1u);
  __syncthreads();
  if (t < 768) hist[0][t] += hist[1][t] + hist[2][t] + hist[3][t];
  __syncthreads();
  if (t < 3) {                                  // 256 bins per channel: a serial scan is shorter than its own reduction tree's barriers
    const unsigned* hc = hist[0] + t * 256;
    int lo = -1, hi = 0;
    unsigned acc = 0;
    for (int i = 0; i < 256; ++i) {
      pre[t * 256 + i] = acc;
      const unsigned v = hc[i];
      acc += v;
      if (v) { if (lo < 0) lo = i; hi = i; }
    }
    stat[t][0] = lo; stat[t][1] = hi;
    stat[t][2] = (int)((acc - hc[hi]) / 255u);  // Equalize: the non-zero bins except the LAST non-zero one, // 255
  }
  __syncthreads();
  if (t < 768) {
    const int c = t >> 8, i = t & 255, lo = stat[c][0], hi = stat[c][1], step = stat[c][2];
    int v = i;
    if (sl.op == RA_AUTOCONTRAST) {
      if (hi > lo) {                            // fp64, every operation rounded on its own (numpy does not fuse)
        const double scale = 255.0 / (double)(hi - lo);
        const double offset = -(double)lo * scale;
        const double prod = (double)i * scale;
        double x = prod + offset;
        x = x < 0.0 ? 0.0 : (x > 255.0 ? 255.0 : x);
        v = (int)x;
      }
    } else if (step > 0) {
      const unsigned q = ((unsigned)(step >> 1) + pre[t]) / (unsigned)step;
      v = q > 255u ? 255 : (int)q;
    }
    lut[t] = (unsigned char)v;
  }
}

// One output pixel of one slot: o[c] from the image `img` (uint8 [S][S][3]) as it stands when the slot starts.
__device__ __forceinline__ void randaug_pixel(const RaSlot& sl, const unsigned char* img, const unsigned char* lut, const short* wtab,
                                              int S, int x, int y, int (&o)[3]) {
#pragma clang fp contract(off)
  const unsigned char* p = img + ((size_t)y * S + x) * 3;
  if (sl.op < RA_AUTOCONTRAST) {                // Identity, or not applied
    o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
  } else if (sl.op <= RA_BRIGHTNESS) {          // the three table ops
    o[0] = lut[p[0]]; o[1] = lut[256 + p[1]]; o[2] = lut[512 + p[2]];
  } else if (sl.op == RA_SHARPNESS) {
    // randaug.py:128-146: degenerate = cv2.filter2D(img, -1, [[1,1,1],[1,5,1],[1,1,1]] / 13) rounded to uint8 = (2 T + 13) / 26 (T / 13 is
    // never a half); out = uint8(degenerate + factor * (img - degenerate)) in fp32 on the interior, the outermost ring keeps the input.
    // .astype(np.uint8) WRAPS (no clamp): the low 8 bits of the value truncated toward zero.
    if (x == 0 || y == 0 || x == S - 1 || y == S - 1) {
      o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
    } else {
      const size_t rs = (size_t)S * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const unsigned char* q = p + c;
        const int T = q[-(ptrdiff_t)rs - 3] + q[-(ptrdiff_t)rs] + q[-(ptrdiff_t)rs + 3] + q[-3] + 5 * q[0] + q[3] + q[rs - 3] + q[rs] + q[rs + 3];
        const float deg = (float)((2 * T + 13) / 26);
        const float d = (float)q[0] - deg;
        const float r = deg + sl.factor * d;
        o[c] = (int)r & 255;
      }
    }
  } else {
    // cv2.warpAffine(INTER_LINEAR, BORDER_CONSTANT (128, 128, 128)), the generic fixed-point path: source coordinates in 1/1024, rounded
    // half-even from fp64, reduced to 1/32; 2 x 2 taps weighted by int16 weights that sum to 2^15 (wtab[fy * 32 + fx][k1 * 2 + k2]).
    const double AB = 1024.0;
    // every fp64 operation rounded on its own (contraction is off in this function), then round-half-even to int32
    const double ax = sl.m[0] * (double)x, bx = sl.m[3] * (double)x, ay = sl.m[1] * (double)y, by = sl.m[4] * (double)y;
    const double xr = ay + sl.m[2], yr = by + sl.m[5];
    const int ad = (int)rint(ax * AB), bd = (int)rint(bx * AB);
    const int X0 = (int)rint(xr * AB) + 16, Y0 = (int)rint(yr * AB) + 16;
    const int X = (X0 + ad) >> 5, Y = (Y0 + bd) >> 5;
    const int sx = X >> 5, sy = Y >> 5;
    if (sx >= S || sx + 1 < 0 || sy >= S || sy + 1 < 0) {
      o[0] = o[1] = o[2] = 128;
    } else {
      const short* w = wtab + (((Y & 31) << 5) + (X & 31)) * 4;
      int a0 = 16384, a1 = 16384, a2 = 16384;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int yy = sy + (k >> 1), xx = sx + (k & 1), wk = w[k];
        int p0 = 128, p1 = 128, p2 = 128;
        if (yy >= 0 && yy < S && xx >= 0 && xx < S) {
          const unsigned char* q = img + ((size_t)yy * S + xx) * 3;
          p0 = q[0]; p1 = q[1]; p2 = q[2];
        }
        a0 += wk * p0; a1 += wk * p1; a2 += wk * p2;
      }
      a0 >>= 15; a1 >>= 15; a2 >>= 15;
      o[0] = a0 < 0 ? 0 : (a0 > 255 ? 255 : a0);
      o[1] = a1 < 0 ? 0 : (a1 > 255 ? 255 : a1);
      o[2] = a2 < 0 ? 0 : (a2 > 255 ? 255 : a2);
    }
  }
}

// A slot that is not the last: bytes to bytes.  Blocks of an image whose slot does nothing return at once.
__global__ __launch_bounds__(256) void randaug_apply_u8_kernel(const RaSlot* slots, unsigned char* buf0, unsigned char* buf1, size_t pitch,
                                                               const unsigned char* luts, const short* wtab, int S) {
  const RaSlot sl = slots[blockIdx.y];
  if (sl.op < RA_AUTOCONTRAST) return;                                                   // block-uniform
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= S * S) return;
  unsigned char* src = (sl.src ? buf1 : buf0) + blockIdx.y * pitch;
  unsigned char* dst = sl.op <= RA_BRIGHTNESS ? src : (sl.src ? buf0 : buf1) + blockIdx.y * pitch;      // table ops: in place
  int o[3];
  randaug_pixel(sl, src, luts + (size_t)blockIdx.y * 768, wtab, S, pix % S, pix / S, o);
  unsigned char* q = dst + (size_t)pix * 3;
  q[0] = (unsigned char)o[0]; q[1] = (unsigned char)o[1]; q[2] = (unsigned char)o[2];
}

// The last slot, fused with ToTensor + Normalize: out[b][c][y][x] = (v / 255 - mean[c]) / std[c], the fp32 expression of
// resample_v_norm_kernel, evaluated once per (byte, channel) and block.  out_u8 (optional): the byte image [n][S][S][3] before ToTensor.
__global__ __launch_bounds__(256) void randaug_apply_norm_kernel(const RaSlot* slots, const unsigned char* buf0, const unsigned char* buf1,
                                                                 size_t pitch, const unsigned char* luts, const short* wtab, int S,
                                                                 float* out, unsigned char* out_u8, float m0, float m1, float m2,
                                                                 float d0, float d1, float d2) {
#pragma clang fp contract(off)
  __shared__ float norm[3][256];
  {
    const float f = (float)threadIdx.x / 255.0f;
    norm[0][threadIdx.x] = (f - m0) / d0;
    norm[1][threadIdx.x] = (f - m1) / d1;
    norm[2][threadIdx.x] = (f - m2) / d2;
  }
  __syncthreads();
  const RaSlot sl = slots[blockIdx.y];
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= S * S) return;
  int o[3];
  randaug_pixel(sl, (sl.src ? buf1 : buf0) + blockIdx.y * pitch, luts + (size_t)blockIdx.y * 768, wtab, S, pix % S, pix / S, o);
  const size_t plane = (size_t)S * S;
  float* q = out + (size_t)blockIdx.y * 3 * plane + pix;
  q[0] = norm[0][o[0]]; q[plane] = norm[1][o[1]]; q[2 * plane] = norm[2][o[2]];
  if (out_u8) {
    unsigned char* u = out_u8 + ((size_t)blockIdx.y * plane + pix) * 3;
    u[0] = (unsigned char)o[0]; u[1] = (unsigned char)o[1]; u[2] = (unsigned char)o[2];
  }
}

}  // namespace

// RandomResizedCrop + RandomHorizontalFlip to bytes.  descs: n ImgDesc whose src / H / W describe the CROP (src = first pixel of the box,
// src_stride = the source's row stride); flips: device int32 [n]; out_u8: uint8, image b at b * pitch as [S][S][3] (pitch >= 3 S^2, a
// multiple of 16).  coef / tmp / max_h as fiber_resize_bicubic_norm_u8 (max_h = tallest crop).  3 kernels.
extern "C" int fiber_crop_resize_flip_u8(const void* descs, const int* flips, int n, int* coef, void* tmp, void* out_u8, long long pitch,
                                         int S, int max_h, hipStream_t stream) {
  if (n <= 0) return FIBER_OK;
  if (S <= 0 || S > 16384 || max_h <= 0 || max_h > 65535 || n > 65535 || !descs || !flips || !coef || !tmp || !out_u8) return FIBER_EINVAL;
  if (pitch < 3ll * S * S || (pitch & 15) || fiber_misaligned(16, out_u8)) return FIBER_EINVAL;
  const ImgDesc* d = reinterpret_cast<const ImgDesc*>(descs);
  hipLaunchKernelGGL(resample_coeffs_kernel, dim3(cdiv(2 * S, 128), n), dim3(128), 0, stream, d, coef, S);
  hipLaunchKernelGGL(resample_h_kernel, dim3(cdiv(S, 256), max_h, n), dim3(256), 0, stream, d, coef,
                     reinterpret_cast<unsigned char*>(tmp), S);
  hipLaunchKernelGGL(resample_v_u8_flip_kernel, dim3(cdiv(S, 256), S, n), dim3(256), 0, stream, d, flips, coef,
                     reinterpret_cast<const unsigned char*>(tmp), reinterpret_cast<unsigned char*>(out_u8), S, (size_t)pitch);
  FIBER_CHECK_LAUNCH();
  return FIBER_OK;
}

// One RandomAugment slot over the batch.  slots: n RaSlot (64 bytes each: int32 op, src; float factor; int32 pad; double m[6]); buf0 /
// buf1: the two uint8 images per sample (layout of fiber_crop_resize_flip_u8's out_u8); luts: uint8 [n][3][256] workspace; wtab: int16
// [1024][4] bilinear weights.  out == NULL: a slot that is not the last (bytes to bytes).  out != NULL: the last slot, fp32 [n,3,S,S] =
// Normalize(ToTensor(.)) with mean / std (HOST pointers to 3 floats), and out_u8 (or NULL): uint8 [n,S,S,3], the image before ToTensor.
// 2 kernels whatever the ops are.
extern "C" int fiber_randaug_slot_u8(const void* slots, int n, void* buf0, void* buf1, long long pitch, void* luts, const void* wtab,
                                     int S, float* out, void* out_u8, const float* mean, const float* std, hipStream_t stream) {
  if (n <= 0) return FIBER_OK;
  if (S <= 0 || S > 16384 || n > 65535 || !slots || !buf0 || !buf1 || !luts || !wtab) return FIBER_EINVAL;
  if (pitch < 3ll * S * S || (pitch & 15) || fiber_misaligned(16, buf0, buf1)) return FIBER_EINVAL;
  if (out && (!mean || !std)) return FIBER_EINVAL;
  const RaSlot* s = reinterpret_cast<const RaSlot*>(slots);
  const unsigned char *b0 = reinterpret_cast<unsigned char*>(buf0), *b1 = reinterpret_cast<unsigned char*>(buf1);
  unsigned char* l = reinterpret_cast<unsigned char*>(luts);
  const short* w = reinterpret_cast<const short*>(wtab);
  hipLaunchKernelGGL(randaug_tables_kernel, dim3(n), dim3(1024), 0, stream, s, b0, b1, (size_t)pitch, l, S);
  if (out)
    hipLaunchKernelGGL(randaug_apply_norm_kernel, dim3(cdiv(S * S, 256), n), dim3(256), 0, stream, s, b0, b1, (size_t)pitch, l, w, S, out,
                       reinterpret_cast<unsigned char*>(out_u8), mean[0], mean[1], mean[2], std[0], std[1], std[2]);
  else
    hipLaunchKernelGGL(randaug_apply_u8_kernel, dim3(cdiv(S * S, 256), n), dim3(256), 0, stream, s, const_cast<unsigned char*>(b0),
                       const_cast<unsigned char*>(b1), (size_t)pitch, l, w, S);
  FIBER_CHECK_LAUNCH();
  return FIBER_OK;
}
