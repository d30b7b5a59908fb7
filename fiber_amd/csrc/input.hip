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
