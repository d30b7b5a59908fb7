// FPN top-down pathway (gfx950): the DropBlock mask and the lateral + nearest-upsample merge of the fine-grained model's neck, forward and
// backward, on channels-last bf16 maps with fp32 arithmetic.
// Replaces, of the fine-grained reference (fine_grained/maskrcnn_benchmark/), modeling/backbone/fpn.py:95-110 (F.interpolate(mode="nearest",
// size=...), the add, the drop_block call) and layers/dropblock.py:33-77 (host torch.rand, the host-to-device copy, max_pool2d, the two
// multiplies and the batch-wide block_mask.sum()), together with what autograd runs behind them.
// The reference draws on the host and reads the normaliser through ATen reductions; here the draw is the counter-based hash of common.h
// (key by value + optional device base, as the dropout kernels: capturable in a hipGraph), the normaliser numel / kept stays in device
// memory, nothing synchronises, and every output element is written exactly once by one thread: no floating-point atomics, so two runs
// give the same bits.  The only atomic is the integer count of kept pixels.
//
// Nearest index rule (all kernels): src = min((int)floorf(dst * ((float)Hc / (float)H)), Hc - 1), the scale formed in fp32 -- what
// upsample_nearest2d computes when size= is given.  The exact rational dst * Hc / H differs from it (first at H = 58, Hc = 30).  The scale
// is divided on the host, so the device never rounds it differently.
#include "common.h"

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ int nearest_src(int dst, float scale, int n_src) {
  const int s = (int)floorf((float)dst * scale);
  return s < n_src - 1 ? s : n_src - 1;
}

// First dst in [0, n_dst] whose source index is >= target: the forward rule itself, bisected (it is monotone in dst)
__device__ __forceinline__ int first_child(int target, float scale, int n_src, int n_dst) {
  int lo = 0, hi = n_dst;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (nearest_src(mid, scale, n_src) >= target) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// dropblock.py:45 (the Bernoulli draw) and :61-74 (block mask).  One thread per pixel; with draw the pixel's own seed is stored and
// the neighbours' seeds are recomputed from (key, index), so no thread reads what another writes.
__global__ __launch_bounds__(256) void dropblock_mask_kernel(unsigned char* __restrict__ seeds, int draw, uint64_t seed,
                                                             const uint64_t* __restrict__ seed_base, uint32_t thresh, int half,
                                                             unsigned char* __restrict__ keep, int* __restrict__ kept, int B, int H, int W) {
  if (seed_base) seed += *seed_base;                       // graph replay: the per-step part of the key lives in device memory
  const long long n = (long long)B * H * W;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  bool k = false;
  if (i < n) {
    const int w = (int)(i % W), h = (int)((i / W) % H);
    const long long img = i - (long long)h * W - w;          // flat index of (b, 0, 0)
    bool any = false;
    for (int y = h - half; y <= h + half; ++y) {
      if (y < 0 || y >= H) continue;
      for (int x = w - half; x <= w + half; ++x) {
        if (x < 0 || x >= W) continue;
        const long long j = img + (long long)y * W + x;
        const bool s = draw ? hash_u32(seed, (uint64_t)j) < thresh : seeds[j] != 0;
        if (draw && j == i) seeds[i] = s ? 1 : 0;
        any |= s;
      }
    }
    k = !any;
    keep[i] = k ? 1 : 0;
  }
  const unsigned long long m = __ballot(k);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(kept, __popcll(m));
}

// fpn.py:97-110 forward.  One thread per 8 channels of one fine pixel; consecutive threads walk the channels, then the pixels of a row.
__global__ __launch_bounds__(256) void fpn_merge_fwd_kernel(const bf16* __restrict__ lateral, const bf16* __restrict__ coarse,
                                                            const unsigned char* __restrict__ keep, const int* __restrict__ kept,
                                                            bf16* __restrict__ inner, bf16* __restrict__ dropped, int B, int H, int W,
                                                            int C8, int Hc, int Wc, float sh, float sw) {
  const size_t nvec = (size_t)B * H * W * C8;
  const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
  if (i >= nvec) return;
  const int c8 = (int)(i % C8);
  const size_t pix = i / C8;
  const int w = (int)(pix % W), h = (int)((pix / W) % H), b = (int)(pix / ((size_t)W * H));
  const bf16x8 lv = reinterpret_cast<const bf16x8*>(lateral)[i];
  float s[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) s[e] = bf2f(lv[e]);
  if (coarse) {
    const int hc = nearest_src(h, sh, Hc), wc = nearest_src(w, sw, Wc);
    const bf16x8 cv = reinterpret_cast<const bf16x8*>(coarse)[(((size_t)b * Hc + hc) * Wc + wc) * C8 + c8];
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] += bf2f(cv[e]);
  }
  if (inner) {
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = f2bf(s[e]);
    reinterpret_cast<bf16x8*>(inner)[i] = o;
  }
  if (dropped) {
    const float k = keep[pix] ? 1.f : 0.f;
    const float scale = (float)((long long)B * H * W) / (float)kept[0];      // kept == 0: what IEEE gives (inf, and 0 * inf = NaN)
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = f2bf(s[e] * k * scale);
    reinterpret_cast<bf16x8*>(dropped)[i] = o;
  }
}

// Backward of the above.  One thread per 8 channels of one COARSE pixel: it finds its children with the forward rule, writes each
// child's d_lateral and sums the unrounded gradients in row-major child order.  Every fine pixel has exactly one parent, so both
// outputs are written exactly once.
__global__ __launch_bounds__(256) void fpn_merge_bwd_kernel(const bf16* __restrict__ d_inner, const bf16* __restrict__ d_dropped,
                                                            const unsigned char* __restrict__ keep, const int* __restrict__ kept,
                                                            bf16* __restrict__ d_lateral, bf16* __restrict__ d_coarse, int B, int H, int W,
                                                            int C8, int Hc, int Wc, float sh, float sw) {
  const size_t nvec = (size_t)B * Hc * Wc * C8;
  const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
  if (i >= nvec) return;
  const int c8 = (int)(i % C8);
  const size_t pix = i / C8;
  const int wc = (int)(pix % Wc), hc = (int)((pix / Wc) % Hc), b = (int)(pix / ((size_t)Wc * Hc));
  const int h0 = first_child(hc, sh, Hc, H), h1 = first_child(hc + 1, sh, Hc, H);
  const int w0 = first_child(wc, sw, Wc, W), w1 = first_child(wc + 1, sw, Wc, W);
  const float scale = d_dropped ? (float)((long long)B * H * W) / (float)kept[0] : 0.f;
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  for (int h = h0; h < h1; ++h) {
    for (int w = w0; w < w1; ++w) {
      const size_t fp = ((size_t)b * H + h) * W + w;
      const size_t fv = fp * C8 + c8;
      float g[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) g[e] = 0.f;
      if (d_inner) {
        const bf16x8 v = reinterpret_cast<const bf16x8*>(d_inner)[fv];
#pragma unroll
        for (int e = 0; e < 8; ++e) g[e] = bf2f(v[e]);
      }
      if (d_dropped) {
        const float k = keep[fp] ? 1.f : 0.f;
        const bf16x8 v = reinterpret_cast<const bf16x8*>(d_dropped)[fv];
#pragma unroll
        for (int e = 0; e < 8; ++e) g[e] += bf2f(v[e]) * k * scale;
      }
      bf16x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) { o[e] = f2bf(g[e]); acc[e] += g[e]; }
      reinterpret_cast<bf16x8*>(d_lateral)[fv] = o;
    }
  }
  if (d_coarse) {
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = f2bf(acc[e]);
    reinterpret_cast<bf16x8*>(d_coarse)[i] = o;
  }
}

bool merge_shape_ok(int B, int H, int W, int C, int Hc, int Wc) {
  if (B < 0 || H <= 0 || W <= 0 || C <= 0 || (C & 7) || Hc <= 0 || Wc <= 0) return false;
  const long long fine = (long long)B * H * W, coarse = (long long)B * Hc * Wc;
  return fine <= 0x7FFFFFFFll && coarse <= 0x7FFFFFFFll && cdiv(C, 8) * (fine > coarse ? fine : coarse) <= 0x7FFFFFFFll * 256;
}

}  // namespace

// keep = 1 - maxpool_{block x block, stride 1, pad block / 2}(seeds), kept[0] = sum keep (overwritten).  draw != 0: seeds[i] is first
// set to hash_u32(seed + *seed_base, i) < (uint32)(gamma * 2^32), i the flat index; draw == 0: seeds are read as given.
extern "C" int fiber_dropblock_mask_u8(unsigned char* seeds, int draw, uint64_t seed, const uint64_t* seed_base, float gamma, int block,
                                       unsigned char* keep, int* kept, int B, int H, int W, hipStream_t stream) {
  if (B < 0 || H <= 0 || W <= 0 || block <= 0 || !(block & 1) || !(gamma >= 0.f) || !(gamma < 1.f)) return FIBER_EINVAL;
  if ((long long)B * H * W > 0x7FFFFFFFll) return FIBER_EINVAL;
  if (!kept || fiber_misaligned(4, kept)) return FIBER_EINVAL;
  if (hipMemsetAsync(kept, 0, sizeof(int), stream) != hipSuccess) return FIBER_ELAUNCH;
  if (B == 0) return FIBER_OK;
  if (!seeds || !keep) return FIBER_EINVAL;
  const uint32_t thresh = (uint32_t)((double)gamma * 4294967296.0);
  const int n = B * H * W;
  hipLaunchKernelGGL(dropblock_mask_kernel, dim3(cdiv(n, 256)), dim3(256), 0, stream, seeds, draw, seed, seed_base, thresh, block / 2, keep,
                     kept, B, H, W);
  FIBER_CHECK_LAUNCH();
  return FIBER_OK;
}

// inner = bf16(s), dropped = bf16(s * keep * scale) with s = f32(lateral) + f32(coarse[src]) unrounded and scale = (float)(B H W) /
// (float)kept[0] read from device memory.  coarse NULL: s = f32(lateral) (DropBlock on a map of its own).  dropped_out needs keep and
// kept, and the other way round.
extern "C" int fiber_fpn_merge_fwd_bf16(const void* lateral, const void* coarse, const unsigned char* keep, const int* kept, void* inner_out,
                                        void* dropped_out, int B, int H, int W, int C, int Hc, int Wc, hipStream_t stream) {
  if (!coarse) Hc = H, Wc = W;
  if (!merge_shape_ok(B, H, W, C, Hc, Wc)) return FIBER_EINVAL;
  if (B == 0) return FIBER_OK;
  if (!lateral || (!inner_out && !dropped_out)) return FIBER_EINVAL;
  if ((dropped_out != nullptr) != (keep != nullptr) || (keep != nullptr) != (kept != nullptr)) return FIBER_EINVAL;
  if (fiber_misaligned(16, lateral, coarse, inner_out, dropped_out) || fiber_misaligned(4, kept)) return FIBER_EINVAL;
  const size_t nvec = (size_t)B * H * W * (C / 8);
  hipLaunchKernelGGL(fpn_merge_fwd_kernel, dim3((unsigned)((nvec + 255) / 256)), dim3(256), 0, stream, (const bf16*)lateral, (const bf16*)coarse,
                     keep, kept, (bf16*)inner_out, (bf16*)dropped_out, B, H, W, C / 8, Hc, Wc, (float)Hc / (float)H, (float)Wc / (float)W);
  FIBER_CHECK_LAUNCH();
  return FIBER_OK;
}

// g = f32(d_inner) + f32(d_dropped) * keep * scale (a NULL term is absent); d_lateral_out = bf16(g); d_coarse_out[b, hc, wc] = bf16(sum of
// the unrounded g over the fine pixels whose source is (hc, wc), fp32, row-major child order; 0 without a child).  d_coarse_out NULL:
// not written (the coarse NULL form of the forward; Hc, Wc are then taken as H, W).  d_dropped needs keep and kept.
extern "C" int fiber_fpn_merge_bwd_bf16(const void* d_inner, const void* d_dropped, const unsigned char* keep, const int* kept,
                                        void* d_lateral_out, void* d_coarse_out, int B, int H, int W, int C, int Hc, int Wc,
                                        hipStream_t stream) {
  if (!d_coarse_out) Hc = H, Wc = W;
  if (!merge_shape_ok(B, H, W, C, Hc, Wc)) return FIBER_EINVAL;
  if (B == 0) return FIBER_OK;
  if (!d_lateral_out || (d_dropped && (!keep || !kept))) return FIBER_EINVAL;
  if (fiber_misaligned(16, d_inner, d_dropped, d_lateral_out, d_coarse_out) || fiber_misaligned(4, kept)) return FIBER_EINVAL;
  const size_t nvec = (size_t)B * Hc * Wc * (C / 8);
  hipLaunchKernelGGL(fpn_merge_bwd_kernel, dim3((unsigned)((nvec + 255) / 256)), dim3(256), 0, stream, (const bf16*)d_inner,
                     (const bf16*)d_dropped, keep, kept, (bf16*)d_lateral_out, (bf16*)d_coarse_out, B, H, W, C / 8, Hc, Wc,
                     (float)Hc / (float)H, (float)Wc / (float)W);
  FIBER_CHECK_LAUNCH();
  return FIBER_OK;
}
