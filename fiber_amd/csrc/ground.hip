// Region-word alignment of the grounding head (gfx950): the dot product between every anchor's 256-channel tower feature and the 256
// projected text tokens, with the binary token focal loss reduced in the epilogue.  Replaces, of the fine-grained reference
// (fine_grained/maskrcnn_benchmark/), modeling/rpn/vldyhead.py:857-891 (permute_and_flatten, matmul / log_scale.exp() + bias, the two
// clamps) and layers/sigmoid_focal_loss.py:130-195 (token_sigmoid_binary_focal_loss + TokenSigmoidFocalLoss.forward's .sum()) as called
// from modeling/rpn/loss.py:1222-1226.  The reference materialises the fp32 [B, A, T] logits and about ten temporaries of that size;
// the loss path here writes no [B, A, T] tensor at all and the backward recomputes the tile, emitting ds = g dloss/ds, scaled by
// exp(-log_scale) (the gradient of the raw dot product), once in bf16 for the two existing GEMMs (dX = ds P, dP = ds^T X).
//
// Tile: one workgroup (4 waves) = 64 anchors x all 256 tokens of one image.  A wave keeps its 16 anchors' X fragments in registers (the B
// operand) and walks the tokens in four chunks of 64 staged in LDS (the A operand), so the accumulator is S^T[token][anchor]: a lane then
// holds FOUR CONSECUTIVE TOKENS of one anchor, which makes every global access of the epilogue (fp32x4 logits, 4 target bytes, bf16x4 ds) a
// plain vector access along the contiguous token axis.  Sums: lane -> wave (xor shuffles) -> workgroup (LDS, fixed order) -> one partial per
// workgroup -> fiber_fold_rows_f32.  No atomics anywhere: two runs give the same bits.
#include "common.h"

namespace {

constexpr int GC = 256, GT = 256;          // channels, tokens (the only supported sizes)
constexpr int G_ANCH = 64;                 // anchors per workgroup
constexpr int G_CHUNK = 64;                // tokens staged per LDS chunk
constexpr int G_LD = GC + 8;               // LDS row stride (bf16): 528 B keeps the 16-byte fragment reads off a common bank
constexpr float G_CLAMP = 50000.f;

struct FocalTerm { float loss, dz; };      // loss and dloss/dz of one element, z = +s (target 1) or -s (target 0)

// softplus / sigmoid from ONE exp and one log: e = exp(-|z|), l = log1p(e); softplus(-z) = max(-z, 0) + l, softplus(z) = max(z, 0) + l,
// p_t = sigmoid(z) = (z >= 0 ? 1 : e) / (1 + e), q = 1 - p_t = (z >= 0 ? e : 1) / (1 + e): nothing is formed by cancellation.
template <bool GRAD>
__device__ __forceinline__ FocalTerm focal_term(float z, float alpha_t, float gamma, bool gamma2) {
  const float az = fabsf(z);
  const float e = __expf(-az);
  const float l = e < 0.015625f ? e * (1.f - e * (0.5f - e * (0.33333334f - 0.25f * e))) : __logf(1.f + e);
  const float r = __builtin_amdgcn_rcpf(1.f + e);
  const float ce = fmaxf(-z, 0.f) + l;
  const float q = (z >= 0.f ? e : 1.f) * r;
  const float mod = gamma2 ? q * q : __expf(-gamma * (fmaxf(z, 0.f) + l));
  FocalTerm o;
  o.loss = alpha_t * ce * mod;
  if (GRAD) {
    const float pt = (z >= 0.f ? 1.f : e) * r;
    o.dz = -alpha_t * mod * (q + gamma * pt * ce);
  } else {
    o.dz = 0.f;
  }
  return o;
}

// MODE bit 0: store the logits; bit 1: accumulate the loss; bit 2: backward (ds, dtbias and dlog_scale partials)
template <int MODE>
__global__ __launch_bounds__(256) void ground_kernel(const bf16* __restrict__ X, const bf16* __restrict__ P, const float* __restrict__ tbias,
                                                     const float* __restrict__ log_scale, const unsigned char* __restrict__ target,
                                                     const unsigned char* __restrict__ text_mask, const float* __restrict__ gup,
                                                     float* __restrict__ logits, bf16* __restrict__ ds, float* __restrict__ part_sum,
                                                     float* __restrict__ part_tb, int B, int A, float alpha, float gamma) {
  constexpr bool LOGITS = MODE & 1, LOSS = MODE & 2, BWD = MODE & 4;
  __shared__ __attribute__((aligned(16))) bf16 Ps[G_CHUNK * G_LD];
  __shared__ float red[4];
  __shared__ float tbs[BWD ? 4 * GT : 4];
  const int b = blockIdx.y, blk = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lq = lane & 15, gq = lane >> 4;
  const int a = blk * G_ANCH + wave * 16 + lq;
  const bool a_ok = a < A;
  const float inv_scale = __expf(-log_scale[0]);
  const float g = BWD ? gup[0] : 0.f;
  const bool gamma2 = gamma == 2.f;

  bf16x8 xf[GC / 32];
  {
    const bf16* xr = X + ((size_t)b * A + (a_ok ? a : 0)) * GC + gq * 8;
#pragma unroll
    for (int ks = 0; ks < GC / 32; ++ks) {
      bf16x8 v = *reinterpret_cast<const bf16x8*>(xr + ks * 32);
      if (!a_ok) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = f2bf(0.f);
      }
      xf[ks] = v;
    }
  }
  const bf16* Pb = P + (size_t)b * GT * GC;
  const size_t row_off = ((size_t)b * A + (a_ok ? a : 0)) * GT;
  float lsum = 0.f;                                        // loss (forward) or -ds (s - tbias) (backward) of this lane

  for (int ch = 0; ch < GT / G_CHUNK; ++ch) {
    if (ch) __syncthreads();                               // the previous chunk's fragment reads
#pragma unroll
    for (int j = 0; j < (G_CHUNK * GC / 8) / 256; ++j) {
      const int i = threadIdx.x + 256 * j, r = i >> 5, c8 = i & 31;
      *reinterpret_cast<bf16x8*>(Ps + r * G_LD + c8 * 8) = *reinterpret_cast<const bf16x8*>(Pb + (size_t)(ch * G_CHUNK + r) * GC + c8 * 8);
    }
    __syncthreads();
#pragma unroll
    for (int tt = 0; tt < G_CHUNK / 16; ++tt) {
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < GC / 32; ++ks) {
        const bf16x8 pf = *reinterpret_cast<const bf16x8*>(Ps + (tt * 16 + lq) * G_LD + ks * 32 + gq * 8);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf, xf[ks], acc, 0, 0, 0);   // S^T[token][anchor]
      }
      const int t0 = ch * G_CHUNK + tt * 16 + gq * 4;      // this lane's four tokens
      const f32x4 tb = *reinterpret_cast<const f32x4*>(tbias + b * GT + t0);
      f32x4 s;
#pragma unroll
      for (int r = 0; r < 4; ++r) s[r] = __builtin_amdgcn_fmed3f(acc[r] * inv_scale + tb[r], -G_CLAMP, G_CLAMP);
      if (LOGITS) {
        if (a_ok) *reinterpret_cast<f32x4*>(logits + row_off + t0) = s;
      }
      if (LOSS || BWD) {
        const uchar4 tm = *reinterpret_cast<const uchar4*>(text_mask + b * GT + t0);
        uchar4 tg = uchar4{0, 0, 0, 0};
        if (a_ok) tg = *reinterpret_cast<const uchar4*>(target + row_off + t0);
        const unsigned char tmv[4] = {tm.x, tm.y, tm.z, tm.w}, tgv[4] = {tg.x, tg.y, tg.z, tg.w};
        float dsv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool pos = tgv[r] != 0, live = a_ok && tmv[r] != 0;
          const float alpha_t = alpha >= 0.f ? (pos ? alpha : 1.f - alpha) : 1.f;
          const FocalTerm f = focal_term<BWD>(pos ? s[r] : -s[r], alpha_t, gamma, gamma2);
          if (LOSS) lsum += live ? f.loss : 0.f;
          if (BWD) {
            const float un = acc[r] * inv_scale;           // s_unclamped - tbias
            const float su = un + tb[r];
            const bool pass = live && su >= -G_CLAMP && su <= G_CLAMP;   // torch.clamp passes the gradient at the bounds
            dsv[r] = pass ? g * (pos ? f.dz : -f.dz) : 0.f;
            lsum -= dsv[r] * un;
          }
        }
        if (BWD) {
          if (a_ok) {
            bf16x4 o;
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = f2bf(dsv[r] * inv_scale);   // gradient of the RAW dot product: what the two GEMMs consume
            *reinterpret_cast<bf16x4*>(ds + row_off + t0) = o;
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {                    // sum over the wave's 16 anchors (the lanes that share gq)
            float v = dsv[r];
            v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4); v += __shfl_xor(v, 8);
            if (lq == 0) tbs[wave * GT + t0 + r] = v;
          }
        }
      }
    }
  }
  if (LOSS || BWD) {
    lsum = wave_sum(lsum);
    if (lane == 0) red[wave] = lsum;
    __syncthreads();
    if (threadIdx.x == 0) part_sum[b * gridDim.x + blk] = (red[0] + red[1]) + (red[2] + red[3]);
    if (BWD) {
      const int t = threadIdx.x;
      part_tb[((size_t)blk * B + b) * GT + t] = (tbs[t] + tbs[GT + t]) + (tbs[2 * GT + t] + tbs[3 * GT + t]);
    }
  }
}

inline int ground_blocks(int A) { return cdiv(A, G_ANCH); }

}  // namespace

// fp32 words of the partial-sum workspace both directions need: one per workgroup (loss / dlog_scale) + one per workgroup and token (dtbias)
extern "C" long fiber_ground_workspace(int B, int A, int T) {
  if (B <= 0 || A <= 0 || T <= 0) return 0;
  const long nb = ground_blocks(A);
  return nb * B + nb * B * T;
}

extern "C" int fiber_ground_fwd_bf16(const void* X, const void* P, const float* tbias, const float* log_scale, const unsigned char* target,
                                     const unsigned char* text_mask, float* logits, float* loss, float* workspace, int B, int A, int T,
                                     int C, float alpha, float gamma, hipStream_t stream) {
  if (B <= 0 || A <= 0) return FIBER_OK;
  if (C != GC || T != GT || !X || !P || !tbias || !log_scale || (!logits && !loss) || !(gamma >= 0.f)) return FIBER_EINVAL;
  if (loss && (!target || !text_mask || !workspace)) return FIBER_EINVAL;
  if (fiber_misaligned(16, X, P, tbias, logits) || fiber_misaligned(4, target, text_mask)) return FIBER_EINVAL;
  const dim3 grid(ground_blocks(A), B), block(256);
#define GROUND_LAUNCH(MODE)                                                                                                              \
  hipLaunchKernelGGL(ground_kernel<MODE>, grid, block, 0, stream, (const bf16*)X, (const bf16*)P, tbias, log_scale, target, text_mask,    \
                     (const float*)nullptr, logits, (bf16*)nullptr, workspace, (float*)nullptr, B, A, alpha, gamma)
  if (logits && loss) GROUND_LAUNCH(3);
  else if (loss) GROUND_LAUNCH(2);
  else GROUND_LAUNCH(1);
#undef GROUND_LAUNCH
  FIBER_CHECK_LAUNCH();
  if (loss) return fiber_fold_rows_f32(workspace, loss, (int)grid.x * B, 1, stream);
  return FIBER_OK;
}

extern "C" int fiber_ground_bwd_bf16(const void* X, const void* P, const float* tbias, const float* log_scale, const unsigned char* target,
                                     const unsigned char* text_mask, const float* g, void* ds, float* dtbias, float* dlog_scale,
                                     float* workspace, int B, int A, int T, int C, float alpha, float gamma, hipStream_t stream) {
  if (B <= 0 || A <= 0) return FIBER_OK;
  if (C != GC || T != GT || !X || !P || !tbias || !log_scale || !target || !text_mask || !g || !ds || !dtbias || !dlog_scale || !workspace ||
      !(gamma >= 0.f))
    return FIBER_EINVAL;
  if (fiber_misaligned(16, X, P, tbias) || fiber_misaligned(8, ds) || fiber_misaligned(4, target, text_mask)) return FIBER_EINVAL;
  const dim3 grid(ground_blocks(A), B), block(256);
  float* part_tb = workspace + (size_t)grid.x * B;
  hipLaunchKernelGGL(ground_kernel<4>, grid, block, 0, stream, (const bf16*)X, (const bf16*)P, tbias, log_scale, target, text_mask, g,
                     (float*)nullptr, (bf16*)ds, workspace, part_tb, B, A, alpha, gamma);
  FIBER_CHECK_LAUNCH();
  int rc = fiber_fold_rows_f32(workspace, dlog_scale, (int)grid.x * B, 1, stream);
  if (rc != FIBER_OK) return rc;
  return fiber_fold_rows_f32(part_tb, dtbias, (int)grid.x, B * T, stream);
}
