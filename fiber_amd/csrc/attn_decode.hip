// Single-token attention for KV-cached caption decoding (gfx950): the new token's causal self-attention against a per-row cache that is
// followed through an ancestry table (beam reorder without copying a cache), and its text->image cross-attention with an image's K/V
// fetched once for all the rows (beams) of that image.  Forward only: no dropout, no lse, no backward.  Replaces, per generated token,
// one full fiber_mha_causal_fwd_bf16 over [N, t + 1] positions and one fiber_mha_fwd_bf16 whose K/V projection was recomputed per beam.
//
// Both kernels are memory-bound (one pass over K and V, a handful of FMAs per byte), so K/V go from global memory straight to VGPRs with
// 16-byte loads and nothing is staged in LDS.  The dot products and P.V run on the VALU with fp32 probabilities, not on MFMAs: with R <= 16
// query rows per image an MFMA tile would be at most R / 16 full, P would have to be rounded to bf16 and moved between the C and the A
// layouts, and at the decoder's R = 5 the VALU form needs 2.5 FMAs per K/V byte, a third of what the VALU sustains at HBM rate (at R = 16
// the two meet; that shape is served, not tuned).  fp32 P keeps every output inside the bf16 store rounding.
//
// Lane layout, shared by both kernels.  A head's D channels are CH = D / 8 chunks of 8 (16 bytes).  A wave takes 64 keys at a time: lane
// (jg, dc), jg = lane / CH, dc = lane % CH, owns chunk dc of the keys jg + JG * i (JG = 64 / CH, i < CH), so every load instruction reads
// JG whole rows of D contiguous channels.  A score is the lane's 8-term partial dot product summed over the CH lanes of its group with xor
// shuffles (every lane of the group then holds the same bits), the tile maximum and the end-of-loop sums run over the jg lanes the same
// way, and P.V needs no transposition: the lane that owns K's chunk owns V's.  Running (max, sum, accumulator) per query in the log2
// domain; a key past the end scores -inf, is never loaded, and contributes an exact 0.
//
// fiber_mha_decode_self_bf16: one wave per (row, head); positions j < t come from slot anc[n, j] (slot n when anc is NULL), position t from
// the row's own qkv, which the same wave also stores to kv_cache[n, t].  Positions < t are only read and position t of slot n is written by
// row n alone, so rows cannot race; nothing beyond position t is read.  An anc entry outside [0, N) marks a position that is no key (padding
// under a key mask, as the causal kernels' finfo.min keys): it is skipped, never dereferenced -- also at position t itself, whose k | v are
// appended all the same; with anc, anc[n, t] is n for a live position.  A row without any key gives 0.
//
// fiber_mha_decode_cross_bf16: one workgroup of 4 waves per (image, head); wave w takes the 64-key tiles w, w + 4, ... for all R queries of
// the image (the queries, scaled, sit in LDS as fp32 and are read as broadcasts), with no barrier inside the key loop, and the four partial
// softmaxes are merged once through LDS in wave order.  Each (image, head) slice of K/V is read once, by one workgroup; adjacent heads are
// adjacent workgroups, so the halves of a 128-byte line that two D = 32 heads share meet in L2.  The tile partition depends on Lk alone and
// each query's arithmetic on its own row alone: a row's bits do not depend on R or on the other rows.  R is padded to a template bound
// (1, 2, 4, 8, 16) that only sizes the register arrays.
#include "common.h"

#pragma clang fp contract(off)   // the same rounding sequence in every instantiation: rows must not depend on the template bound

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr int XW = 4;            // waves of a cross-attention workgroup
constexpr int XR = 16;           // most rows per image

__device__ __forceinline__ void cvt8(bf16x8 v, float (&f)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] = bf2f(v[e]);
}

// One tile of up to 64 keys for RB queries.  kp[i] / vp[i]: the lane's 16-byte chunk of key jg + JG * i (read only where live[i]);
// q(r, f): the lane's chunk of query r, times scale * log2 e; (m, l, acc): the running softmax of the lane's keys, rescaled wave-uniformly.
template <int D, int RB, class Q>
__device__ __forceinline__ void decode_tile(const bf16* const (&kp)[D / 8], const bf16* const (&vp)[D / 8], const bool (&live)[D / 8],
                                            int R, Q q, float (&m)[RB], float (&l)[RB], float (&acc)[RB][8]) {
  constexpr int CH = D / 8;
  float kf[CH][8], vf[CH][8];
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    bf16x8 k8 = {}, v8 = {};
    if (live[i]) {
      k8 = *reinterpret_cast<const bf16x8*>(kp[i]);
      v8 = *reinterpret_cast<const bf16x8*>(vp[i]);
    }
    cvt8(k8, kf[i]);
    cvt8(v8, vf[i]);
  }
#pragma unroll
  for (int r = 0; r < RB; ++r) {
    if (r >= R) continue;
    float qf[8];
    q(r, qf);
    float s[CH];
    float tmax = -INFINITY;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      float d = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) d = __builtin_fmaf(qf[e], kf[i][e], d);
#pragma unroll
      for (int o = 1; o < CH; o <<= 1) d += __shfl_xor(d, o);
      s[i] = live[i] ? d : -INFINITY;
      tmax = fmaxf(tmax, s[i]);
    }
#pragma unroll
    for (int o = CH; o < 64; o <<= 1) tmax = fmaxf(tmax, __shfl_xor(tmax, o));
    const float mn = fmaxf(m[r], tmax);                    // finite: a tile that is processed has a live key
    const float alpha = __builtin_amdgcn_exp2f(m[r] - mn);
    m[r] = mn;
    l[r] *= alpha;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[r][e] *= alpha;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const float p = __builtin_amdgcn_exp2f(s[i] - mn);
      l[r] += p;
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[r][e] = __builtin_fmaf(p, vf[i][e], acc[r][e]);
    }
  }
}

// sums over the jg lanes: afterwards every lane holds the wave's totals for its chunk dc
template <int D>
__device__ __forceinline__ void reduce_keys(float& l, float (&acc)[8]) {
#pragma unroll
  for (int o = D / 8; o < 64; o <<= 1) {
    l += __shfl_xor(l, o);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += __shfl_xor(acc[e], o);
  }
}

template <int D>
__global__ __launch_bounds__(64) void decode_self_kernel(const bf16* __restrict__ qkv, bf16* __restrict__ cache, const int* __restrict__ anc,
                                                         bf16* __restrict__ o, int N, int heads, int t, int Lmax, int ldqkv, int ldo,
                                                         float scale) {
  constexpr int CH = D / 8, JG = 64 / CH;
  const int lane = threadIdx.x, jg = lane / CH, dc = lane % CH;
  const int n = blockIdx.x / heads, h = blockIdx.x % heads;
  const int C = heads * D;
  const size_t col = (size_t)h * D + (size_t)dc * 8;
  const bf16* row = qkv + (size_t)n * ldqkv;

  const bf16* kp[CH];
  const bf16* vp[CH];
  bool live[CH];
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    const int j = jg + JG * i;
    kp[i] = row + C + col;                                   // position t: the row's own new k | v
    vp[i] = row + 2 * (size_t)C + col;
    live[i] = false;
    if (j <= t) {
      const int slot = anc ? anc[(size_t)n * Lmax + j] : n;
      live[i] = (unsigned)slot < (unsigned)N;                // (position t: anc[n, t] only says whether the position is a key at all)
      if (j < t) {
        const bf16* p = cache + ((size_t)(live[i] ? slot : n) * Lmax + j) * (2 * (size_t)C) + col;
        kp[i] = p;
        vp[i] = p + C;
      }
    }
  }
  float qs[8];
  cvt8(*reinterpret_cast<const bf16x8*>(row + col), qs);
  const float sc = scale * LOG2E;
#pragma unroll
  for (int e = 0; e < 8; ++e) qs[e] *= sc;

  float m[1] = {-INFINITY}, l[1] = {0.f}, acc[1][8] = {};
  decode_tile<D, 1>(kp, vp, live, 1, [&](int, float (&f)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = qs[e];
  }, m, l, acc);
  reduce_keys<D>(l[0], acc[0]);

  if (lane < CH) {
    bf16x8 out;
#pragma unroll
    for (int e = 0; e < 8; ++e) out[e] = f2bf(l[0] > 0.f ? acc[0][e] / l[0] : 0.f);     // every position skipped: 0
    *reinterpret_cast<bf16x8*>(o + (size_t)n * ldo + col) = out;
  }
  if (lane < 2 * CH) {                                       // append: lanes [0, CH) copy k, [CH, 2 CH) copy v
    const size_t c = (size_t)(lane / CH) * C + (size_t)h * D + (size_t)(lane % CH) * 8;
    *reinterpret_cast<bf16x8*>(cache + ((size_t)n * Lmax + t) * (2 * (size_t)C) + c) = *reinterpret_cast<const bf16x8*>(row + C + c);
  }
}

template <int D, int RB>
__global__ __launch_bounds__(XW * 64) void decode_cross_kernel(const bf16* __restrict__ q, const bf16* __restrict__ kv, bf16* __restrict__ o,
                                                               int R, int heads, int Lk, int ldq, int ldo, float scale) {
  constexpr int CH = D / 8, JG = 64 / CH;
  __shared__ __attribute__((aligned(16))) float sm_q[XR][D];
  __shared__ __attribute__((aligned(16))) float sm_acc[XW][XR][D];
  __shared__ float sm_m[XW][XR], sm_l[XW][XR];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, jg = lane / CH, dc = lane % CH;
  const int g = blockIdx.x / heads, h = blockIdx.x % heads;
  const int C = heads * D;
  const size_t col = (size_t)h * D + (size_t)dc * 8;

  if (tid < R * CH) {                                        // R * CH <= 128: thread (r, chunk) scales one chunk of one query
    const int r = tid / CH, c = tid % CH;
    float f[8];
    cvt8(*reinterpret_cast<const bf16x8*>(q + ((size_t)g * R + r) * ldq + (size_t)h * D + c * 8), f);
    const float sc = scale * LOG2E;
#pragma unroll
    for (int e = 0; e < 8; ++e) sm_q[r][c * 8 + e] = f[e] * sc;
  }
  __syncthreads();

  float m[RB], l[RB], acc[RB][8];
#pragma unroll
  for (int r = 0; r < RB; ++r) {
    m[r] = -INFINITY;
    l[r] = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[r][e] = 0.f;
  }
  const bf16* base = kv + (size_t)g * Lk * (2 * (size_t)C) + col;
  const int tiles = (Lk + 63) / 64;
  for (int tile = wave; tile < tiles; tile += XW) {
    const bf16* kp[CH];
    const bf16* vp[CH];
    bool live[CH];
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int j = tile * 64 + jg + JG * i;
      live[i] = j < Lk;
      kp[i] = base + (size_t)(live[i] ? j : 0) * (2 * (size_t)C);
      vp[i] = kp[i] + C;
    }
    decode_tile<D, RB>(kp, vp, live, R, [&](int r, float (&f)[8]) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(&sm_q[r][dc * 8]), b = *reinterpret_cast<const f32x4*>(&sm_q[r][dc * 8 + 4]);
      f[0] = a[0], f[1] = a[1], f[2] = a[2], f[3] = a[3], f[4] = b[0], f[5] = b[1], f[6] = b[2], f[7] = b[3];
    }, m, l, acc);
  }
#pragma unroll
  for (int r = 0; r < RB; ++r) {
    if (r >= R) continue;
    reduce_keys<D>(l[r], acc[r]);
    if (lane < CH) {
#pragma unroll
      for (int e = 0; e < 8; ++e) sm_acc[wave][r][dc * 8 + e] = acc[r][e];
      if (lane == 0) sm_m[wave][r] = m[r], sm_l[wave][r] = l[r];
    }
  }
  __syncthreads();

  if (tid < R * CH) {                                        // merge in wave order; a wave without a tile has m = -inf, l = 0: factor 0
    const int r = tid / CH, c = tid % CH;
    float M = sm_m[0][r];
#pragma unroll
    for (int w = 1; w < XW; ++w) M = fmaxf(M, sm_m[w][r]);
    float L = 0.f, out[8] = {};
#pragma unroll
    for (int w = 0; w < XW; ++w) {
      const float f = __builtin_amdgcn_exp2f(sm_m[w][r] - M);
      L = __builtin_fmaf(sm_l[w][r], f, L);
#pragma unroll
      for (int e = 0; e < 8; ++e) out[e] = __builtin_fmaf(sm_acc[w][r][c * 8 + e], f, out[e]);
    }
    bf16x8 ob;
#pragma unroll
    for (int e = 0; e < 8; ++e) ob[e] = f2bf(out[e] / L);
    *reinterpret_cast<bf16x8*>(o + ((size_t)g * R + r) * ldo + (size_t)h * D + c * 8) = ob;
  }
}

template <int D>
int launch_cross(const bf16* q, const bf16* kv, bf16* o, int G, int R, int heads, int Lk, int ldq, int ldo, float scale, hipStream_t stream) {
  const dim3 grid((unsigned)(G * heads)), block(XW * 64);
#define FIBER_XDEC(RB) hipLaunchKernelGGL((decode_cross_kernel<D, RB>), grid, block, 0, stream, q, kv, o, R, heads, Lk, ldq, ldo, scale)
  if (R <= 1) FIBER_XDEC(1);
  else if (R <= 2) FIBER_XDEC(2);
  else if (R <= 4) FIBER_XDEC(4);
  else if (R <= 8) FIBER_XDEC(8);
  else FIBER_XDEC(16);
#undef FIBER_XDEC
  FIBER_CHECK_LAUNCH();
  return FIBER_OK;
}

}  // namespace

extern "C" int fiber_mha_decode_self_bf16(const void* qkv, void* kv_cache, const int* anc, void* o, int N, int heads, int D, int t, int Lmax,
                                          int ldqkv, int ldo, float scale, hipStream_t stream) {
  if ((D != 32 && D != 64) || N < 0 || heads < 1 || Lmax < 1 || Lmax > 64 || t < 0 || t >= Lmax) return FIBER_EINVAL;
  const long long C = (long long)heads * D;
  if (ldqkv % 8 || ldo % 8 || ldqkv < 3 * C || ldo < C || (long long)N * heads > 0x7fffffffLL) return FIBER_EINVAL;
  if (N == 0) return FIBER_OK;
  if (!qkv || !kv_cache || !o || fiber_misaligned(16, qkv, kv_cache, o) || fiber_misaligned(4, anc)) return FIBER_EINVAL;
  const dim3 grid((unsigned)(N * heads)), block(64);
  const bf16* x = (const bf16*)qkv;
  bf16* cache = (bf16*)kv_cache;
  if (D == 32) hipLaunchKernelGGL(decode_self_kernel<32>, grid, block, 0, stream, x, cache, anc, (bf16*)o, N, heads, t, Lmax, ldqkv, ldo, scale);
  else hipLaunchKernelGGL(decode_self_kernel<64>, grid, block, 0, stream, x, cache, anc, (bf16*)o, N, heads, t, Lmax, ldqkv, ldo, scale);
  FIBER_CHECK_LAUNCH();
  return FIBER_OK;
}

extern "C" int fiber_mha_decode_cross_bf16(const void* q, const void* kv, void* o, int N, int R, int heads, int Lk, int D, int ldq, int ldo,
                                           float scale, hipStream_t stream) {
  if ((D != 32 && D != 64) || N < 0 || R < 1 || R > XR || N % R || heads < 1 || Lk < 1) return FIBER_EINVAL;
  const long long C = (long long)heads * D;
  if (ldq % 8 || ldo % 8 || ldq < C || ldo < C || (long long)(N / R) * heads > 0x7fffffffLL) return FIBER_EINVAL;
  if (N == 0) return FIBER_OK;
  if (!q || !kv || !o || fiber_misaligned(16, q, kv, o)) return FIBER_EINVAL;
  if (D == 32) return launch_cross<32>((const bf16*)q, (const bf16*)kv, (bf16*)o, N / R, R, heads, Lk, ldq, ldo, scale, stream);
  return launch_cross<64>((const bf16*)q, (const bf16*)kv, (bf16*)o, N / R, R, heads, Lk, ldq, ldo, scale, stream);
}
