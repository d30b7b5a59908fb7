// Input-side kernels of the FIBER fused path (gfx950): RoBERTa embeddings and Swin patch-embed im2col.
//
//   roberta_embed  pos = cumsum(ids != pad) * (ids != pad) + pad ; y = dropout(LN(word[ids] + type[0] + position[pos]))
//                  (roberta.py:169-199, 877-888).  Tables stay fp32 (the master parameters): only B*S rows are gathered.
//   backward       recomputes the pre-LN sum from the tables, LN backward in registers, per-row gradients into a workspace;
//                  a stable rank sort of (id, row) and (position, row), then segment sums in a fixed order write the touched rows of
//                  the word / position tables, and the LayerNorm / token-type partials are folded in a fixed order (no atomics).
//   im2col         PatchEmbed's Conv2d(3->C, k=4, s=4) is a GEMM over non-overlapping patches (timm 0.4.12 PatchEmbed,
//                  used at swin_transformer.py:588): rows = patches, K = 48 ordered [c][kh][kw], zero padded to 64.
#include <climits>

#include "common.h"

namespace {

template <int NV>
__global__ __launch_bounds__(256) void roberta_embed_fwd_kernel(const int64_t* __restrict__ ids, const float* __restrict__ word,
                                                                const float* __restrict__ pos_tab, const float* __restrict__ type_tab,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                bf16* __restrict__ y, int* __restrict__ pos_out,
                                                                float* __restrict__ mean, float* __restrict__ rstd, int S, int C,
                                                                int pad, float eps, float p_drop, uint64_t seed,
                                                                const uint64_t* __restrict__ seed_base) {
  if (seed_base) seed += *seed_base;
  __shared__ int spos[1024];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) {
    int run = 0;
    for (int s = 0; s < S; ++s) {
      const int m = ids[(size_t)b * S + s] != pad;
      run += m;
      spos[s] = run * m + pad;
    }
  }
  __syncthreads();
  const int nvec = C >> 2;                       // float4 vectors
  const uint32_t thresh = (uint32_t)((double)p_drop * 4294967296.0);
  const float inv_keep = 1.f / (1.f - p_drop);
  for (int s = wave; s < S; s += 4) {
    const size_t row = (size_t)b * S + s;
    const int64_t id = ids[row];
    const int ps = spos[s];
    if (lane == 0) pos_out[row] = ps;
    float v[NV][4];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int vi = lane + i * 64;
      if (vi < nvec) {
        const float4 w = *reinterpret_cast<const float4*>(word + (size_t)id * C + vi * 4);
        const float4 pp = *reinterpret_cast<const float4*>(pos_tab + (size_t)ps * C + vi * 4);
        const float4 t = *reinterpret_cast<const float4*>(type_tab + vi * 4);
        v[i][0] = w.x + t.x + pp.x; v[i][1] = w.y + t.y + pp.y; v[i][2] = w.z + t.z + pp.z; v[i][3] = w.w + t.w + pp.w;
        sum += v[i][0] + v[i][1] + v[i][2] + v[i][3];
      } else { v[i][0] = v[i][1] = v[i][2] = v[i][3] = 0.f; }
    }
    const float mu = wave_sum(sum) / C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i)
      if (lane + i * 64 < nvec)
#pragma unroll
        for (int e = 0; e < 4; ++e) { const float d = v[i][e] - mu; q += d * d; }
    const float rs = rsqrtf(wave_sum(q) / C + eps);
    if (lane == 0) { mean[row] = mu; rstd[row] = rs; }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int vi = lane + i * 64;
      if (vi < nvec) {
        const float4 g = *reinterpret_cast<const float4*>(gamma + vi * 4), bb = *reinterpret_cast<const float4*>(beta + vi * 4);
        const float gg[4] = {g.x, g.y, g.z, g.w}, be[4] = {bb.x, bb.y, bb.z, bb.w};
        bf16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float r = (v[i][e] - mu) * rs * gg[e] + be[e];
          if (p_drop > 0.f) r = drop_keep_e(drop_base(seed, (size_t)row * C + vi * 4), e, thresh) ? r * inv_keep : 0.f;
          o[e] = f2bf(r);
        }
        *reinterpret_cast<bf16x4*>(y + row * C + vi * 4) = o;
      }
    }
  }
}

template <int NV>
__global__ __launch_bounds__(256) void roberta_embed_bwd_kernel(const bf16* __restrict__ dy, const int64_t* __restrict__ ids,
                                                                const int* __restrict__ pos, const float* __restrict__ word,
                                                                const float* __restrict__ pos_tab, const float* __restrict__ type_tab,
                                                                const float* __restrict__ gamma, const float* __restrict__ mean,
                                                                const float* __restrict__ rstd, float* __restrict__ de_ws,
                                                                float* __restrict__ part, int rows,
                                                                int C, int pad, float p_drop, uint64_t seed,
                                                                const uint64_t* __restrict__ seed_base) {
  if (seed_base) seed += *seed_base;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nvec = C >> 2;
  const uint32_t thresh = (uint32_t)((double)p_drop * 4294967296.0);
  const float inv_keep = 1.f / (1.f - p_drop);
  float ag[NV][4], ab[NV][4], at[NV][4];
#pragma unroll
  for (int i = 0; i < NV; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) ag[i][e] = ab[i][e] = at[i][e] = 0.f;
  for (int row = blockIdx.x * 4 + wave; row < rows; row += gridDim.x * 4) {
    const int64_t id = ids[row];
    const int ps = pos[row];
    const float mu = mean[row], rs = rstd[row];
    float xh[NV][4], dg[NV][4];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int vi = lane + i * 64;
      if (vi < nvec) {
        const float4 w = *reinterpret_cast<const float4*>(word + (size_t)id * C + vi * 4);
        const float4 pp = *reinterpret_cast<const float4*>(pos_tab + (size_t)ps * C + vi * 4);
        const float4 t = *reinterpret_cast<const float4*>(type_tab + vi * 4);
        const float4 g = *reinterpret_cast<const float4*>(gamma + vi * 4);
        const float x[4] = {w.x + t.x + pp.x, w.y + t.y + pp.y, w.z + t.z + pp.z, w.w + t.w + pp.w};
        const float gg[4] = {g.x, g.y, g.z, g.w};
        const bf16x4 d4 = *reinterpret_cast<const bf16x4*>(dy + (size_t)row * C + vi * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float d = bf2f(d4[e]);
          if (p_drop > 0.f) d = drop_keep_e(drop_base(seed, (size_t)row * C + vi * 4), e, thresh) ? d * inv_keep : 0.f;
          xh[i][e] = (x[e] - mu) * rs;
          dg[i][e] = d * gg[e];
          s1 += dg[i][e];
          s2 += dg[i][e] * xh[i][e];
          ag[i][e] += d * xh[i][e];
          ab[i][e] += d;
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) xh[i][e] = dg[i][e] = 0.f;
      }
    }
    s1 = wave_sum(s1) / C;
    s2 = wave_sum(s2) / C;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int vi = lane + i * 64;
      if (vi < nvec) {
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          o[e] = rs * (dg[i][e] - s1 - xh[i][e] * s2);
          at[i][e] += o[e];
        }
        *reinterpret_cast<float4*>(de_ws + (size_t)row * C + vi * 4) = float4{o[0], o[1], o[2], o[3]};
      }
    }
  }
  // this wave's partial column sums: part[blockIdx.x * 4 + wave][dgamma | dbeta | dtype] (folded by embed_segsum_kernel)
  float* pw = part + (size_t)(blockIdx.x * 4 + wave) * 3 * C;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int vi = lane + i * 64;
    if (vi < nvec) {
      *reinterpret_cast<float4*>(pw + vi * 4) = float4{ag[i][0], ag[i][1], ag[i][2], ag[i][3]};
      *reinterpret_cast<float4*>(pw + C + vi * 4) = float4{ab[i][0], ab[i][1], ab[i][2], ab[i][3]};
      *reinterpret_cast<float4*>(pw + 2 * C + vi * 4) = float4{at[i][0], at[i][1], at[i][2], at[i][3]};
    }
  }
}

// Stable sort of the rows by key (blockIdx.y = 0: word id, 1: position) as ranks: rank(r) = #{k : key_k < key_r} + #{k < r : key_k == key_r}.
// Block = 64 rows (one per lane) x 8 waves, each wave counting over an eighth of all rows with the keys broadcast by readlane; the eight
// integer counts are added in LDS.  sorted[rank] = r, skey[rank] = key_r.  O(rows^2) integer compares: 20480 rows are about 420 M.
__global__ __launch_bounds__(512) void embed_rank_kernel(const int64_t* __restrict__ ids, const int* __restrict__ pos, int rows,
                                                         int* __restrict__ sorted, int* __restrict__ skey) {
  __shared__ int cnt_s[8][64];
  const int which = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = blockIdx.x * 64 + lane;
  auto key_of = [&](int k) { return which ? pos[k] : (int)ids[k]; };
  const int mine = r < rows ? key_of(r) : INT_MAX;
  const int span = ((rows + 511) / 512) * 64;            // an eighth of the rows, in whole 64-row chunks
  const int k1 = min(rows, (wave + 1) * span);
  int cnt = 0;
  for (int k0 = wave * span; k0 < k1; k0 += 64) {
    const int kk = k0 + lane < rows ? key_of(k0 + lane) : INT_MAX;
#pragma unroll
    for (int j = 0; j < 64; ++j) {
      const int kj = __builtin_amdgcn_readlane(kk, j);
      cnt += (kj < mine) | ((kj == mine) & (k0 + j < r));
    }
  }
  cnt_s[wave][lane] = cnt;
  __syncthreads();
  if (wave == 0 && r < rows) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < 8; ++w) t += cnt_s[w][lane];
    sorted[(size_t)which * rows + t] = r;
    skey[(size_t)which * rows + t] = mine;
  }
}

// out[key] = sum of de[row] over each key segment of the sorted order, in a fixed order; pad keys are skipped (nn.Embedding(padding_idx=pad):
// the pad row of both tables never receives a gradient, roberta.py:146,163).  Block = 16 sorted positions x 64 columns: 16 groups of 16 lanes
// (one float4 each).  A group whose position starts a segment of at most 32 rows sums it in ascending row order; longer segments (<s>,
// frequent words, the positions every sample reaches) are summed by the whole block: group g takes members g, g + 16, ... in ascending
// order, then the 16 group sums are added in order.  The trailing blocks fold the per-wave partials of dgamma / dbeta / dtype in a fixed order.
__global__ __launch_bounds__(256) void embed_segsum_kernel(const float* __restrict__ de, const int* __restrict__ sorted, const int* __restrict__ skey,
                                                           const float* __restrict__ part, float* __restrict__ dword, float* __restrict__ dpos,
                                                           float* __restrict__ dtype, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                           int rows, int C, int pad, int nparts, int ntile, int nchunk) {
  __shared__ float4 red[16][16];
  __shared__ int lkey[16], wfirst[4];
  const int tid = threadIdx.x;
  int bid = blockIdx.x;
  if (bid >= 2 * ntile * nchunk) {                       // fold: one column of [dgamma | dbeta | dtype] per thread
    const int j = (bid - 2 * ntile * nchunk) * 256 + tid, N = 3 * C;
    if (j >= N) return;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int y = 0;
    for (; y + 3 < nparts; y += 4) {
      s0 += part[(size_t)y * N + j]; s1 += part[(size_t)(y + 1) * N + j];
      s2 += part[(size_t)(y + 2) * N + j]; s3 += part[(size_t)(y + 3) * N + j];
    }
    for (; y < nparts; ++y) s0 += part[(size_t)y * N + j];
    const float t = (s0 + s1) + (s2 + s3);
    if (j < C) dgamma[j] = t; else if (j < 2 * C) dbeta[j - C] = t; else dtype[j - 2 * C] = t;
    return;
  }
  const int which = bid / (ntile * nchunk);
  bid -= which * ntile * nchunk;
  const int tile = bid / nchunk, chunk = bid - tile * nchunk;
  const int* srt = sorted + (size_t)which * rows;
  const int* sk = skey + (size_t)which * rows;
  float* out = which ? dpos : dword;
  const int g = tid >> 4, cl = tid & 15, gl0 = (tid & 63) & ~15;
  const int col = chunk * 64 + cl * 4;
  const bool colok = col < C;                            // C % 4 == 0: a float4 is wholly inside or outside
  const int i = tile * 16 + g;
  int key = 0, end = -1;
  bool head = false;
  if (i < rows) {
    key = sk[i];
    head = key != pad && (i == 0 || sk[i - 1] != key);
  }
  if (head) {                                            // the segment's end within the next 32 positions, 16 lanes at a time
    for (int e0 = i + 1; e0 < i + 33 && end < 0; e0 += 16) {
      const int e = e0 + cl;
      const unsigned long long bal = __ballot(e >= rows || sk[min(e, rows - 1)] != key);
      const unsigned bits = (unsigned)(bal >> gl0) & 0xFFFFu;
      if (bits) end = e0 + __builtin_ctz(bits);
    }
  }
  if (cl == 0) lkey[g] = head && end < 0 ? key : INT_MIN;
  if (head && end >= 0) {
    float4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int m0 = i; m0 < end; m0 += 16) {
      const int mi = m0 + cl < end ? srt[m0 + cl] : 0;
      const int cnt = min(16, end - m0);
      for (int q = 0; q < cnt; ++q) {
        const int row = __shfl(mi, gl0 + q);
        if (colok) {
          const float4 v = *reinterpret_cast<const float4*>(de + (size_t)row * C + col);
          acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
      }
    }
    if (colok) *reinterpret_cast<float4*>(out + (size_t)key * C + col) = acc;
  }
  __syncthreads();
  for (int h = 0; h < 16; ++h) {                         // long segments, whole block
    const int hk = lkey[h];
    if (hk == INT_MIN) continue;
    const int hs = tile * 16 + h;
    int hend = rows;
    for (int e0 = hs + 1; e0 < rows; e0 += 256) {        // first position past the segment
      const int e = e0 + tid;
      const unsigned long long bal = __ballot(e < rows && sk[min(e, rows - 1)] != hk);
      if ((tid & 63) == 0) wfirst[tid >> 6] = bal ? e0 + (tid & ~63) + __builtin_ctzll(bal) : INT_MAX;
      __syncthreads();
      const int f = min(min(wfirst[0], wfirst[1]), min(wfirst[2], wfirst[3]));
      __syncthreads();
      if (f != INT_MAX) { hend = f; break; }
    }
    float4 acc = {0.f, 0.f, 0.f, 0.f};
    if (colok) {
#pragma unroll 4
      for (int m = hs + g; m < hend; m += 16) {
        const float4 v = *reinterpret_cast<const float4*>(de + (size_t)srt[m] * C + col);
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
      }
    }
    red[g][cl] = acc;
    __syncthreads();
    if (g == 0 && colok) {
      float4 t = red[0][cl];
      for (int gg = 1; gg < 16; ++gg) { const float4 v = red[gg][cl]; t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w; }
      *reinterpret_cast<float4*>(out + (size_t)hk * C + col) = t;
    }
    __syncthreads();
  }
}

// img fp32 [B,3,H,W] -> cols bf16 [B*(H/4)*(W/4), 64]; column = c*16 + kh*4 + kw for c<3, zeros for 48..63.
// PAIR: the 2B-sample batch of the one-pass MLM + ITM step, [img ; where(sel, img, alt)] (objectives.py:56-61 builds the ITM half with a
// python loop over samples; compute_mlm_itm_fused concatenates the halves), gathered straight from the two sources: sample b < B reads
// img[b], sample B + b reads sel[b] ? img[b] : alt[b] -- no torch.where / torch.cat pass over the fp32 images (3.2 GB of traffic at B = 256).
template <bool PAIR>
__global__ __launch_bounds__(256) void im2col4_kernel(const float* __restrict__ img, const float* __restrict__ alt, const unsigned char* __restrict__ sel,
                                                      bf16* __restrict__ cols, int B, int H, int W) {
  const int Hp = H >> 2, Wp = W >> 2;
  const size_t total = (size_t)(PAIR ? 2 * B : B) * Hp * Wp * 16;   // 16 groups of 4 columns per patch
  for (size_t idx = blockIdx.x * (size_t)256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const int grp = idx & 15;
    const size_t patch = idx >> 4;
    const int j = patch % Wp, i = (patch / Wp) % Hp;
    int b = patch / ((size_t)Wp * Hp);
    const float* src = img;
    if constexpr (PAIR) {
      if (b >= B) { b -= B; if (!sel[b]) src = alt; }
    }
    bf16x4 o;
    if (grp < 12) {
      const int c = grp >> 2, kh = grp & 3;
      const float4 v = *reinterpret_cast<const float4*>(src + (((size_t)b * 3 + c) * H + i * 4 + kh) * W + j * 4);
      o[0] = f2bf(v.x); o[1] = f2bf(v.y); o[2] = f2bf(v.z); o[3] = f2bf(v.w);
    } else {
      o[0] = o[1] = o[2] = o[3] = f2bf(0.f);
    }
    *reinterpret_cast<bf16x4*>(cols + patch * 64 + grp * 4) = o;
  }
}

}  // namespace

// ids int64 [B,S]; tables fp32; y bf16 [B*S, C]; pos_out int32 [B*S]; mean/rstd fp32 [B*S].  C % 4 == 0, C <= 2048, S <= 1024
extern "C" int fiber_roberta_embed_fwd(const int64_t* ids, const float* word, const float* pos_tab, const float* type_tab,
                                       const float* gamma, const float* beta, void* y, int* pos_out, float* mean, float* rstd,
                                       int B, int S, int C, int pad, float eps, float p_drop, uint64_t seed, const uint64_t* seed_base,
                                       hipStream_t stream) {
  if (B <= 0) return FIBER_OK;
  if ((C & 3) || S > 1024 || C > 2048) return FIBER_EINVAL;
  if (fiber_misaligned(16, word, pos_tab, type_tab, gamma, beta) || fiber_misaligned(8, y)) return FIBER_EINVAL;   // float4 / bf16x4
  const int nv = cdiv(C >> 2, 64);
#define L(NV) hipLaunchKernelGGL((roberta_embed_fwd_kernel<NV>), dim3(B), dim3(256), 0, stream, ids, word, pos_tab, type_tab, gamma, beta, (bf16*)y, pos_out, mean, rstd, S, C, pad, eps, p_drop, seed, seed_base)
  if (nv <= 1) L(1); else if (nv <= 2) L(2); else if (nv <= 4) L(4); else L(8);
#undef L
  FIBER_CHECK_LAUNCH();
  return FIBER_OK;
}

// Workspace floats of fiber_roberta_embed_bwd: per-row gradients [B*S, C], per-wave partials [1024, 3C], two sorted orders [2][2][B*S] ints
extern "C" long fiber_roberta_embed_bwd_workspace(int B, int S, int C) {
  const long rows = (long)B * S;
  return rows * C + 1024L * 3 * C + 4 * rows;
}

// dword / dpos: the rows of the ids / positions present are OVERWRITTEN (the caller zeroes the tables for the others); dtype row 0, dgamma,
// dbeta: overwritten.  Every sum has a fixed order, so two runs give the same bits.  workspace: fiber_roberta_embed_bwd_workspace floats.
extern "C" int fiber_roberta_embed_bwd(const void* dy, const int64_t* ids, const int* pos, const float* word, const float* pos_tab,
                                       const float* type_tab, const float* gamma, const float* mean, const float* rstd,
                                       float* dword, float* dpos, float* dtype, float* dgamma, float* dbeta, float* workspace, int B, int S,
                                       int C, int pad, float p_drop, uint64_t seed, const uint64_t* seed_base, hipStream_t stream) {
  if (B <= 0 || S <= 0) return FIBER_OK;
  if ((C & 3) || C > 2048 || !workspace) return FIBER_EINVAL;
  if (fiber_misaligned(16, word, pos_tab, type_tab, gamma, dword, dpos, workspace) || fiber_misaligned(8, dy)) return FIBER_EINVAL;
  const int rows = B * S, nv = cdiv(C >> 2, 64);
  int grid = cdiv(rows, 4 * 4);
  grid = grid < 1 ? 1 : (grid > 256 ? 256 : grid);
  float* de = workspace;
  float* part = de + (size_t)rows * C;
  int* sorted = reinterpret_cast<int*>(part + (size_t)1024 * 3 * C);
  int* skey = sorted + 2 * (size_t)rows;
#define L(NV) hipLaunchKernelGGL((roberta_embed_bwd_kernel<NV>), dim3(grid), dim3(256), 0, stream, (const bf16*)dy, ids, pos, word, pos_tab, type_tab, gamma, mean, rstd, de, part, rows, C, pad, p_drop, seed, seed_base)
  if (nv <= 1) L(1); else if (nv <= 2) L(2); else if (nv <= 4) L(4); else L(8);
#undef L
  FIBER_CHECK_LAUNCH();
  hipLaunchKernelGGL(embed_rank_kernel, dim3(cdiv(rows, 64), 2), dim3(512), 0, stream, ids, pos, rows, sorted, skey);
  FIBER_CHECK_LAUNCH();
  const int ntile = cdiv(rows, 16), nchunk = cdiv(C, 64);
  hipLaunchKernelGGL(embed_segsum_kernel, dim3(2 * ntile * nchunk + cdiv(3 * C, 256)), dim3(256), 0, stream, de, sorted, skey, part, dword,
                     dpos, dtype, dgamma, dbeta, rows, C, pad, grid * 4, ntile, nchunk);
  FIBER_CHECK_LAUNCH();
  return FIBER_OK;
}

// img fp32 [B,3,H,W] (H, W multiples of 4) -> cols bf16 [B*(H/4)*(W/4), 64]
extern "C" int fiber_im2col_patch4(const float* img, void* cols, int B, int H, int W, hipStream_t stream) {
  if ((H & 3) || (W & 3) || fiber_misaligned(16, img) || fiber_misaligned(8, cols)) return FIBER_EINVAL;
  if (B <= 0) return FIBER_OK;                           // (a zero-sized grid is a launch error)
  const size_t total = (size_t)B * (H / 4) * (W / 4) * 16;
  size_t g = (total + 255) / 256;
  hipLaunchKernelGGL(im2col4_kernel<false>, dim3((int)(g > 4096 ? 4096 : g)), dim3(256), 0, stream, img, nullptr, nullptr, (bf16*)cols, B, H, W);
  FIBER_CHECK_LAUNCH();
  return FIBER_OK;
}

// img, alt fp32 [B,3,H,W]; sel uint8 [B] -> cols bf16 [2B*(H/4)*(W/4), 64] of the batch [img ; where(sel, img, alt)]
extern "C" int fiber_im2col_patch4_pair(const float* img, const float* alt, const unsigned char* sel, void* cols, int B, int H, int W,
                                        hipStream_t stream) {
  if ((H & 3) || (W & 3) || fiber_misaligned(16, img, alt) || fiber_misaligned(8, cols)) return FIBER_EINVAL;
  if (B <= 0) return FIBER_OK;
  const size_t total = (size_t)2 * B * (H / 4) * (W / 4) * 16;
  size_t g = (total + 255) / 256;
  hipLaunchKernelGGL(im2col4_kernel<true>, dim3((int)(g > 4096 ? 4096 : g)), dim3(256), 0, stream, img, alt, sel, (bf16*)cols, B, H, W);
  FIBER_CHECK_LAUNCH();
  return FIBER_OK;
}
