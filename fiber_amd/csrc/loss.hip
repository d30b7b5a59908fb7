// Cross-entropy over a wide vocabulary for bf16 logits (gfx950): forward = per-row log-sum-exp + picked logit in ONE read of
// the logits, backward = (softmax - onehot) * scale in one read + one write.  Replaces, on the caller side of the path
// (objectives.py:24-28: F.cross_entropy(mlm_logits.view(-1, vocab), labels, ignore_index=-100) over B*40 x 50265 logits), the
// ATen chain bf16->fp32 copy (2 GB) + log_softmax forward + backward + fp32->bf16, ~3.5 ms and 6 GB of temporaries per step.
// Rows are V = 50265 elements long, so a row starts at an arbitrary 2-byte offset: each row is walked as an unaligned head
// (<= 7 elements), 16-byte vectors, and a tail.
#include "common.h"

namespace {

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// one workgroup (256 threads) per row
// pred (nullable): arg max of the row, smallest index among equal maxima (what torch.argmax returns; bf16 logits DO tie), -1 on ignored rows --
// the accuracy metric of the step (my_metrics.py:5-28 takes logits.argmax over ALL rows, a 1-GB pass, and then drops the ignored ones).
__global__ __launch_bounds__(256) void ce_fwd_kernel(const bf16* __restrict__ x, const long long* __restrict__ labels,
                                                     float* __restrict__ loss, float* __restrict__ lse, int* __restrict__ pred, int V, long long ignore) {
  __shared__ float red_m[4], red_s[4];
  __shared__ int red_i[4];
  const int row = blockIdx.x;
  const long long lab = labels[row];
  if (lab == ignore) {                                   // ignored rows cost nothing (85 % of the MLM rows)
    if (threadIdx.x == 0) { loss[row] = 0.f; lse[row] = 0.f; if (pred) pred[row] = -1; }
    return;
  }
  const bf16* xr = x + (size_t)row * V;
  const int head = (int)((8 - (((size_t)row * V) & 7)) & 7);          // elements before the first 16-byte boundary
  const int nvec = (V - head) >> 3, tail0 = head + nvec * 8;
  float m = -INFINITY, s = 0.f;                          // online softmax: s = sum exp(x - m)
  int am = V;                                            // index of this thread's first maximum (its indices are visited in ascending order)
  auto add = [&](float v, int j) {
    if (v > m) { s = s * __expf(m - v) + 1.f; m = v; am = j; } else { s += __expf(v - m); }
  };
  if ((int)threadIdx.x < head) add(bf2f(xr[threadIdx.x]), threadIdx.x);
  for (int i = threadIdx.x; i < nvec; i += 256) {
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(xr + head + i * 8);
    float mx = bf2f(v[0]);
#pragma unroll
    for (int e = 1; e < 8; ++e) mx = fmaxf(mx, bf2f(v[e]));
    if (mx > m) {
      s *= __expf(m - mx); m = mx;
      int e0 = 7;
#pragma unroll
      for (int e = 6; e >= 0; --e) if (bf2f(v[e]) == mx) e0 = e;
      am = head + i * 8 + e0;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) s += __expf(bf2f(v[e]) - m);
  }
  if (tail0 + (int)threadIdx.x < V) add(bf2f(xr[tail0 + threadIdx.x]), tail0 + threadIdx.x);
  const float wm = wave_max(m);
  int wi = m == wm ? am : V;                             // smallest index among the lanes that hold the wave's maximum
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) wi = min(wi, __shfl_xor(wi, o));
  s = wave_sum(m == -INFINITY ? 0.f : s * __expf(m - wm));
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red_m[wave] = wm; red_s[wave] = s; red_i[wave] = wi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float M = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));
    float S = 0.f;
    int I = V;
    for (int w = 0; w < 4; ++w) {
      S += red_m[w] == -INFINITY ? 0.f : red_s[w] * __expf(red_m[w] - M);
      if (red_m[w] == M) I = min(I, red_i[w]);
    }
    const float l = M + __logf(S);
    lse[row] = l;
    loss[row] = l - bf2f(xr[lab]);
    if (pred) pred[row] = I;
  }
}

__global__ __launch_bounds__(256) void ce_bwd_kernel(const bf16* __restrict__ x, const long long* __restrict__ labels,
                                                     const float* __restrict__ lse, const float* __restrict__ scale,
                                                     bf16* __restrict__ dx, int V, long long ignore) {
  const int row = blockIdx.x;
  const long long lab = labels[row];
  const bf16* xr = x + (size_t)row * V;
  bf16* dr = dx + (size_t)row * V;
  const int head = (int)((8 - (((size_t)row * V) & 7)) & 7);
  const int nvec = (V - head) >> 3, tail0 = head + nvec * 8;
  if (lab == ignore) {                                   // zero gradient row
    const bf16 z = f2bf(0.f);
    if ((int)threadIdx.x < head) dr[threadIdx.x] = z;
    bf16x8 zv;
#pragma unroll
    for (int e = 0; e < 8; ++e) zv[e] = z;
    for (int i = threadIdx.x; i < nvec; i += 256) *reinterpret_cast<bf16x8*>(dr + head + i * 8) = zv;
    if (tail0 + (int)threadIdx.x < V) dr[tail0 + threadIdx.x] = z;
    return;
  }
  const float l = lse[row], sc = scale[0];
  auto g1 = [&](int j) { return (__expf(bf2f(xr[j]) - l) - (j == lab ? 1.f : 0.f)) * sc; };
  if ((int)threadIdx.x < head) dr[threadIdx.x] = f2bf(g1(threadIdx.x));
  for (int i = threadIdx.x; i < nvec; i += 256) {
    const int j0 = head + i * 8;
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(xr + j0);
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = f2bf((__expf(bf2f(v[e]) - l) - (j0 + e == lab ? 1.f : 0.f)) * sc);
    *reinterpret_cast<bf16x8*>(dr + j0) = o;
  }
  if (tail0 + (int)threadIdx.x < V) dr[tail0 + threadIdx.x] = f2bf(g1(tail0 + threadIdx.x));
}

// Column sums over the LABELLED rows of dlogits (rows whose label is the ignore index are exactly zero: ce_bwd_kernel wrote them): the bias
// gradient of the vocabulary decoder without reading the 85 % zero rows.  Workgroup = 256 columns x one slab of rows; the slab's labelled
// rows are listed in LDS first, then every thread walks its column over that list.  part [slabs][V] fp32; fiber_fold_rows_f32 adds the slabs.
__global__ __launch_bounds__(256) void colsum_labelled_kernel(const bf16* __restrict__ x, const long long* __restrict__ labels, float* __restrict__ part,
                                                              int rows, int V, int rows_per_slab, long long ignore) {
  extern __shared__ int list[];
  __shared__ int count;
  const int r0 = blockIdx.y * rows_per_slab, r1 = min(rows, r0 + rows_per_slab);
  if (threadIdx.x < 64) {                                // wave 0 lists the slab's labelled rows in ascending order (fixed summation order)
    int base = 0;
    for (int c0 = r0; c0 < r1; c0 += 64) {
      const int r = c0 + threadIdx.x;
      const bool keep = r < r1 && labels[r] != ignore;
      const unsigned long long mask = __ballot(keep);
      if (keep) list[base + __popcll(mask & ((1ull << threadIdx.x) - 1ull))] = r;
      base += __popcll(mask);
    }
    if (threadIdx.x == 0) count = base;
  }
  __syncthreads();
  const int n = count;
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= V) return;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  int i = 0;
  for (; i + 3 < n; i += 4) {
    a0 += bf2f(x[(size_t)list[i] * V + col]); a1 += bf2f(x[(size_t)list[i + 1] * V + col]);
    a2 += bf2f(x[(size_t)list[i + 2] * V + col]); a3 += bf2f(x[(size_t)list[i + 3] * V + col]);
  }
  for (; i < n; ++i) a0 += bf2f(x[(size_t)list[i] * V + col]);
  part[(size_t)blockIdx.y * V + col] = (a0 + a1) + (a2 + a3);
}

}  // namespace

// loss[r] = logsumexp(x[r, :]) - x[r, labels[r]] (0 where labels[r] == ignore_index); lse[r] saved for the backward.
// x: bf16 [rows, V] contiguous; labels: int64 [rows]; V > 16.
// pred (nullable): int32 [rows], arg max of every labelled row (smallest index among equal maxima), -1 on ignored rows.
extern "C" int fiber_ce_fwd_bf16(const void* logits, const long long* labels, float* loss, float* lse, int* pred, int rows, int V,
                                 long long ignore_index, hipStream_t stream) {
  if (rows <= 0) return FIBER_OK;
  if (V <= 16 || fiber_misaligned(16, logits)) return FIBER_EINVAL;   // (each row's unaligned head is worked out from row * V)
  hipLaunchKernelGGL(ce_fwd_kernel, dim3(rows), dim3(256), 0, stream, (const bf16*)logits, labels, loss, lse, pred, V, ignore_index);
  FIBER_CHECK_LAUNCH();
  return FIBER_OK;
}

// dlogits[r, j] = (exp(x[r, j] - lse[r]) - [j == labels[r]]) * scale[0]  (zero rows where labels[r] == ignore_index);
// scale: one fp32 in device memory (upstream gradient / number of valid rows), so no host synchronisation is needed.
extern "C" int fiber_ce_bwd_bf16(const void* logits, const long long* labels, const float* lse, const float* scale, void* dlogits,
                                 int rows, int V, long long ignore_index, hipStream_t stream) {
  if (rows <= 0) return FIBER_OK;
  if (V <= 16 || fiber_misaligned(16, logits, dlogits)) return FIBER_EINVAL;
  hipLaunchKernelGGL(ce_bwd_kernel, dim3(rows), dim3(256), 0, stream, (const bf16*)logits, labels, lse, scale, (bf16*)dlogits, V,
                     ignore_index);
  FIBER_CHECK_LAUNCH();
  return FIBER_OK;
}

// out[j] = sum over the rows r with labels[r] != ignore_index of x[r, j] (x: bf16 [rows, V], the dlogits fiber_ce_bwd_bf16 wrote: its other
// rows are zero).  workspace: fp32 [fiber_colsum_labelled_slabs(rows) * V].
// A slab's row list lives in LDS (one int per row of the slab): fiber_colsum_labelled_max_rows() is the largest row count whose slab plan
// fits; callers with more rows sum the columns another way (the entry point refuses them with FIBER_EINVAL).
constexpr int LABELLED_LIST_ROWS = 60 * 1024 / (int)sizeof(int), LABELLED_MAX_SLABS = 8;
extern "C" int fiber_colsum_labelled_slabs(int rows) { return rows >= 4096 ? LABELLED_MAX_SLABS : rows >= 512 ? 4 : 1; }
extern "C" int fiber_colsum_labelled_max_rows(void) { return LABELLED_MAX_SLABS * LABELLED_LIST_ROWS; }
extern "C" int fiber_colsum_labelled_bf16(const void* x, const long long* labels, float* out, float* workspace, int rows, int V,
                                          long long ignore_index, hipStream_t stream) {
  if (rows <= 0 || V <= 0) return FIBER_OK;
  const int slabs = fiber_colsum_labelled_slabs(rows), rps = cdiv(rows, slabs);
  if (rps > LABELLED_LIST_ROWS) return FIBER_EINVAL;
  float* part = slabs > 1 ? workspace : out;
  if (slabs > 1 && !workspace) return FIBER_EINVAL;
  hipLaunchKernelGGL(colsum_labelled_kernel, dim3(cdiv(V, 256), slabs), dim3(256), (size_t)rps * sizeof(int), stream, (const bf16*)x, labels, part,
                     rows, V, rps, ignore_index);
  FIBER_CHECK_LAUNCH();
  if (slabs > 1) return fiber_fold_rows_f32(part, out, slabs, V, stream);
  return FIBER_OK;
}

// ---- CIDEr-optimised caption training (objectives.py:712-896): sampled decoding and the sequence log-probability loss --------------------
namespace {

constexpr int SAMPLE_MAX_K = 8;
constexpr float FORCED_LOGIT = -10000.f;                 // the [MASK] logit of objectives.py:757

// Gumbel noise of one draw: g = -log(-log(u)), u = (h + 0.5) 2^-32.  In fp32 u rounds to 1 for h >= 2^32 - 128 (g = inf), so the upper half of
// the range takes -log(u) = -log1p(-(1 - u)) with 1 - u = (~h + 0.5) 2^-32.
__device__ __forceinline__ float gumbel_of(uint32_t h) {
  const float a = (h & 0x80000000u) ? -log1pf(-(((float)(~h) + 0.5f) * 0x1p-32f)) : -logf(((float)h + 0.5f) * 0x1p-32f);
  return -logf(a);
}

// one workgroup (256 threads) per row: K Gumbel-max draws and the row's log-sum-exp in ONE read of the row, no probability tensor.
// rows = bs * beam (5..250 at the named config) is far below the CU count (256): most of the device idles during a decode step's draw.  That is
// accepted -- a step re-runs the whole text stack, beside which rows * K * V ~ 1e7 draws (three 64-bit multiplies and two logarithms each) are small.
template <int K>
__global__ __launch_bounds__(256) void sample_rows_kernel(const bf16* __restrict__ x, const unsigned char* __restrict__ ended,
                                                          long long* __restrict__ tokens, float* __restrict__ logp,
                                                          unsigned char* __restrict__ ended_out, int V, int forced, uint64_t key,
                                                          const uint64_t* __restrict__ seed_base, long long pad_id, long long sep_id) {
  __shared__ float red_m[4], red_s[4], red_b[4][K];
  __shared__ int red_i[4][K];
  const int row = blockIdx.x;
  if (ended && ended[row]) {                             // an ended beam is padded; its row is not read
    if ((int)threadIdx.x < K) {
      tokens[(size_t)row * K + threadIdx.x] = pad_id; logp[(size_t)row * K + threadIdx.x] = 0.f; ended_out[(size_t)row * K + threadIdx.x] = 1;
    }
    return;
  }
  if (seed_base) key += *seed_base;
  const bf16* xr = x + (size_t)row * V;
  const int head = (int)((8 - (((size_t)row * V) & 7)) & 7);
  const int nvec = (V - head) >> 3, tail0 = head + nvec * 8;
  float m = -INFINITY, s = 0.f;                          // online softmax, as ce_fwd_kernel
  float best[K];
  int bi[K];                                             // first index of this thread's best perturbed score (indices ascend per thread)
#pragma unroll
  for (int k = 0; k < K; ++k) { best[k] = -INFINITY; bi[k] = V; }
  const uint64_t draw0 = (uint64_t)row * (uint64_t)K;
  auto draw = [&](float z, int j) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float sc = z + gumbel_of(hash_u32(key, (draw0 + (uint64_t)k) * (uint64_t)V + (uint64_t)j));
      if (sc > best[k]) { best[k] = sc; bi[k] = j; }
    }
  };
  auto one = [&](int j) {
    const float v = j == forced ? FORCED_LOGIT : bf2f(xr[j]);
    if (v > m) { s = s * __expf(m - v) + 1.f; m = v; } else { s += __expf(v - m); }
    draw(v, j);
  };
  if ((int)threadIdx.x < head) one(threadIdx.x);
  for (int i = threadIdx.x; i < nvec; i += 256) {
    const int j0 = head + i * 8;
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(xr + j0);
    float f[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = j0 + e == forced ? FORCED_LOGIT : bf2f(v[e]);
    float mx = f[0];
#pragma unroll
    for (int e = 1; e < 8; ++e) mx = fmaxf(mx, f[e]);
    if (mx > m) { s *= __expf(m - mx); m = mx; }
#pragma unroll
    for (int e = 0; e < 8; ++e) s += __expf(f[e] - m);
#pragma unroll
    for (int e = 0; e < 8; ++e) draw(f[e], j0 + e);
  }
  if (tail0 + (int)threadIdx.x < V) one(tail0 + threadIdx.x);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float wm = wave_max(m);
  s = wave_sum(m == -INFINITY ? 0.f : s * __expf(m - wm));
  if (lane == 0) { red_m[wave] = wm; red_s[wave] = s; }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float wb = wave_max(best[k]);
    int wi = best[k] == wb ? bi[k] : V;                  // smallest index among the lanes that hold the wave's maximum
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) wi = min(wi, __shfl_xor(wi, o));
    if (lane == 0) { red_b[wave][k] = wb; red_i[wave][k] = wi; }
  }
  __syncthreads();
  if ((int)threadIdx.x < K) {
    const int k = threadIdx.x;
    const float M = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));
    float S = 0.f;
    for (int w = 0; w < 4; ++w) S += red_m[w] == -INFINITY ? 0.f : red_s[w] * __expf(red_m[w] - M);
    const double l = (double)M + log((double)S);           // one rounding for logp: z_tok - l is formed in fp64 (K threads per row)
    const float B = fmaxf(fmaxf(red_b[0][k], red_b[1][k]), fmaxf(red_b[2][k], red_b[3][k]));
    int I = V;
    for (int w = 0; w < 4; ++w)
      if (red_b[w][k] == B) I = min(I, red_i[w][k]);
    I = min(I, V - 1);                                   // (only a row of NaN logits leaves I == V)
    const size_t o = (size_t)row * K + k;
    tokens[o] = I;
    logp[o] = (float)((double)(I == forced ? FORCED_LOGIT : bf2f(xr[I])) - l);
    ended_out[o] = (I == pad_id || I == sep_id) ? 1 : 0;
  }
}

// lp[r] = log(exp(x[r, l] - lse[r]) + 1e-9), l = labels[r]; 0 (and lse 0) where l == pad_id.  A label outside [0, V) is treated like pad_id.
__global__ __launch_bounds__(256) void seqlogp_fwd_kernel(const bf16* __restrict__ x, const long long* __restrict__ labels, float* __restrict__ lp,
                                                          float* __restrict__ lse, int V, long long pad_id) {
  __shared__ float red_m[4], red_s[4];
  const int row = blockIdx.x;
  const long long lab = labels[row];
  if (lab == pad_id || (unsigned long long)lab >= (unsigned long long)V) {
    if (threadIdx.x == 0) { lp[row] = 0.f; lse[row] = 0.f; }
    return;
  }
  const bf16* xr = x + (size_t)row * V;
  const int head = (int)((8 - (((size_t)row * V) & 7)) & 7);
  const int nvec = (V - head) >> 3, tail0 = head + nvec * 8;
  float m = -INFINITY, s = 0.f;
  auto add = [&](float v) {
    if (v > m) { s = s * __expf(m - v) + 1.f; m = v; } else { s += __expf(v - m); }
  };
  if ((int)threadIdx.x < head) add(bf2f(xr[threadIdx.x]));
  for (int i = threadIdx.x; i < nvec; i += 256) {
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(xr + head + i * 8);
    float mx = bf2f(v[0]);
#pragma unroll
    for (int e = 1; e < 8; ++e) mx = fmaxf(mx, bf2f(v[e]));
    if (mx > m) { s *= __expf(m - mx); m = mx; }
#pragma unroll
    for (int e = 0; e < 8; ++e) s += __expf(bf2f(v[e]) - m);
  }
  if (tail0 + (int)threadIdx.x < V) add(bf2f(xr[tail0 + threadIdx.x]));
  const float wm = wave_max(m);
  s = wave_sum(m == -INFINITY ? 0.f : s * __expf(m - wm));
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red_m[wave] = wm; red_s[wave] = s; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float M = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));
    float S = 0.f;
    for (int w = 0; w < 4; ++w) S += red_m[w] == -INFINITY ? 0.f : red_s[w] * __expf(red_m[w] - M);
    // The row's last steps in fp64 (one thread per row): x_l - lse and lp are both near 20 in magnitude where the epsilon matters, and an fp32
    // rounding of each (ulp 2^-19) plus that of lse would use up the whole 2^-23 (1 + |lse| + |x_l|) allowance.  One rounding each instead.
    const double l = (double)M + log((double)S);
    lse[row] = (float)l;
    lp[row] = (float)log(exp((double)bf2f(xr[lab]) - l) + 1e-9);   // the epsilon INSIDE the logarithm, as objectives.py:818
  }
}

// dx[r, j] = rowscale[r] * (p_l / (p_l + 1e-9)) * ([j == l] - p_j), p = exp(x - lse); exact zero rows where l == pad_id (or outside [0, V)).
__global__ __launch_bounds__(256) void seqlogp_bwd_kernel(const bf16* __restrict__ x, const long long* __restrict__ labels,
                                                          const float* __restrict__ lse, const float* __restrict__ rowscale,
                                                          bf16* __restrict__ dx, int V, long long pad_id) {
  const int row = blockIdx.x;
  const long long lab = labels[row];
  const bf16* xr = x + (size_t)row * V;
  bf16* dr = dx + (size_t)row * V;
  const int head = (int)((8 - (((size_t)row * V) & 7)) & 7);
  const int nvec = (V - head) >> 3, tail0 = head + nvec * 8;
  if (lab == pad_id || (unsigned long long)lab >= (unsigned long long)V) {
    const bf16 z = f2bf(0.f);
    if ((int)threadIdx.x < head) dr[threadIdx.x] = z;
    bf16x8 zv;
#pragma unroll
    for (int e = 0; e < 8; ++e) zv[e] = z;
    for (int i = threadIdx.x; i < nvec; i += 256) *reinterpret_cast<bf16x8*>(dr + head + i * 8) = zv;
    if (tail0 + (int)threadIdx.x < V) dr[tail0 + threadIdx.x] = z;
    return;
  }
  const float l = lse[row];
  const float pl = expf(bf2f(xr[lab]) - l);
  const float c = rowscale[row] * (pl / (pl + 1e-9f));
  auto g1 = [&](int j) { return ((j == lab ? 1.f : 0.f) - __expf(bf2f(xr[j]) - l)) * c; };
  if ((int)threadIdx.x < head) dr[threadIdx.x] = f2bf(g1(threadIdx.x));
  for (int i = threadIdx.x; i < nvec; i += 256) {
    const int j0 = head + i * 8;
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(xr + j0);
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = f2bf(((j0 + e == lab ? 1.f : 0.f) - __expf(bf2f(v[e]) - l)) * c);
    *reinterpret_cast<bf16x8*>(dr + j0) = o;
  }
  if (tail0 + (int)threadIdx.x < V) dr[tail0 + threadIdx.x] = f2bf(g1(tail0 + threadIdx.x));
}

}  // namespace

// K tokens per row drawn with replacement from softmax(x[r, :]) by Gumbel-max: tokens[r, k] = arg max_j (z_j - log(-log(u))), smallest index among
// equal maxima, u = (hash_u32(key, (r K + k) V + j) + 0.5) 2^-32 (key = seed + *seed_base), z = x with column forced_id read as -10000 (forced_id < 0:
// none); logp[r, k] = z_tok - logsumexp(z); ended_out[r, k] = tok in {pad_id, sep_id}.  ended (nullable, uint8 [rows]): such a row is not read, its
// tokens are pad_id, its logp 0, its ended_out 1.  x: bf16 [rows, V] contiguous, V > 16, 1 <= K <= 8.
extern "C" int fiber_sample_rows_bf16(const void* logits, const unsigned char* ended, long long* tokens, float* logp, unsigned char* ended_out,
                                      int rows, int V, int K, int forced_id, uint64_t seed, const uint64_t* seed_base, long long pad_id,
                                      long long sep_id, hipStream_t stream) {
  if (rows <= 0) return FIBER_OK;
  if (V <= 16 || K < 1 || K > SAMPLE_MAX_K || forced_id >= V || fiber_misaligned(16, logits)) return FIBER_EINVAL;
#define FIBER_SAMPLE_K(k)                                                                                                              \
  case k:                                                                                                                              \
    hipLaunchKernelGGL(sample_rows_kernel<k>, dim3(rows), dim3(256), 0, stream, (const bf16*)logits, ended, tokens, logp, ended_out, V, \
                       forced_id, seed, seed_base, pad_id, sep_id);                                                                     \
    break;
  switch (K) {                                           // K is a compile-time constant of the kernel: the per-draw state stays in registers
    FIBER_SAMPLE_K(1) FIBER_SAMPLE_K(2) FIBER_SAMPLE_K(3) FIBER_SAMPLE_K(4) FIBER_SAMPLE_K(5) FIBER_SAMPLE_K(6) FIBER_SAMPLE_K(7) FIBER_SAMPLE_K(8)
  }
#undef FIBER_SAMPLE_K
  FIBER_CHECK_LAUNCH();
  return FIBER_OK;
}

// lp[r] = log(softmax(x[r, :])[labels[r]] + 1e-9) (0 where labels[r] == pad_id), lse[r] saved for the backward (0 on those rows).
extern "C" int fiber_seqlogp_fwd_bf16(const void* logits, const long long* labels, float* lp, float* lse, int rows, int V, long long pad_id,
                                      hipStream_t stream) {
  if (rows <= 0) return FIBER_OK;
  if (V <= 16 || fiber_misaligned(16, logits)) return FIBER_EINVAL;
  hipLaunchKernelGGL(seqlogp_fwd_kernel, dim3(rows), dim3(256), 0, stream, (const bf16*)logits, labels, lp, lse, V, pad_id);
  FIBER_CHECK_LAUNCH();
  return FIBER_OK;
}

// dlogits[r, j] = rowscale[r] * (p_l / (p_l + 1e-9)) * ([j == l] - p_j); rowscale: fp32 [rows] in device memory (the upstream gradient of lp[r]),
// so no host synchronisation is needed; zero rows where labels[r] == pad_id.
extern "C" int fiber_seqlogp_bwd_bf16(const void* logits, const long long* labels, const float* lse, const float* rowscale, void* dlogits,
                                      int rows, int V, long long pad_id, hipStream_t stream) {
  if (rows <= 0) return FIBER_OK;
  if (V <= 16 || fiber_misaligned(16, logits, dlogits)) return FIBER_EINVAL;
  hipLaunchKernelGGL(seqlogp_bwd_kernel, dim3(rows), dim3(256), 0, stream, (const bf16*)logits, labels, lse, rowscale, (bf16*)dlogits, V, pad_id);
  FIBER_CHECK_LAUNCH();
  return FIBER_OK;
}
