// Image-text retrieval evaluation (gfx950): the rank of the first matching candidate of every query, in both directions, and the
// recall@k tallies, from one fp32 score matrix without a sort, a temporary of the matrix's size or a host round trip.
// Replaces, of the coarse-grained reference (coarse_grained/fiber/modules/), objectives.py:361-383 (compute_itc_recall) and :477-497
// (compute_itm_recall): six torch.topk calls, six gathers of the id tables and six (ids == topk_ids).float().max().mean().
//
// Semantics.  scores fp32 [Ni, Nt] with row stride ld >= Nt, row = image, column = text; iids int32 [Ni], tiids int32 [Nt] (the image id
// each caption belongs to).  A query (text retrieval: an image row against the Nt captions; image retrieval: a caption column against
// the Ni images) orders its N candidates by descending score, EQUAL SCORES BY ASCENDING CANDIDATE INDEX.  rank = the 0-based position of
// the first candidate whose id equals the query's id; rank = N when none matches.  hit@k = rank < k, also for k > N (torch.topk would
// raise there; a query without a match then counts as a hit, which is what the rule says).  With (s*, c*) the best match -- maximum
// score, then minimum index -- rank = the number of NON-matching candidates c with s_c > s*, or s_c == s* and c < c*.  Two passes over
// the query's scores: find (s*, c*), then count.  Comparisons with NaN are false: a NaN candidate outranks nothing and, unless it is the
// first match met, is never the best match.
//
// Launch plan.  Text retrieval: one wave per image row, lanes striding the row (256-byte coalesced reads); (s*, c*) and the count are
// combined with wave shuffles.  Image retrieval: one workgroup of RT_WAVES waves per strip of 64 columns; a lane owns a column, so
// every row segment is one 256-byte read; wave w takes rows w, w + RT_WAVES, ...; (s*, c*) and the count are combined across the waves
// through LDS in wave order.  hits int32 [2, nk] (row 0 = image retrieval, row 1 = text retrieval: the reference's return order) is
// zeroed on the stream and receives integer atomic adds, which are order-independent: two runs give the same bits.  No floating-point
// atomics, no host read-back; everything runs on the caller's stream.
#include <climits>

#include "common.h"

namespace {

constexpr int RT_MAX_K = 8;
constexpr int RT_WAVES = 8;

// (s, c) beats (bs, bc): bc == INT_MAX means "none yet"
__device__ __forceinline__ bool rt_better(float s, int c, float bs, int bc) {
  return c != INT_MAX && (bc == INT_MAX || s > bs || (s == bs && c < bc));
}

__global__ __launch_bounds__(64) void retr_rows_kernel(const float* __restrict__ scores, const int* __restrict__ iids,
                                                       const int* __restrict__ tiids, const int* __restrict__ ks,
                                                       int* __restrict__ rank_tr, int* __restrict__ hits, int Nt, long long ld, int nk) {
  const int lane = threadIdx.x;
  const int i = blockIdx.x;
  const float* row = scores + (size_t)i * (size_t)ld;
  const int id = iids[i];
  float bs = 0.f;
  int bc = INT_MAX;
  for (int c = lane; c < Nt; c += 64) {                    // ascending c within a lane: an equal score never replaces
    if (tiids[c] != id) continue;
    const float s = row[c];
    if (bc == INT_MAX || s > bs) bs = s, bc = c;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float os = __shfl_xor(bs, o, 64);
    const int oc = __shfl_xor(bc, o, 64);
    if (rt_better(os, oc, bs, bc)) bs = os, bc = oc;
  }
  bs = __shfl(bs, 0, 64);                                  // one answer for the wave whatever NaNs did to the butterfly
  bc = __shfl(bc, 0, 64);
  int rank = Nt;
  if (bc != INT_MAX) {
    int n = 0;
    for (int c = lane; c < Nt; c += 64) {
      const float s = row[c];
      if (tiids[c] != id && (s > bs || (s == bs && c < bc))) ++n;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    rank = n;
  }
  if (lane == 0) rank_tr[i] = rank;
  if (lane < nk && rank < ks[lane]) atomicAdd(&hits[nk + lane], 1);
}

__global__ __launch_bounds__(RT_WAVES * 64) void retr_cols_kernel(const float* __restrict__ scores, const int* __restrict__ iids,
                                                                  const int* __restrict__ tiids, const int* __restrict__ ks,
                                                                  int* __restrict__ rank_ir, int* __restrict__ hits, int Ni, int Nt,
                                                                  long long ld, int nk) {
  __shared__ float sh_s[RT_WAVES][64];
  __shared__ int sh_c[RT_WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;
  const bool live = c < Nt;
  const int id = live ? tiids[c] : 0;
  const float* col = scores + (live ? c : 0);
  float bs = 0.f;
  int br = INT_MAX;
  if (live) {
    for (int r = wave; r < Ni; r += RT_WAVES) {            // ascending r within a wave
      if (iids[r] != id) continue;
      const float s = col[(size_t)r * (size_t)ld];
      if (br == INT_MAX || s > bs) bs = s, br = r;
    }
  }
  sh_s[wave][lane] = bs;
  sh_c[wave][lane] = br;
  __syncthreads();
  bs = sh_s[0][lane], br = sh_c[0][lane];
#pragma unroll
  for (int w = 1; w < RT_WAVES; ++w)                       // every wave folds in the same order: the same (s*, r*) in all of them
    if (rt_better(sh_s[w][lane], sh_c[w][lane], bs, br)) bs = sh_s[w][lane], br = sh_c[w][lane];
  __syncthreads();
  int n = 0;
  if (live && br != INT_MAX) {
    for (int r = wave; r < Ni; r += RT_WAVES) {
      const float s = col[(size_t)r * (size_t)ld];
      if (iids[r] != id && (s > bs || (s == bs && r < br))) ++n;
    }
  }
  sh_c[wave][lane] = n;
  __syncthreads();
  if (wave != 0 || !live) return;
  int rank = Ni;
  if (br != INT_MAX) {
    rank = 0;
#pragma unroll
    for (int w = 0; w < RT_WAVES; ++w) rank += sh_c[w][lane];
  }
  rank_ir[c] = rank;
  for (int k = 0; k < nk; ++k)
    if (rank < ks[k]) atomicAdd(&hits[k], 1);
}

}  // namespace

extern "C" int fiber_retrieval_ranks(const float* scores, const int* iids, const int* tiids, const int* ks, int* rank_tr, int* rank_ir,
                                     int* hits, int Ni, int Nt, long long ld, int nk, hipStream_t stream) {
  if (Ni < 0 || Nt < 0 || ld < Nt || nk < 0 || nk > RT_MAX_K) return FIBER_EINVAL;
  if ((Ni > 0 && (!iids || !rank_tr)) || (Nt > 0 && (!tiids || !rank_ir)) || (Ni > 0 && Nt > 0 && !scores) || (nk > 0 && (!ks || !hits)))
    return FIBER_EINVAL;
  if (fiber_misaligned(4, scores, iids, tiids, ks, rank_tr, rank_ir, hits)) return FIBER_EINVAL;
  if (nk > 0 && hipMemsetAsync(hits, 0, sizeof(int) * 2 * (size_t)nk, stream) != hipSuccess) return FIBER_ELAUNCH;
  if (Ni > 0) {
    hipLaunchKernelGGL(retr_rows_kernel, dim3((unsigned)Ni), dim3(64), 0, stream, scores, iids, tiids, ks, rank_tr, hits, Nt, ld, nk);
    FIBER_CHECK_LAUNCH();
  }
  if (Nt > 0) {
    hipLaunchKernelGGL(retr_cols_kernel, dim3((unsigned)((Nt + 63) / 64)), dim3(RT_WAVES * 64), 0, stream, scores, iids, tiids, ks,
                       rank_ir, hits, Ni, Nt, ld, nk);
    FIBER_CHECK_LAUNCH();
  }
  return FIBER_OK;
}
