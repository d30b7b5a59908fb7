// Phrase-grounding evaluation (gfx950): recall@k of fixed-shape Detections against per-phrase ground truth without a host round trip.
// Replaces, of the fine-grained reference (fine_grained/maskrcnn_benchmark/), engine/inference.py:311-327 (flickr_post_process: the boxes
// bucketed by label in score order plus a [0, 0, 0, 0] sentinel), data/datasets/evaluation/flickr/flickr_eval.py:173-204 + :365-383
// (box_iou and the recall@k tally of Flickr30kEntitiesRecallEvaluator.evaluate), data/datasets/refexp.py:58-74 (RefExpEvaluator.summarize)
// and layers/set_loss.py:15-52 (generalized_box_iou).  The reference does all of it per sentence in Python lists and numpy on the host.
// One wave per (image, phrase).  A detection's rank among its phrase's detections is a ballot + popcount per chunk of 64 with the running
// total carried across chunks.  The tallies are integer atomic adds: order-independent, so two runs give the same bits.
// IoU in the reference's operation order with contraction off; fp64 and fp32 divisions are the correctly rounded ones.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int GE_MAX_K = 8;
constexpr int GE_CATS = 64;

// flickr_eval.py:173-204 on one pair: (x1, y1, x2, y2), no +1
__device__ __forceinline__ double iou_f64(double a0, double a1, double a2, double a3, double g0, double g1, double g2, double g3) {
  const double area1 = (a2 - a0) * (a3 - a1);
  const double area2 = (g2 - g0) * (g3 - g1);
  const double w = fmax(fmin(a2, g2) - fmax(a0, g0), 0.0);
  const double h = fmax(fmin(a3, g3) - fmax(a1, g1), 0.0);
  const double inter = w * h;
  const double uni = area1 + area2 - inter;
  return inter / uni;
}

// set_loss.py:15-52 on one pair, fp32
__device__ __forceinline__ float giou_f32(float a0, float a1, float a2, float a3, float g0, float g1, float g2, float g3) {
  const float area1 = (a2 - a0) * (a3 - a1);
  const float area2 = (g2 - g0) * (g3 - g1);
  const float w = fmaxf(fminf(a2, g2) - fmaxf(a0, g0), 0.f);
  const float h = fmaxf(fminf(a3, g3) - fmaxf(a1, g1), 0.f);
  const float inter = w * h;
  const float uni = area1 + area2 - inter;
  const float iou = inter / uni;
  const float cw = fmaxf(fmaxf(a2, g2) - fminf(a0, g0), 0.f);
  const float ch = fmaxf(fmaxf(a3, g3) - fminf(a1, g1), 0.f);
  const float area = cw * ch;
  return iou - (area - uni) / area;
}

__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// mode 0: Flickr recall (fp64 IoU, rank among the detections labelled p + 1, sentinel after the last); mode 1: RefExp precision (fp32
// GIoU of boxes rounded to fp32, rank = position, no sentinel; count == 0 is a miss with best = -1).
__global__ __launch_bounds__(64) void ground_recall_kernel(const float* __restrict__ boxes, const int* __restrict__ labels,
                                                           const int* __restrict__ count, const double* __restrict__ gt,
                                                           const int* __restrict__ gt_count, const unsigned long long* __restrict__ cat_mask,
                                                           const int* __restrict__ topk, int* __restrict__ hit, double* __restrict__ best,
                                                           unsigned long long* __restrict__ positives,
                                                           unsigned long long* __restrict__ totals, int D, int P, int G, int K, int ncat,
                                                           double thresh, int mode) {
  const int lane = threadIdx.x;
  const size_t bp = blockIdx.x;                            // b * P + p
  const int b = (int)(bp / P), p = (int)(bp - (size_t)b * P);
  const int gc = min(gt_count[bp], G);
  if (gc <= 0) {                                           // no such phrase: written, counted nowhere
    if (lane < K) {
      hit[bp * K + lane] = 0;
      best[bp * K + lane] = 0.0;
    }
    return;
  }
  const int n = min(max(count[b], 0), D);
  const double* g = gt + bp * (size_t)G * 4;
  int ks[GE_MAX_K];
  double bk[GE_MAX_K];
#pragma unroll
  for (int k = 0; k < GE_MAX_K; ++k) {
    ks[k] = k < K ? topk[k] : 0;
    bk[k] = mode == 0 ? 0.0 : -1.0;                        // IoU >= 0 (the sentinel is always ranked); GIoU > -1
  }
  int carried = 0;
  for (int base = 0; base < n; base += 64) {
    const int i = base + lane;
    const bool in = i < n;
    const size_t row = (size_t)b * D + (in ? i : 0);
    const bool mine = in && (mode == 1 || labels[row] == p + 1);
    const unsigned long long word = __ballot(mine);
    if (mine) {
      const int rank = carried + __popcll(word & ((1ull << lane) - 1ull));
      const f32x4 bx = *reinterpret_cast<const f32x4*>(boxes + row * 4);
      double v;
      if (mode == 0) {
        v = 0.0;
        for (int j = 0; j < gc; ++j)
          v = fmax(v, iou_f64((double)bx[0], (double)bx[1], (double)bx[2], (double)bx[3], g[j * 4], g[j * 4 + 1], g[j * 4 + 2], g[j * 4 + 3]));
      } else {
        float vf = -1.f;
        for (int j = 0; j < gc; ++j)
          vf = fmaxf(vf, giou_f32(bx[0], bx[1], bx[2], bx[3], (float)g[j * 4], (float)g[j * 4 + 1], (float)g[j * 4 + 2], (float)g[j * 4 + 3]));
        v = (double)vf;
      }
#pragma unroll
      for (int k = 0; k < GE_MAX_K; ++k)
        if (ks[k] < 0 || rank < ks[k]) bk[k] = fmax(bk[k], v);
    }
    carried += __popcll(word);
  }
  if (mode == 0 && lane == 0) {                            // the sentinel [0, 0, 0, 0] at rank `carried`
    double v = 0.0;
    for (int j = 0; j < gc; ++j) v = fmax(v, iou_f64(0.0, 0.0, 0.0, 0.0, g[j * 4], g[j * 4 + 1], g[j * 4 + 2], g[j * 4 + 3]));
#pragma unroll
    for (int k = 0; k < GE_MAX_K; ++k)
      if (ks[k] < 0 || carried < ks[k]) bk[k] = fmax(bk[k], v);
  }
  unsigned hits = 0u;                                      // bit k: hit at topk[k] (wave-uniform after the reduction)
#pragma unroll
  for (int k = 0; k < GE_MAX_K; ++k) {
    if (k >= K) break;
    const double m = wave_max_f64(bk[k]);
    const bool h = mode == 0 ? m >= thresh : (float)m >= (float)thresh;
    if (h) hits |= 1u << k;
    if (lane == 0) {
      hit[bp * K + k] = h ? 1 : 0;
      best[bp * K + k] = m;
    }
  }
  const unsigned long long cats = ncat >= 64 ? cat_mask[bp] : cat_mask[bp] & ((1ull << ncat) - 1ull);
  if ((cats >> lane) & 1ull) {
    for (int k = 0; k < K; ++k) {
      atomicAdd(&totals[k * GE_CATS + lane], 1ull);
      if ((hits >> k) & 1u) atomicAdd(&positives[k * GE_CATS + lane], 1ull);
    }
  }
}

}  // namespace

extern "C" int fiber_ground_recall(const float* boxes, const int* labels, const int* count, const double* gt, const int* gt_count,
                                   const unsigned long long* cat_mask, const int* topk, int* hit, double* best, long long* positives,
                                   long long* totals, int B, int D, int P, int G, int K, int ncat, double thresh, int mode,
                                   hipStream_t stream) {
  if (mode != 0 && mode != 1) return FIBER_EINVAL;
  if (B < 0 || D < 0 || P < 0 || G < 0 || K < 0 || K > GE_MAX_K || ncat < 0 || ncat > GE_CATS) return FIBER_EINVAL;
  if (mode == 1 && P > 1) return FIBER_EINVAL;
  if ((long long)B * P > 0x7fffffffLL) return FIBER_EINVAL;
  if (B == 0 || P == 0 || K == 0) return FIBER_OK;
  if (!count || !gt_count || !cat_mask || !topk || !hit || !best || !positives || !totals) return FIBER_EINVAL;
  if ((D > 0 && (!boxes || (mode == 0 && !labels))) || (G > 0 && !gt)) return FIBER_EINVAL;
  if (fiber_misaligned(16, boxes) || fiber_misaligned(8, gt, cat_mask, best, positives, totals) ||
      fiber_misaligned(4, labels, count, gt_count, topk, hit))
    return FIBER_EINVAL;
  hipLaunchKernelGGL(ground_recall_kernel, dim3((unsigned)(B * P)), dim3(64), 0, stream, boxes, labels, count, gt, gt_count, cat_mask, topk,
                     hit, best, reinterpret_cast<unsigned long long*>(positives), reinterpret_cast<unsigned long long*>(totals), D, P, G,
                     K, ncat, thresh, mode);
  FIBER_CHECK_LAUNCH();
  return FIBER_OK;
}
