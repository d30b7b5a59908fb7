// Grounding training (gfx950): ATSS target assignment and the box-regression (GIoU) / centerness losses without a host synchronisation.
// Replaces, of the fine-grained reference (fine_grained/maskrcnn_benchmark/), modeling/rpn/loss.py:626-827 (prepare_targets),
// structures/boxlist_ops.py:96-135 (boxlist_iou, +1 convention), modeling/box_coder.py:22-95 (encode / decode), loss.py:583-624 (GIoULoss),
// :829-844 (compute_centerness_targets), BCEWithLogitsLoss(reduction="sum") and the pos_inds gathers (:1194, :1237-1254).
// The reference loops over images with topk, boolean gathers, nonzero and .item() on [A, G] matrices; here every shape follows from
// (B, Gmax, level sizes, T): padding gts (g >= num_gt[b]) are never read for a decision, unassigned anchors are masked, sums run
// lane -> wave -> workgroup -> one partial per workgroup -> fiber_fold_rows_f32.  The only atomics are integer (a 64-bit max, a count):
// their results do not depend on arrival order, so two runs give the same bits.  IoU, encode, decode and the 0.01 test are evaluated in
// the reference's operation order with contraction off.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int ATSS_MAX_LEVELS = 8;
constexpr int ATSS_MAX_K = 128;            // candidates per gt: two per lane of the threshold kernel
constexpr int DT = 256;                    // tokens (the only supported size)
constexpr float CLIP = 4.135166556742356f; // log(1000 / 16)

struct Levels {
  int n;
  int off[ATSS_MAX_LEVELS + 1];            // anchor offsets of the levels in the concatenated anchors
  int slot[ATSS_MAX_LEVELS + 1];           // candidate-slot offsets: slot[l + 1] - slot[l] = k_l = min(topk, A_l)
};

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long w = __shfl_xor(v, o);
    v = w < v ? w : v;
  }
  return v;
}

// boxlist_iou (boxlist_ops.py:116-130) of anchor `an` (boxlist1) and gt `gt` (boxlist2)
__device__ __forceinline__ float iou_plus_one(f32x4 an, f32x4 gt) {
  const float area1 = (an[2] - an[0] + 1.f) * (an[3] - an[1] + 1.f);
  const float area2 = (gt[2] - gt[0] + 1.f) * (gt[3] - gt[1] + 1.f);
  const float w = fmaxf(fminf(an[2], gt[2]) - fmaxf(an[0], gt[0]) + 1.f, 0.f);
  const float h = fmaxf(fminf(an[3], gt[3]) - fmaxf(an[1], gt[1]) + 1.f, 0.f);
  const float inter = w * h;
  return inter / (area1 + area2 - inter);
}

// Stage 1 (loss.py:699-719): one wave per (level, gt, image); k_l rounds of a wave-wide arg-min over the level's anchors on the key
// (distance bits << 32 | anchor index), each round taking the smallest key above the previous pick: equal distances go to the lowest
// anchor index.  Distances are >= 0, so their bit patterns order as the floats do.
__global__ __launch_bounds__(64) void atss_candidates_kernel(const float* __restrict__ anchors, const float* __restrict__ gt_boxes,
                                                             const int* __restrict__ num_gt, int* __restrict__ cand_idx,
                                                             float* __restrict__ cand_iou, Levels lv, int Gmax, int K) {
  const int l = blockIdx.x, g = blockIdx.y, b = blockIdx.z, lane = threadIdx.x;
  if (g >= num_gt[b]) return;                              // padding row: never read
  const f32x4 gt = *reinterpret_cast<const f32x4*>(gt_boxes + ((size_t)b * Gmax + g) * 4);
  const float gcx = (gt[2] + gt[0]) / 2.0f, gcy = (gt[3] + gt[1]) / 2.0f;
  const int lo = lv.off[l], hi = lv.off[l + 1], k = lv.slot[l + 1] - lv.slot[l];
  const size_t out = ((size_t)b * Gmax + g) * K + lv.slot[l];
  unsigned long long prev = 0ull;
  for (int r = 0; r < k; ++r) {
    unsigned long long best = ~0ull;
    for (int a = lo + lane; a < hi; a += 64) {
      const f32x4 an = *reinterpret_cast<const f32x4*>(anchors + (size_t)a * 4);
      const float dx = (an[2] + an[0]) / 2.0f - gcx, dy = (an[3] + an[1]) / 2.0f - gcy;
      const float d = sqrtf(dx * dx + dy * dy);
      const unsigned long long key = ((unsigned long long)__builtin_bit_cast(unsigned, d) << 32) | (unsigned)a;
      if ((r == 0 || key > prev) && key < best) best = key;
    }
    best = wave_min_u64(best);
    prev = best;
    if (lane == 0) {
      const int a = (int)(unsigned)best;                    // (a NaN distance still orders: the pick stays inside [lo, hi))
      const bool ok = best != ~0ull;
      cand_idx[out + r] = ok ? a : -1;
      cand_iou[out + r] = ok ? iou_plus_one(*reinterpret_cast<const f32x4*>(anchors + (size_t)a * 4), gt) : 0.f;
    }
  }
}

// Stages 2 and 3 (loss.py:721-755): one wave per (gt, image).  Lane j holds candidates j and j + 64; mean and unbiased std by the
// xor-butterfly (a fixed order); a positive candidate enters the anchor's key (iou bits << 32 | 0xFFFFFFFF - g) by a 64-bit integer max:
// highest IoU wins, equal IoU goes to the lowest gt index.  key 0 = unassigned (a positive's IoU is > 0, and g < 2^32 - 1 anyway).
__global__ __launch_bounds__(64) void atss_resolve_kernel(const float* __restrict__ anchors, const float* __restrict__ gt_boxes,
                                                          const int* __restrict__ num_gt, const int* __restrict__ cand_idx,
                                                          const float* __restrict__ cand_iou, unsigned long long* __restrict__ key,
                                                          int Gmax, int A, int K) {
  const int g = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  if (g >= num_gt[b]) return;
  const size_t row = ((size_t)b * Gmax + g) * K;
  const int j0 = lane, j1 = lane + 64;
  const float i0 = j0 < K ? cand_iou[row + j0] : 0.f, i1 = j1 < K ? cand_iou[row + j1] : 0.f;
  const float mean = wave_sum(i0 + i1) / (float)K;
  const float d0 = j0 < K ? i0 - mean : 0.f, d1 = j1 < K ? i1 - mean : 0.f;
  const float sd = sqrtf(wave_sum(d0 * d0 + d1 * d1) / (float)(K - 1));
  const float thresh = mean + sd;
  const f32x4 gt = *reinterpret_cast<const f32x4*>(gt_boxes + ((size_t)b * Gmax + g) * 4);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int j = h ? j1 : j0;
    const float iou = h ? i1 : i0;
    if (j >= K) continue;
    const int a = cand_idx[row + j];
    if (a < 0 || a >= A) continue;
    const f32x4 an = *reinterpret_cast<const f32x4*>(anchors + (size_t)a * 4);
    const float acx = (an[2] + an[0]) / 2.0f, acy = (an[3] + an[1]) / 2.0f;
    const float m = fminf(fminf(acx - gt[0], acy - gt[1]), fminf(gt[2] - acx, gt[3] - acy));
    if (iou >= thresh && m > 0.01f) {
      const unsigned long long kk = ((unsigned long long)__builtin_bit_cast(unsigned, iou) << 32) | (0xFFFFFFFFu - (unsigned)g);
      atomicMax(key + (size_t)b * A + a, kk);
    }
  }
}

// One pass over the anchors (loss.py:756-804): 16 lanes per anchor, lane c of them stores bytes [16 c, 16 c + 16) of the token row.
__global__ __launch_bounds__(256) void atss_finalize_kernel(const float* __restrict__ anchors, const float* __restrict__ gt_boxes,
                                                            const int* __restrict__ gt_labels, const unsigned char* __restrict__ pmap,
                                                            const unsigned long long* __restrict__ key, int* __restrict__ matched,
                                                            int* __restrict__ labels, float* __restrict__ reg, unsigned char* __restrict__ tok,
                                                            int* __restrict__ num_pos, int Gmax, int A) {
  const int b = blockIdx.y, sub = threadIdx.x >> 4, c = threadIdx.x & 15;
  const int a = blockIdx.x * 16 + sub;
  const bool in = a < A;
  const unsigned long long kk = in ? key[(size_t)b * A + a] : 0ull;
  const unsigned gk = 0xFFFFFFFFu - (unsigned)kk;
  const bool hit = kk != 0ull && gk < (unsigned)Gmax;       // (a key this file did not write cannot index past the gts)
  const int g = hit ? (int)gk : -1;
  const int lab = hit ? gt_labels[(size_t)b * Gmax + g] : 0;
  if (in) {
    const size_t row = (size_t)b * A + a;
    uint4 t = uint4{0u, 0u, 0u, 0u};
    if (hit) t = *reinterpret_cast<const uint4*>(pmap + ((size_t)b * Gmax + g) * DT + c * 16);
    else if (c == 15) t.w = 1u << 24;                       // the one-hot on token T - 1 (loss.py:767-769)
    *reinterpret_cast<uint4*>(tok + row * DT + c * 16) = t;
    if (c == 0) {
      f32x4 r = f32x4{0.f, 0.f, 0.f, 0.f};
      if (hit) {                                            // BoxCoder.encode (box_coder.py:32-47), weights (10, 10, 5, 5)
        const f32x4 an = *reinterpret_cast<const f32x4*>(anchors + (size_t)a * 4);
        const f32x4 gt = *reinterpret_cast<const f32x4*>(gt_boxes + ((size_t)b * Gmax + g) * 4);
        const float ew = an[2] - an[0] + 1.f, eh = an[3] - an[1] + 1.f;
        const float ecx = an[0] + 0.5f * ew, ecy = an[1] + 0.5f * eh;
        const float gw = gt[2] - gt[0] + 1.f, gh = gt[3] - gt[1] + 1.f;
        const float gcx = gt[0] + 0.5f * gw, gcy = gt[1] + 0.5f * gh;
        r[0] = 10.f * (gcx - ecx) / ew;
        r[1] = 10.f * (gcy - ecy) / eh;
        r[2] = 5.f * logf(gw / ew);
        r[3] = 5.f * logf(gh / eh);
      }
      matched[row] = g;
      labels[row] = lab;
      *reinterpret_cast<f32x4*>(reg + row * 4) = r;
    }
  }
  const unsigned long long pos = __ballot(in && c == 0 && lab > 0);
  if ((threadIdx.x & 63) == 0 && pos) atomicAdd(num_pos + b, __popcll(pos));
}

// ---- losses ---------------------------------------------------------------------------------------------------------------------------
struct Box { float x1, y1, x2, y2, w, h; };                  // w, h: the decoded extents exp(d) * anchor extent

// BoxCoder.decode (box_coder.py:64-93) of the code (r0, r1, r2, r3) against anchor `an`
__device__ __forceinline__ Box decode(f32x4 an, float r0, float r1, float r2, float r3) {
  const float w = an[2] - an[0] + 1.f, h = an[3] - an[1] + 1.f;
  const float cx = an[0] + 0.5f * w, cy = an[1] + 0.5f * h;
  const float dx = r0 / 10.f, dy = r1 / 10.f;
  const float dw = fminf(r2 / 5.f, CLIP), dh = fminf(r3 / 5.f, CLIP);
  const float px = dx * w + cx, py = dy * h + cy;
  Box o;
  o.w = expf(dw) * w;
  o.h = expf(dh) * h;
  o.x1 = px - 0.5f * o.w;
  o.y1 = py - 0.5f * o.h;
  o.x2 = px + 0.5f * o.w - 1.f;
  o.y2 = py + 0.5f * o.h - 1.f;
  return o;
}

// compute_centerness_targets (loss.py:829-842) from the decoded target box
__device__ __forceinline__ float centerness_target(f32x4 an, const Box& t) {
  const float acx = (an[2] + an[0]) / 2.f, acy = (an[3] + an[1]) / 2.f;
  const float l = acx - t.x1, tp = acy - t.y1, r = t.x2 - acx, bt = t.y2 - acy;
  return sqrtf((fminf(l, r) / fmaxf(l, r)) * (fminf(tp, bt) / fmaxf(tp, bt)));
}

// torch's subgradients: maximum / minimum give the whole gradient to the selected argument and half to each on a tie
__device__ __forceinline__ float sel_gt(float a, float b) { return a > b ? 1.f : (a == b ? 0.5f : 0.f); }

struct Giou {
  float loss;                                                // 1 - giou
  float dx1, dy1, dx2, dy2;                                  // d loss / d decoded prediction corners (before the max with x1 / y1)
};

// GIoULoss (loss.py:585-618) of the decoded prediction p and target t; grad: also the derivative with respect to p's corners
__device__ __forceinline__ Giou giou_loss(const Box& p, const Box& t, bool grad) {
  const float px2 = fmaxf(p.x1, p.x2), py2 = fmaxf(p.y1, p.y2);
  const float pw = px2 - p.x1, ph = py2 - p.y1;
  const float parea = pw * ph;
  const float tarea = (t.x2 - t.x1) * (t.y2 - t.y1);
  const float ix1 = fmaxf(p.x1, t.x1), iy1 = fmaxf(p.y1, t.y1), ix2 = fminf(px2, t.x2), iy2 = fminf(py2, t.y2);
  const bool m = (iy2 > iy1) && (ix2 > ix1);
  const float iw = ix2 - ix1, ih = iy2 - iy1;
  const float inter = m ? iw * ih : 0.f;
  const float ex1 = fminf(p.x1, t.x1), ey1 = fminf(p.y1, t.y1), ex2 = fmaxf(px2, t.x2), ey2 = fmaxf(py2, t.y2);
  const float ew = ex2 - ex1, eh = ey2 - ey1;
  const float earea = ew * eh + 1e-7f;
  const float uni = parea + tarea - inter + 1e-7f;
  const float iou = inter / uni;
  Giou o;
  o.loss = 1.f - (iou - (earea - uni) / earea);
  o.dx1 = o.dy1 = o.dx2 = o.dy2 = 0.f;
  if (grad) {
    // giou = I / U - 1 + U / E; loss = 1 - giou
    const float dI0 = -1.f / uni;
    const float dU = inter / (uni * uni) - 1.f / earea;
    const float dE = uni / (earea * earea);
    const float dI = dI0 - dU;                               // U = P + T - I + eps
    const float dP = dU;
    // corners after the max (x1, y1, px2, py2).  ex1 = min(p.x1, t.x1): to p.x1 where p.x1 < t.x1; ex2 = max(px2, t.x2)
    float gx1 = -dP * ph - dE * eh * sel_gt(t.x1, p.x1), gy1 = -dP * pw - dE * ew * sel_gt(t.y1, p.y1);
    float gx2 = dP * ph + dE * eh * sel_gt(px2, t.x2), gy2 = dP * pw + dE * ew * sel_gt(py2, t.y2);
    if (m) {
      gx1 -= dI * ih * sel_gt(p.x1, t.x1);                   // ix1 = max(p.x1, t.x1)
      gy1 -= dI * iw * sel_gt(p.y1, t.y1);
      gx2 += dI * ih * sel_gt(t.x2, px2);                    // ix2 = min(px2, t.x2): to px2 where px2 < t.x2
      gy2 += dI * iw * sel_gt(t.y2, py2);
    }
    // px2 = max(p.x1, p.x2)
    const float sx = sel_gt(p.x2, p.x1), sy = sel_gt(p.y2, p.y1);
    o.dx1 = gx1 + gx2 * (1.f - sx);
    o.dy1 = gy1 + gy2 * (1.f - sy);
    o.dx2 = gx2 * sx;
    o.dy2 = gy2 * sy;
  }
  return o;
}

// BCEWithLogits of logit z against target w: max(z, 0) - z w + log(1 + exp(-|z|))
__device__ __forceinline__ float bce_logits(float z, float w) { return fmaxf(z, 0.f) - z * w + log1pf(expf(-fabsf(z))); }

// Forward, one level: dense over the level's anchors, masked by labels > 0.  part[(row0 + workgroup) * 3 + {0, 1, 2}] =
// sum w (1 - giou), sum w, sum BCE(ctr, w) over the workgroup's anchors.
__global__ __launch_bounds__(256) void atss_loss_fwd_kernel(const float* __restrict__ reg, const float* __restrict__ ctr,
                                                            const float* __restrict__ anchors, const int* __restrict__ labels,
                                                            const float* __restrict__ tgt, float* __restrict__ part,
                                                            float* __restrict__ w_out, int A, int Al, int off, int row0) {
  __shared__ float red[4][3];
  const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  if (i < Al) {
    const size_t row = (size_t)b * A + off + i;
    float w = 0.f;
    if (labels[row] > 0) {
      const f32x4 an = *reinterpret_cast<const f32x4*>(anchors + (size_t)(off + i) * 4);
      const f32x4 tg = *reinterpret_cast<const f32x4*>(tgt + row * 4);
      const float* r = reg + (size_t)b * 4 * Al + i;
      const Box t = decode(an, tg[0], tg[1], tg[2], tg[3]);
      const Box p = decode(an, r[0], r[Al], r[2 * (size_t)Al], r[3 * (size_t)Al]);
      w = centerness_target(an, t);
      s0 = giou_loss(p, t, false).loss * w;
      s1 = w;
      s2 = bce_logits(ctr[(size_t)b * Al + i], w);
    }
    if (w_out) w_out[row] = w;
  }
  s0 = wave_sum(s0), s1 = wave_sum(s1), s2 = wave_sum(s2);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red[wave][0] = s0, red[wave][1] = s1, red[wave][2] = s2;
  __syncthreads();
  if (threadIdx.x < 3) {
    const int j = threadIdx.x;
    part[((size_t)row0 + (size_t)b * gridDim.x + blockIdx.x) * 3 + j] = (red[0][j] + red[1][j]) + (red[2][j] + red[3][j]);
  }
}

// Backward, one level: d bbox_reg [B, 4, H, W] and d centerness [B, 1, H, W] in place, zeros on unassigned anchors.  g: the upstream
// gradients of (sum w (1 - giou), sum w, sum BCE) in device memory; the targets w carry no gradient.
__global__ __launch_bounds__(256) void atss_loss_bwd_kernel(const float* __restrict__ reg, const float* __restrict__ ctr,
                                                            const float* __restrict__ anchors, const int* __restrict__ labels,
                                                            const float* __restrict__ tgt, const float* __restrict__ g,
                                                            float* __restrict__ dreg, float* __restrict__ dctr, int A, int Al, int off) {
  const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (i >= Al) return;
  const size_t row = (size_t)b * A + off + i;
  float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f, dc = 0.f;
  if (labels[row] > 0) {
    const f32x4 an = *reinterpret_cast<const f32x4*>(anchors + (size_t)(off + i) * 4);
    const f32x4 tg = *reinterpret_cast<const f32x4*>(tgt + row * 4);
    const float* r = reg + (size_t)b * 4 * Al + i;
    const float r2 = r[2 * (size_t)Al], r3 = r[3 * (size_t)Al];
    const Box t = decode(an, tg[0], tg[1], tg[2], tg[3]);
    const Box p = decode(an, r[0], r[Al], r2, r3);
    const float w = centerness_target(an, t);
    const Giou q = giou_loss(p, t, true);
    const float gl = g[0] * w;
    const float aw = an[2] - an[0] + 1.f, ah = an[3] - an[1] + 1.f;
    // x1 = px - pw / 2, x2 = px + pw / 2 - 1; px = r0 / 10 * aw + cx; pw = exp(dw) * aw, dw = min(r2 / 5, CLIP) (clamp passes the gradient at <=)
    d0 = gl * (q.dx1 + q.dx2) * aw / 10.f;
    d1 = gl * (q.dy1 + q.dy2) * ah / 10.f;
    d2 = r2 / 5.f <= CLIP ? gl * 0.5f * (q.dx2 - q.dx1) * p.w / 5.f : 0.f;
    d3 = r3 / 5.f <= CLIP ? gl * 0.5f * (q.dy2 - q.dy1) * p.h / 5.f : 0.f;
    const float z = ctr[(size_t)b * Al + i];
    const float e = expf(-fabsf(z));
    const float sig = (z >= 0.f ? 1.f : e) / (1.f + e);
    dc = g[2] * (sig - w);
  }
  float* o = dreg + (size_t)b * 4 * Al + i;
  o[0] = d0, o[Al] = d1, o[2 * (size_t)Al] = d2, o[3 * (size_t)Al] = d3;
  dctr[(size_t)b * Al + i] = dc;
}

bool levels_from(const int* level_off, int L, int A, int topk, Levels& lv) {
  if (!level_off || L <= 0 || L > ATSS_MAX_LEVELS || topk <= 0) return false;
  lv.n = L;
  lv.slot[0] = 0;
  for (int l = 0; l <= L; ++l) {
    lv.off[l] = level_off[l];
    if (l && (lv.off[l] < lv.off[l - 1])) return false;
    if (l) lv.slot[l] = lv.slot[l - 1] + (lv.off[l] - lv.off[l - 1] < topk ? lv.off[l] - lv.off[l - 1] : topk);
  }
  return lv.off[0] == 0 && lv.off[L] == A;
}

}  // namespace

// Number of candidates per gt, sum_l min(topk, A_l) (level_off: HOST array of L + 1 anchor offsets); -1 for arguments the kernels refuse
extern "C" int fiber_atss_num_candidates(const int* level_off, int L, int topk) {
  Levels lv;
  if (!level_off || L <= 0 || L > ATSS_MAX_LEVELS || !levels_from(level_off, L, level_off[L], topk, lv)) return -1;
  return lv.slot[L] >= 2 && lv.slot[L] <= ATSS_MAX_K ? lv.slot[L] : -1;
}

extern "C" int fiber_atss_candidates_f32(const float* anchors, const int* level_off, int L, const float* gt_boxes, const int* num_gt,
                                         int* cand_idx, float* cand_iou, int B, int Gmax, int A, int topk, hipStream_t stream) {
  Levels lv;
  if (B < 0 || Gmax < 0 || A <= 0 || B > 65535 || Gmax > 65535 || !levels_from(level_off, L, A, topk, lv)) return FIBER_EINVAL;
  if (lv.slot[L] < 2 || lv.slot[L] > ATSS_MAX_K) return FIBER_EINVAL;      // < 2: the reference's unbiased std is NaN
  if (B == 0 || Gmax == 0) return FIBER_OK;
  if (!anchors || !gt_boxes || !num_gt || !cand_idx || !cand_iou) return FIBER_EINVAL;
  if (fiber_misaligned(16, anchors, gt_boxes) || fiber_misaligned(4, num_gt, cand_idx, cand_iou)) return FIBER_EINVAL;
  hipLaunchKernelGGL(atss_candidates_kernel, dim3(L, Gmax, B), dim3(64), 0, stream, anchors, gt_boxes, num_gt, cand_idx, cand_iou, lv, Gmax,
                     lv.slot[L]);
  FIBER_CHECK_LAUNCH();
  return FIBER_OK;
}

extern "C" int fiber_atss_resolve_f32(const float* anchors, const float* gt_boxes, const int* num_gt, const int* cand_idx,
                                      const float* cand_iou, unsigned long long* key, int B, int Gmax, int A, int K, hipStream_t stream) {
  if (B < 0 || Gmax < 0 || A <= 0 || B > 65535 || K < 2 || K > ATSS_MAX_K) return FIBER_EINVAL;
  if (B == 0) return FIBER_OK;
  if (!key || fiber_misaligned(8, key)) return FIBER_EINVAL;
  if (hipMemsetAsync(key, 0, (size_t)B * A * sizeof(unsigned long long), stream) != hipSuccess) return FIBER_ELAUNCH;
  if (Gmax == 0) return FIBER_OK;
  if (!anchors || !gt_boxes || !num_gt || !cand_idx || !cand_iou) return FIBER_EINVAL;
  if (fiber_misaligned(16, anchors, gt_boxes) || fiber_misaligned(4, num_gt, cand_idx, cand_iou)) return FIBER_EINVAL;
  hipLaunchKernelGGL(atss_resolve_kernel, dim3(Gmax, B), dim3(64), 0, stream, anchors, gt_boxes, num_gt, cand_idx, cand_iou, key, Gmax, A, K);
  FIBER_CHECK_LAUNCH();
  return FIBER_OK;
}

extern "C" int fiber_atss_finalize_f32(const float* anchors, const float* gt_boxes, const int* gt_labels, const unsigned char* positive_map,
                                       const unsigned long long* key, int* matched, int* labels, float* reg_targets,
                                       unsigned char* token_targets, int* num_pos, int B, int Gmax, int A, int T, hipStream_t stream) {
  if (T != DT || B < 0 || Gmax < 0 || A <= 0 || B > 65535) return FIBER_EINVAL;
  if (B == 0) return FIBER_OK;
  if (!anchors || !key || !matched || !labels || !reg_targets || !token_targets || !num_pos) return FIBER_EINVAL;
  if (Gmax > 0 && (!gt_boxes || !gt_labels || !positive_map)) return FIBER_EINVAL;
  if (fiber_misaligned(16, anchors, gt_boxes, positive_map, reg_targets, token_targets) || fiber_misaligned(8, key) ||
      fiber_misaligned(4, gt_labels, matched, labels, num_pos))
    return FIBER_EINVAL;
  if (hipMemsetAsync(num_pos, 0, (size_t)B * sizeof(int), stream) != hipSuccess) return FIBER_ELAUNCH;
  hipLaunchKernelGGL(atss_finalize_kernel, dim3(cdiv(A, 16), B), dim3(256), 0, stream, anchors, gt_boxes, gt_labels, positive_map, key, matched,
                     labels, reg_targets, token_targets, num_pos, Gmax, A);
  FIBER_CHECK_LAUNCH();
  return FIBER_OK;
}

// Rows of `part` one level's forward writes
extern "C" int fiber_atss_loss_rows(int B, int A_level) { return B > 0 && A_level > 0 ? B * cdiv(A_level, 256) : 0; }

extern "C" int fiber_atss_loss_fwd_f32(const float* bbox_reg, const float* centerness, const float* anchors, const int* labels,
                                       const float* reg_targets, float* part, float* ctr_targets, int B, int A, int A_level, int offset,
                                       int row0, hipStream_t stream) {
  if (B < 0 || A <= 0 || A_level < 0 || offset < 0 || (long long)offset + A_level > A || row0 < 0 || B > 65535) return FIBER_EINVAL;
  if (B == 0 || A_level == 0) return FIBER_OK;
  if (!bbox_reg || !centerness || !anchors || !labels || !reg_targets || !part) return FIBER_EINVAL;
  if (fiber_misaligned(16, anchors, reg_targets) || fiber_misaligned(4, bbox_reg, centerness, labels, part, ctr_targets)) return FIBER_EINVAL;
  hipLaunchKernelGGL(atss_loss_fwd_kernel, dim3(cdiv(A_level, 256), B), dim3(256), 0, stream, bbox_reg, centerness, anchors, labels,
                     reg_targets, part, ctr_targets, A, A_level, offset, row0);
  FIBER_CHECK_LAUNCH();
  return FIBER_OK;
}

extern "C" int fiber_atss_loss_bwd_f32(const float* bbox_reg, const float* centerness, const float* anchors, const int* labels,
                                       const float* reg_targets, const float* g, float* d_bbox_reg, float* d_centerness, int B, int A,
                                       int A_level, int offset, hipStream_t stream) {
  if (B < 0 || A <= 0 || A_level < 0 || offset < 0 || (long long)offset + A_level > A || B > 65535) return FIBER_EINVAL;
  if (B == 0 || A_level == 0) return FIBER_OK;
  if (!bbox_reg || !centerness || !anchors || !labels || !reg_targets || !g || !d_bbox_reg || !d_centerness) return FIBER_EINVAL;
  if (fiber_misaligned(16, anchors, reg_targets) || fiber_misaligned(4, bbox_reg, centerness, labels, g, d_bbox_reg, d_centerness))
    return FIBER_EINVAL;
  hipLaunchKernelGGL(atss_loss_bwd_kernel, dim3(cdiv(A_level, 256), B), dim3(256), 0, stream, bbox_reg, centerness, anchors, labels,
                     reg_targets, g, d_bbox_reg, d_centerness, A, A_level, offset);
  FIBER_CHECK_LAUNCH();
  return FIBER_OK;
}
