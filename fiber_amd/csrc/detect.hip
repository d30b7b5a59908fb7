// Grounding inference (gfx950): from VLDyHead's outputs to boxes without a host synchronisation.  Replaces, of the fine-grained reference
// (fine_grained/maskrcnn_benchmark/), modeling/rpn/inference.py:620-650 + :741-795 (sigmoid, convert_grounding_to_od_logits[_v2], the
// candidate test, the centerness product), :657-676 + modeling/box_coder.py:52-95 + BoxList.clip_to_image + remove_small_boxes (decode),
// csrc/cuda/ml_nms.cu:15-75 (ml_nms_kernel) and the host loop ml_nms.cu:122-140 with select_over_all_levels (inference.py:717-738).
// The reference's path synchronises per level and image (nonzero, a data-dependent topk, a boolean gather) and walks the N x N/64 mask on
// the CPU; everything here has fixed shapes: padding entries carry score -1 and sink to the end of the per-image sort.
// No atomics anywhere: two runs give the same bits.  IoU and decode are evaluated in the reference's operation order with contraction off.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int DT = 256;                    // tokens (the only supported size)
constexpr int SEL_WORDS = 4;               // removed-bitmap words per lane of the select kernel
constexpr int SEL_MAX_N = 64 * 64 * SEL_WORDS;   // 16384 candidates per image (refcoco: 5 x 3000)
constexpr int SRC_A_BITS = 18, SRC_C_BITS = 10;  // source = level << 28 | a << 10 | c

// the one-exp sigmoid of ground.hip's focal_term: e = exp(-|z|), sigmoid(z) = (z >= 0 ? 1 : e) / (1 + e)
__device__ __forceinline__ float sigmoid1(float z) {
  const float e = __expf(-fabsf(z));
  return (z >= 0.f ? 1.f : e) * __builtin_amdgcn_rcpf(1.f + e);
}

// One wave per anchor: the 256 token probabilities go through LDS, lane c (+64, ...) folds its class's tokens in CSR order.
// Sample b reads the C + 1 offsets at class_ptr + b * ptr_stride (absolute offsets into the one tok_idx); ptr_stride 0 = one map for all.
__global__ __launch_bounds__(256) void det_scores_kernel(const float* __restrict__ logits, const float* __restrict__ ctr,
                                                         const int* __restrict__ class_ptr_all, const int* __restrict__ tok_idx,
                                                         float* __restrict__ out, int A, int C, float thresh, int use_max,
                                                         int ptr_stride) {
  __shared__ __attribute__((aligned(16))) float prob[4][DT];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, b = blockIdx.y;
  const int a = blockIdx.x * 4 + wave;
  if (a >= A) return;                                      // whole wave; no workgroup barrier below
  const int* __restrict__ class_ptr = class_ptr_all + (size_t)b * ptr_stride;
  const size_t row = (size_t)b * A + a;
  const f32x4 z = *reinterpret_cast<const f32x4*>(logits + row * DT + lane * 4);
  f32x4 p;
#pragma unroll
  for (int r = 0; r < 4; ++r) p[r] = sigmoid1(z[r]);
  *reinterpret_cast<f32x4*>(&prob[wave][lane * 4]) = p;
  const float cs = sigmoid1(ctr[row]);
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  for (int c = lane; c < C; c += 64) {
    const int lo = class_ptr[c], hi = class_ptr[c + 1];
    float agg = 0.f;
    if (hi > lo) {
      if (use_max) {
        agg = prob[wave][tok_idx[lo]];
        for (int i = lo + 1; i < hi; ++i) agg = fmaxf(agg, prob[wave][tok_idx[i]]);
      } else {
        for (int i = lo; i < hi; ++i) agg += prob[wave][tok_idx[i]];
        agg = agg / (float)(hi - lo);
      }
    }
    out[row * C + c] = agg > thresh ? agg * cs : -1.f;
  }
}

__global__ __launch_bounds__(256) void det_decode_kernel(const float* __restrict__ val, const long long* __restrict__ idx,
                                                         const float* __restrict__ reg, const float* __restrict__ anchors,
                                                         const float* __restrict__ sizes, float* __restrict__ boxes,
                                                         float* __restrict__ scores, int* __restrict__ labels, int* __restrict__ source,
                                                         int k, int A, int C, int N, int off, int level, float min_size) {
  const int j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (j >= k) return;
  const float v = val[(size_t)b * k + j];
  const long long flat = idx[(size_t)b * k + j];
  const size_t o = (size_t)b * N + off + j;
  f32x4 box = f32x4{0.f, 0.f, 0.f, 0.f};
  float sc = -1.f;
  int lab = 0, src = -1;
  if (v >= 0.f && flat >= 0 && flat < (long long)A * C) {
    const int a = (int)(flat / C), c = (int)(flat - (long long)a * C);
    const f32x4 an = *reinterpret_cast<const f32x4*>(anchors + (size_t)a * 4);
    const float* r = reg + (size_t)b * 4 * A + a;
    const float w = an[2] - an[0] + 1.f, h = an[3] - an[1] + 1.f;
    const float cx = an[0] + 0.5f * w, cy = an[1] + 0.5f * h;
    const float clip = 4.135166556742356f;                 // log(1000 / 16)
    const float dx = r[0] / 10.f, dy = r[A] / 10.f;
    const float dw = fminf(r[2 * (size_t)A] / 5.f, clip), dh = fminf(r[3 * (size_t)A] / 5.f, clip);
    const float px = dx * w + cx, py = dy * h + cy;
    const float pw = expf(dw) * w, ph = expf(dh) * h;
    const float iw = sizes[b * 2] - 1.f, ih = sizes[b * 2 + 1] - 1.f;
    box[0] = fminf(fmaxf(px - 0.5f * pw, 0.f), iw);
    box[1] = fminf(fmaxf(py - 0.5f * ph, 0.f), ih);
    box[2] = fminf(fmaxf(px + 0.5f * pw - 1.f, 0.f), iw);
    box[3] = fminf(fmaxf(py + 0.5f * ph - 1.f, 0.f), ih);
    lab = c + 1;
    src = (level << (SRC_A_BITS + SRC_C_BITS)) | (a << SRC_C_BITS) | c;
    // remove_small_boxes: both sides (with the +1 of the xywh conversion) >= min_size; a NaN side fails the test
    const bool big = (box[2] - box[0] + 1.f >= min_size) && (box[3] - box[1] + 1.f >= min_size);
    sc = big ? sqrtf(v) : -1.f;
  }
  *reinterpret_cast<f32x4*>(boxes + o * 4) = box;
  scores[o] = sc;
  labels[o] = lab;
  source[o] = src;
}

__device__ __forceinline__ float lane_bcast(float v, int l) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}

// One wave64 = rows [64 by, 64 by + 64) x columns [64 bx, 64 bx + 64): lane l holds row box l and column box l; for each row the
// 64 compares are one per lane and the ballot is the row's word.  Word bit j of row i: j > i, same label, IoU > thresh, both live.
__global__ __launch_bounds__(64) void det_nms_mask_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                          const int* __restrict__ labels, unsigned long long* __restrict__ mask, int N,
                                                          float thresh) {
  const int bx = blockIdx.x, by = blockIdx.y, b = blockIdx.z, lane = threadIdx.x;
  if (bx < by) return;                                     // below the diagonal: never read by the select kernel
  const int NB = gridDim.x;
  const int ri = by * 64 + lane, ci = bx * 64 + lane;
  const bool r_in = ri < N, c_in = ci < N;
  const size_t rb = (size_t)b * N + (r_in ? ri : 0), cb = (size_t)b * N + (c_in ? ci : 0);
  const f32x4 rbox = *reinterpret_cast<const f32x4*>(boxes + rb * 4);
  const f32x4 cbox = *reinterpret_cast<const f32x4*>(boxes + cb * 4);
  const int rlab = labels[rb], clab = labels[cb];
  const bool r_ok = r_in && scores[rb] >= 0.f, c_ok = c_in && scores[cb] >= 0.f;
  const float Sb = (cbox[2] - cbox[0] + 1.f) * (cbox[3] - cbox[1] + 1.f);
  const unsigned long long rows_ok = __ballot(r_ok);
  unsigned long long mine = 0ull;
#pragma unroll 8
  for (int r = 0; r < 64; ++r) {
    const float a0 = lane_bcast(rbox[0], r), a1 = lane_bcast(rbox[1], r), a2 = lane_bcast(rbox[2], r), a3 = lane_bcast(rbox[3], r);
    const int al = __builtin_amdgcn_readlane(rlab, r);
    const float left = fmaxf(a0, cbox[0]), right = fminf(a2, cbox[2]);
    const float top = fmaxf(a1, cbox[1]), bottom = fminf(a3, cbox[3]);
    const float width = fmaxf(right - left + 1.f, 0.f), height = fmaxf(bottom - top + 1.f, 0.f);
    const float inter = width * height;
    const float Sa = (a2 - a0 + 1.f) * (a3 - a1 + 1.f);
    const float iou = inter / (Sa + Sb - inter);
    unsigned long long word = __ballot(c_ok && al == clab && iou > thresh);
    if (bx == by) word &= r == 63 ? 0ull : ~0ull << (r + 1);
    if (!((rows_ok >> r) & 1ull)) word = 0ull;
    if (lane == r) mine = word;
  }
  if (r_in) mask[((size_t)b * N + ri) * NB + bx] = mine;
}

__device__ __forceinline__ unsigned long long lane_bcast64(unsigned long long v, int l) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
  return ((unsigned long long)hi << 32) | lo;
}

// One wave per image walks the sorted candidates a block of 64 at a time.  Lane l owns removed-bitmap words l, l + 64, ... in registers.
// A block's 64 diagonal mask words (row i, word i / 64) do not depend on any decision: the next block's are in flight while this block
// is resolved on wave-uniform values.  The rows of the candidates just kept are then OR-ed into the words to the right.
__global__ __launch_bounds__(64) void det_nms_select_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                            const int* __restrict__ labels, const int* __restrict__ source,
                                                            const unsigned long long* __restrict__ mask, float* __restrict__ oboxes,
                                                            float* __restrict__ oscores, int* __restrict__ olabels,
                                                            int* __restrict__ osource, int* __restrict__ ocount, int N, int D) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int NB = (N + 63) >> 6;
  const unsigned long long* M = mask + (size_t)b * N * NB;
  unsigned long long remv[SEL_WORDS];
#pragma unroll
  for (int s = 0; s < SEL_WORDS; ++s) remv[s] = 0ull;
  int count = 0;
  unsigned long long diag_next = lane < N ? M[(size_t)lane * NB] : 0ull;
  for (int nb = 0; nb < NB && count < D; ++nb) {
    const int i = nb * 64 + lane;
    const unsigned long long diag = diag_next;
    {
      const int in = i + 64;
      diag_next = (nb + 1 < NB && in < N) ? M[(size_t)in * NB + nb + 1] : 0ull;
    }
    const float sc = i < N ? scores[(size_t)b * N + i] : -1.f;
    const unsigned long long valid = __ballot(sc >= 0.f);
    if (valid == 0ull) break;                              // sorted: nothing but padding from here on
    unsigned long long own = 0ull;
#pragma unroll
    for (int s = 0; s < SEL_WORDS; ++s) own = (nb >> 6) == s ? remv[s] : own;
    unsigned long long cur = lane_bcast64(own, nb & 63) | ~valid;
    unsigned long long keep = 0ull;
    for (int l = 0; l < 64 && count < D; ++l) {
      if ((cur >> l) & 1ull) continue;
      keep |= 1ull << l;
      ++count;
      cur |= lane_bcast64(diag, l);
    }
    if ((keep >> lane) & 1ull) {
      const int rank = count - __popcll(keep) + __popcll(keep & ((1ull << lane) - 1ull));
      const size_t src = (size_t)b * N + i, dst = (size_t)b * D + rank;
      *reinterpret_cast<f32x4*>(oboxes + dst * 4) = *reinterpret_cast<const f32x4*>(boxes + src * 4);
      oscores[dst] = sc;
      olabels[dst] = labels[src];
      osource[dst] = source[src];
    }
    for (unsigned long long m = keep; m; m &= m - 1ull) {
      const size_t row = (size_t)(nb * 64 + __builtin_ctzll(m)) * NB;
#pragma unroll
      for (int s = 0; s < SEL_WORDS; ++s) {
        const int w = s * 64 + lane;
        if (w > nb && w < NB) remv[s] |= M[row + w];
      }
    }
  }
  for (int d = count + lane; d < D; d += 64) {
    const size_t dst = (size_t)b * D + d;
    *reinterpret_cast<f32x4*>(oboxes + dst * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
    oscores[dst] = -1.f;
    olabels[dst] = 0;
    osource[dst] = -1;
  }
  if (lane == 0) ocount[b] = count;
}

constexpr int MRG_THREADS = 1024;          // 16 waves: the binary searches are LDS-latency bound, more waves hide it
constexpr int MRG_MAX_N = 16384;           // K * D: the image's scores as fp32 fill 64 KB of LDS (LVIS: 31 x 300)
constexpr int MRG_MAX_K = 64;

// how many of the descending list s[0, n) are >= v (strict = false) or > v (strict = true)
__device__ __forceinline__ int merge_count(const float* s, int n, float v, bool strict) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const float m = s[mid];
    if (strict ? m > v : m >= v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// One workgroup per image merges its K descending lists.  Candidate (k, s) ranks at s + #{>= it in every earlier chunk} + #{> it in every
// later chunk}: equal scores go to the earlier chunk, then the earlier slot, the ranks are a permutation of [0, total) and every rank
// < N is one plain store.  rank <= total - 1 whatever the scores hold (each term is bounded by its list's length), so no score pattern,
// NaN and unsorted lists included, writes out of bounds; with such input the ranks may collide and the result is unspecified.
__global__ __launch_bounds__(MRG_THREADS) void det_merge_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                                const int* __restrict__ labels, const int* __restrict__ source,
                                                                const int* __restrict__ count, const int* __restrict__ table,
                                                                float* __restrict__ oboxes, float* __restrict__ oscores,
                                                                int* __restrict__ olabels, int* __restrict__ osource,
                                                                int* __restrict__ ochunk, int* __restrict__ ocount, int K, int D, int Cc,
                                                                int N) {
  extern __shared__ __attribute__((aligned(16))) float sc[];       // [K * D]
  const int b = blockIdx.x, tid = threadIdx.x, KD = K * D;
  const size_t base = (size_t)b * KD;
  const int* __restrict__ cnt = count + (size_t)b * K;
  for (int i = tid; i < KD; i += MRG_THREADS) sc[i] = scores[base + i];
  int total = 0;
  for (int k = 0; k < K; ++k) total += min(max(cnt[k], 0), D);
  __syncthreads();
  for (int i = tid; i < KD; i += MRG_THREADS) {
    const int k = i / D, s = i - k * D;
    if (s >= min(max(cnt[k], 0), D)) continue;              // whatever the slots past count hold is ignored
    const float v = sc[i];
    int rank = s;
    for (int j = 0; j < K; ++j)
      if (j != k) rank += merge_count(sc + j * D, min(max(cnt[j], 0), D), v, j > k);
    if (rank >= N) continue;
    const size_t src = base + i, dst = (size_t)b * N + rank;
    const int local = labels[src];
    *reinterpret_cast<f32x4*>(oboxes + dst * 4) = *reinterpret_cast<const f32x4*>(boxes + src * 4);
    oscores[dst] = v;
    olabels[dst] = (local >= 1 && local <= Cc) ? table[(size_t)k * Cc + local - 1] : 0;
    osource[dst] = source[src];
    ochunk[dst] = k;
  }
  const int kept = min(total, N);
  for (int r = kept + tid; r < N; r += MRG_THREADS) {        // the padding fiber_det_nms_select writes
    const size_t dst = (size_t)b * N + r;
    *reinterpret_cast<f32x4*>(oboxes + dst * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
    oscores[dst] = -1.f;
    olabels[dst] = 0;
    osource[dst] = -1;
    ochunk[dst] = -1;
  }
  if (tid == 0) ocount[b] = kept;
}

// ---- multi-scale test-time augmentation (data/datasets/evaluation/box_aug.py) -----------------------------------------------------------
constexpr int AUG_THREADS = 256;
constexpr int AUG_MAX_T = 1 << 20;         // candidates per image over all views (24 views x SEL_MAX_N = 393216 fit)
constexpr int AUG_DEAD_LABEL = 1 << 30;    // the label dead slots are sorted under: behind every class

struct AugView {                           // one record per image and view (32 bytes)
  float scaled_w;                          // width of the resized image (the frame the candidates are in)
  float ratio_w, ratio_h;                  // original / resized, computed in double, rounded to fp32
  int equal_ratio;                         // BoxList.resize's first branch: ratio_w on all four coordinates
  int flip;
  int has_range;
  float min2, max2;                        // the squares of TEST.RANGES' pair
};

// first index of the ascending list l[0, n) that is >= v
__device__ __forceinline__ int aug_lower_bound(const int* __restrict__ l, int n, int v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (l[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// is `label` in the ascending table?
__device__ __forceinline__ bool aug_allowed(const int* __restrict__ classes, int C, int label) {
  const int at = aug_lower_bound(classes, C, label);
  return at < C && classes[at] == label;
}

// One thread per candidate of one view: un-flip in the scaled frame (BoxList.transpose), remove_boxes' strict area test there, then
// BoxList.resize to the original frame; every slot [off, off + Nv) of the image's concatenated buffers is written.
__global__ __launch_bounds__(AUG_THREADS) void det_aug_collect_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                                      const int* __restrict__ labels, const int* __restrict__ source,
                                                                      const AugView* __restrict__ table, const int* __restrict__ classes,
                                                                      float* __restrict__ oboxes, float* __restrict__ oscores,
                                                                      int* __restrict__ olabels, int* __restrict__ osource,
                                                                      int* __restrict__ oview, int Nv, int T, int off, int view, int C) {
  const int n = blockIdx.x * AUG_THREADS + threadIdx.x, b = blockIdx.y;
  if (n >= Nv) return;
  const size_t src = (size_t)b * Nv + n, dst = (size_t)b * T + off + n;
  const AugView p = table[b];
  f32x4 box = *reinterpret_cast<const f32x4*>(boxes + src * 4);
  const float sc = scores[src];
  const int lab = labels[src];
  bool live = sc >= 0.f && aug_allowed(classes, C, lab);
  if (p.flip) {
    const float x1 = p.scaled_w - box[2] - 1.f, x2 = p.scaled_w - box[0] - 1.f;
    box[0] = x1;
    box[2] = x2;
  }
  if (p.has_range) {
    const float w = box[2] - box[0] + 1.f, h = box[3] - box[1] + 1.f;
    const float area = w * h;
    live = live && area > p.min2 && area < p.max2;
  }
  const float ry = p.equal_ratio ? p.ratio_w : p.ratio_h;
  box[0] = box[0] * p.ratio_w;
  box[1] = box[1] * ry;
  box[2] = box[2] * p.ratio_w;
  box[3] = box[3] * ry;
  *reinterpret_cast<f32x4*>(oboxes + dst * 4) = live ? box : f32x4{0.f, 0.f, 0.f, 0.f};
  oscores[dst] = live ? sc : -1.f;
  olabels[dst] = live ? lab : 0;
  osource[dst] = live ? source[src] : -1;
  oview[dst] = live ? view : -1;
}

// One workgroup per (class-table entry, image) over candidates sorted by (label ascending, score descending, slot ascending), dead slots
// under AUG_DEAD_LABEL.  The leader is the first undecided slot of the segment; every thread strides over the slots from the leader on
// and decides the undecided ones against the leader alone: mode 0 (greedy NMS, nms.cu) marks IoU > thresh suppressed; mode 1 (bbox_vote)
// takes IoU >= thresh, the leader included, into the cluster and sums score * box and score.  The same pass finds the next leader as the
// smallest slot left undecided, so the loop runs once per kept box or cluster, not once per slot.  state: 0 undecided (as it arrives),
// 1 kept, 2 gone; slot i is read and written by thread (i - lo) % AUG_THREADS only.  The sums go lane tree -> wave 0..3 in that order:
// two runs give the same bits.  lo <= hi <= T whatever the labels hold, and every index used lies in [lo, hi).
__global__ __launch_bounds__(AUG_THREADS) void det_aug_merge_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                                    const int* __restrict__ labels, const int* __restrict__ classes,
                                                                    int* __restrict__ state, float* __restrict__ oboxes, int T,
                                                                    float thresh, int mode) {
  __shared__ float red[AUG_THREADS / 64][5];
  __shared__ int red_next[AUG_THREADS / 64], red_n[AUG_THREADS / 64];
  const int b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const size_t base = (size_t)b * T;
  const int* __restrict__ lab = labels + base;
  const int label = classes[blockIdx.x];
  if (label < 0 || label >= AUG_DEAD_LABEL) return;
  const int lo = aug_lower_bound(lab, T, label);
  const int hi = lo + aug_lower_bound(lab + lo, T - lo, label + 1);
  if (hi <= lo) return;                                    // whole workgroup: no barrier has been reached
  const float* __restrict__ bx = boxes + base * 4;
  const float* __restrict__ sc = scores + base;
  int* __restrict__ st = state + base;
  float* __restrict__ ob = oboxes + base * 4;
  int leader = lo;
  while (leader < hi) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(bx + (size_t)leader * 4);
    const float Sa = (a[2] - a[0] + 1.f) * (a[3] - a[1] + 1.f);
    float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    int next = hi, members = 0;
    // the first slot >= leader that this thread owns
    int i = leader + ((tid - (leader - lo)) % AUG_THREADS + AUG_THREADS) % AUG_THREADS;
    for (; i < hi; i += AUG_THREADS) {
      if (i != leader && st[i] != 0) continue;
      const f32x4 c = *reinterpret_cast<const f32x4*>(bx + (size_t)i * 4);
      const float left = fmaxf(a[0], c[0]), right = fminf(a[2], c[2]);
      const float top = fmaxf(a[1], c[1]), bottom = fminf(a[3], c[3]);
      const float width = fmaxf(right - left + 1.f, 0.f), height = fmaxf(bottom - top + 1.f, 0.f);
      const float inter = width * height;
      const float Sb = (c[2] - c[0] + 1.f) * (c[3] - c[1] + 1.f);
      const float iou = inter / (Sa + Sb - inter);
      const bool hit = i == leader || (mode ? iou >= thresh : iou > thresh);
      if (hit) {
        st[i] = i == leader ? 1 : 2;
        if (mode) {
          const float s = sc[i];
          acc[0] += c[0] * s;
          acc[1] += c[1] * s;
          acc[2] += c[2] * s;
          acc[3] += c[3] * s;
          acc[4] += s;
          ++members;
        }
      } else {
        next = min(next, i);
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      next = min(next, __shfl_xor(next, o));
      if (mode) {
        members += __shfl_xor(members, o);
#pragma unroll
        for (int r = 0; r < 5; ++r) acc[r] += __shfl_xor(acc[r], o);
      }
    }
    if (lane == 0) {
      red_next[wave] = next;
      red_n[wave] = members;
#pragma unroll
      for (int r = 0; r < 5; ++r) red[wave][r] = acc[r];
    }
    __syncthreads();
    next = red_next[0];
    members = red_n[0];
#pragma unroll
    for (int r = 0; r < 5; ++r) acc[r] = red[0][r];
#pragma unroll
    for (int w = 1; w < AUG_THREADS / 64; ++w) {
      next = min(next, red_next[w]);
      members += red_n[w];
#pragma unroll
      for (int r = 0; r < 5; ++r) acc[r] += red[w][r];
    }
    if (tid == 0) {
      f32x4 out = a;
      if (mode && members > 1) out = f32x4{acc[0] / acc[4], acc[1] / acc[4], acc[2] / acc[4], acc[3] / acc[4]};
      *reinterpret_cast<f32x4*>(ob + (size_t)leader * 4) = out;
    }
    __syncthreads();                                       // red is rewritten by the next round
    leader = next;                                         // > the old leader: every round decides its leader
  }
}

}  // namespace

// Largest T (candidates per image over all views) of fiber_det_aug_collect / fiber_det_aug_merge
extern "C" int fiber_det_aug_max_candidates(void) { return AUG_MAX_T; }

extern "C" int fiber_det_aug_collect(const float* boxes, const float* scores, const int* labels, const int* source, const void* table,
                                     const int* classes, float* out_boxes, float* out_scores, int* out_labels, int* out_source,
                                     int* out_view, int B, int Nv, int T, int offset, int view, int C, hipStream_t stream) {
  static_assert(sizeof(AugView) == 32, "the host packs 32-byte records");
  if (B < 0 || Nv < 0 || T < 0 || T > AUG_MAX_T || offset < 0 || (long long)offset + Nv > T || view < 0 || C < 0 || B > 65535)
    return FIBER_EINVAL;
  if (B == 0 || Nv == 0) return FIBER_OK;
  if (!boxes || !scores || !labels || !source || !table || (C > 0 && !classes) || !out_boxes || !out_scores || !out_labels ||
      !out_source || !out_view)
    return FIBER_EINVAL;
  if (fiber_misaligned(16, boxes, out_boxes) ||
      fiber_misaligned(4, scores, labels, source, table, classes, out_scores, out_labels, out_source, out_view))
    return FIBER_EINVAL;
  hipLaunchKernelGGL(det_aug_collect_kernel, dim3(cdiv(Nv, AUG_THREADS), B), dim3(AUG_THREADS), 0, stream, boxes, scores, labels, source,
                     static_cast<const AugView*>(table), classes, out_boxes, out_scores, out_labels, out_source, out_view, Nv, T, offset,
                     view, C);
  FIBER_CHECK_LAUNCH();
  return FIBER_OK;
}

extern "C" int fiber_det_aug_merge(const float* boxes, const float* scores, const int* labels, const int* classes, int* state,
                                   float* out_boxes, int B, int T, int C, float thresh, int mode, hipStream_t stream) {
  if (B < 0 || T < 0 || T > AUG_MAX_T || C < 0 || B > 65535 || (mode != 0 && mode != 1) || !(thresh > 0.f)) return FIBER_EINVAL;
  if (B == 0 || T == 0 || C == 0) return FIBER_OK;
  if (!boxes || !scores || !labels || !classes || !state || !out_boxes) return FIBER_EINVAL;
  if (fiber_misaligned(16, boxes, out_boxes) || fiber_misaligned(4, scores, labels, classes, state)) return FIBER_EINVAL;
  hipLaunchKernelGGL(det_aug_merge_kernel, dim3(C, B), dim3(AUG_THREADS), 0, stream, boxes, scores, labels, classes, state, out_boxes, T,
                     thresh, mode);
  FIBER_CHECK_LAUNCH();
  return FIBER_OK;
}

// Largest K * D (candidates per image over all chunks) the merge kernel stages in LDS
extern "C" int fiber_det_merge_max_candidates(void) { return MRG_MAX_N; }

extern "C" int fiber_det_merge(const float* boxes, const float* scores, const int* labels, const int* source, const int* count,
                               const int* label_table, float* out_boxes, float* out_scores, int* out_labels, int* out_source,
                               int* out_chunk, int* out_count, int B, int K, int D, int Cc, int N, hipStream_t stream) {
  if (B < 0 || K < 0 || D < 0 || Cc < 0 || N < 0 || K > MRG_MAX_K || (long long)K * D > MRG_MAX_N || N > K * D) return FIBER_EINVAL;
  if (B == 0 || K * D == 0) return FIBER_OK;
  if (N == 0) return FIBER_EINVAL;
  if (!boxes || !scores || !labels || !source || !count || (Cc > 0 && !label_table) || !out_boxes || !out_scores || !out_labels ||
      !out_source || !out_chunk || !out_count)
    return FIBER_EINVAL;
  if (fiber_misaligned(16, boxes, out_boxes) ||
      fiber_misaligned(4, scores, labels, source, count, label_table, out_scores, out_labels, out_source, out_chunk, out_count))
    return FIBER_EINVAL;
  hipLaunchKernelGGL(det_merge_kernel, dim3(B), dim3(MRG_THREADS), (size_t)K * D * sizeof(float), stream, boxes, scores, labels, source,
                     count, label_table, out_boxes, out_scores, out_labels, out_source, out_chunk, out_count, K, D, Cc, N);
  FIBER_CHECK_LAUNCH();
  return FIBER_OK;
}

// Largest N (candidates per image after the per-level top-k) the select kernel's register bitmap holds
extern "C" int fiber_det_max_candidates(void) { return SEL_MAX_N; }

// ptr_stride: elements between the class_ptr rows of consecutive samples (per-sample positive maps: phrase grounding, referring
// expressions); 0 = every sample reads the same C + 1 offsets.
extern "C" int fiber_det_scores_rows_f32(const float* logits, const float* centerness, const int* class_ptr, const int* tok_idx,
                                         float* out, int B, int A, int T, int C, float pre_nms_thresh, int agg_max, int ptr_stride,
                                         hipStream_t stream) {
  if (T != DT || C <= 0 || B < 0 || A < 0) return FIBER_EINVAL;
  if (ptr_stride != 0 && ptr_stride < C + 1) return FIBER_EINVAL;
  if (B == 0 || A == 0) return FIBER_OK;
  if (!logits || !centerness || !class_ptr || !tok_idx || !out) return FIBER_EINVAL;
  if (fiber_misaligned(16, logits) || fiber_misaligned(4, centerness, class_ptr, tok_idx, out)) return FIBER_EINVAL;
  hipLaunchKernelGGL(det_scores_kernel, dim3(cdiv(A, 4), B), dim3(256), 0, stream, logits, centerness, class_ptr, tok_idx, out, A, C,
                     pre_nms_thresh, agg_max, ptr_stride);
  FIBER_CHECK_LAUNCH();
  return FIBER_OK;
}

extern "C" int fiber_det_scores_f32(const float* logits, const float* centerness, const int* class_ptr, const int* tok_idx, float* out,
                                    int B, int A, int T, int C, float pre_nms_thresh, int agg_max, hipStream_t stream) {
  return fiber_det_scores_rows_f32(logits, centerness, class_ptr, tok_idx, out, B, A, T, C, pre_nms_thresh, agg_max, 0, stream);
}

extern "C" int fiber_det_decode_f32(const float* topk_val, const long long* topk_idx, const float* bbox_reg, const float* anchors,
                                    const float* image_sizes, float* boxes, float* scores, int* labels, int* source, int B, int k, int A,
                                    int C, int N, int offset, int level, float min_size, hipStream_t stream) {
  if (C <= 0 || C > (1 << SRC_C_BITS) || A < 0 || A > (1 << SRC_A_BITS) || level < 0 || level >= 8 || B < 0 || k < 0 || N < 0 ||
      offset < 0 || (long long)offset + k > N)
    return FIBER_EINVAL;
  if (B == 0 || k == 0) return FIBER_OK;
  if (!topk_val || !topk_idx || !bbox_reg || !anchors || !image_sizes || !boxes || !scores || !labels || !source) return FIBER_EINVAL;
  if (fiber_misaligned(16, anchors, boxes) || fiber_misaligned(8, topk_idx) ||
      fiber_misaligned(4, topk_val, bbox_reg, image_sizes, scores, labels, source))
    return FIBER_EINVAL;
  hipLaunchKernelGGL(det_decode_kernel, dim3(cdiv(k, 256), B), dim3(256), 0, stream, topk_val, topk_idx, bbox_reg, anchors, image_sizes,
                     boxes, scores, labels, source, k, A, C, N, offset, level, min_size);
  FIBER_CHECK_LAUNCH();
  return FIBER_OK;
}

extern "C" int fiber_det_nms_mask(const float* boxes, const float* scores, const int* labels, unsigned long long* mask, int B, int N,
                                  float nms_thresh, hipStream_t stream) {
  if (B < 0 || N < 0 || N > SEL_MAX_N || B > 65535) return FIBER_EINVAL;
  if (B == 0 || N == 0) return FIBER_OK;
  if (!boxes || !scores || !labels || !mask) return FIBER_EINVAL;
  if (fiber_misaligned(16, boxes) || fiber_misaligned(8, mask) || fiber_misaligned(4, scores, labels)) return FIBER_EINVAL;
  const int NB = cdiv(N, 64);
  hipLaunchKernelGGL(det_nms_mask_kernel, dim3(NB, NB, B), dim3(64), 0, stream, boxes, scores, labels, mask, N, nms_thresh);
  FIBER_CHECK_LAUNCH();
  return FIBER_OK;
}

extern "C" int fiber_det_nms_select(const float* boxes, const float* scores, const int* labels, const int* source,
                                    const unsigned long long* mask, float* out_boxes, float* out_scores, int* out_labels,
                                    int* out_source, int* out_count, int B, int N, int D, hipStream_t stream) {
  if (B < 0 || N < 0 || N > SEL_MAX_N || D <= 0) return FIBER_EINVAL;
  if (B == 0 || N == 0) return FIBER_OK;
  if (!boxes || !scores || !labels || !source || !mask || !out_boxes || !out_scores || !out_labels || !out_source || !out_count)
    return FIBER_EINVAL;
  if (fiber_misaligned(16, boxes, out_boxes) || fiber_misaligned(8, mask) ||
      fiber_misaligned(4, scores, labels, source, out_scores, out_labels, out_source, out_count))
    return FIBER_EINVAL;
  hipLaunchKernelGGL(det_nms_select_kernel, dim3(B), dim3(64), 0, stream, boxes, scores, labels, source, mask, out_boxes, out_scores,
                     out_labels, out_source, out_count, N, D);
  FIBER_CHECK_LAUNCH();
  return FIBER_OK;
}
