// Box average precision by the LVIS protocol (gfx950): greedy matching of fixed-shape Detections against packed ground truth per batch, and
// the precision / recall tables of every category in one launch, without a host round trip.
// Replaces, of the fine-grained reference (fine_grained/maskrcnn_benchmark/data/datasets/evaluation/lvis/lvis_eval.py), :137-148
// (LVISResults.limit_dets_per_image), :237-241 (the federated filter of _prepare), :293-317 (compute_iou), :319-411 (evaluate_img) and
// :413-524 (accumulate).  The reference walks images x categories x area ranges x IoU thresholds in Python on the host.
// Matching: one wave per (image, area range, threshold).  The detections are walked in their stored descending-score order; the lanes take
// the ground truths of the detection's category, a wave-wide maximum over the key (non-ignored, IoU, index) picks the winner, and the
// matched set lives as one bit per (lane, chunk of 64) in a register.  The per-slot words are OR-ed and num_gt is added with integer
// atomics: order-independent, so two runs give the same bits.
// Accumulation: one wave per (category, area range, threshold) over chunks of 64 records.  The cumulative true / false positive counts are
// ballots + popcounts carried as integers; the chunks are walked from the last to the first so that the running maximum of the precision
// from the right is one carried double; the record at which the recall first reaches a threshold writes that threshold's precision.
// fp64 throughout, contraction off, no fast-math: every division is the correctly rounded one.
// The COCO protocol (pycocotools' COCOeval for boxes, which the reference calls at evaluation/coco/coco_eval.py:366-386) shares the walk,
// the key and the accumulation; its matching kernel differs in the crowd rule and in a cap per (image, category): ap_match_coco_kernel.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int AP_MAX_GT = 4096;                            // 64 lanes x the 64 bits of a lane's matched word
constexpr int AP_CHUNK = 64;
constexpr int AP_ACC_WAVES = 4;
constexpr int AP_COCO_MAX_CAT = 4096;                      // one int of dynamic LDS per category: at most 16 KiB for the one wave of a workgroup
typedef unsigned long long u64;

// (non-ignored, IoU, index) of lane `o` against this lane's: the larger key stays.  ni < 0: no candidate.
__device__ __forceinline__ void key_max(int& ni, double& iou, int& g, int oni, double oiou, int og) {
  const bool take = oni > ni || (oni == ni && (oiou > iou || (oiou == iou && og > g)));
  if (take) {
    ni = oni;
    iou = oiou;
    g = og;
  }
}

__global__ __launch_bounds__(64) void ap_match_kernel(const float* __restrict__ boxes, const int* __restrict__ labels, const int* __restrict__ count,
                                                      const double* __restrict__ gt, const double* __restrict__ gt_area,
                                                      const int* __restrict__ gt_cat, const unsigned char* __restrict__ gt_ignore,
                                                      const int* __restrict__ gt_count, const u64* __restrict__ neg, const u64* __restrict__ nel,
                                                      const double* __restrict__ iou_thrs, const double* __restrict__ area_rng,
                                                      u64* __restrict__ match, u64* __restrict__ ignore, unsigned char* __restrict__ valid,
                                                      u64* __restrict__ num_gt, int D, int G, int C, int W, int T, int A, int max_dets) {
  const int lane = threadIdx.x;
  const int p = blockIdx.x;                                // (b * A + a) * T + t
  const int t = p % T, a = (p / T) % A, b = p / (T * A);
  int n = min(max(count[b], 0), D);
  if (max_dets >= 0) n = min(n, max_dets);                 // :137-148: the stored order is descending score
  const int gc = min(max(gt_count[b], 0), G);
  const int nchunk = (gc + 63) >> 6;
  const double lo = area_rng[2 * a], hi = area_rng[2 * a + 1];
  const double thr = fmin(iou_thrs[t], 1.0 - 1e-10);       // :360
  const u64 bit = 1ull << (a * T + t);
  const bool first = a == 0 && t == 0;
  const double* g4 = gt + (size_t)b * G * 4;
  const double* ga = gt_area + (size_t)b * G;
  const int* gcat = gt_cat + (size_t)b * G;
  const unsigned char* gig = gt_ignore + (size_t)b * G;

  if (t == 0) {                                            // :467, per (category, area range)
    for (int g = lane; g < gc; g += 64) {
      const int c = gcat[g];
      const bool ig = gig[g] != 0 || ga[g] < lo || ga[g] > hi;
      if ((unsigned)c < (unsigned)C && !ig) atomicAdd(&num_gt[(size_t)c * A + a], 1ull);
    }
  }

  u64 taken = 0;                                           // bit j: ground truth j * 64 + lane is matched at this (a, t)
  for (int d = 0; d < D; ++d) {
    const size_t slot = (size_t)b * D + d;
    if (d >= n) {                                          // match / ignore were zeroed before the launch
      if (first && lane == 0) valid[slot] = 0;
      continue;
    }
    const int c = labels[slot] - 1;
    const bool known = (unsigned)c < (unsigned)C;
    const bool in_neg = known && ((neg[(size_t)b * W + (c >> 6)] >> (c & 63)) & 1ull);
    const bool in_nel = known && ((nel[(size_t)b * W + (c >> 6)] >> (c & 63)) & 1ull);
    const f32x4 bx = *reinterpret_cast<const f32x4*>(boxes + slot * 4);
    const float wf = bx[2] - bx[0], hf = bx[3] - bx[1];    // convert_to_xywh subtracts in fp32 (:985-987)
    const double dx = (double)bx[0], dy = (double)bx[1], dw = (double)wf, dh = (double)hf;
    const double da = dw * dh;                             // :113
    int ni = -1, bg = -1;
    double biou = 0.0;
    bool present = false;
    for (int j = 0; j < nchunk; ++j) {
      const int g = (j << 6) + lane;
      if (!known || g >= gc || gcat[g] != c) continue;
      present = true;
      if ((taken >> j) & 1ull) continue;                   // :366
      const double gx = g4[g * 4], gy = g4[g * 4 + 1], gw = g4[g * 4 + 2], gh = g4[g * 4 + 3];
      const double iw = fmax(fmin(dx + dw, gx + gw) - fmax(dx, gx), 0.0);
      const double ih = fmax(fmin(dy + dh, gy + gh) - fmax(dy, gy), 0.0);
      const double inter = iw * ih;
      const double iou = inter / (da + gw * gh - inter);
      if (!(iou >= thr)) continue;                         // :372
      const bool ig = gig[g] != 0 || ga[g] < lo || ga[g] > hi;      // :328
      key_max(ni, biou, bg, ig ? 0 : 1, iou, g);
    }
    const bool listed = __ballot(present) != 0ull;
    if (__ballot(ni >= 0) != 0ull) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const int oni = __shfl_xor(ni, o, 64), og = __shfl_xor(bg, o, 64);
        const double oiou = __shfl_xor(biou, o, 64);
        key_max(ni, biou, bg, oni, oiou, og);
      }
      if (lane == (bg & 63)) taken |= 1ull << (bg >> 6);   // :387
    }
    const bool v = known && (listed || in_neg);            // :239
    if (lane == 0) {
      if (v) {
        const bool m = ni >= 0;
        const bool ig = m ? ni == 0 : (da < lo || da > hi || in_nel);      // :384, :391-398
        if (m) atomicOr(&match[slot], bit);
        if (ig) atomicOr(&ignore[slot], bit);
      }
      if (first) valid[slot] = v ? 1 : 0;
    }
  }
}

// COCOeval.evaluateImg for boxes: the LVIS kernel's walk with the COCO API's crowd rule and its cap per (image, category).  A crowd ground
// truth divides by the detection's area, is never consumed (no bit in `taken`) and counts as ignored; a detection whose rank within its
// category reaches `cap` is skipped by every wave.  The rank counters live in LDS, one per category: the counter of category c is read and
// advanced by lane c & 63 alone and broadcast, so no two lanes ever touch one address and the single wave needs no barrier after the
// zeroing.  Every branch around the shuffles is wave-uniform (d, n and the label are).
__global__ __launch_bounds__(64) void ap_match_coco_kernel(const float* __restrict__ boxes, const int* __restrict__ labels,
                                                           const int* __restrict__ count, const double* __restrict__ gt,
                                                           const double* __restrict__ gt_area, const int* __restrict__ gt_cat,
                                                           const unsigned char* __restrict__ gt_crowd, const int* __restrict__ gt_count,
                                                           const double* __restrict__ iou_thrs, const double* __restrict__ area_rng,
                                                           u64* __restrict__ match, u64* __restrict__ ignore, int* __restrict__ rank,
                                                           unsigned char* __restrict__ valid, u64* __restrict__ num_gt, int D, int G, int C,
                                                           int T, int A, int cap, int plus_one) {
  extern __shared__ int seen[];                            // C ints: the detections of each category met so far in this image
  const int lane = threadIdx.x;
  const int p = blockIdx.x;                                // (b * A + a) * T + t
  const int t = p % T, a = (p / T) % A, b = p / (T * A);
  const int n = min(max(count[b], 0), D);
  const int gc = min(max(gt_count[b], 0), G);
  const int nchunk = (gc + 63) >> 6;
  const double lo = area_rng[2 * a], hi = area_rng[2 * a + 1];
  const double thr = fmin(iou_thrs[t], 1.0 - 1e-10);
  const u64 bit = 1ull << (a * T + t);
  const bool first = a == 0 && t == 0;
  const double* g4 = gt + (size_t)b * G * 4;
  const double* ga = gt_area + (size_t)b * G;
  const int* gcat = gt_cat + (size_t)b * G;
  const unsigned char* gcr = gt_crowd + (size_t)b * G;
  for (int i = lane; i < C; i += 64) seen[i] = 0;          // C <= AP_COCO_MAX_CAT; index i belongs to lane i & 63
  __syncthreads();

  if (t == 0) {                                            // per (category, area range)
    for (int g = lane; g < gc; g += 64) {
      const int c = gcat[g];
      const bool ig = gcr[g] != 0 || ga[g] < lo || ga[g] > hi;
      if ((unsigned)c < (unsigned)C && !ig) atomicAdd(&num_gt[(size_t)c * A + a], 1ull);
    }
  }

  u64 taken = 0;                                           // bit j: ground truth j * 64 + lane is matched at this (a, t); never a crowd one
  for (int d = 0; d < D; ++d) {
    const size_t slot = (size_t)b * D + d;
    if (d >= n) {                                          // match / ignore were zeroed before the launch
      if (first && lane == 0) {
        rank[slot] = -1;
        valid[slot] = 0;
      }
      continue;
    }
    const int c = labels[slot] - 1;
    const bool known = (unsigned)c < (unsigned)C;
    int r = -1;
    if (known) {
      int mine = 0;
      if (lane == (c & 63)) {
        mine = seen[c];
        seen[c] = mine + 1;
      }
      r = __shfl(mine, c & 63, 64);
    }
    const bool v = known && r < cap;                       // only the first maxDets[-1] of an (image, category) exist
    if (first && lane == 0) {
      rank[slot] = r;
      valid[slot] = v ? 1 : 0;
    }
    if (!v) continue;
    const f32x4 bx = *reinterpret_cast<const f32x4*>(boxes + slot * 4);
    float wf = bx[2] - bx[0], hf = bx[3] - bx[1];
    if (plus_one) {                                        // BoxList.convert("xywh"): + TO_REMOVE, a second fp32 rounding
      wf = wf + 1.0f;
      hf = hf + 1.0f;
    }
    const double dx = (double)bx[0], dy = (double)bx[1], dw = (double)wf, dh = (double)hf;
    const double da = dw * dh;
    int ni = -1, bg = -1;
    double biou = 0.0;
    for (int j = 0; j < nchunk; ++j) {
      const int g = (j << 6) + lane;
      if (g >= gc || gcat[g] != c) continue;
      const bool crowd = gcr[g] != 0;
      if (!crowd && ((taken >> j) & 1ull)) continue;       // a crowd region can be matched again
      const double gx = g4[g * 4], gy = g4[g * 4 + 1], gw = g4[g * 4 + 2], gh = g4[g * 4 + 3];
      const double iw = fmin(dx + dw, gx + gw) - fmax(dx, gx);
      const double ih = fmin(dy + dh, gy + gh) - fmax(dy, gy);
      const double inter = (iw <= 0.0 || ih <= 0.0) ? 0.0 : iw * ih;
      const double iou = crowd ? inter / da : inter / (da + gw * gh - inter);
      if (!(iou >= thr)) continue;                         // also a NaN from a detection of no area
      const bool ig = crowd || ga[g] < lo || ga[g] > hi;
      key_max(ni, biou, bg, ig ? 0 : 1, iou, g);
    }
    if (__ballot(ni >= 0) != 0ull) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const int oni = __shfl_xor(ni, o, 64), og = __shfl_xor(bg, o, 64);
        const double oiou = __shfl_xor(biou, o, 64);
        key_max(ni, biou, bg, oni, oiou, og);
      }
      if (lane == (bg & 63) && gcr[bg] == 0) taken |= 1ull << (bg >> 6);
    }
    if (lane == 0) {
      const bool m = ni >= 0;
      const bool ig = m ? ni == 0 : (da < lo || da > hi);
      if (m) atomicOr(&match[slot], bit);
      if (ig) atomicOr(&ignore[slot], bit);
    }
  }
}

// number of rec_thrs <= x (rec_thrs ascending)
__device__ __forceinline__ int thrs_le(const double* __restrict__ rec_thrs, int R, double x) {
  int lo = 0, hi = R;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (rec_thrs[mid] <= x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(64 * AP_ACC_WAVES) void ap_accumulate_kernel(const u64* __restrict__ match, const u64* __restrict__ ignore,
                                                                          const long long* __restrict__ seg_ptr,
                                                                          const long long* __restrict__ num_gt,
                                                                          const double* __restrict__ rec_thrs, double* __restrict__ precision,
                                                                          double* __restrict__ recall, long long N, int C, int T, int A, int R,
                                                                          long long problems) {
  const int lane = threadIdx.x & 63;
  const long long p = (long long)blockIdx.x * AP_ACC_WAVES + (threadIdx.x >> 6);      // (c * A + a) * T + t
  if (p >= problems) return;
  const int t = (int)(p % T), a = (int)((p / T) % A), c = (int)(p / ((long long)T * A));
  const size_t ca = (size_t)c * A + a;
  const long long ng = num_gt[ca];
  double* prec = precision + ((size_t)t * R * C + c) * A + a;        // + r * C * A
  const size_t rstride = (size_t)C * A;
  double* rec = recall + ((size_t)t * C + c) * A + a;
  if (ng <= 0) {                                           // :469: both stay -1
    for (int r = lane; r < R; r += 64) prec[r * rstride] = -1.0;
    if (lane == 0) *rec = -1.0;
    return;
  }
  const long long s0 = min(max(seg_ptr[c], 0LL), N), s1 = min(max(seg_ptr[c + 1], s0), N);
  const long long n = s1 - s0;
  const int sh = a * T + t;
  const double dng = (double)ng;
  const u64 le = lane == 63 ? ~0ull : (1ull << (lane + 1)) - 1ull;
  long long tp_total = 0, fp_total = 0;                    // forward: the totals; the chunks are then walked back from them
  for (long long base = 0; base < n; base += AP_CHUNK) {
    const long long i = base + lane;
    bool m = false, ig = true;
    if (i < n) {
      m = (match[s0 + i] >> sh) & 1ull;
      ig = (ignore[s0 + i] >> sh) & 1ull;
    }
    tp_total += __popcll(__ballot(m && !ig));
    fp_total += __popcll(__ballot(!m && !ig));
  }
  const double rc_last = (double)tp_total / dng;           // :488
  if (lane == 0) *rec = n > 0 ? rc_last : 0.0;             // :489-492
  const int reached = n > 0 ? thrs_le(rec_thrs, R, rc_last) : 0;
  for (int r = reached + lane; r < R; r += 64) prec[r * rstride] = 0.0;       // :508-514: no record reaches these
  if (n == 0) return;
  long long tp_end = tp_total, fp_end = fp_total;
  double carry = -1.0;                                     // below every precision
  for (long long base = ((n - 1) / AP_CHUNK) * AP_CHUNK; base >= 0; base -= AP_CHUNK) {
    const long long i = base + lane;
    const bool in = i < n;
    bool m = false, ig = true;
    if (in) {
      m = (match[s0 + i] >> sh) & 1ull;
      ig = (ignore[s0 + i] >> sh) & 1ull;
    }
    const bool tp = m && !ig, fp = !m && !ig;              // :472-473
    const u64 wt = __ballot(tp), wf = __ballot(fp);
    const long long tp0 = tp_end - __popcll(wt), fp0 = fp_end - __popcll(wf);
    const long long tpi = tp0 + __popcll(wt & le), fpi = fp0 + __popcll(wf & le);      // :475-476, inclusive
    const double dtp = (double)tpi, dfp = (double)fpi;
    double v = in ? dtp / (dfp + dtp + 2.220446049250313e-16) : -1.0;      // :495, np.spacing(1) = 2^-52
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {                     // :502-504: the maximum to the right
      const double other = __shfl_down(v, o, 64);
      if (lane + o < 64) v = fmax(v, other);
    }
    v = fmax(v, carry);
    carry = __shfl(v, 0, 64);
    if (in && (i == 0 || tp)) {                            // the first index whose recall reaches a threshold (:506)
      const int r1 = thrs_le(rec_thrs, R, dtp / dng);
      const int r0 = i == 0 ? 0 : thrs_le(rec_thrs, R, (double)(tpi - (tp ? 1 : 0)) / dng);
      for (int r = r0; r < r1; ++r) prec[r * rstride] = v;
    }
    tp_end = tp0;
    fp_end = fp0;
  }
}

}  // namespace

extern "C" int fiber_ap_max_gt(void) { return AP_MAX_GT; }
extern "C" int fiber_ap_chunk(void) { return AP_CHUNK; }

extern "C" int fiber_ap_match(const float* boxes, const int* labels, const int* count, const double* gt, const double* gt_area, const int* gt_cat,
                              const unsigned char* gt_ignore, const int* gt_count, const unsigned long long* neg_mask,
                              const unsigned long long* nel_mask, const double* iou_thrs, const double* area_rng, unsigned long long* match,
                              unsigned long long* ignore, unsigned char* valid, long long* num_gt, int B, int D, int G, int C, int T, int A,
                              int max_dets, hipStream_t stream) {
  if (B < 0 || D < 0 || G < 0 || C <= 0 || T <= 0 || A <= 0) return FIBER_EINVAL;
  if ((long long)T * A > 64 || G > AP_MAX_GT) return FIBER_EINVAL;
  if ((long long)B * T * A > 0x7fffffffLL || (long long)B * D > 0x7fffffffLL) return FIBER_EINVAL;
  if (B == 0) return FIBER_OK;
  if (!count || !gt_count || !neg_mask || !nel_mask || !iou_thrs || !area_rng || !num_gt) return FIBER_EINVAL;
  if (D > 0 && (!boxes || !labels || !match || !ignore || !valid)) return FIBER_EINVAL;
  if (G > 0 && (!gt || !gt_area || !gt_cat || !gt_ignore)) return FIBER_EINVAL;
  if (fiber_misaligned(16, boxes) || fiber_misaligned(8, gt, gt_area, neg_mask, nel_mask, iou_thrs, area_rng, match, ignore, num_gt) ||
      fiber_misaligned(4, labels, count, gt_cat, gt_count))
    return FIBER_EINVAL;
  if (D > 0) {
    if (hipMemsetAsync(match, 0, (size_t)B * D * 8, stream) != hipSuccess) return FIBER_ELAUNCH;
    if (hipMemsetAsync(ignore, 0, (size_t)B * D * 8, stream) != hipSuccess) return FIBER_ELAUNCH;
  }
  hipLaunchKernelGGL(ap_match_kernel, dim3((unsigned)(B * T * A)), dim3(64), 0, stream, boxes, labels, count, gt, gt_area, gt_cat, gt_ignore,
                     gt_count, neg_mask, nel_mask, iou_thrs, area_rng, match, ignore, valid, reinterpret_cast<u64*>(num_gt), D, G, C,
                     (C + 63) / 64, T, A, max_dets);
  FIBER_CHECK_LAUNCH();
  return FIBER_OK;
}

extern "C" int fiber_ap_coco_max_categories(void) { return AP_COCO_MAX_CAT; }

extern "C" int fiber_ap_match_coco(const float* boxes, const int* labels, const int* count, const double* gt, const double* gt_area,
                                   const int* gt_cat, const unsigned char* gt_crowd, const int* gt_count, const double* iou_thrs,
                                   const double* area_rng, unsigned long long* match, unsigned long long* ignore, int* rank,
                                   unsigned char* valid, long long* num_gt, int B, int D, int G, int C, int T, int A, int cap, int plus_one,
                                   hipStream_t stream) {
  if (B < 0 || D < 0 || G < 0 || C <= 0 || T <= 0 || A <= 0 || cap < 0 || (plus_one != 0 && plus_one != 1)) return FIBER_EINVAL;
  if ((long long)T * A > 64 || G > AP_MAX_GT || C > AP_COCO_MAX_CAT) return FIBER_EINVAL;
  if ((long long)B * T * A > 0x7fffffffLL || (long long)B * D > 0x7fffffffLL) return FIBER_EINVAL;
  if (B == 0) return FIBER_OK;
  if (!count || !gt_count || !iou_thrs || !area_rng || !num_gt) return FIBER_EINVAL;
  if (D > 0 && (!boxes || !labels || !match || !ignore || !rank || !valid)) return FIBER_EINVAL;
  if (G > 0 && (!gt || !gt_area || !gt_cat || !gt_crowd)) return FIBER_EINVAL;
  if (fiber_misaligned(16, boxes) || fiber_misaligned(8, gt, gt_area, iou_thrs, area_rng, match, ignore, num_gt) ||
      fiber_misaligned(4, labels, count, gt_cat, gt_count, rank))
    return FIBER_EINVAL;
  if (D > 0) {
    if (hipMemsetAsync(match, 0, (size_t)B * D * 8, stream) != hipSuccess) return FIBER_ELAUNCH;
    if (hipMemsetAsync(ignore, 0, (size_t)B * D * 8, stream) != hipSuccess) return FIBER_ELAUNCH;
  }
  hipLaunchKernelGGL(ap_match_coco_kernel, dim3((unsigned)(B * T * A)), dim3(64), (size_t)C * sizeof(int), stream, boxes, labels, count, gt, gt_area, gt_cat, gt_crowd,
                     gt_count, iou_thrs, area_rng, match, ignore, rank, valid, reinterpret_cast<u64*>(num_gt), D, G, C, T, A, cap, plus_one);
  FIBER_CHECK_LAUNCH();
  return FIBER_OK;
}

extern "C" int fiber_ap_accumulate(const unsigned long long* match, const unsigned long long* ignore, const long long* seg_ptr,
                                   const long long* num_gt, const double* rec_thrs, double* precision, double* recall, long long N, int C,
                                   int T, int A, int R, hipStream_t stream) {
  if (N < 0 || C <= 0 || T <= 0 || A <= 0 || R < 0) return FIBER_EINVAL;
  if ((long long)T * A > 64) return FIBER_EINVAL;
  const long long problems = (long long)C * T * A;
  if ((problems + AP_ACC_WAVES - 1) / AP_ACC_WAVES > 0x7fffffffLL) return FIBER_EINVAL;
  if (!seg_ptr || !num_gt || !recall || (R > 0 && (!rec_thrs || !precision)) || (N > 0 && (!match || !ignore))) return FIBER_EINVAL;
  if (fiber_misaligned(8, match, ignore, seg_ptr, num_gt, rec_thrs, precision, recall)) return FIBER_EINVAL;
  hipLaunchKernelGGL(ap_accumulate_kernel, dim3((unsigned)((problems + AP_ACC_WAVES - 1) / AP_ACC_WAVES)), dim3(64 * AP_ACC_WAVES), 0, stream,
                     match, ignore, seg_ptr, num_gt, rec_thrs, precision, recall, N, C, T, A, R, problems);
  FIBER_CHECK_LAUNCH();
  return FIBER_OK;
}
