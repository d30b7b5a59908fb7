// The grounding solver's optimizer step in three launches (gfx950): the global gradient norm, the clip coefficient with the
// per-tensor bias corrections, and torch's AdamW with the model EMA and the bf16 working copies in the same pass.
//
// Replaces, on the caller side of the fine-grained path, maskrcnn_benchmark/solver/build.py:8-55 (clip_grad_norm_ over every
// parameter wrapped around torch.optim.AdamW, one parameter group per parameter), utils/ema.py:36-45 (ema = d ema + (1 - d) p
// per state-dict entry, ~4 ATen kernels each) and the non-finite skip of GradScaler.step (engine/trainer.py:162-168).
// torch's form of the rule, NOT the transformers form of optim.hip: decay first (p *= 1 - lr wd), eps added to the
// bias-corrected sqrt(v):
//   g' = c g;  m' = b1 m + (1-b1) g';  v' = b2 v + (1-b2) g' g';  p1 = p decay;  p' = p1 - s1 m' / (sqrt(v') r2 + eps)
//   decay = 1 - lr wd,  s1 = lr / (1 - b1^t),  r2 = 1 / sqrt(1 - b2^t),  c = min(1, max_norm / (norm + 1e-6))
// Every tensor carries its own lr, wd and step count t; the counts live in device memory and are advanced by the finalize
// kernel only when the step is taken, so the host never reads anything back.
// Traffic: 4 B/element for the norm, 38 B/element for the update with a bf16 copy and an EMA (reads p, g, m, v, ema; writes p, m, v,
// copy, ema).  Tables as in adamw_multi_kernel (optim.hip): device pointers per tensor, numel[n], (tensor, chunk) pairs.
#include "common.h"

namespace {

constexpr int CHUNK = 4096;   // elements per workgroup: fiber_adamw_chunk() (checked by the entry points)
constexpr int COLS = 7;       // table row: param, grad, exp_avg, exp_avg_sq, bf16 copy or 0, ema or 0, coefficient row (device pointers)

// ---- 1. sum of g^2 per chunk, fp64 -------------------------------------------------------------------------------------------
__device__ __forceinline__ double sq(float g) { return (double)g * (double)g; }      // exact: 24 x 24 bits fit 53

__global__ __launch_bounds__(256) void grad_sqnorm_multi_kernel(const long long* __restrict__ table, const long long* __restrict__ numel,
                                                                const int* __restrict__ chunks, double* __restrict__ partial) {
  __shared__ double wave_sum[4];
  const int t = chunks[2 * blockIdx.x], c = chunks[2 * blockIdx.x + 1];
  const long long gp = table[COLS * t + 1];
  const float* g = reinterpret_cast<const float*>(gp);
  const long long n = numel[t];
  const long long lo = (long long)c * CHUNK, hi = lo + CHUNK < n ? lo + CHUNK : n;
  double acc = 0.0;
  if ((gp & 15) == 0) {
    long long i = lo + threadIdx.x * 4;
    for (; i + 3 < hi; i += 1024) {
      const float4 gg = *reinterpret_cast<const float4*>(g + i);
      acc += sq(gg.x); acc += sq(gg.y); acc += sq(gg.z); acc += sq(gg.w);
    }
    for (i = lo + ((hi - lo) & ~3LL) + threadIdx.x; i < hi; i += 256) acc += sq(g[i]);   // ragged tail of the tensor
  } else {
    for (long long i = lo + threadIdx.x; i < hi; i += 256) acc += sq(g[i]);               // a DDP bucket view off 16 bytes
  }
  // the wave, then the four waves: a fixed order, so two launches over the same table give the same bits
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
}

// ---- 2. norm, clip coefficient, skip flag; step counts and coefficient rows -----------------------------------------------------
struct SolverState { float norm, clip; int skip, skipped_steps; };

__global__ __launch_bounds__(256) void solver_finalize_kernel(const double* __restrict__ partial, int npartial, float max_norm,
                                                              const float* __restrict__ lr_wd, int* __restrict__ steps,
                                                              float* __restrict__ coef, int n, float b1, float b2, SolverState* state) {
  __shared__ double red[256];
  __shared__ int skip_s;
  double acc = 0.0;
  for (int i = threadIdx.x; i < npartial; i += 256) acc += partial[i];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double sum = red[0];
    const bool finite = isfinite(sum);
    const double norm = sqrt(sum);
    double c = (double)max_norm / (norm + 1e-6);          // clip_grad_norm_'s rule; max_norm = +inf: clipping off
    c = c < 1.0 ? c : 1.0;
    state->norm = (float)norm;
    state->clip = finite ? (float)c : 0.f;
    state->skip = finite ? 0 : 1;
    state->skipped_steps += finite ? 0 : 1;
    skip_s = finite ? 0 : 1;
  }
  __syncthreads();
  if (skip_s) return;                                     // a skipped step advances no count
  for (int i = threadIdx.x; i < n; i += 256) {
    const int t = steps[i] + 1;
    steps[i] = t;
    const double lr = (double)lr_wd[2 * i], wd = (double)lr_wd[2 * i + 1];
    coef[4 * i + 0] = (float)(1.0 - lr * wd);
    coef[4 * i + 1] = (float)(lr / (1.0 - pow((double)b1, (double)t)));
    coef[4 * i + 2] = (float)(1.0 / sqrt(1.0 - pow((double)b2, (double)t)));
    coef[4 * i + 3] = 0.f;
  }
}

// ---- 3. the update -------------------------------------------------------------------------------------------------------------
struct TorchAdamArgs {
  const long long* table;     // [n][COLS]
  const long long* numel;     // [n]
  const int* chunks;          // [nchunks][2]
  float b1, b2, eps, ema_decay;
  const SolverState* state;
};

struct Coef { float c, decay, s1, r2, b1, omb1, b2, omb2, eps; };

__device__ __forceinline__ void adam1(float& p, float g, float& m, float& v, const Coef& k) {
  g = k.c * g;
  m = k.b1 * m + k.omb1 * g;
  v = k.b2 * v + k.omb2 * g * g;
  const float p1 = p * k.decay;
  p = p1 - k.s1 * m / (sqrtf(v) * k.r2 + k.eps);
}

__device__ __forceinline__ void ema1(float& e, float p, float d, float omd) { e = d * e + omd * p; }

// ema = d ema + (1 - d) src over [lo, hi): the EMA line alone (a skipped step, and fiber_ema_multi_f32)
__device__ __forceinline__ void ema_range(const float* __restrict__ src, float* __restrict__ e, long long lo, long long hi, float d, bool vec) {
  const float omd = 1.f - d;
  if (vec) {
    long long i = lo + threadIdx.x * 4;
    for (; i + 3 < hi; i += 1024) {
      const float4 pp = *reinterpret_cast<const float4*>(src + i);
      float4 ee = *reinterpret_cast<float4*>(e + i);
      ema1(ee.x, pp.x, d, omd); ema1(ee.y, pp.y, d, omd); ema1(ee.z, pp.z, d, omd); ema1(ee.w, pp.w, d, omd);
      *reinterpret_cast<float4*>(e + i) = ee;
    }
    for (i = lo + ((hi - lo) & ~3LL) + threadIdx.x; i < hi; i += 256) { float ee = e[i]; ema1(ee, src[i], d, omd); e[i] = ee; }
  } else {
    for (long long i = lo + threadIdx.x; i < hi; i += 256) { float ee = e[i]; ema1(ee, src[i], d, omd); e[i] = ee; }
  }
}

__global__ __launch_bounds__(256) void adamw_torch_multi_kernel(TorchAdamArgs a) {
  const int t = a.chunks[2 * blockIdx.x], c = a.chunks[2 * blockIdx.x + 1];
  const long long* row = a.table + (long long)COLS * t;
  float* p = reinterpret_cast<float*>(row[0]);
  const float* g = reinterpret_cast<const float*>(row[1]);
  float* m = reinterpret_cast<float*>(row[2]);
  float* v = reinterpret_cast<float*>(row[3]);
  bf16* w = reinterpret_cast<bf16*>(row[4]);
  float* e = reinterpret_cast<float*>(row[5]);
  const float* cf = reinterpret_cast<const float*>(row[6]);
  const long long n = a.numel[t];
  const long long lo = (long long)c * CHUNK, hi = lo + CHUNK < n ? lo + CHUNK : n;
  // as in adamw_multi_kernel: p / m / v / ema / the copy are allocations of their own (aligned) unless a caller hands in views;
  // gradients may be views into DDP's flat buckets at any multiple of 4 bytes
  const bool vec = (((row[0] | row[2] | row[3] | row[5]) & 15) == 0) && ((row[4] & 7) == 0);
  const bool gvec = (row[1] & 15) == 0;
  const float d = a.ema_decay, omd = 1.f - d;
  if (a.state->skip) {                                       // non-finite gradients: p, m, v and the copy stay; the EMA still moves
    if (e) ema_range(p, e, lo, hi, d, ((row[0] | row[5]) & 15) == 0);
    return;
  }
  const Coef k{a.state->clip, cf[0], cf[1], cf[2], a.b1, 1.f - a.b1, a.b2, 1.f - a.b2, a.eps};
  long long i = lo + threadIdx.x * 4;
  if (vec && gvec && hi - lo == CHUNK) {
    // a full chunk: every load of the thread's four float4 columns requested before the first update (optim.hip)
    float4 pp[4], gg[4], mm[4], vv[4], ee[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      pp[u] = *reinterpret_cast<float4*>(p + i + u * 1024); gg[u] = *reinterpret_cast<const float4*>(g + i + u * 1024);
      mm[u] = *reinterpret_cast<float4*>(m + i + u * 1024); vv[u] = *reinterpret_cast<float4*>(v + i + u * 1024);
      if (e) ee[u] = *reinterpret_cast<float4*>(e + i + u * 1024);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      adam1(pp[u].x, gg[u].x, mm[u].x, vv[u].x, k); adam1(pp[u].y, gg[u].y, mm[u].y, vv[u].y, k);
      adam1(pp[u].z, gg[u].z, mm[u].z, vv[u].z, k); adam1(pp[u].w, gg[u].w, mm[u].w, vv[u].w, k);
      *reinterpret_cast<float4*>(p + i + u * 1024) = pp[u];
      *reinterpret_cast<float4*>(m + i + u * 1024) = mm[u];
      *reinterpret_cast<float4*>(v + i + u * 1024) = vv[u];
      if (w) {
        bf16x4 o;
        o[0] = f2bf(pp[u].x); o[1] = f2bf(pp[u].y); o[2] = f2bf(pp[u].z); o[3] = f2bf(pp[u].w);
        *reinterpret_cast<bf16x4*>(w + i + u * 1024) = o;
      }
      if (e) {
        ema1(ee[u].x, pp[u].x, d, omd); ema1(ee[u].y, pp[u].y, d, omd); ema1(ee[u].z, pp[u].z, d, omd); ema1(ee[u].w, pp[u].w, d, omd);
        *reinterpret_cast<float4*>(e + i + u * 1024) = ee[u];
      }
    }
  } else if (vec) {
    for (; i + 3 < hi; i += 1024) {
      float4 pp = *reinterpret_cast<float4*>(p + i);
      const float4 gg = gvec ? *reinterpret_cast<const float4*>(g + i) : float4{g[i], g[i + 1], g[i + 2], g[i + 3]};
      float4 mm = *reinterpret_cast<float4*>(m + i), vv = *reinterpret_cast<float4*>(v + i);
      adam1(pp.x, gg.x, mm.x, vv.x, k); adam1(pp.y, gg.y, mm.y, vv.y, k);
      adam1(pp.z, gg.z, mm.z, vv.z, k); adam1(pp.w, gg.w, mm.w, vv.w, k);
      *reinterpret_cast<float4*>(p + i) = pp;
      *reinterpret_cast<float4*>(m + i) = mm;
      *reinterpret_cast<float4*>(v + i) = vv;
      if (w) {
        bf16x4 o;
        o[0] = f2bf(pp.x); o[1] = f2bf(pp.y); o[2] = f2bf(pp.z); o[3] = f2bf(pp.w);
        *reinterpret_cast<bf16x4*>(w + i) = o;
      }
      if (e) {
        float4 ee = *reinterpret_cast<float4*>(e + i);
        ema1(ee.x, pp.x, d, omd); ema1(ee.y, pp.y, d, omd); ema1(ee.z, pp.z, d, omd); ema1(ee.w, pp.w, d, omd);
        *reinterpret_cast<float4*>(e + i) = ee;
      }
    }
    // ragged tail of the tensor (n % 4 != 0): only the last chunk has one
    for (i = lo + ((hi - lo) & ~3LL) + threadIdx.x; i < hi; i += 256) {
      float pp = p[i], mm = m[i], vv = v[i];
      adam1(pp, g[i], mm, vv, k);
      p[i] = pp; m[i] = mm; v[i] = vv;
      if (w) w[i] = f2bf(pp);
      if (e) { float ee = e[i]; ema1(ee, pp, d, omd); e[i] = ee; }
    }
  } else {
    for (i = lo + threadIdx.x; i < hi; i += 256) {
      float pp = p[i], mm = m[i], vv = v[i];
      adam1(pp, g[i], mm, vv, k);
      p[i] = pp; m[i] = mm; v[i] = vv;
      if (w) w[i] = f2bf(pp);
      if (e) { float ee = e[i]; ema1(ee, pp, d, omd); e[i] = ee; }
    }
  }
}

__global__ __launch_bounds__(256) void ema_multi_kernel(const long long* __restrict__ table, const long long* __restrict__ numel,
                                                        const int* __restrict__ chunks, float d) {
  const int t = chunks[2 * blockIdx.x], c = chunks[2 * blockIdx.x + 1];
  const long long sp = table[2 * t], ep = table[2 * t + 1];
  const long long n = numel[t];
  const long long lo = (long long)c * CHUNK, hi = lo + CHUNK < n ? lo + CHUNK : n;
  ema_range(reinterpret_cast<const float*>(sp), reinterpret_cast<float*>(ep), lo, hi, d, ((sp | ep) & 15) == 0);
}

}  // namespace

// Sum of squares of every gradient of the table, one fp64 partial per chunk: partial[k] = sum of g^2 over chunk k (each product exact
// in fp64), reduced in a fixed order.  table: int64[n*7] device pointers, the row of fiber_adamw_torch_multi_f32 (only column 1, the
// gradient, is read); numel: int64[n]; chunks: int32[nchunks*2] (tensor, chunk) pairs of fiber_adamw_chunk() elements; partial:
// double[nchunks]; all in device memory.  Gradients are not modified.
extern "C" int fiber_grad_sqnorm_multi_f32(const long long* table, const long long* numel, const int* chunks, int nchunks,
                                           double* partial, hipStream_t stream) {
  if (nchunks <= 0) return FIBER_OK;
  if (!table || !numel || !chunks || !partial || fiber_adamw_chunk() != CHUNK) return FIBER_EINVAL;
  hipLaunchKernelGGL(grad_sqnorm_multi_kernel, dim3(nchunks), dim3(256), 0, stream, table, numel, chunks, partial);
  FIBER_CHECK_LAUNCH();
  return FIBER_OK;
}

// One workgroup: sum = partial[0..npartial) in index order (strided over the threads, then a fixed tree), in fp64
// norm = sqrt(sum), c = min(1, max_norm / (norm + 1e-6)) (max_norm = +inf: no clipping).  A non-finite sum sets c = 0, skip = 1 and
// adds one to skipped_steps; otherwise every tensor i < n gets steps[i] += 1 and its coefficient row
// coef[4 i ..] = {1 - lr wd, lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t), 0}, each computed in fp64 and rounded once, from
// lr_wd float[n][2] = {lr, weight_decay}.  state: {float norm, float c, int32 skip, int32 skipped_steps} (16 bytes, zeroed once by the
// caller).  Everything in device memory.
extern "C" int fiber_solver_finalize(const double* partial, int npartial, float max_norm, const float* lr_wd, int* steps, float* coef,
                                     int n, float beta1, float beta2, void* state, hipStream_t stream) {
  if (npartial < 0 || n < 0 || !state || (npartial > 0 && !partial) || (n > 0 && (!lr_wd || !steps || !coef))) return FIBER_EINVAL;
  if (!(max_norm > 0.f)) return FIBER_EINVAL;
  hipLaunchKernelGGL(solver_finalize_kernel, dim3(1), dim3(256), 0, stream, partial, npartial, max_norm, lr_wd, steps, coef, n, beta1,
                     beta2, (SolverState*)state);
  FIBER_CHECK_LAUNCH();
  return FIBER_OK;
}

// torch.optim.AdamW for every tensor of the table in one launch, with the gradient scaled by state->c, the bf16 working copy and the
// model EMA (ema = ema_decay ema + (1 - ema_decay) p') written in the same pass.  table: int64[n*7] device pointers {param fp32, grad
// fp32, exp_avg, exp_avg_sq, bf16 copy or 0, ema fp32 or 0, coefficient row float[4] of fiber_solver_finalize}; numel, chunks as above;
// state: the block fiber_solver_finalize wrote.  With state->skip set p, exp_avg, exp_avg_sq and the copy are left as they are and the
// EMA is taken from the unchanged p.  Gradients are not modified.
extern "C" int fiber_adamw_torch_multi_f32(const long long* table, const long long* numel, const int* chunks, int nchunks, float beta1,
                                           float beta2, float eps, float ema_decay, const void* state, hipStream_t stream) {
  if (nchunks <= 0) return FIBER_OK;
  if (!table || !numel || !chunks || !state || fiber_adamw_chunk() != CHUNK) return FIBER_EINVAL;
  TorchAdamArgs a{table, numel, chunks, beta1, beta2, eps, ema_decay, (const SolverState*)state};
  hipLaunchKernelGGL(adamw_torch_multi_kernel, dim3(nchunks), dim3(256), 0, stream, a);
  FIBER_CHECK_LAUNCH();
  return FIBER_OK;
}

// The EMA line alone, for entries no optimizer of ours steps: ema = decay ema + (1 - decay) src.  table: int64[n*2] device pointers
// {src fp32, ema fp32}; numel, chunks as above.
extern "C" int fiber_ema_multi_f32(const long long* table, const long long* numel, const int* chunks, int nchunks, float decay,
                                   hipStream_t stream) {
  if (nchunks <= 0) return FIBER_OK;
  if (!table || !numel || !chunks || fiber_adamw_chunk() != CHUNK) return FIBER_EINVAL;
  hipLaunchKernelGGL(ema_multi_kernel, dim3(nchunks), dim3(256), 0, stream, table, numel, chunks, decay);
  FIBER_CHECK_LAUNCH();
  return FIBER_OK;
}
