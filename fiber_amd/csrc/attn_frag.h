// Fragment helpers shared by the attention kernels (attn.hip, attn_x.hip, win_attn.hip): one spelling each.
#pragma once
#include <type_traits>

#include "common.h"

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;

// shift-mask region of image coordinate x (swin_transformer.py:327-350): 0 | 1 | 2 = before the last window | its unshifted part | the wrapped part
__device__ __forceinline__ int region_of(int x, int n, int ws, int shift) { return x < n - ws ? 0 : (x < n - shift ? 1 : 2); }

__device__ __forceinline__ bf16x8 pack8(const f32x4& a, const f32x4& b) {
  bf16x8 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) { o[e] = f2bf(a[e]); o[4 + e] = f2bf(b[e]); }
  return o;
}
__device__ __forceinline__ bf16x8 zero8() {
  bf16x8 z;
#pragma unroll
  for (int e = 0; e < 8; ++e) z[e] = f2bf(0.f);
  return z;
}
__device__ __forceinline__ f32x4 exp2x4(f32x4 a) {
  return f32x4{__builtin_amdgcn_exp2f(a[0]), __builtin_amdgcn_exp2f(a[1]), __builtin_amdgcn_exp2f(a[2]), __builtin_amdgcn_exp2f(a[3])};
}

// MFMA operand A (transposed fragment) out of a ROW-MAJOR [token][head_dim] image of row stride STRIDE elements: rows {t0*16+g*4..+3} U
// {t0*16+16+g*4..+3}, column d0 + l.  ds_read_b64_tr_b16 hands lane l of a 16-lane group column l of the 4x16 block whose
// (row l>>2, 4-column piece l&3) address that lane supplies, so a transposed copy of the image never has to be written
// (8 ds_write_b16 per staged chunk less).
template <int STRIDE>
__device__ __forceinline__ bf16x8 trr_frag(const bf16* rm, int d0, int t0, int g, int l) {
  const bf16* a = rm + (t0 * 16 + g * 4 + (l >> 2)) * STRIDE + d0 + (l & 3) * 4;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a + 16 * STRIDE));
  s16x8 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) { o[e] = lo[e]; o[4 + e] = hi[e]; }
  return __builtin_bit_cast(bf16x8, o);
}

// uniform base pointer + 32-bit BYTE offset: the form the backend turns into `global_load/store v, voff, s[base:base+1]`
template <typename T>
__device__ __forceinline__ T* at(T* base, unsigned elem_off) {
  using C = std::conditional_t<std::is_const<T>::value, const char, char>;
  return reinterpret_cast<T*>(reinterpret_cast<C*>(base) + elem_off * (unsigned)sizeof(T));
}
