// wgrad_common.hpp -- what the two position-tiled weight-gradient kernels share (conv_wgrad.hip:
// dy staged in LDS; conv_wgrad_direct.hip: dy straight from memory): the vector types, the LDS /
// global load primitives, and the host code that fills the common members of their parameter
// structs.  The primitives are inline asm where hipcc's waitcnt pass must not see the load.
#pragma once
#include "stream_common.hpp"
#include <algorithm>
#include <type_traits>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* lds_vp;
typedef const __attribute__((address_space(1))) void* gbl_vp;

// LDS-DMA: 4 / 16 bytes per lane from global memory into LDS
__device__ __forceinline__ void wg_glds4(const float* g, float* l) {
  __builtin_amdgcn_global_load_lds((gbl_vp)g, (lds_vp)l, 4, 0, 0);
}
__device__ __forceinline__ void wg_glds16(const float* g, float* l) {
  __builtin_amdgcn_global_load_lds((gbl_vp)g, (lds_vp)l, 16, 0, 0);
}
__device__ __forceinline__ unsigned wg_lds_addr(const void* p) {
  return (unsigned)(uintptr_t)(lds_vp)p;
}
__device__ __forceinline__ float wg_lds_ld(unsigned addr) {
  float v;
  asm volatile("ds_read_b32 %0, %1" : "=v"(v) : "v"(addr));
  return v;
}
__device__ __forceinline__ i32x4 wg_lds_ld128(unsigned addr) {
  i32x4 v;
  asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(addr));
  return v;
}
// ... with the instruction's immediate offset field written out (also where it is 0)
template <int OFF>
__device__ __forceinline__ float wg_lds_ld_off(unsigned addr) {
  float v;
  asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "i"(OFF));
  return v;
}
template <int OFF>
__device__ __forceinline__ f32x4 wg_lds_ld128_off(unsigned addr) {
  f32x4 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "i"(OFF));
  return v;
}
__device__ __forceinline__ f32x4 wg_gl_ld128(const float* sbase, unsigned voff) {
  f32x4 v;
  asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(v) : "v"(voff), "s"(sbase));
  return v;
}
// bf16 operand form (e2_set_mfma_dtype): four f32 rounded to bf16, nearest even, by plain casts
// (two v_cvt_pk_bf16_f32; NOT inline asm: the compiler must see the VALU write to place the wait
// states in front of the MFMA that reads it)
__device__ __forceinline__ s16x4 wg_pack_bf16(float a, float b, float c, float d) {
  union { bf16x4 h; s16x4 v; } r;
  r.h = (bf16x4){(__bf16)a, (__bf16)b, (__bf16)c, (__bf16)d};
  return r.v;
}

// ---- host side --------------------------------------------------------------------------------
// input spans a work-group stages per position tile: (input channels its BNn columns touch) x kd
static inline int wg_maxspans(const WgradArgs& a, int BNn) {
  const int T = a.kd * a.kh * a.kw;
  int cis = (BNn - 1) / T + 2;
  if (cis > a.Cin) cis = a.Cin;
  return cis * a.kd;
}

// The members WgradP and WdP have in common, from the call's arguments and its tiling: MT 16-row
// blocks and NB 16-column blocks per work-group, tiles of BP out of the K positions of a plane, PS
// position splits.  (Lpad, bufFloats, the position count itself and its divider: the caller's.)
template <class P>
static int wg_fill(P& p, const WgradArgs& a, int MT, int NB, int K, int BP, int PS) {
  p.x = a.x; p.dy = a.dy; p.dw = a.dw;
  p.Cin = a.Cin; p.Cout = a.Cout; p.kd = a.kd; p.kh = a.kh; p.kw = a.kw;
  p.THW = a.kh * a.kw; p.T = a.kd * p.THW;
  p.Do = a.Do; p.Ho = a.Ho; p.Wo = a.Wo;
  p.xsN = a.xsN; p.xsC = a.xsC; p.xsZ = a.xsZ; p.xsY = a.xsY;
  p.dsN = a.dsN; p.dsC = a.dsC; p.dsZ = a.dsZ; p.dsY = a.dsY;
  p.flip = a.flip;
  p.upR = a.upR > 1 ? a.upR : 1;
  const long NTOT = (long)a.Cin * p.T;
  E2_REQUIRE(NTOT < (1L << 30), "wgrad: Cin*T too large");
  p.NTOT = (int)NTOT;
  p.maxSpans = wg_maxspans(a, 16 * NB);
  p.nMT = e2_cdiv(e2_cdiv(a.Cout, 16), MT);
  p.nNT = e2_cdiv(e2_cdiv(p.NTOT, 16), NB);
  p.nPT = e2_cdiv(K, BP);
  p.tilesTotal = a.N * a.Do * p.nPT;
  p.nPS = std::max(1, std::min(PS, p.tilesTotal));
  p.Din = a.Do + a.kd - 1;
  p.N = a.N;
  p.dbg = e2_dbg_env_int("E2_WGRAD_DBG");
  return 0;
}

// the MT both kernels have instances for (the cost model's loops), and the run-time MT of a tiling
// as a template argument: f(std::integral_constant<int, MT>), or -1 where there is no such instance
static const int kWgMTs[] = {1, 2, 3, 4, 5, 7};
template <class F>
static int wg_with_mt(int MT, F&& f) {
  switch (MT) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 7: return f(std::integral_constant<int, 7>{});
  }
  return -1;
}
