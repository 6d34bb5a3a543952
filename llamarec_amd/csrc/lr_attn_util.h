// lr_attn_util.h -- device helpers shared by the MFMA flash-attention kernels (through lr_attn_body.h the head_dim-64, -96,
// -128 and -256 bodies, and the staging of llama_attn.hip and llama_attn_cached.hip): LDS-DMA issued from inline asm, the
// workgroup-to-tile order, gfx950's lane-swap reductions, and max instructions on raw MFMA outputs. What the four bodies share
// beyond these is lr_attn_body.h.
#ifndef LR_ATTN_UTIL_H
#define LR_ATTN_UTIL_H

#include "llama_kernels.h"

// LDS-DMA through a buffer descriptor as INLINE ASM. With the builtin (__builtin_amdgcn_raw_ptr_buffer_load_lds) hipcc
// knows an LDS write is pending on the vector-memory counter and -- unable to prove that a ds_read_b64_tr_b16 (the V^T
// fragment reads) touches another stage buffer -- puts `s_waitcnt vmcnt(0)` in front of the first transposed read of every
// key block: each wave then sat out the landing of the NEXT block's tiles in the middle of the current block (found in
// round 3 in the .s of the product kernel; it is also why requesting the V fragments earlier was slower). The asm form is
// invisible to that pass; the one wait that is needed stands in front of the block's barrier, written by hand.
// (M0 is a reserved register to hipcc: it cannot be named as a clobber, and nothing else in these kernels uses it --
// gfx9+ LDS instructions do not read M0.)
typedef int fa_int4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ fa_int4 fa_make_rsrc(const void* base, int num_records) {
  const unsigned long long b = reinterpret_cast<unsigned long long>(base);
  fa_int4 r;
  r[0] = __builtin_amdgcn_readfirstlane((int)(unsigned)b);
  r[1] = __builtin_amdgcn_readfirstlane((int)((b >> 32) & 0xffffu));   // stride 0
  r[2] = __builtin_amdgcn_readfirstlane(num_records);
  r[3] = 0x00020000;
  return r;
}
__device__ __forceinline__ void fa_glds16(const void* gsrc, const void* lds_wave_base) {   // per-lane source address
  const unsigned m0v = (unsigned)(size_t)((__attribute__((address_space(3))) const char*)lds_wave_base);
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(m0v), "v"(gsrc) : "memory");
}
__device__ __forceinline__ void fa_dma16(fa_int4 rsrc, const void* lds_wave_base, unsigned voff) {
  const unsigned m0v = (unsigned)(size_t)((__attribute__((address_space(3))) const char*)lds_wave_base);
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(m0v), "v"(voff), "s"(rsrc)
               : "memory");
}

// workgroup -> ((prompt, head) pair, query tile) of the head_dim-64, -96, -128 and -256 kernels, variant 2's order: a pair per
// dispatch stream (blockIdx.x & 7), heavy tiles first, the two lightest tiles of every pair at the end of the launch. The
// launch holds 8 * ceil(n_pairs / 8) * max_qblocks workgroups; the caller returns when pair >= n_pairs. Neither result is
// known to the compiler as wave-uniform yet.
__device__ __forceinline__ void fa_tile_of_workgroup(int n_pairs, int max_qblocks, int& pair, int& qb) {
  const int id = blockIdx.x, stream = id & 7, j = id >> 3;
  const int ppx = (n_pairs + 7) >> 3;
  const int n_light = min(max_qblocks, 2), n_heavy = max_qblocks - n_light;
  int pl;
  if (j < ppx * n_heavy) {
    pl = j / n_heavy;
    qb = max_qblocks - 1 - j % n_heavy;
  } else {
    const int j2 = j - ppx * n_heavy;
    pl = j2 / n_light;
    qb = n_light - 1 - j2 % n_light;
  }
  pair = pl * 8 + stream;
}

// x[lane] (op) x[lane ^ 16] and x[lane] (op) x[lane ^ 32] without the LDS crossbar: gfx950's row / half swaps
// (v_permlane16_swap, v_permlane32_swap) hand both partners to every lane at VALU speed; __shfl_xor compiles
// to ds_bpermute_b32 (~100+ cycles of dependent latency, four of them on every key block's critical path).
// hipcc pitfall: __builtin_bit_cast(float, r[1]) on the builtin's 2-vector result reads element 0 (the cast
// takes the vector's address) -- copy the elements into scalars first.
__device__ __forceinline__ void fa_swap16(float v, float& a, float& b) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  const auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  const unsigned r0 = r[0], r1 = r[1];
  a = __builtin_bit_cast(float, r0);
  b = __builtin_bit_cast(float, r1);
}
__device__ __forceinline__ void fa_swap32(float v, float& a, float& b) {
  const unsigned u = __builtin_bit_cast(unsigned, v);
  const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  const unsigned r0 = r[0], r1 = r[1];
  a = __builtin_bit_cast(float, r0);
  b = __builtin_bit_cast(float, r1);
}
// v_max3_f32 on raw MFMA outputs: fmaxf() makes hipcc canonicalise every input first (a v_max_f32 x, x per score);
// the scores are finite or -inf here, where max is exact whatever the association
__device__ __forceinline__ float fa_max3(float a, float b, float c) {
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
__device__ __forceinline__ float fa_max2(float a, float b) {
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ float fa_max_xor16_32(float v) {
  float a, b;
  fa_swap16(v, a, b);
  fa_swap32(fa_max2(a, b), a, b);
  return fa_max2(a, b);
}
__device__ __forceinline__ float fa_sum_xor16_32(float v) {
  float a, b;
  fa_swap16(v, a, b);
  fa_swap32(a + b, a, b);
  return a + b;
}

#endif
