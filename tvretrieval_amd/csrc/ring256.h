// What the 256 x 256 LDS-DMA ring kernels share (gemm256.hip, gemm256p.hip, q2c_ring.hip, q2c_persist.hip): the geometry
// of a ring slot and the force-inlined device primitives around it.  The ring depths and the slice width are dispatch.h's;
// the kernels' K loops and epilogues stay their own (their register budgets differ on purpose).
#pragma once
#include "common.h"

namespace ring256 {
constexpr int ROWB = dispatch::SLICE_BYTES;               // bytes of K per row per slice
constexpr int OPER_BYTES = dispatch::RING_ROWS * ROWB;    // one operand of a slice: 16 KiB
constexpr int SLOT_BYTES = 2 * OPER_BYTES;                // both operands
}  // namespace ring256

// LDS-DMA from inline asm, counted by hand (see q2c_ring.hip): M0 carries the wave-uniform LDS byte address, lane l lands
// at M0 + 16 l; voff is a lane's byte offset from the scalar base.
__device__ __forceinline__ void ring_dma16(uint32_t voff, const char* sbase, uint32_t lds_dst) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(sbase), "s"(lds_dst)
      : "memory");
}
// two consecutive 1 KiB pieces of one operand, M0 advanced by immediates
__device__ __forceinline__ void ring_dma_pair(uint32_t v0, uint32_t v1, const char* sb, uint32_t lds_dst) {
  asm volatile(
      "s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %3\n\t"
      "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3"
      :
      : "v"(v0), "v"(v1), "s"(lds_dst), "s"(sb)
      : "memory", "scc");
}
// four consecutive 1 KiB pieces of one operand
__device__ __forceinline__ void ring_dma_quad(uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3, const char* sb,
                                              uint32_t lds_dst) {
  asm volatile(
      "s_mov_b32 m0, %4\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %5\n\t"
      "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %5\n\t"
      "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %5\n\t"
      "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %3, %5"
      :
      : "v"(v0), "v"(v1), "v"(v2), "v"(v3), "s"(lds_dst), "s"(sb)
      : "memory", "scc");
}

// first K chunk of a tile / segment: C = 0 as an inline constant (no 128 v_mov to clear the accumulators)
template <typename T> struct RingInit;
template <> struct RingInit<float> {
  __device__ static __forceinline__ void chunk(f32x4& acc, const uint4& a, const uint4& b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.x), __uint_as_float(b.x), f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.y), __uint_as_float(b.y), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.z), __uint_as_float(b.z), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.w), __uint_as_float(b.w), acc, 0, 0, 0);
  }
};
template <> struct RingInit<bf16_t> {
  __device__ static __forceinline__ void chunk(f32x4& acc, const uint4& a, const uint4& b) {
    union { uint4 u; bf16x8_v v; } ua, ub;
    ua.u = a; ub.u = b;
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ua.v, ub.v, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
  }
};
template <> struct RingInit<f16_t> {
  __device__ static __forceinline__ void chunk(f32x4& acc, const uint4& a, const uint4& b) {
    union { uint4 u; f16x8_v v; } ua, ub;
    ua.u = a; ub.u = b;
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ua.v, ub.v, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
  }
};

// the 16 bytes of `v` in the lane a DPP control word selects (row_shr:1 0x111, row_shl:1 0x101, ...)
template <int CTRL>
__device__ __forceinline__ uint4 ring_dpp_u4(const uint4& v) {
  uint4 r;
  r.x = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v.x, CTRL, 0xf, 0xf, false);
  r.y = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v.y, CTRL, 0xf, 0xf, false);
  r.z = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v.z, CTRL, 0xf, 0xf, false);
  r.w = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v.w, CTRL, 0xf, 0xf, false);
  return r;
}

// lane id from the hardware, as a VOLATILE asm: neither hoisted out of the tile / segment loop nor kept live across the K
// loop (246-256 VGPRs there; a spilled lane id returns through a scratch load whose s_waitcnt vmcnt(0) drains the DMA stream)
__device__ __forceinline__ int ring_lane_now() {
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return l;
}

// bank swizzle of a slot row's four 16-byte pieces
__device__ __forceinline__ int ring_swz(int row) { return (0x78 >> (((row >> 2) & 3) << 1)) & 3; }
