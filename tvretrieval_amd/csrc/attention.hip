// K3/K4/K5: multi-head attention of the XML encoders.
//   reference: BertSelfAttention.forward   xml/model_components.py:266-303
//              BertAttention.forward       xml/model_components.py:207-216
//              cross_context_encoder       xml/model_xml.py:357-373
//              get_modularized_queries     xml/model_xml.py:410-423
//
// Attention core: one workgroup (4 waves) per (sequence, head).  L <= 128, so the whole K tile, then the
// whole V^T tile, live in LDS and the L x L score tile lives in registers (16-row query tiles, two per wave):
//   phase A  S = Q K^T  (MFMA, K rows from LDS)  ->  s/sqrt(dh) + (1-mask)*-1e4  ->  softmax in registers
//   phase B  O = P V    (P through a per-wave LDS patch to reach the A-operand layout, V^T rows from LDS)
// Statistics and accumulation are f32 for both storage types.
#include <type_traits>

#include "gemm.h"
#include "internal.h"

template <typename T> struct ChunkOf { static constexpr int elems = 64 / (int)sizeof(T); };  // K elems per MFMA chunk

// gfx950 LDS transpose read: within each 16-lane group, lane i passes the address of 4 consecutive 16-bit elements --
// row (i >> 2), columns 4 (i & 3) .. + 3 of a [4 rows][16 columns] block (any row stride) -- and receives COLUMN i of
// rows 0..3 (probed: tools/microbench/tr_probe.hip).  With V kept row-major [key][dh] in LDS, two such reads give a lane
// the 8 consecutive keys of its dh column = the B operand of v_mfma_f32_16x16x32_bf16 for P V, no transposed copy of V.
typedef short xml_v4s __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint2 lds_read_tr16(const char* p) {
  const xml_v4s r = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) xml_v4s*)p);
  return __builtin_bit_cast(uint2, r);
}

#ifdef XML_DEBUG_VARIANTS
__device__ unsigned long long g_attn_probe[16];
extern "C" int xml_debug_read_attn_probe(unsigned long long* host_out) {
  return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_attn_probe), sizeof(unsigned long long) * 16) == hipSuccess ? 0 : -4;
}
#define XML_ATTN_PROBE(i) do { if (abl == 8 && blockIdx.x == 1 && blockIdx.y == 300 && threadIdx.x == 64) g_attn_probe[i] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define XML_ATTN_PROBE(i) do { } while (0)
#endif

template <typename T, typename OutT, int DH>
__global__ __launch_bounds__(256) void attention_core_kernel(const T* __restrict__ Q, int ldq,
                                                             const T* __restrict__ Kp, int ldk,
                                                             const T* __restrict__ Vp, int ldv,
                                                             const float* __restrict__ q_mask,
                                                             const float* __restrict__ k_mask, OutT* __restrict__ out,
                                                             int ldo, int lq, int lk, float inv_div_unused,
                                                             float sqrt_dh) {
  constexpr int CE = ChunkOf<T>::elems;       // 32 (bf16) / 16 (f32)
  constexpr int VEC = 16 / (int)sizeof(T);    // elements per 16-byte vector
  constexpr int DCH = DH / CE;                // chunks along dh
  constexpr int DT16 = DH / 16;               // 16-wide output tiles along dh
  constexpr int MAXNT = 8;                    // key tiles of 16 (L <= 128)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int abl = (int)inv_div_unused;        // timing ablations (debug build only): 1 no output stores, 2 no phase B,
                                              // 3 no exp / division in the softmax, 4 no P patch writes
  // head fastest: the heads of one sequence run side by side and read neighbouring 2*DH-byte pieces of the same rows of
  // the projected Q / K / V at about the same time (with the sequence index fastest, each head's pass touched a third of
  // every 128-byte-line triple of a row long after the other heads had)
  const int head = blockIdx.x, n = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  const int lkp = (lk + CE - 1) / CE * CE;    // keys padded to the MFMA K chunk
  const int nkt = (lk + 15) / 16;             // key tiles that hold at least one real key
  const int k_stride = DH * (int)sizeof(T) + 16;     // bytes, +16 keeps ds_read_b128 conflict-free
  const int vt_stride = lkp * (int)sizeof(T) + 16;
  // bf16: V stays row-major [key][dh] (16-byte stores) and phase B reads it with ds_read_b64_tr_b16.  (The transposed
  // copy V^T was written element by element: (c * 8 + e) * 272 bytes + 2 r puts the 24 lanes of a key row on ONE bank --
  // 96 such ds_write_b16 per thread, about a quarter of this kernel's time.)  f32 keeps the transposed copy.
  constexpr bool TR = sizeof(T) == 2;
  const int kv_bytes = TR ? lkp * k_stride : max(((lk + 15) / 16 * 16) * k_stride, DH * vt_stride);
  char* s_kv = smem;
  char* s_p = smem + kv_bytes + wave * (16 * vt_stride);

  const T* qbase = Q + (int64_t)n * lq * ldq + head * DH;
  const T* kbase = Kp + (int64_t)n * lk * ldk + head * DH;
  const T* vbase = Vp + (int64_t)n * lk * ldv + head * DH;
  XML_ATTN_PROBE(0);

  // ---- stage K rows ------------------------------------------------------------------------------
  // All global loads of a tile are issued before the first LDS store (register batch): written as load -> store per
  // iteration, hipcc serialised them (one s_waitcnt vmcnt(0) per 16-byte load: 12 memory round trips for K, 12 for V, 6
  // per query tile -- most of this kernel's time).  V does not depend on the scores: it is fetched here as well and lands
  // while phase A runs.
  constexpr int VPR = DH / VEC;                // 16-byte vectors per row
  constexpr int NVB = 128 * VPR / 256;         // vectors per thread of a full 128-row tile
  {
    const int rows16 = (lk + 15) / 16 * 16;
    uint4 kb[NVB];
#pragma unroll
    for (int j = 0; j < NVB; ++j) {
      const int i = tid + j * 256;
      const int r = i / VPR, c = i % VPR;
      kb[j] = make_uint4(0, 0, 0, 0);
      if (r < lk && abl != 6) kb[j] = ld_global16(kbase + (int64_t)r * ldk + c * VEC);
    }
#pragma unroll
    for (int j = 0; j < NVB; ++j) {
      const int i = tid + j * 256;
      const int r = i / VPR, c = i % VPR;
      if (r < rows16) *reinterpret_cast<uint4*>(s_kv + r * k_stride + c * 16) = kb[j];
    }
  }
  uint4 vb[NVB];
#pragma unroll
  for (int j = 0; j < NVB; ++j) {
    const int i = tid + j * 256;
    const int r = i / VPR, c = i % VPR;
    vb[j] = make_uint4(0, 0, 0, 0);
    if (r < lk && abl != 6) vb[j] = ld_global16(vbase + (int64_t)r * ldv + c * VEC);
  }
  // the query fragments of both tiles of this wave are fetched here too: one memory round trip for K, V and Q instead of
  // K / V, then Q of tile 0, then Q of tile 1 one after the other behind the barrier
  const int nqt = (lq + 15) / 16;
  uint4 qa_all[2][DCH];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int qrow = (wave + t * 4) * 16 + fr;
#pragma unroll
    for (int c = 0; c < DCH; ++c) {
      qa_all[t][c] = make_uint4(0, 0, 0, 0);
      if (wave + t * 4 < nqt && qrow < lq && abl != 6) qa_all[t][c] = ld_global16(qbase + (int64_t)qrow * ldq + c * CE + fg * VEC);
    }
  }
  // the masks ride the same round trip (they were dependent global loads in the middle of phase A): key mask of this
  // lane's 8 columns (the same for both query tiles), query mask of its 2 x 4 rows (cross-attention only)
  float km[MAXNT], qmk[2][4];
#pragma unroll
  for (int j = 0; j < MAXNT; ++j) {
    const int col = j * 16 + fr;
    km[j] = (col < lk) ? k_mask[(int64_t)n * lk + col] : 0.f;
  }
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = (wave + t * 4) * 16 + fg * 4 + r;
      qmk[t][r] = (q_mask && row < lq) ? q_mask[(int64_t)n * lq + row] : 1.f;
    }
  XML_ATTN_PROBE(1);
  __syncthreads();
  XML_ATTN_PROBE(2);

  if (abl == 7) {      // loads + K staging only
    if (vb[0].x == 0x12345678u && qa_all[0][0].x == 0x9abcdefu) out[0] = (OutT)0;
    return;
  }
  // ---- phase A: scores + softmax, two query tiles per wave -----------------------------------------
  f32x4 p[2][MAXNT];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int qt = wave + t * 4;
#pragma unroll
    for (int j = 0; j < MAXNT; ++j) p[t][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (qt >= nqt) continue;
    const uint4 (&qa)[DCH] = qa_all[t];
    if (nkt == MAXNT) {
      // full-length sequences (the corpus-encode shape): no per-tile branch.  With `if (j < nkt)` around every MFMA each
      // ds_read_b128 sat in its own basic block behind an `s_waitcnt lgkmcnt(0)` -- the LDS latency was paid 48 times
      // per query tile (the phase probe: 18 K cycles for 96 MFMAs); here the reads of a chunk are issued as a batch
#pragma unroll
      for (int c = 0; c < DCH; ++c) {
        uint4 b[MAXNT];
#pragma unroll
        for (int j = 0; j < MAXNT; ++j)
          b[j] = *reinterpret_cast<const uint4*>(s_kv + (j * 16 + fr) * k_stride + c * 64 + fg * 16);
#pragma unroll
        for (int j = 0; j < MAXNT; ++j) Mma<T>::chunk(p[t][j], qa[c], b[j]);
      }
    } else {
#pragma unroll
      for (int c = 0; c < DCH; ++c) {
#pragma unroll
        for (int j = 0; j < MAXNT; ++j) {
          if (j < nkt) {
            const uint4 b = *reinterpret_cast<const uint4*>(s_kv + (j * 16 + fr) * k_stride + c * 64 + fg * 16);
            Mma<T>::chunk(p[t][j], qa[c], b);
          }
        }
      }
    }
    // element (row = fg*4 + r, col = j*16 + fr).  f32 storage (the parity configuration) keeps the reference's exact
    // operations (x / sqrt(dh), expf, p / sum); bf16 storage -- whose outputs are rounded to 8 mantissa bits anyway --
    // multiplies by reciprocals and uses the hardware exp2 (v_exp_f32): the three slow-path math calls per element were a
    // third of this kernel's compute time
    constexpr bool FAST = sizeof(T) == 2;
    const float inv_sqrt_dh = 1.0f / sqrt_dh;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float qm = qmk[t][r];
      float mx = -INFINITY;
#pragma unroll
      for (int j = 0; j < MAXNT; ++j) {
        const int col = j * 16 + fr;
        float s = -INFINITY;
        if (col < lk) s = (FAST ? p[t][j][r] * inv_sqrt_dh : p[t][j][r] / sqrt_dh) + (1.f - qm * km[j]) * -10000.f;
        p[t][j][r] = s;
        mx = fmaxf(mx, s);
      }
      mx = lane16_max_dpp(mx);      // DPP row rotations: the __shfl_xor form goes through the LDS crossbar (ds_bpermute)
      float sum = 0.f;
#pragma unroll
      for (int j = 0; j < MAXNT; ++j) {
        const float x = p[t][j][r] - mx;       // exp(-inf) = 0 for padded key columns
        const float e = abl == 3 ? x : FAST ? __builtin_amdgcn_exp2f(x * 1.4426950408889634f) : expf(x);
        p[t][j][r] = e;
        sum += e;
      }
      sum = lane16_sum_dpp(sum);
      const float inv_sum = 1.0f / sum;
#pragma unroll
      for (int j = 0; j < MAXNT; ++j) p[t][j][r] = abl == 3 ? p[t][j][r] : FAST ? p[t][j][r] * inv_sum : p[t][j][r] / sum;
    }
  }
  XML_ATTN_PROBE(3);
  __syncthreads();
  XML_ATTN_PROBE(4);

  // ---- stage V (bf16: row-major; f32: V^T) over K from the registers fetched above --------------------
  if constexpr (TR) {
#pragma unroll
    for (int j = 0; j < NVB; ++j) {
      const int i = tid + j * 256;
      const int r = i / VPR, c = i % VPR;  // key r, dh vector c; rows lk..lkp-1 are the zeros loaded above
      if (r < lkp) *reinterpret_cast<uint4*>(s_kv + r * k_stride + c * 16) = vb[j];
    }
  } else {
#pragma unroll
    for (int j = 0; j < NVB; ++j) {
      const int i = tid + j * 256;
      const int r = i / VPR, c = i % VPR;  // key r, dh vector c
      if (r < lkp) {
        float vals[VEC];
        unpack16<T>(vb[j], vals);
#pragma unroll
        for (int e = 0; e < VEC; ++e)
          DT<T>::st(reinterpret_cast<T*>(s_kv + (c * VEC + e) * vt_stride) + r, vals[e]);
      }
    }
  }
  __syncthreads();
  XML_ATTN_PROBE(5);

  // ---- phase B: O = P V ----------------------------------------------------------------------------
  const int nkc = lkp / CE;
  if (abl == 2) return;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int qt = wave + t * 4;
    if (qt >= nqt) continue;
    // P (C layout) -> per-wave LDS patch [16][lkp] as T
#pragma unroll
    for (int j = 0; j < MAXNT; ++j) {
      const int col = j * 16 + fr;
      if (col < lkp && abl != 4) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          DT<T>::st(reinterpret_cast<T*>(s_p + (fg * 4 + r) * vt_stride) + col, p[t][j][r]);
      }
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the patch is wave-private, no block barrier needed
    __builtin_amdgcn_wave_barrier();
    f32x4 o[DT16];
#pragma unroll
    for (int d = 0; d < DT16; ++d) o[d] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < nkc; ++c) {
      const uint4 a = *reinterpret_cast<const uint4*>(s_p + fr * vt_stride + c * 64 + fg * 16);
      if constexpr (TR) {
        // keys c*32 + fg*8 + 0..7 of dh column d*16 + fr: two transpose reads of [4 keys][16 dh] blocks
        const char* vb0 = s_kv + (c * 32 + fg * 8 + (fr >> 2)) * k_stride + (fr & 3) * 8;
#pragma unroll
        for (int d = 0; d < DT16; ++d) {
          const uint2 lo = lds_read_tr16(vb0 + d * 32), hi = lds_read_tr16(vb0 + d * 32 + 4 * k_stride);
          Mma<T>::chunk(o[d], a, make_uint4(lo.x, lo.y, hi.x, hi.y));
        }
      } else {
#pragma unroll
        for (int d = 0; d < DT16; ++d) {
          const uint4 b = *reinterpret_cast<const uint4*>(s_kv + (d * 16 + fr) * vt_stride + c * 64 + fg * 16);
          Mma<T>::chunk(o[d], a, b);
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
    if (abl == 1 && o[0][0] != 12345.678f) continue;
    // (bf16 out through the freed P patch as 16-byte stores was measured: 576 us per 2048-video call against 391 us for
    // these 2-byte stores -- the extra LDS round trip and two wave barriers per half cost more than the write path saves)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = qt * 16 + fg * 4 + r;
      if (row >= lq) continue;
      OutT* po = out + ((int64_t)n * lq + row) * ldo + head * DH;
#pragma unroll
      for (int d = 0; d < DT16; ++d) DT<OutT>::st(po + d * 16 + fr, o[d][r]);
    }
  }
  XML_ATTN_PROBE(6);
}

// Short sequences (lq, lk <= 32: the query encoder, 30 tokens): ONE WAVE per (sequence, head), four independent units
// per workgroup.  The 4-wave kernel above leaves two of its waves without a query tile at lq <= 32 and synchronises
// the block twice; here a wave stages its own K tile / V^T tile in its private LDS region and never meets a block
// barrier (wave-level ordering only).  Same arithmetic, same order of operations per output element.
template <typename T, typename OutT, int DH>
__global__ __launch_bounds__(256) void attention_core_small_kernel(const T* __restrict__ Q, int ldq,
                                                                   const T* __restrict__ Kp, int ldk,
                                                                   const T* __restrict__ Vp, int ldv,
                                                                   const float* __restrict__ q_mask,
                                                                   const float* __restrict__ k_mask,
                                                                   OutT* __restrict__ out, int ldo, int lq, int lk,
                                                                   int n_heads, int64_t n_units, float sqrt_dh,
                                                                   const int32_t* __restrict__ cu) {
  // cu != NULL (packed / variable-length self-attention, xml_attention_block_varlen): sequence n is rows cu[n] .. cu[n+1]-1
  // of Q / K / V / out, every key valid; lq == lk is then the LONGEST sequence (it sizes the LDS strides), the unit's own
  // length drives the loads, the masks and the loops.
  constexpr int CE = ChunkOf<T>::elems;
  constexpr int VEC = 16 / (int)sizeof(T);
  constexpr int DCH = DH / CE;
  constexpr int DT16 = DH / 16;
  constexpr int NT = 2;                       // key tiles of 16 (lk <= 32)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t unit = (int64_t)blockIdx.x * 4 + wave;
  if (unit >= n_units) return;                // (no block barrier below)
  const int64_t n = unit / n_heads;
  const int head = (int)(unit - n * n_heads);
  const int fr = lane & 15, fg = lane >> 4;
  const int lkp_max = (lk + CE - 1) / CE * CE;
  int64_t row_q = n * lq, row_k = n * lk;       // first row of this unit's sequence in Q / out and in K / V
  if (cu) {
    const int r0 = __builtin_amdgcn_readfirstlane(cu[n]), r1 = __builtin_amdgcn_readfirstlane(cu[n + 1]);
    row_q = row_k = r0;
    lq = lk = r1 - r0;
  }
  const int lkp = (lk + CE - 1) / CE * CE;
  const int nkt = (lk + 15) / 16;
  const int k_stride = DH * (int)sizeof(T) + 16;
  const int vt_stride = lkp_max * (int)sizeof(T) + 16;
  constexpr bool TR = sizeof(T) == 2;         // bf16: V stays row-major, P V reads it with ds_read_b64_tr_b16 (see above)
  const int kv_bytes = TR ? 32 * k_stride : max(32 * k_stride, DH * vt_stride);
  const int wave_bytes = kv_bytes + 16 * vt_stride;
  char* s_kv = smem + wave * wave_bytes;
  char* s_p = s_kv + kv_bytes;
  auto wave_sync = [&]() {
    __builtin_amdgcn_s_waitcnt(0xc07f);       // lgkmcnt(0)
    __builtin_amdgcn_wave_barrier();
  };

  const T* qbase = Q + row_q * ldq + head * DH;
  const T* kbase = Kp + row_k * ldk + head * DH;
  const T* vbase = Vp + row_k * ldv + head * DH;

  constexpr int VPR = DH / VEC;               // 16-byte vectors per row
  constexpr int NV = 32 * VPR / 64;           // vectors per lane of a 32-row tile
  {   // K rows -> LDS.  All loads of the tile are issued before the first store: one memory round trip, not NV
    uint4 buf[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int i = lane + j * 64;
      const int r = i / VPR, c = i % VPR;
      buf[j] = make_uint4(0, 0, 0, 0);
      if (r < lk) buf[j] = ld_global16(kbase + (int64_t)r * ldk + c * VEC);
    }
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int i = lane + j * 64;
      const int r = i / VPR, c = i % VPR;
      *reinterpret_cast<uint4*>(s_kv + r * k_stride + c * 16) = buf[j];
    }
  }
  // Q fragments of both query tiles and V (independent of the scores): fetched now, they arrive while K is staged /
  // phase A runs
  uint4 qa[2][DCH];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int c = 0; c < DCH; ++c) {
      const int qrow = t * 16 + fr;
      qa[t][c] = make_uint4(0, 0, 0, 0);
      if (qrow < lq) qa[t][c] = ld_global16(qbase + (int64_t)qrow * ldq + c * CE + fg * VEC);
    }
  uint4 vbuf[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int i = lane + j * 64;
    const int r = i / VPR, c = i % VPR;
    vbuf[j] = make_uint4(0, 0, 0, 0);
    if (r < lk) vbuf[j] = ld_global16(vbase + (int64_t)r * ldv + c * VEC);
  }
  wave_sync();

  f32x4 p[2][NT];
  constexpr bool FAST = sizeof(T) == 2;       // bf16 storage: reciprocals + v_exp_f32, as in attention_core_kernel
  const float inv_sqrt_dh = 1.0f / sqrt_dh;
  const int nqt = (lq + 15) / 16;
  float km[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int col = j * 16 + fr;
    km[j] = (col < lk) ? (cu ? 1.f : k_mask[row_k + col]) : 0.f;
  }
#pragma unroll
  for (int t = 0; t < 2; ++t) {
#pragma unroll
    for (int j = 0; j < NT; ++j) p[t][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (t >= nqt) continue;
#pragma unroll
    for (int c = 0; c < DCH; ++c) {
#pragma unroll
      for (int j = 0; j < NT; ++j) {      // (no `j < nkt` branch: K rows beyond lk are zeros in LDS, their scores are masked)
        const uint4 b = *reinterpret_cast<const uint4*>(s_kv + (j * 16 + fr) * k_stride + c * 64 + fg * 16);
        Mma<T>::chunk(p[t][j], qa[t][c], b);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = t * 16 + fg * 4 + r;
      const float qm = (q_mask && row < lq) ? q_mask[row_q + row] : 1.f;
      float mx = -INFINITY;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int col = j * 16 + fr;
        float sc = -INFINITY;
        if (col < lk) sc = (FAST ? p[t][j][r] * inv_sqrt_dh : p[t][j][r] / sqrt_dh) + (1.f - qm * km[j]) * -10000.f;
        p[t][j][r] = sc;
        mx = fmaxf(mx, sc);
      }
      mx = lane16_max_dpp(mx);      // DPP row rotations: the __shfl_xor form goes through the LDS crossbar (ds_bpermute)
      float sum = 0.f;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const float x = p[t][j][r] - mx;
        const float e = FAST ? __builtin_amdgcn_exp2f(x * 1.4426950408889634f) : expf(x);
        p[t][j][r] = e;
        sum += e;
      }
      sum = lane16_sum_dpp(sum);
      const float inv_sum = 1.0f / sum;
#pragma unroll
      for (int j = 0; j < NT; ++j) p[t][j][r] = FAST ? p[t][j][r] * inv_sum : p[t][j][r] / sum;
    }
  }
  wave_sync();                                // every lane is done reading K

  if constexpr (TR) {   // V rows -> LDS as they are (16-byte stores), over K
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int i = lane + j * 64;
      const int r = i / VPR, c = i % VPR;
      *reinterpret_cast<uint4*>(s_kv + r * k_stride + c * 16) = vbuf[j];      // rows >= lk: the zeros loaded above
    }
  } else {   // V^T -> LDS (overwrites K); rows lk .. lkp-1 are zero (lkp <= 32)
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int i = lane + j * 64;
      const int r = i / VPR, c = i % VPR;
      if (r < lkp) {
        float vals[VEC];
        unpack16<T>(vbuf[j], vals);
#pragma unroll
        for (int e = 0; e < VEC; ++e)
          DT<T>::st(reinterpret_cast<T*>(s_kv + (c * VEC + e) * vt_stride) + r, vals[e]);
      }
    }
  }
  wave_sync();

  const int nkc = lkp / CE;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    if (t >= nqt) continue;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int col = j * 16 + fr;
      if (col < lkp) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          DT<T>::st(reinterpret_cast<T*>(s_p + (fg * 4 + r) * vt_stride) + col, p[t][j][r]);
      }
    }
    wave_sync();
    f32x4 o[DT16];
#pragma unroll
    for (int d = 0; d < DT16; ++d) o[d] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < nkc; ++c) {
      const uint4 a = *reinterpret_cast<const uint4*>(s_p + fr * vt_stride + c * 64 + fg * 16);
      if constexpr (TR) {
        const char* vb0 = s_kv + (c * 32 + fg * 8 + (fr >> 2)) * k_stride + (fr & 3) * 8;
#pragma unroll
        for (int d = 0; d < DT16; ++d) {
          const uint2 lo = lds_read_tr16(vb0 + d * 32), hi = lds_read_tr16(vb0 + d * 32 + 4 * k_stride);
          Mma<T>::chunk(o[d], a, make_uint4(lo.x, lo.y, hi.x, hi.y));
        }
      } else {
#pragma unroll
        for (int d = 0; d < DT16; ++d) {
          const uint4 b = *reinterpret_cast<const uint4*>(s_kv + (d * 16 + fr) * vt_stride + c * 64 + fg * 16);
          Mma<T>::chunk(o[d], a, b);
        }
      }
    }
    wave_sync();                              // the patch is rewritten by the next query tile
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = t * 16 + fg * 4 + r;
      if (row >= lq) continue;
      OutT* po = out + (row_q + row) * ldo + head * DH;
#pragma unroll
      for (int d = 0; d < DT16; ++d) DT<OutT>::st(po + d * 16 + fr, o[d][r]);
    }
  }
}

template <typename T, typename OutT, int DH>
static int launch_attn(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const float* q_mask,
                       const float* k_mask, void* out, int64_t n, int lq, int lk, int hidden, int n_heads,
                       bool small, hipStream_t st) {
  if (small) {
    const size_t lds_s = dispatch::attn_small_lds_bytes(lk, DH, DT<T>::id);
    auto ks = attention_core_small_kernel<T, OutT, DH>;
    if (lds_s > 64 * 1024 && !xml_lds_attr_once<attention_core_small_kernel<T, OutT, DH>>(dispatch::LDS_BYTES))
      return XML_ERR_LAUNCH;
    const int64_t units = n * n_heads;
    const dim3 grid((unsigned)((units + dispatch::ATTN_SMALL_UNITS - 1) / dispatch::ATTN_SMALL_UNITS));
    hipLaunchKernelGGL(ks, grid, dim3(256), lds_s, st, (const T*)q, ldq, (const T*)k, ldk, (const T*)v, ldv, q_mask, k_mask,
                       (OutT*)out, hidden, lq, lk, n_heads, units, sqrtf((float)DH), (const int32_t*)nullptr);
    XML_CHECK_LAUNCH();
    return XML_OK;
  }
  const size_t lds = dispatch::attn_lds_bytes(lk, DH, DT<T>::id);
  auto kern = attention_core_kernel<T, OutT, DH>;
  if (lds > 64 * 1024 && !xml_lds_attr_once<attention_core_kernel<T, OutT, DH>>(dispatch::LDS_BYTES)) return XML_ERR_LAUNCH;
  // (debug build: g_q2c_ablation selects a timing ablation inside the kernel; constant 0 in the product build)
  hipLaunchKernelGGL(kern, dim3(n_heads, (unsigned)n), dim3(256), lds, st, (const T*)q, ldq, (const T*)k, ldk,
                     (const T*)v, ldv, q_mask, k_mask, (OutT*)out, hidden, lq, lk, (float)g_q2c_ablation,
                     sqrtf((float)DH));
  XML_CHECK_LAUNCH();
  return XML_OK;
}

template <typename T, typename OutT>
static int dispatch_attn_dh(int dh, const void* q, int ldq, const void* k, int ldk, const void* v, int ldv,
                            const float* q_mask, const float* k_mask, void* out, int64_t n, int lq, int lk,
                            int hidden, int n_heads, bool small, hipStream_t st) {
#define XML_ATTN_CASE(D)                                                                                     \
  case D:                                                                                                    \
    return launch_attn<T, OutT, D>(q, ldq, k, ldk, v, ldv, q_mask, k_mask, out, n, lq, lk, hidden, n_heads, \
                                   small, st);
  switch (dh) {
    XML_ATTN_HEAD_SIZES(XML_ATTN_CASE)
    default:
      return XML_ERR_UNSUPPORTED;
  }
#undef XML_ATTN_CASE
}

int xmli_attention_core(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const float* q_mask,
                        const float* k_mask, void* out, int out_f32, int64_t n, int lq, int lk, int hidden,
                        int n_heads, int dt, hipStream_t st) {
  XML_ENTER();
  if (n <= 0 || lq <= 0 || lk <= 0) return XML_ERR_BAD_ARG;
  const int form = dispatch::attn_kernel(lq, lk, hidden, n_heads, dt);
  if (form == XML_ATTN_REFUSED_HEADS) return XML_ERR_BAD_ARG;
  if (form == XML_ATTN_REFUSED_LENGTH || form == XML_ATTN_REFUSED_LDS) return XML_ERR_UNSUPPORTED;
  const int dh = hidden / n_heads;
  const bool small = form == XML_ATTN_SMALL;      // (XML_ATTN_REFUSED_DH: no case of the switch on dh)
  if (dt == XML_F32)
    return dispatch_attn_dh<float, float>(dh, q, ldq, k, ldk, v, ldv, q_mask, k_mask, out, n, lq, lk, hidden,
                                          n_heads, small, st);
  if (dt == XML_BF16) {
    if (out_f32)
      return dispatch_attn_dh<bf16_t, float>(dh, q, ldq, k, ldk, v, ldv, q_mask, k_mask, out, n, lq, lk, hidden,
                                             n_heads, small, st);
    return dispatch_attn_dh<bf16_t, bf16_t>(dh, q, ldq, k, ldk, v, ldv, q_mask, k_mask, out, n, lq, lk, hidden,
                                            n_heads, small, st);
  }
  return XML_ERR_BAD_ARG;
}

// public: the attention core alone -- BertSelfAttention.forward behind its three projections
extern "C" int xml_attention_core(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, const float* q_mask,
                                  const float* k_mask, void* out, int64_t n, int lq, int lk, int hidden, int n_heads, int dt,
                                  xml_stream_t stream) {
  XML_ENTER();
  if (!q || !k || !v || !k_mask || !out) return XML_ERR_BAD_ARG;
  if (dt != XML_F32 && dt != XML_BF16) return XML_ERR_BAD_ARG;
  if (ldq < hidden || ldk < hidden || ldv < hidden || (ldq | ldk | ldv | hidden) % 8) return XML_ERR_UNSUPPORTED;
  return xmli_attention_core(q, ldq, k, ldk, v, ldv, q_mask, k_mask, out, 0, n, lq, lk, hidden, n_heads, dt,
                             (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------------
// public: BertAttention block.   ws = [ qkv (rows x 3H) dt | att (rows x H) dt | pre-LN (rows x H) f32 ]
// ---------------------------------------------------------------------------------------------------
extern "C" size_t xml_attention_block_workspace_bytes(int64_t n, int seq_len, int hidden, int dt) {
  const size_t rows = (size_t)n * seq_len;
  const size_t pre = align_up(rows * hidden * 4, 256);      // f32 pre-LN rows, or the fused epilogue's per-workgroup scratch
  const size_t lnw = dispatch::gemm_ln_fused((int64_t)rows, hidden, hidden, dt) ? xmli_gemm_ln_workspace_bytes((int64_t)rows, hidden) : 0;
  return align_up(rows * 3 * hidden * dt_size(dt), 256) + align_up(rows * hidden * dt_size(dt), 256) +
         (pre > lnw ? pre : lnw) + xmli_gemm_split_ws_bytes((int64_t)rows, hidden, dt);
}

extern "C" int xml_attention_block(const void* x, const float* key_mask, const void* wqkv, const float* bqkv,
                                   const void* wo, const float* bo, const float* ln_g, const float* ln_b, void* y,
                                   int64_t n, int seq_len, int hidden, int n_heads, int dt, void* ws, size_t ws_bytes,
                                   xml_stream_t stream) {
  XML_ENTER();
  if (!x || !key_mask || !wqkv || !bqkv || !wo || !bo || !ln_g || !ln_b || !y || !ws) return XML_ERR_BAD_ARG;
  if (n <= 0 || seq_len <= 0 || !xmli_model_dt_ok(dt)) return XML_ERR_BAD_ARG;
  if (seq_len > dispatch::ATTN_MAX_L || hidden % 8) return XML_ERR_UNSUPPORTED;
  if (ws_bytes < xml_attention_block_workspace_bytes(n, seq_len, hidden, dt)) return XML_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int64_t rows = n * seq_len;
  const int adt = xmli_act_dt(dt);              // XML_F16S: f32 activations, split-f16 projections
  char* qkv = (char*)ws;
  char* att = qkv + align_up((size_t)rows * 3 * hidden * dt_size(dt), 256);
  char* pre = att + align_up((size_t)rows * hidden * dt_size(dt), 256);
  char* sws = dt == XML_F16S ? (char*)ws + xml_attention_block_workspace_bytes(n, seq_len, hidden, dt) -
                                   xmli_gemm_split_ws_bytes(rows, hidden, dt) : nullptr;
  int rc = xmli_gemm(x, wqkv, bqkv, nullptr, qkv, rows, 3 * hidden, hidden, 0, 0, 1, 0, dt, st, sws);
  if (rc) return rc;
  const size_t es = dt_size(dt);
  rc = xmli_attention_core(qkv, 3 * hidden, qkv + (size_t)hidden * es, 3 * hidden, qkv + (size_t)2 * hidden * es,
                           3 * hidden, nullptr, key_mask, att, 0, n, seq_len, seq_len, hidden, n_heads, adt, st);
  if (rc) return rc;
  if (dispatch::gemm_ln_fused(rows, hidden, hidden, dt) && y != x &&   // BertSelfOutput: dense + residual + LayerNorm in one launch
      xmli_gemm_ln(att, wo, bo, x, ln_g, ln_b, y, rows, hidden, hidden, 0, /*residual*/ 2, 1, dt, pre, st) == XML_OK)
    return XML_OK;
  rc = xmli_gemm(att, wo, bo, x, pre, rows, hidden, hidden, 0, /*residual*/ 2, 1, /*out_f32*/ 1, dt, st, sws);
  if (rc) return rc;
  return xmli_gemm_ln_tail((const float*)pre, ln_g, ln_b, y, rows, hidden, dt, st);
}

// ---------------------------------------------------------------------------------------------------
// public: BertAttention block on PACKED variable-length sequences (the query encoder without its padding rows).
//   x / y (rows, hidden): the valid tokens of n sequences back to back, sequence i = rows cu[i] .. cu[i+1]-1, every
//   sequence 1 .. max_len <= 32 tokens long.  Same arithmetic per valid token as xml_attention_block on the padded batch:
//   the projections and the LayerNorm are row-wise, and a padded key contributes exp(-10000 + s - max) = +0 to the softmax
//   and 0 * v to P V, so dropping it changes nothing.   ws = [ qkv | att | pre-LN f32 or the fused epilogue's scratch ] as above.
// ---------------------------------------------------------------------------------------------------
template <typename T, int DH>
static int launch_attn_varlen(const char* qkv, int hidden, const int32_t* cu, void* att, int64_t n, int max_len,
                              int n_heads, int dt, hipStream_t st) {
  const size_t lds_s = dispatch::attn_small_lds_bytes(max_len, DH, dt);
  if (lds_s > (size_t)dispatch::LDS_BYTES) return XML_ERR_UNSUPPORTED;
  if (lds_s > 64 * 1024 && !xml_lds_attr_once<attention_core_small_kernel<T, T, DH>>(dispatch::LDS_BYTES)) return XML_ERR_LAUNCH;
  const int64_t units = n * n_heads;
  const T* q = (const T*)qkv;
  const dim3 grid((unsigned)((units + dispatch::ATTN_SMALL_UNITS - 1) / dispatch::ATTN_SMALL_UNITS));
  hipLaunchKernelGGL((attention_core_small_kernel<T, T, DH>), grid, dim3(256), lds_s, st, q,
                     3 * hidden, q + hidden, 3 * hidden, q + 2 * hidden, 3 * hidden, (const float*)nullptr,
                     (const float*)nullptr, (T*)att, hidden, max_len, max_len, n_heads, units, sqrtf((float)DH), cu);
  XML_CHECK_LAUNCH();
  return XML_OK;
}

extern "C" size_t xml_attention_block_varlen_workspace_bytes(int64_t rows, int hidden, int dt) {
  const size_t pre = align_up((size_t)rows * hidden * 4, 256);
  const size_t lnw = dispatch::gemm_ln_fused(rows, hidden, hidden, dt) ? xmli_gemm_ln_workspace_bytes(rows, hidden) : 0;
  return align_up((size_t)rows * 3 * hidden * dt_size(dt), 256) + align_up((size_t)rows * hidden * dt_size(dt), 256) +
         (pre > lnw ? pre : lnw) + xmli_gemm_split_ws_bytes(rows, hidden, dt);
}

extern "C" int xml_attention_block_varlen(const void* x, const int32_t* cu_seqlens, const void* wqkv, const float* bqkv,
                                          const void* wo, const float* bo, const float* ln_g, const float* ln_b, void* y,
                                          int64_t rows, int64_t n, int max_len, int hidden, int n_heads, int dt, void* ws,
                                          size_t ws_bytes, xml_stream_t stream) {
  XML_ENTER();
  if (!x || !cu_seqlens || !wqkv || !bqkv || !wo || !bo || !ln_g || !ln_b || !y || !ws) return XML_ERR_BAD_ARG;
  if (rows <= 0 || n <= 0 || max_len <= 0 || n_heads <= 0 || !xmli_model_dt_ok(dt)) return XML_ERR_BAD_ARG;
  if (max_len > dispatch::ATTN_SMALL_MAX_L || hidden % 8 || hidden % n_heads) return XML_ERR_UNSUPPORTED;
  if (ws_bytes < xml_attention_block_varlen_workspace_bytes(rows, hidden, dt)) return XML_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int adt = xmli_act_dt(dt);
  char* qkv = (char*)ws;
  char* att = qkv + align_up((size_t)rows * 3 * hidden * dt_size(dt), 256);
  char* pre = att + align_up((size_t)rows * hidden * dt_size(dt), 256);
  char* sws = dt == XML_F16S ? (char*)ws + xml_attention_block_varlen_workspace_bytes(rows, hidden, dt) -
                                   xmli_gemm_split_ws_bytes(rows, hidden, dt) : nullptr;
  int rc = xmli_gemm(x, wqkv, bqkv, nullptr, qkv, rows, 3 * hidden, hidden, 0, 0, 1, 0, dt, st, sws);
  if (rc) return rc;
  const int dh = hidden / n_heads;
  rc = XML_ERR_UNSUPPORTED;
#define XML_VL_CASE(D)                                                                                              \
  case D:                                                                                                           \
    rc = adt == XML_F32 ? launch_attn_varlen<float, D>(qkv, hidden, cu_seqlens, att, n, max_len, n_heads, adt, st)    \
                        : launch_attn_varlen<bf16_t, D>(qkv, hidden, cu_seqlens, att, n, max_len, n_heads, adt, st);  \
    break;
  switch (dh) {
    XML_ATTN_HEAD_SIZES(XML_VL_CASE)
    default: break;
  }
#undef XML_VL_CASE
  if (rc) return rc;
  if (dispatch::gemm_ln_fused(rows, hidden, hidden, dt) && y != x &&
      xmli_gemm_ln(att, wo, bo, x, ln_g, ln_b, y, rows, hidden, hidden, 0, /*residual*/ 2, 1, dt, pre, st) == XML_OK)
    return XML_OK;
  rc = xmli_gemm(att, wo, bo, x, pre, rows, hidden, hidden, 0, /*residual*/ 2, 1, /*out_f32*/ 1, dt, st, sws);
  if (rc) return rc;
  return xmli_gemm_ln_tail((const float*)pre, ln_g, ln_b, y, rows, hidden, dt, st);
}

// ---------------------------------------------------------------------------------------------------
// public: cross-attention + residual LayerNorm.
//   ws = [ q (n*lq x H) dt | kv (n*lk x 2H) dt | att f32 (n*lq x H) ]
// ---------------------------------------------------------------------------------------------------
extern "C" size_t xml_cross_attention_workspace_bytes(int64_t n, int lq, int lk, int hidden, int dt) {
  return align_up((size_t)n * lq * hidden * dt_size(dt), 256) + align_up((size_t)n * lk * 2 * hidden * dt_size(dt), 256) +
         align_up((size_t)n * lq * hidden * 4, 256) + xmli_gemm_split_ws_bytes(n * (lq > lk ? lq : lk), hidden, dt);
}

extern "C" int xml_cross_attention(const void* main_x, const float* main_mask, const void* side_x,
                                   const float* side_mask, const void* wq, const float* bq, const void* wkv,
                                   const float* bkv, const float* ln_g, const float* ln_b, void* y, int64_t n, int lq,
                                   int lk, int hidden, int n_heads, int dt, void* ws, size_t ws_bytes,
                                   xml_stream_t stream) {
  XML_ENTER();
  if (!main_x || !main_mask || !side_x || !side_mask || !wq || !bq || !wkv || !bkv || !ln_g || !ln_b || !y || !ws)
    return XML_ERR_BAD_ARG;
  if (n <= 0 || lq <= 0 || lk <= 0 || !xmli_model_dt_ok(dt)) return XML_ERR_BAD_ARG;
  if (lq > dispatch::ATTN_MAX_L || lk > dispatch::ATTN_MAX_L || hidden % 8) return XML_ERR_UNSUPPORTED;
  if (ws_bytes < xml_cross_attention_workspace_bytes(n, lq, lk, hidden, dt)) return XML_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const size_t es = dt_size(dt);
  const int adt = xmli_act_dt(dt);
  char* q = (char*)ws;
  char* kv = q + align_up((size_t)n * lq * hidden * es, 256);
  char* att = kv + align_up((size_t)n * lk * 2 * hidden * es, 256);
  char* sws = dt == XML_F16S ? att + align_up((size_t)n * lq * hidden * 4, 256) : nullptr;
  int rc = xmli_gemm(main_x, wq, bq, nullptr, q, n * lq, hidden, hidden, 0, 0, 1, 0, dt, st, sws);
  if (rc) return rc;
  rc = xmli_gemm(side_x, wkv, bkv, nullptr, kv, n * lk, 2 * hidden, hidden, 0, 0, 1, 0, dt, st, sws);
  if (rc) return rc;
  rc = xmli_attention_core(q, hidden, kv, 2 * hidden, kv + (size_t)hidden * es, 2 * hidden, main_mask, side_mask, att,
                           /*out_f32*/ 1, n, lq, lk, hidden, n_heads, adt, st);
  if (rc) return rc;
  return xmli_add_layernorm(att, XML_F32, main_x, ln_g, ln_b, y, n * lq, hidden, hidden, adt, st);
}

// ---------------------------------------------------------------------------------------------------
// public: K5 modular pooling.  One workgroup per query.
// ---------------------------------------------------------------------------------------------------
// ATT (xml_modular_pool_att[_varlen], all three kernels): the softmax weights leave as well, att (n, lq, n_mod) f32 in the
// PADDED layout -- the values the weighting loop multiplies with, 0 at padded positions; nothing else changes, so the pooled
// vectors are bitwise those of the plain instantiation.
template <typename T, bool ATT = false>
__global__ __launch_bounds__(256) void modular_pool_kernel(const T* __restrict__ enc, const float* __restrict__ mask,
                                                           const float* __restrict__ wm, T* __restrict__ out,
                                                           int64_t n, int lq, int hidden, int n_mod,
                                                           float* __restrict__ att = nullptr) {
  __shared__ float s_att[2][128];
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const T* e = enc + (int64_t)q * lq * hidden;
  for (int l = wave; l < lq; l += 4) {
    for (int m = 0; m < n_mod; ++m) {
      float s = 0.f;
      for (int h = lane; h < hidden; h += 64) s += DT<T>::ld(e + (int64_t)l * hidden + h) * wm[m * hidden + h];
      s = wave_sum(s);
      if (lane == 0) {
        const float mk = mask[(int64_t)q * lq + l];
        s_att[m][l] = s * mk + (1.f - mk) * -1e10f;  // mask_logits, xml/model_xml.py:640-641
      }
    }
  }
  __syncthreads();
  if (tid < n_mod) {
    float mx = -INFINITY;
    for (int l = 0; l < lq; ++l) mx = fmaxf(mx, s_att[tid][l]);
    float sum = 0.f;
    for (int l = 0; l < lq; ++l) {
      const float ev = expf(s_att[tid][l] - mx);
      s_att[tid][l] = ev;
      sum += ev;
    }
    for (int l = 0; l < lq; ++l) s_att[tid][l] /= sum;
  }
  __syncthreads();
  if constexpr (ATT) {
    for (int i = tid; i < lq * n_mod; i += 256) att[(int64_t)q * lq * n_mod + i] = s_att[i % n_mod][i / n_mod];
  }
  for (int h = tid; h < hidden; h += 256) {
    for (int m = 0; m < n_mod; ++m) {
      float acc = 0.f;
      for (int l = 0; l < lq; ++l) acc += s_att[m][l] * DT<T>::ld(e + (int64_t)l * hidden + h);
      DT<T>::st(out + ((int64_t)m * n + q) * hidden + h, acc);
    }
  }
}

// Short sequences (lq <= 32, hidden % 8 == 0, hidden <= 1024 -- the query encoder: 30 tokens): every token row is
// read ONCE with 16-byte loads and stays in registers (a wave owns tokens wave, wave + 4, ...); scores go through
// LDS for the softmax, each wave weights its own rows, the four partial sums meet in LDS.
template <typename T, bool ATT = false>
__global__ __launch_bounds__(256) void modular_pool_small_kernel(const T* __restrict__ enc, const float* __restrict__ mask,
                                                                 const float* __restrict__ wm, T* __restrict__ out,
                                                                 int64_t n, int lq, int hidden, int n_mod,
                                                                 const int32_t* __restrict__ cu,
                                                                 float* __restrict__ att = nullptr) {
  // cu != NULL (xml_modular_pool_varlen): packed tokens, query q = rows cu[q] .. cu[q+1]-1, all valid (mask unused)
  __shared__ float s_att[2][32];
  __shared__ float s_part[4][2][1024];
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nvec = hidden >> 3;
  const int lq_pad = lq;                // (ATT: row length of the padded attention output)
  int64_t row0 = (int64_t)q * lq;
  if (cu) {
    const int r0 = cu[q], r1 = cu[q + 1];
    row0 = r0;
    lq = r1 - r0;
  }
  const T* e = enc + row0 * hidden;
  float x[8][16];                       // up to 8 tokens per wave, 2 vectors of 8 per lane
  float w0[16], w1[16];
  // Every load of this kernel is UNCONDITIONAL, from a clamped (always valid) index, and zeroed by a select afterwards: with
  // `if (l < lq && v < nvec) load` hipcc loses its vmcnt count at the branch join and waits vmcnt(0) behind each 16-byte
  // load -- 16 memory round trips per workgroup in a row (seen in the ISA; the kernel ran at 1.2 TB/s).
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int v = lane + k * 64;
    const int vc = v < nvec ? v : 0;
    ld8<float>(wm + vc * 8, w0 + k * 8);
    ld8<float>(wm + (n_mod > 1 ? hidden : 0) + vc * 8, w1 + k * 8);
  }
  float mk8[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const int l = wave + t * 4;
    const int lc = l < lq ? l : 0;
    mk8[t] = cu ? 1.f : mask[row0 + lc];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int v = lane + k * 64;
      ld8<T>(e + (int64_t)lc * hidden + (v < nvec ? v : 0) * 8, x[t] + k * 8);
    }
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const bool von = lane + k * 64 < nvec;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      w0[k * 8 + j] = von ? w0[k * 8 + j] : 0.f;
      w1[k * 8 + j] = (von && n_mod > 1) ? w1[k * 8 + j] : 0.f;
    }
  }
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const bool lon = wave + t * 4 < lq;
    mk8[t] = lon ? mk8[t] : 0.f;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const bool on = lon && lane + k * 64 < nvec;
#pragma unroll
      for (int j = 0; j < 8; ++j) x[t][k * 8 + j] = on ? x[t][k * 8 + j] : 0.f;
    }
  }
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const int l = wave + t * 4;
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
#pragma unroll
      for (int j = 0; j < 8; ++j) { s0 += x[t][k * 8 + j] * w0[k * 8 + j]; s1 += x[t][k * 8 + j] * w1[k * 8 + j]; }
    }
    s0 = wave_sum(s0);
    s1 = wave_sum(s1);
    if (lane == 0 && l < lq) {
      const float mk = mk8[t];
      s_att[0][l] = s0 * mk + (1.f - mk) * -1e10f;   // mask_logits, xml/model_xml.py:640-641
      s_att[1][l] = s1 * mk + (1.f - mk) * -1e10f;
    }
  }
  __syncthreads();
  if (tid < 64) {                      // softmax over the tokens: lanes 0-31 modality 0, lanes 32-63 modality 1
    const int m = tid >> 5, l = tid & 31;
    const bool on = m < n_mod && l < lq;
    const float sv = on ? s_att[m][l] : -INFINITY;
    float mx = sv;
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));     // within each 32-lane half
    const float ev = on ? expf(sv - mx) : 0.f;
    float sum = ev;
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (on) s_att[m][l] = ev / sum;
    if constexpr (ATT) {
      if (m < n_mod && l < lq_pad) att[((int64_t)q * lq_pad + l) * n_mod + m] = on ? ev / sum : 0.f;
    }
  }
  __syncthreads();
  float a0[16], a1[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) { a0[i] = 0.f; a1[i] = 0.f; }
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const int l = wave + t * 4;
    if (l < lq) {
      const float p0 = s_att[0][l], p1 = n_mod > 1 ? s_att[1][l] : 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) { a0[i] += p0 * x[t][i]; a1[i] += p1 * x[t][i]; }
    }
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int v = lane + k * 64;
    if (v < nvec)
#pragma unroll
      for (int j = 0; j < 8; ++j) { s_part[wave][0][v * 8 + j] = a0[k * 8 + j]; s_part[wave][1][v * 8 + j] = a1[k * 8 + j]; }
  }
  __syncthreads();
  for (int i = tid; i < n_mod * hidden; i += 256) {
    const int m = i / hidden, h = i - m * hidden;
    DT<T>::st(out + ((int64_t)m * n + q) * hidden + h,
              s_part[0][m][h] + s_part[1][m][h] + s_part[2][m][h] + s_part[3][m][h]);
  }
}

// hidden <= 256 (the reference's as-trained size): ONE WAVE per query, no LDS, no barriers.  Half h of the wave takes tokens
// h, h + 2, ...; lane v of a half holds 8 consecutive features of each of its tokens (16 tokens x 8 floats in registers).
// The workgroup-per-query kernel above spends its time on a workgroup's launch, two barriers and an LDS reduction for 9 KB
// of data, and at hidden = 256 half its lanes hold nothing: 126 us for the 10 895 queries of TVR val, this one ~25.
template <typename T, bool ATT = false>
__global__ __launch_bounds__(256) void modular_pool_wave_kernel(const T* __restrict__ enc, const float* __restrict__ mask,
                                                                const float* __restrict__ wm, T* __restrict__ out,
                                                                int64_t n, int lq, int hidden, int n_mod,
                                                                const int32_t* __restrict__ cu,
                                                                float* __restrict__ att = nullptr) {
  const int lane = threadIdx.x & 63, half = lane >> 5, v = lane & 31;
  const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= n) return;
  const int nvec = hidden >> 3;
  const int lq_pad = lq;                // (ATT: row length of the padded attention output)
  int64_t row0 = q * lq;
  if (cu) {
    const int r0 = cu[q], r1 = cu[q + 1];
    row0 = r0;
    lq = r1 - r0;
  }
  const bool von = v < nvec;
  const int vc = von ? v : 0;
  float w0[8], w1[8];
  ld8<float>(wm + vc * 8, w0);
  ld8<float>(wm + (n_mod > 1 ? hidden : 0) + vc * 8, w1);
  float x[16][8], mk[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {                 // unconditional loads from clamped indices (see the kernel above)
    const int l = 2 * i + half, lc = l < lq ? l : 0;
    mk[i] = cu ? 1.f : mask[row0 + lc];
    ld8<T>(enc + (row0 + lc) * hidden + vc * 8, x[i]);
  }
  float s0[16], s1[16], mx0 = -INFINITY, mx1 = -INFINITY;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const bool lon = 2 * i + half < lq;
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      x[i][j] = (lon && von) ? x[i][j] : 0.f;
      a += x[i][j] * w0[j];
      b += x[i][j] * w1[j];
    }
    a = lane16_sum_dpp(a); b = lane16_sum_dpp(b);
    a += __shfl_xor(a, 16, 64); b += __shfl_xor(b, 16, 64);          // the 32 lanes of this half
    const float m = lon ? mk[i] : 0.f;
    s0[i] = lon ? a * m + (1.f - m) * -1e10f : -INFINITY;            // mask_logits, xml/model_xml.py:640-641
    s1[i] = lon ? b * m + (1.f - m) * -1e10f : -INFINITY;
    mx0 = fmaxf(mx0, s0[i]); mx1 = fmaxf(mx1, s1[i]);
  }
  mx0 = fmaxf(mx0, __shfl_xor(mx0, 32, 64)); mx1 = fmaxf(mx1, __shfl_xor(mx1, 32, 64));
  float sum0 = 0.f, sum1 = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    s0[i] = 2 * i + half < lq ? expf(s0[i] - mx0) : 0.f;
    s1[i] = 2 * i + half < lq ? expf(s1[i] - mx1) : 0.f;
    sum0 += s0[i]; sum1 += s1[i];
  }
  sum0 += __shfl_xor(sum0, 32, 64); sum1 += __shfl_xor(sum1, 32, 64);
  float a0[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, a1[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const float p0 = s0[i] / sum0, p1 = n_mod > 1 ? s1[i] / sum1 : 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) { a0[j] += p0 * x[i][j]; a1[j] += p1 * x[i][j]; }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) { a0[j] += __shfl_xor(a0[j], 32, 64); a1[j] += __shfl_xor(a1[j], 32, 64); }
  if (von) {      // half 0 stores modality 0, half 1 modality 1
    if (half == 0) st8<T>(out + q * hidden + v * 8, a0);
    else if (n_mod > 1) st8<T>(out + ((int64_t)n + q) * hidden + v * 8, a1);
  }
  if constexpr (ATT) {
    // The weights, in a pass of their own BEHIND the pooled store: inside the weighting loop the extra use of p0 / p1 changed
    // which of its multiply-adds hipcc fuses (packed multiplies + adds became fmas), i.e. the pooled bits.  Every lane of a
    // half holds the exponentials of tokens 2 i + half; the same IEEE division gives the factor the loop multiplied with.
    // Lane i of the half stores token 2 i + half (s0 / s1 are 0 beyond the query's own tokens).
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int l = 2 * i + half;
      if (v == i && l < lq_pad) {
        float* ap = att + (q * lq_pad + l) * n_mod;
        ap[0] = s0[i] / sum0;
        if (n_mod > 1) ap[1] = s1[i] / sum1;
      }
    }
  }
}

template <typename T>
static void launch_modular_pool_small(const void* enc, const float* mask, const float* w_m, void* out, int64_t n, int lq,
                                      int hidden, int n_mod, const int32_t* cu, hipStream_t st, float* att = nullptr) {
  if (att) {
    if (hidden <= 256)
      hipLaunchKernelGGL((modular_pool_wave_kernel<T, true>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, (const T*)enc,
                         mask, w_m, (T*)out, n, lq, hidden, n_mod, cu, att);
    else
      hipLaunchKernelGGL((modular_pool_small_kernel<T, true>), dim3((unsigned)n), dim3(256), 0, st, (const T*)enc, mask, w_m,
                         (T*)out, n, lq, hidden, n_mod, cu, att);
    return;
  }
  if (hidden <= 256)
    hipLaunchKernelGGL(modular_pool_wave_kernel<T>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, (const T*)enc, mask, w_m,
                       (T*)out, n, lq, hidden, n_mod, cu, (float*)nullptr);
  else
    hipLaunchKernelGGL(modular_pool_small_kernel<T>, dim3((unsigned)n), dim3(256), 0, st, (const T*)enc, mask, w_m, (T*)out,
                       n, lq, hidden, n_mod, cu, (float*)nullptr);
}

extern "C" int xml_modular_pool(const void* enc, const float* mask, const float* w_m, void* out, int64_t n, int lq,
                                int hidden, int n_mod, int dt, xml_stream_t stream) {
  XML_ENTER();
  if (!enc || !mask || !w_m || !out || n <= 0 || lq <= 0 || hidden <= 0) return XML_ERR_BAD_ARG;
  if (n_mod < 1 || n_mod > 2 || lq > 128) return XML_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  if (lq <= 32 && hidden % 8 == 0 && hidden <= 1024) {
    if (dt == XML_F32) launch_modular_pool_small<float>(enc, mask, w_m, out, n, lq, hidden, n_mod, nullptr, st);
    else if (dt == XML_BF16) launch_modular_pool_small<bf16_t>(enc, mask, w_m, out, n, lq, hidden, n_mod, nullptr, st);
    else return XML_ERR_BAD_ARG;
    XML_CHECK_LAUNCH();
    return XML_OK;
  }
  if (dt == XML_F32)
    hipLaunchKernelGGL(modular_pool_kernel<float>, dim3((unsigned)n), dim3(256), 0, st, (const float*)enc, mask, w_m,
                       (float*)out, n, lq, hidden, n_mod, (float*)nullptr);
  else if (dt == XML_BF16)
    hipLaunchKernelGGL(modular_pool_kernel<bf16_t>, dim3((unsigned)n), dim3(256), 0, st, (const bf16_t*)enc, mask,
                       w_m, (bf16_t*)out, n, lq, hidden, n_mod, (float*)nullptr);
  else
    return XML_ERR_BAD_ARG;
  XML_CHECK_LAUNCH();
  return XML_OK;
}

// K5 on packed variable-length queries (xml_attention_block_varlen's layout): out[m][q] = sum_l a[l][m] enc[cu[q] + l],
// a = softmax over the query's own tokens.  max_len <= 32, hidden % 8 == 0, hidden <= 1024, every query >= 1 token.
extern "C" int xml_modular_pool_varlen(const void* enc, const int32_t* cu_seqlens, const float* w_m, void* out, int64_t n,
                                       int max_len, int hidden, int n_mod, int dt, xml_stream_t stream) {
  XML_ENTER();
  if (!enc || !cu_seqlens || !w_m || !out || n <= 0 || max_len <= 0 || hidden <= 0) return XML_ERR_BAD_ARG;
  if (n_mod < 1 || n_mod > 2 || max_len > 32 || hidden % 8 || hidden > 1024) return XML_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  if (dt == XML_F32) launch_modular_pool_small<float>(enc, nullptr, w_m, out, n, max_len, hidden, n_mod, cu_seqlens, st);
  else if (dt == XML_BF16) launch_modular_pool_small<bf16_t>(enc, nullptr, w_m, out, n, max_len, hidden, n_mod, cu_seqlens, st);
  else return XML_ERR_BAD_ARG;
  XML_CHECK_LAUNCH();
  return XML_OK;
}

// K5 + its softmax weights (XML.get_modularized_queries(return_modular_att=True), xml/model_xml.py:410-423): the ATT
// instantiations of the three kernels above, chosen by the same shape rules as xml_modular_pool / _varlen.
extern "C" int xml_modular_pool_att(const void* enc, const float* mask, const float* w_m, void* out, float* att, int64_t n,
                                    int lq, int hidden, int n_mod, int dt, xml_stream_t stream) {
  XML_ENTER();
  if (!enc || !mask || !w_m || !out || !att || n <= 0 || lq <= 0 || hidden <= 0) return XML_ERR_BAD_ARG;
  if (n_mod < 1 || n_mod > 2 || lq > 128) return XML_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  if (lq <= 32 && hidden % 8 == 0 && hidden <= 1024) {
    if (dt == XML_F32) launch_modular_pool_small<float>(enc, mask, w_m, out, n, lq, hidden, n_mod, nullptr, st, att);
    else if (dt == XML_BF16) launch_modular_pool_small<bf16_t>(enc, mask, w_m, out, n, lq, hidden, n_mod, nullptr, st, att);
    else return XML_ERR_BAD_ARG;
    XML_CHECK_LAUNCH();
    return XML_OK;
  }
  if (dt == XML_F32)
    hipLaunchKernelGGL((modular_pool_kernel<float, true>), dim3((unsigned)n), dim3(256), 0, st, (const float*)enc, mask, w_m,
                       (float*)out, n, lq, hidden, n_mod, att);
  else if (dt == XML_BF16)
    hipLaunchKernelGGL((modular_pool_kernel<bf16_t, true>), dim3((unsigned)n), dim3(256), 0, st, (const bf16_t*)enc, mask,
                       w_m, (bf16_t*)out, n, lq, hidden, n_mod, att);
  else
    return XML_ERR_BAD_ARG;
  XML_CHECK_LAUNCH();
  return XML_OK;
}

extern "C" int xml_modular_pool_att_varlen(const void* enc, const int32_t* cu_seqlens, const float* w_m, void* out,
                                           float* att, int64_t n, int max_len, int hidden, int n_mod, int dt,
                                           xml_stream_t stream) {
  XML_ENTER();
  if (!enc || !cu_seqlens || !w_m || !out || !att || n <= 0 || max_len <= 0 || hidden <= 0) return XML_ERR_BAD_ARG;
  if (n_mod < 1 || n_mod > 2 || max_len > 32 || hidden % 8 || hidden > 1024) return XML_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  if (dt == XML_F32) launch_modular_pool_small<float>(enc, nullptr, w_m, out, n, max_len, hidden, n_mod, cu_seqlens, st, att);
  else if (dt == XML_BF16)
    launch_modular_pool_small<bf16_t>(enc, nullptr, w_m, out, n, max_len, hidden, n_mod, cu_seqlens, st, att);
  else return XML_ERR_BAD_ARG;
  XML_CHECK_LAUNCH();
  return XML_OK;
}
