// Subset views of a resident index (include/xmlhip_index_view.h; tvretrieval_amd/subset.py): the 16-row
// blocks of the allowed videos are GATHERED out of a resident K6 image -- fixed, length-bucketed or packed, all the same
// slice-major image in blocks -- into a small packed image of their own, with their mask bits.  src_block names, per
// destination block, the source block (>= 0) or "unused" (-2; anything out of range counts as -2).
// A pure copy, 16 bytes per lane: a workgroup owns one (destination tile, slice) chunk of 16 KiB, wave w its blocks w + 4 i,
// so a lane has four independent 16-byte loads in flight and a workgroup 16 KiB -- at 8 resident workgroups per CU that is
// four times the ~32 KiB per CU that keeps HBM streaming.  Source and destination are different buffers, so nothing has to
// pass through LDS and there is no barrier.  Source offsets are 64-bit: the source is corpus-sized.
// The workgroups of slice 0 also store the tile's 8 mask words of their modality, whole: thread w < 8 owns word w, i.e. the
// 16 bits of blocks 2 w and 2 w + 1 -- plain stores, no atomics.
#include "../../include/xmlhip_index_view.h"
#include "index_rows.h"

namespace {

__global__ __launch_bounds__(256) void index_gather_blocks_kernel(
    const int32_t* __restrict__ src_block, const char* __restrict__ k6_src_a, const uint32_t* __restrict__ bits_src_a,
    const char* __restrict__ k6_src_b, const uint32_t* __restrict__ bits_src_b, int64_t n_blocks_src,
    char* __restrict__ k6_dst_a, uint32_t* __restrict__ bits_dst_a, char* __restrict__ k6_dst_b,
    uint32_t* __restrict__ bits_dst_b, int slices) {
  const int t = threadIdx.x;
  const int lane = t & 63;
  const int64_t tile = blockIdx.x;
  const int slice = blockIdx.y;
  const bool second = blockIdx.z != 0;
  // the tile's 16 entries: ONE vector load per wave, lane j < 16 holds entry j; out of range -> unused
  int word = lane < 16 ? src_block[tile * 16 + lane] : -2;
  if (word < 0 || (int64_t)word >= n_blocks_src) word = -2;
  const char* k6_src = second ? k6_src_b : k6_src_a;
  char* k6_dst = second ? k6_dst_b : k6_dst_a;
  char* dst_chunk = k6img::block_slice(k6_dst, tile * 16, slices, slice);
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  int src[4];
  uint4 v[4];
  k6img::load_wave_blocks(k6_src, word, 0, wave, slices, slice, lane, src, v);
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (src[i] >= 0) st_global16(dst_chunk + (wave + 4 * i) * k6img::BLOCK_BYTES + lane * 16, v[i]);
  // ---- the tile's mask words of this modality: slice 0, thread w < 8 = word w = blocks 2 w (low half) and 2 w + 1
  // (the two entries are fetched by EVERY lane, before the branch: a shuffle reads nothing from a lane that has left)
  const int pair[2] = {__shfl(word, (2 * lane) & 15), __shfl(word, (2 * lane + 1) & 15)};
  if (slice != 0 || t >= 8) return;
  const uint32_t* bits_src = second ? bits_src_b : bits_src_a;
  uint32_t* bits_dst = second ? bits_dst_b : bits_dst_a;
  uint32_t out = 0u;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int s = pair[half];
    uint32_t b = 0u;
    if (s >= 0) b = bits_src ? (bits_src[s >> 1] >> ((s & 1) * 16)) & 0xffffu : 0xffffu;
    out |= b << (half * 16);
  }
  bits_dst[tile * 8 + t] = out;
}

}  // namespace

extern "C" int xml_index_gather_blocks(int n_mod, const int32_t* src_block, int n_tiles_dst, const void* k6_src_a,
                                       const uint32_t* bits_src_a, const void* k6_src_b, const uint32_t* bits_src_b,
                                       int64_t n_blocks_src, void* k6_dst_a, int32_t* bits_dst_a, void* k6_dst_b,
                                       int32_t* bits_dst_b, int hidden, int dt, xml_stream_t stream) {
  XML_ENTER();
  if (n_mod != 1 && n_mod != 2) return XML_ERR_BAD_ARG;
  if (!src_block || !k6_src_a || !k6_dst_a || !bits_dst_a) return XML_ERR_BAD_ARG;
  if (n_mod == 2 && (!k6_src_b || !k6_dst_b || !bits_dst_b)) return XML_ERR_BAD_ARG;
  if (n_tiles_dst <= 0 || n_blocks_src <= 0) return XML_ERR_BAD_ARG;
  if (dt != XML_F32 && dt != XML_BF16) return XML_ERR_BAD_ARG;
  if (!xml_q2c_tiled_ok(128, hidden, dt)) return XML_ERR_UNSUPPORTED;
  const int slices = hidden * (dt == XML_F32 ? 4 : 2) / 64;      // 64-byte slices per row (xml_q2c_tiled_ok: whole ones)
  if (slices <= 0 || slices > 65535) return XML_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)n_tiles_dst, (unsigned)slices, (unsigned)n_mod);
  hipLaunchKernelGGL(index_gather_blocks_kernel, grid, dim3(256), 0, (hipStream_t)stream, src_block, (const char*)k6_src_a,
                     bits_src_a, n_mod == 2 ? (const char*)k6_src_b : nullptr, n_mod == 2 ? bits_src_b : nullptr,
                     n_blocks_src, (char*)k6_dst_a, (uint32_t*)bits_dst_a, n_mod == 2 ? (char*)k6_dst_b : nullptr,
                     n_mod == 2 ? (uint32_t*)bits_dst_b : nullptr, slices);
  XML_CHECK_LAUNCH();
  return XML_OK;
}
