// Compaction of the PACKED image of a resident index (xml_q2c_scores_packed; DESIGN.md section 20b;
// include/xmlhip_index_compact.h): whole 16-row blocks are moved inside tensors that are already allocated, so that the free
// blocks of a tile become one run at its end.  The three things K6 reads move together -- the image rows, the per-block
// codes, the 16 mask bits per block and modality; the per-slot state (feat2, imask, vlen, slot_ids, live) is no operand: a
// slot keeps its number.
// A record is 17 int32 {tile, src[16]}: destination block b of `tile` receives the block with GLOBAL number src[b] >= 0 (of
// any tile), stays as it is (src[b] == -1) or becomes unused (src[b] == -2: code -2, bits 0; its rows stay, as after a clear).
// Launch contract (the host's planner, index_update.BlockTable.check_compact, guarantees it): at most one record per tile;
// every destination block was free before the launch or is a block of the same tile that the record itself moves; a source
// block in ANOTHER tile than its destination is not written by any record of the launch; the blocks mapped from one run are
// contiguous and in order.
// Within a tile the mapping may be any permutation -- a run may slide left over its own old blocks: a workgroup loads the
// source KiB of every destination block of its (tile, slice) chunk, puts them into LDS, and stores only behind the barrier.
// The loaded data goes THROUGH LDS rather than staying in registers across the barrier: a barrier does not wait for another
// wave's outstanding vector loads, the LDS write (which needs the loaded value) does.  The same holds for codes and bits.
// A record whose tile is outside [0, n_tiles) or with a src outside {-2, -1} u [0, 16 n_tiles) is dropped whole.
#include "../../include/xmlhip_index_compact.h"
#include "index_rows.h"

namespace {

constexpr int REC = 17;                 // int32 per record

__global__ __launch_bounds__(256) void index_move_blocks_packed_kernel(
    const int32_t* __restrict__ records, char* k6_a, int32_t* bits_a, char* k6_b, int32_t* bits_b, int32_t* codes,
    int n_tiles, int slices) {
  __shared__ uint4 stage[k6img::CHUNK_BYTES / 16];      // one (tile, slice) chunk
  __shared__ int s_code[16];
  __shared__ unsigned int s_bits[16];
  // the record: ONE vector load per wave, lane j < 17 holds word j (17 dependent scalar loads cost 17 latencies)
  const int t = threadIdx.x;
  const int lane = t & 63;
  const int word = lane < REC ? records[(int64_t)blockIdx.y * REC + lane] : -1;
  const bool good = lane == 0 ? (word >= 0 && word < n_tiles) : (word >= -2 && word < n_tiles * 16);
  if (!__all(good)) return;                                // a bad record writes nothing (every wave sees the same words)
  const int tile = __builtin_amdgcn_readlane(word, 0);
  const bool second = blockIdx.z != 0;
  char* k6 = second ? k6_b : k6_a;
  const int slice = blockIdx.x;

  // ---- the image: chunk (tile, slice); wave w owns blocks w + 4 i, a lane 16 bytes of each
  char* dst_chunk = k6img::block_slice(k6, (int64_t)tile * 16, slices, slice);
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  int src[4];
  uint4 v[4];
  k6img::load_wave_blocks(k6, word, 1, wave, slices, slice, lane, src, v);
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (src[i] >= 0) stage[(wave + 4 * i) * 64 + (t & 63)] = v[i];
  // ---- workgroup 0 of (record, modality): the tile's mask words; of modality 0 also its codes.  Thread b < 16 = block b
  const bool tables = slice == 0 && t < 16;
  const int mine = __shfl_down(word, 1);                   // thread b < 16 of wave 0: src[b]
  if (tables) {
    const int from = mine >= 0 ? mine : tile * 16 + t;     // a kept block keeps its bits, a freed one gets none
    const unsigned int w = reinterpret_cast<const unsigned int*>(second ? bits_b : bits_a)[from >> 1];
    s_bits[t] = mine == -2 ? 0u : (w >> ((from & 1) * 16)) & 0xffffu;
    if (!second && mine >= 0) s_code[t] = codes[mine];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (src[i] >= 0) st_global16(dst_chunk + (wave + 4 * i) * k6img::BLOCK_BYTES + (t & 63) * 16, stage[(wave + 4 * i) * 64 + (t & 63)]);
  if (!tables) return;
  if (t < 8) reinterpret_cast<unsigned int*>(second ? bits_b : bits_a)[tile * 8 + t] = s_bits[2 * t] | s_bits[2 * t + 1] << 16;
  if (!second && mine != -1) {
    int c = -2;
    if (mine >= 0) c = s_code[t] >= 0 ? s_code[t] : (t == 7 ? -3 : -1);   // a non-last block at 7 goes on into block 8
    codes[tile * 16 + t] = c;
  }
}

}  // namespace

extern "C" int xml_index_move_blocks_packed(int n_mod, const int32_t* records, int n, void* k6_a, int32_t* bits_a, void* k6_b,
                                            int32_t* bits_b, int32_t* codes, int n_tiles, int hidden, int dt,
                                            xml_stream_t stream) {
  XML_ENTER();
  if (n_mod != 1 && n_mod != 2) return XML_ERR_BAD_ARG;
  if (!records || !k6_a || !bits_a || !codes) return XML_ERR_BAD_ARG;
  if (n_mod == 2 && (!k6_b || !bits_b)) return XML_ERR_BAD_ARG;
  if (n <= 0 || n > 65535 || n_tiles <= 0 || n_tiles > (1 << 26)) return XML_ERR_BAD_ARG;
  if (dt != XML_F32 && dt != XML_BF16) return XML_ERR_BAD_ARG;
  if (!xml_q2c_tiled_ok(128, hidden, dt)) return XML_ERR_UNSUPPORTED;
  const int slices = hidden * (dt == XML_F32 ? 4 : 2) / 64;      // 64-byte slices per row (xml_q2c_tiled_ok: whole ones)
  if (slices <= 0 || slices > 65535) return XML_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)slices, (unsigned)n, (unsigned)n_mod);
  hipLaunchKernelGGL(index_move_blocks_packed_kernel, grid, dim3(256), 0, (hipStream_t)stream, records, (char*)k6_a, bits_a,
                     n_mod == 2 ? (char*)k6_b : nullptr, n_mod == 2 ? bits_b : nullptr, codes, n_tiles, slices);
  XML_CHECK_LAUNCH();
  return XML_OK;
}
