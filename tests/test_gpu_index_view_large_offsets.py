"""xml_index_gather_blocks past 2^31 elements and 4 GiB offsets (tests/large_offsets.py; profiles/large_offsets.md): blocks
gathered out of a bf16 source image of NV_BIG videos -- video 0, the last one, and the videos around every threshold -- must
be bitwise the blocks gathered from a twin image that holds just those videos."""
import time

import numpy as np
import pytest
import torch

import large_offsets as LO
from test_gpu_kernels import DEV
from tvretrieval_amd import ops, subset

pytestmark = pytest.mark.gpu

NV, L, H = LO.NV_BIG, LO.LPAD, LO.HIDDEN
SAMPLE = LO.sample_videos(NV, L, H, 2)
ALL = ("T1", "T2", "T3")


def test_gather_blocks_from_a_corpus_sized_image():
    assert not LO.missed_thresholds(SAMPLE, NV, L, H, 2) and SAMPLE[0] == 0 and SAMPLE[-1] == NV - 1
    slices, per = H * 2 // 64, 16 * 1024 // 2                 # int16 elements of one (tile, slice) chunk
    g = torch.Generator(device=DEV).manual_seed(77)
    big = torch.empty((NV // 2, slices, 2, per // 2), dtype=torch.int16, device=DEV)       # [tile][slice][video of the tile]
    for t0 in range(0, NV // 2, 1368):
        big[t0:t0 + 1368] = torch.randint(-2 ** 15, 2 ** 15, (min(1368, NV // 2 - t0), slices, 2, per // 2), device=DEV,
                                          generator=g, dtype=torch.int16)
    LO.assert_crosses(big.numel(), 2, ALL)
    bits_big = torch.randint(-2 ** 31, 2 ** 31, (NV, 4), device=DEV, generator=g, dtype=torch.int64).to(torch.int32)
    n = len(SAMPLE)
    st = torch.as_tensor(SAMPLE, device=DEV)
    twin = torch.zeros(((n + 1) // 2, slices, 2, per // 2), dtype=torch.int16, device=DEV)
    pos = torch.arange(n, device=DEV)
    twin[pos // 2, :, pos % 2] = big[st // 2, :, st % 2]
    bits_twin = torch.zeros((2 * ((n + 1) // 2), 4), dtype=torch.int32, device=DEV)
    bits_twin[:n] = bits_big[st]
    members = np.asarray(SAMPLE)
    sb_big, codes, firsts = subset.place_members(members, np.full(n, 8), 8 * members)
    sb_twin, codes2, _ = subset.place_members(members, np.full(n, 8), 8 * np.arange(n))
    assert (codes == codes2).all()
    n_tiles = codes.shape[0] // 2
    outs = []
    for sb, img, bits, nsrc in ((sb_twin, twin, bits_twin, 16 * twin.shape[0]), (sb_big, big, bits_big, 8 * NV)):      # (big second: a warm launch is timed)
        dst = torch.full((n_tiles * slices * per,), -1, dtype=torch.int16, device=DEV).view(torch.bfloat16)
        bd = torch.full((2 * n_tiles, 4), -1, dtype=torch.int32, device=DEV)
        sbd = torch.from_numpy(sb).to(DEV)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ops.index_gather_blocks(sbd, [img.view(-1).view(torch.bfloat16)], [bits.view(-1)], nsrc, [dst], [bd], H)
        torch.cuda.synchronize()
        outs.append((dst, bd, time.perf_counter() - t0))
    print("LARGE test_gather_blocks_from_a_corpus_sized_image: gather of %d blocks from the %.2f GB image %.2f ms, from the "
          "twin %.2f ms" % (8 * n, big.numel() * 2 / 1e9, outs[1][2] * 1e3, outs[0][2] * 1e3))
    assert torch.equal(outs[0][0].view(torch.int16), outs[1][0].view(torch.int16))
    assert torch.equal(outs[0][1], outs[1][1])
    # ... and the twin's own gather is the restatement: video i of the sample lies whole at its run
    # (runs of 8 blocks are placed back to back, two to a tile)
    assert firsts.tolist() == (8 * np.arange(n)).tolist()
    got = outs[1][0].view(torch.int16).view(n_tiles, slices, 2, per // 2)
    assert torch.equal(got[pos // 2, :, pos % 2], big[st // 2, :, st % 2])
    del big, twin
    torch.cuda.empty_cache()
