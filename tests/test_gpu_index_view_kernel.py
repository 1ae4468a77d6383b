"""xml_index_gather_blocks (include/xmlhip_index_view.h) through ops.index_gather_blocks against a numpy restatement of the
layout in the header's words, bitwise: blocks of 1 KiB per 64-byte slice, mask bits of block g in word g >> 1 (upper half for
odd g).  Source of 20 tiles, destinations of 1, 3 and 20 tiles pre-filled with 0xFF: unwritten image rows keep the fill,
every mask word is written."""
import numpy as np
import pytest
import torch

from test_gpu_kernels import DEV
from tvretrieval_amd import ops

pytestmark = pytest.mark.gpu

SRC_TILES = 20
N_SRC = 16 * SRC_TILES
SHAPES = [pytest.param(torch.bfloat16, 256, id="bf16-h256"), pytest.param(torch.float32, 128, id="f32-h128"),
          pytest.param(torch.float32, 192, id="f32-h192")]
OUT_OF_RANGE = [-1, -3, -100, N_SRC, N_SRC + 1, 2 ** 31 - 1, -2 ** 31]


def src_blocks(n_tiles, seed):
    """One entry per destination block: random sources and unused blocks, out-of-range entries, and the named runs."""
    rng = np.random.default_rng(seed)
    n = 16 * n_tiles
    sb = np.where(rng.random(n) < 0.6, rng.integers(0, N_SRC, n), -2).astype(np.int64)
    spare = np.asarray([g for g in range(10, n - 1) if not (n_tiles >= 3 and (16 <= g < 24 or 32 <= g < 40))])
    bad = rng.choice(spare, min(max(3, n_tiles), len(spare)), replace=False)
    sb[bad] = rng.choice(OUT_OF_RANGE, len(bad))               # entries outside {-2} u [0, N_SRC): handled as -2
    sb[9] = -2
    sb[0] = 5                                    # a run of one block, from the first source tile
    sb[1:9] = np.arange(16, 24)                  # 8 blocks that straddle 7|8 in the DESTINATION only
    if n_tiles >= 3:
        sb[16:24] = np.arange(4, 12)             # 8 blocks that straddle 7|8 in the SOURCE only
        sb[32:40] = np.arange(N_SRC - 16, N_SRC - 8)      # a run of the last source tile
    sb[n - 1] = N_SRC - 1                        # the last destination block <- the last source block
    return sb.astype(np.int32)


def model(sb, src_u8, src_words, slices):
    """numpy restatement: src_u8 per modality (SRC_TILES, slices, 16, 1024) uint8, src_words per modality (N_SRC / 2,) uint32
    or None -> (images (T, slices, 16, 1024) uint8 over a 0xFF fill, written mask (T, 16), words (T * 8,) uint32)."""
    n_tiles = len(sb) // 16
    ok = (sb >= 0) & (sb < N_SRC)
    imgs, words = [], []
    for u8, w in zip(src_u8, src_words):
        out = np.full((n_tiles, slices, 16, 1024), 0xFF, dtype=np.uint8)
        half = np.zeros(len(sb), dtype=np.uint32)
        for g in np.nonzero(ok)[0]:
            s = int(sb[g])
            out[g // 16, :, g % 16] = u8[s // 16, :, s % 16]
            half[g] = 0xFFFF if w is None else (int(w[s >> 1]) >> (16 * (s & 1))) & 0xFFFF
        imgs.append(out)
        words.append(half[0::2] | (half[1::2] << np.uint32(16)))
    return imgs, ok.reshape(n_tiles, 16), words


@pytest.mark.parametrize("mode", ["one-modality", "two-modalities", "two-first-all-valid"])
@pytest.mark.parametrize("n_tiles", [1, 3, 20])
@pytest.mark.parametrize("dtype, hidden", SHAPES)
def test_gather_blocks_against_the_numpy_layout(dtype, hidden, n_tiles, mode):
    es = torch.empty(0, dtype=dtype).element_size()
    slices = hidden * es // 64
    n_mod = 1 if mode == "one-modality" else 2
    g = torch.Generator().manual_seed(100 * n_tiles + hidden + n_mod)
    sb = src_blocks(n_tiles, 7 * n_tiles + hidden)
    src_u8 = [torch.randint(0, 256, (SRC_TILES, slices, 16, 1024), generator=g, dtype=torch.uint8) for _ in range(n_mod)]
    src_w = [torch.randint(-2 ** 31, 2 ** 31, (N_SRC // 2,), generator=g, dtype=torch.int64).to(torch.int32) for _ in range(n_mod)]
    if mode == "two-first-all-valid":
        src_w[0] = None                          # NULL bits for one modality, given for the other
    k6_src = [u.to(DEV).view(-1).view(dtype) for u in src_u8]
    bits_src = [None if w is None else w.to(DEV) for w in src_w]
    k6_dst = [torch.full((n_tiles * slices * 16 * 1024,), 0xFF, dtype=torch.uint8, device=DEV).view(dtype) for _ in range(n_mod)]
    bits_dst = [torch.full((2 * n_tiles, 4), -1, dtype=torch.int32, device=DEV) for _ in range(n_mod)]
    keep = [t.clone() for t in k6_src]
    ops.index_gather_blocks(torch.from_numpy(sb).to(DEV), k6_src, bits_src, N_SRC, k6_dst, bits_dst, hidden)
    torch.cuda.synchronize()
    imgs, written, words = model(sb, [u.numpy() for u in src_u8],
                                 [None if w is None else w.numpy().view(np.uint32) for w in src_w], slices)
    for m in range(n_mod):
        got = k6_dst[m].view(torch.uint8).cpu().numpy().reshape(n_tiles, slices, 16, 1024)
        assert (got == imgs[m]).all(), "modality %d: image" % m
        assert (np.moveaxis(got, 1, 2)[~written].reshape(-1) == 0xFF).all(), "an unused block's rows were written"
        gw = bits_dst[m].cpu().numpy().view(np.uint32).reshape(-1)
        assert (gw == words[m]).all(), "modality %d: mask words" % m
        assert torch.equal(k6_src[m].view(torch.uint8), keep[m].view(torch.uint8))
    assert written.sum() >= 10 and (~written).sum() >= 3


def test_the_wrapper_refuses_what_does_not_fit():
    from tvretrieval_amd._lib import XmlHipError
    dt, hidden = torch.float32, 128
    per = ops.q2c_tiled_numel(256, hidden, dt)
    src = [torch.zeros(2 * per, dtype=dt, device=DEV)]
    dst = [torch.zeros(per, dtype=dt, device=DEV)]
    bits = [torch.zeros((2, 4), dtype=torch.int32, device=DEV)]
    sb = torch.full((16,), -2, dtype=torch.int32, device=DEV)
    ops.index_gather_blocks(sb, src, [None], 32, dst, bits, hidden)
    with pytest.raises(XmlHipError):             # the source holds 32 blocks, not 48
        ops.index_gather_blocks(sb, src, [None], 48, dst, bits, hidden)
    with pytest.raises(XmlHipError):             # source mask words for 16 blocks only
        ops.index_gather_blocks(sb, src, [torch.zeros(8, dtype=torch.int32, device=DEV)], 32, dst, bits, hidden)
    with pytest.raises(XmlHipError):             # a destination of another size
        ops.index_gather_blocks(sb, src, [None], 32, [torch.zeros(2 * per, dtype=dt, device=DEV)], bits, hidden)
    with pytest.raises(XmlHipError):
        ops.index_gather_blocks(sb[:15], src, [None], 32, dst, bits, hidden)
    with pytest.raises(XmlHipError):             # a hidden size the tiled kernel does not take
        ops.index_gather_blocks(sb, src, [None], 32, dst, bits, 100)
