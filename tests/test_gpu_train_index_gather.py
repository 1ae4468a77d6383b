"""xml_index_gather_video_rows (include/xmlhip_train_index.h) through ops.index_gather_video_rows against a numpy restatement
that reads the image by the layout formula of include/xmlhip_index_view.h, bitwise: tiles of 16 blocks of 16 rows, the 16 rows
of a block for one 64-byte slice 1 KiB contiguous at tile * slices * 16384 + slice * 16384 + block * 1024; clip c of batch item
i is image row 16 * first_block[i] + c.  The sources hold random BYTES (every bit pattern is copied as it is), the outputs are
pre-filled with 0xFF and compared in every element.

Forms: the fixed image (video v = blocks 8 v ..), a length-bucketed plan image (first blocks from subset.invert_pack_plan), a
packed image with hand-placed runs -- one crossing blocks 7 | 8 of its tile, one ending in the image's last block -- and a
row-major source with lpad = 32.  Video lengths {1, 15, 16, 17, 100, 128}, batch lengths {1, 17, 100, 128} (both shorter and
longer than a video), n in {1, 3, 130}, a slot twice in a batch, slot -1 and slot n_videos, a first block of -1 and one behind
the image, one and two modalities."""
import numpy as np
import pytest
import torch

from test_gpu_kernels import DEV
from tvretrieval_amd import ops, subset

pytestmark = pytest.mark.gpu

# the last: the narrowest bf16 rows xml_q2c_tiled_ok takes (6 slices: a chunk count that is no power of two)
SHAPES = [pytest.param(torch.bfloat16, 128, id="bf16-h128"), pytest.param(torch.float32, 64, id="f32-h64"),
          pytest.param(torch.bfloat16, 192, id="bf16-h192")]
VLENS = [1, 15, 16, 17, 100, 128, 64, 33]
FORMS = ["fixed", "plan", "packed", "rows"]
# the packed image: 3 tiles; slot -> first block.  slot 4 (100 clips = 7 blocks) lies on blocks 5 .. 11 of tile 0: across 7 | 8;
# slot 5 (128 clips = 8 blocks) ends in the image's last block
PACKED_TILES = 3
PACKED_FIRST = [0, 1, 2, 3, 5, 40, 16, 20]


def make_source(form, dtype, hidden, n_mod, seed):
    """-> dict: vlen (nv,) int32, lpad, n_blocks, first (nv,) int64 first block per slot (zeros for rows), and per modality
    cn_u8 (the K6 operand's bytes: (tiles, slices, 16, 1024) or (nv, lpad, row bytes)), f2_u8 (nv, lpad, row bytes), mask."""
    es = torch.empty(0, dtype=dtype).element_size()
    rb, slices = hidden * es, hidden * es // 64
    g = torch.Generator().manual_seed(seed)
    nv = len(VLENS)
    lpad = 32 if form == "rows" else 128
    vlen = np.minimum(np.asarray(VLENS), lpad).astype(np.int32)
    plan = None
    if form == "fixed":
        first, tiles = 8 * np.arange(nv), (nv * 128 + 255) // 256
        n_blocks = 8 * nv
    elif form == "plan":
        plan = ops.PackPlan([(torch.arange(128)[None, :] < torch.as_tensor(vlen)[:, None]).float()])
        first, tiles = subset.invert_pack_plan(plan)[0], plan.n_tiles
        n_blocks = 16 * tiles
    elif form == "packed":
        first, tiles, n_blocks = np.asarray(PACKED_FIRST), PACKED_TILES, 16 * PACKED_TILES
    else:
        first, tiles, n_blocks = np.zeros(nv, dtype=np.int64), 0, 0
    src = dict(vlen=vlen, lpad=lpad, n_blocks=n_blocks, first=np.asarray(first, dtype=np.int64), mods=[], plan=plan, tiles=tiles)
    for _ in range(n_mod):
        shape = (nv, lpad, rb) if form == "rows" else (tiles, slices, 16, 1024)
        src["mods"].append(dict(cn_u8=torch.randint(0, 256, shape, generator=g, dtype=torch.uint8),
                                f2_u8=torch.randint(0, 256, (nv, lpad, rb), generator=g, dtype=torch.uint8),
                                mask=torch.rand((nv, lpad), generator=g) if form == "rows" else
                                (torch.rand((nv, lpad), generator=g) < 0.8).float()))
    return src


def image_row(u8, row):
    """The bytes of image row `row` by the header's formula: (slices * 64,) uint8."""
    tile, block, r = row >> 8, (row >> 4) & 15, row & 15
    return u8[tile, :, block, r * 64:(r + 1) * 64].reshape(-1)


def model(form, src, slots, first_block, length):
    """numpy restatement -> per modality (cn (n, length, row bytes) uint8, f2 alike, mask (n, length) f32)."""
    nv, lpad = len(src["vlen"]), src["lpad"]
    outs = []
    for mod in src["mods"]:
        cn_u8, f2_u8, mask = mod["cn_u8"].numpy(), mod["f2_u8"].numpy(), mod["mask"].numpy()
        rb = f2_u8.shape[2]
        cn, f2 = np.zeros((len(slots), length, rb), np.uint8), np.zeros((len(slots), length, rb), np.uint8)
        mk = np.zeros((len(slots), length), np.float32)
        for i, s in enumerate(slots):
            if not 0 <= s < nv:
                continue
            for c in range(min(length, lpad, int(src["vlen"][s]))):
                if form == "rows":
                    cn[i, c] = cn_u8[s, c]
                else:
                    row = 16 * int(first_block[i]) + c
                    if first_block[i] < 0 or (row >> 4) >= src["n_blocks"]:
                        continue
                    cn[i, c] = image_row(cn_u8, row)
                f2[i, c], mk[i, c] = f2_u8[s, c], mask[s, c]
        outs.append((cn, f2, mk))
    return outs


def batch_of(form, src, n, seed):
    """-> (slots (n,), first_block (n,)) int64: every slot, one twice, -1 and n_videos, a dead and an outside first block."""
    rng = np.random.default_rng(seed)
    nv = len(src["vlen"])
    slots = rng.integers(0, nv, n)
    special = {}
    if n >= 3:
        slots[0], slots[1], slots[2] = 4, 4, 5                # the same slot twice; the run that crosses 7 | 8; the last block
    if n >= 130:
        slots[3:3 + nv] = np.arange(nv)
        slots[20], slots[21], slots[22] = -1, nv, 2 ** 31 - 1
        special = {30: -1, 31: src["n_blocks"], 32: src["n_blocks"] - 1, 33: -2 ** 31}
    first = np.where((slots >= 0) & (slots < nv), src["first"][np.clip(slots, 0, nv - 1)], 7)
    for i, fb in special.items():
        slots[i], first[i] = 5, fb                            # slot 5: 128 valid clips, so every row depends on the block check
    return slots.astype(np.int64), first.astype(np.int64)


def device_operands(form, src, dtype, hidden):
    nv, lpad = len(src["vlen"]), src["lpad"]
    cn_src, f2_src, mask_src = [], [], []
    for mod in src["mods"]:
        data = mod["cn_u8"].to(DEV).view(-1).view(dtype)
        cn_src.append(data.view(nv, lpad, hidden) if form == "rows" else ops.TiledRows(data, nv * 128, hidden, (nv, 128, hidden)))
        f2_src.append(mod["f2_u8"].to(DEV).view(-1).view(dtype).view(nv, lpad, hidden))
        mask_src.append(mod["mask"].to(DEV))
    return cn_src, f2_src, mask_src


@pytest.mark.parametrize("n_mod", [1, 2])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype, hidden", SHAPES)
def test_gather_video_rows_against_the_numpy_layout(dtype, hidden, form, n_mod):
    src = make_source(form, dtype, hidden, n_mod, 300 + hidden + 10 * n_mod + FORMS.index(form))
    if form == "plan":                                         # the plan's own row map agrees with the first blocks used here
        rm = src["plan"].row_map.numpy()
        assert (rm[src["first"] * 16] == np.arange(len(VLENS)) * 128).all()
    if form == "packed":
        assert PACKED_FIRST[4] % 16 < 8 < PACKED_FIRST[4] % 16 + 7 and PACKED_FIRST[5] + 8 == 16 * PACKED_TILES
    cn_src, f2_src, mask_src = device_operands(form, src, dtype, hidden)
    keep = [t.clone() for t in f2_src] + [(t if form == "rows" else t.data).clone() for t in cn_src]
    vlen = torch.from_numpy(src["vlen"]).to(DEV)
    rb = hidden * torch.empty(0, dtype=dtype).element_size()
    lengths = [1, 17, 32] if form == "rows" else [1, 17, 100, 128]
    n_rows = 0
    for length in lengths:
        for n in (1, 3, 130):
            slots, first = batch_of(form, src, n, 7 * n + length)
            sd = torch.from_numpy(slots.astype(np.int32)).to(DEV)
            fd = torch.from_numpy(first.astype(np.int32)).to(DEV)
            out = [(torch.full((n, length, rb), 0xFF, dtype=torch.uint8, device=DEV).view(dtype).view(n, length, hidden),
                    torch.full((n, length, rb), 0xFF, dtype=torch.uint8, device=DEV).view(dtype).view(n, length, hidden),
                    torch.full((n, length), float("nan"), dtype=torch.float32, device=DEV)) for _ in range(n_mod)]
            got = ops.index_gather_video_rows(sd, None if form == "rows" else fd, vlen, cn_src, f2_src, mask_src, length,
                                              n_blocks=src["n_blocks"], out=out)
            torch.cuda.synchronize()
            want = model(form, src, slots, first, length)
            for m in range(n_mod):
                assert got[m][0].data_ptr() == out[m][0].data_ptr()
                for name, g, w in zip(("cn", "f2"), got[m][:2], want[m][:2]):
                    gb = g.contiguous().view(torch.uint8).cpu().numpy().reshape(n, length, rb)
                    bad = np.nonzero((gb != w).any(2))
                    assert not len(bad[0]), "%s modality %d, L %d, n %d: %d rows differ, the first (item, clip) (%d, %d), slot %d" % (
                        name, m, length, n, len(bad[0]), bad[0][0], bad[1][0], slots[bad[0][0]])
                assert (got[m][2].cpu().numpy().view(np.uint32) == want[m][2].view(np.uint32)).all(), ("mask", m, length, n)
                n_rows += int((want[m][2] != 0).sum())
    fresh = ops.index_gather_video_rows(sd, None if form == "rows" else fd, vlen, cn_src, f2_src, mask_src, length,
                                        n_blocks=src["n_blocks"])      # the wrapper's own outputs: same bits
    for m in range(n_mod):
        for a, b in zip(fresh[m], got[m]):
            assert a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))
    for t, k in zip(f2_src + [(t if form == "rows" else t.data) for t in cn_src], keep):
        assert torch.equal(t.view(torch.uint8), k.view(torch.uint8)), "a source was written"
    assert n_rows > 1000


def test_the_wrapper_refuses_what_does_not_fit():
    from tvretrieval_amd._lib import XmlHipError
    dt, hidden = torch.bfloat16, 128
    src = make_source("fixed", dt, hidden, 2, 1)
    cn_src, f2_src, mask_src = device_operands("fixed", src, dt, hidden)
    vlen = torch.from_numpy(src["vlen"]).to(DEV)
    ids = torch.zeros(3, dtype=torch.int32, device=DEV)
    ops.index_gather_video_rows(ids, ids, vlen, cn_src, f2_src, mask_src, 5, n_blocks=src["n_blocks"])
    for bad in (dict(length=129), dict(length=0), dict(n_blocks=src["n_blocks"] + 64), dict(n_blocks=0), dict(first_block=None),
                dict(first_block=ids[:2]), dict(vlen=vlen[:3]), dict(slots=ids.long()), dict(f2_src=f2_src[:1]),
                dict(cn_src=[cn_src[0], f2_src[1]]), dict(mask_src=[mask_src[0], mask_src[1][:, :64].contiguous()])):
        a = dict(slots=ids, first_block=ids, vlen=vlen, cn_src=cn_src, f2_src=f2_src, mask_src=mask_src, length=5,
                 n_blocks=src["n_blocks"])
        a.update(bad)
        with pytest.raises(XmlHipError):
            ops.index_gather_video_rows(**a)
    rows = [f2_src[0][:, :32].contiguous()]                   # row-major: hidden % 8 suffices, but 100 is not
    with pytest.raises(XmlHipError):
        odd = torch.zeros((8, 32, 100), dtype=dt, device=DEV)
        ops.index_gather_video_rows(ids, None, vlen, [odd], [odd], [mask_src[0][:, :32].contiguous()], 5)
    ops.index_gather_video_rows(ids, None, vlen, rows, rows, [mask_src[0][:, :32].contiguous()], 5)
