"""inference.pack_video_allow on the host: the allow-bit layout of a restricted search (video v = bit v & 31 of word
v >> 5, padding bits 0) against numpy's own little-endian bit packing."""
import numpy as np
import pytest
import torch

from tvretrieval_amd.inference import pack_video_allow


def _want(a):
    a = np.atleast_2d(a)
    pad = (-a.shape[1]) % 32
    return np.packbits(np.pad(a, ((0, 0), (0, pad))), axis=1, bitorder="little").view(np.int32)


@pytest.mark.parametrize("nv", [1, 31, 32, 33, 300])
@pytest.mark.parametrize("rows", [None, 1, 7])
def test_pack_matches_numpy_packbits(nv, rows):
    rng = np.random.default_rng(100 * nv + (rows or 0))
    a = rng.random((nv,) if rows is None else (rows, nv)) < 0.5
    a.reshape(-1)[0] = True
    a.reshape(-1)[-1] = True                                   # the last video: the highest bit in use
    w = pack_video_allow(a)
    assert isinstance(w, np.ndarray) and w.dtype == np.int32 and w.flags["C_CONTIGUOUS"]
    assert w.shape == ((rows or 1), (nv + 31) // 32)
    assert np.array_equal(w, _want(a))
    # unpacking gives the input back, and the padding bits are 0
    bits = np.unpackbits(w.view(np.uint8), axis=1, bitorder="little")
    assert np.array_equal(bits[:, :nv].astype(bool), np.atleast_2d(a))
    assert not bits[:, nv:].any()
    # a CPU tensor is host input too
    wt = pack_video_allow(torch.from_numpy(a))
    assert isinstance(wt, np.ndarray) and np.array_equal(wt, w)


def test_pack_all_and_none():
    for nv in (1, 32, 45):
        ones = pack_video_allow(np.ones(nv, dtype=bool))
        assert np.array_equal(ones, _want(np.ones(nv, dtype=bool)))
        assert ones.view(np.uint32)[0, -1] == (0xffffffff >> ((-nv) % 32))
        assert not pack_video_allow(np.zeros((3, nv), dtype=bool)).any()


def test_pack_rejects_wrong_dtype_and_shape():
    with pytest.raises(ValueError, match="bool"):
        pack_video_allow(np.ones(8, dtype=np.int32))
    with pytest.raises(ValueError, match="bool"):
        pack_video_allow(torch.ones(8))
    with pytest.raises(ValueError, match="shape"):
        pack_video_allow(np.ones((2, 3, 4), dtype=bool))
    with pytest.raises(ValueError, match="shape"):
        pack_video_allow(np.ones((2, 0), dtype=bool))
    with pytest.raises(ValueError, match="shape"):
        pack_video_allow(np.bool_(True))
