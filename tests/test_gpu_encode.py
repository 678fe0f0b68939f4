"""The encode stage on the GPU (rt_encode_atlas / rt_encode_atlas_device, k_encode_atlas of csrc/k_encode.hip.h) against the
numpy restatement of the encoding rule (tests/encode_util.py, held to paper by tests/test_encode_model.py): every word, both
formats, at sizes of one texel, one row, one column, a partial second and a partial third workgroup, on the special values
scattered among random colours with w in {-1, -2, 0.3}.  Where the model's half is a NaN the device's need only be one.  The
host and the device entry agree, the input is not written, RT_LIGHTMAP_F32 is the bytes unchanged, and the refusals are
RT_ERR_INVALID with the prefix "encode atlas:" and leave the context usable.  No scene is uploaded anywhere here."""
import ctypes

import numpy as np
import pytest

import encode_util as eu

pytestmark = pytest.mark.gpu

RT_ERR_INVALID = -1
SIZES = ((1, 1), (1, 9), (9, 1), (17, 33), (64, 5))   # 17 x 33 = 561 texels: a partial third workgroup; 64 x 5 = 320: a second


@pytest.fixture(scope="module")
def r(W):
    W._build.build_rt()
    renderer = W.WebGPURenderer(0)
    yield renderer
    renderer.destroy()


@pytest.fixture(scope="module")
def cases():
    """size -> (atlas, model RGBE8 words, model halves), made once"""
    out = {}
    for k, (width, height) in enumerate(SIZES):
        a = eu.special_atlas(width, height, 20 + k)
        out[(width, height)] = (a, eu.encode_rgbe(a).reshape(height, width), eu.encode_f16(a).reshape(height, width, 4))
    return out


def test_the_inputs_are_not_empty(cases):
    a, rgbe, f16 = cases[(17, 33)]
    w = a[:, :, 3].ravel()
    assert all((w == v).any() for v in np.array([-1.0, -2.0, 0.3], np.float32))
    assert (rgbe == 0).any() and (rgbe != 0).sum() > 100 and np.isnan(a).any() and np.isinf(a).any()
    assert eu.f16_is_nan(f16).any() and ((f16 & 0x7fff) == 0x7c00).any()
    assert len(np.unique(rgbe >> 24)) > 30


@pytest.mark.parametrize("size", SIZES)
def test_every_word_is_the_models(r, cases, size):
    width, height = size
    a, rgbe, f16 = cases[size]
    before = a.copy()
    got = r.encodeAtlas(a, "rgbe")
    assert got.shape == (height, width) and got.dtype == np.uint32
    assert np.array_equal(got, rgbe), np.argwhere(got != rgbe)[:8].tolist()
    half = r.encodeAtlas(a, "f16")
    assert half.shape == (height, width, 4) and half.dtype == np.float16
    assert eu.same_f16(half.view(np.uint16), f16)
    same = r.encodeAtlas(a, "f32")
    assert np.array_equal(same.view(np.uint32).reshape(-1), a.view(np.uint32).reshape(-1))
    assert np.array_equal(a.view(np.uint32), before.view(np.uint32)), "the input was written"


def test_the_device_entry_agrees_and_leaves_its_input(r, cases):
    import torch
    for size in ((17, 33), (1, 1)):
        width, height = size
        a, rgbe, f16 = cases[size]
        d_in = torch.from_numpy(a.view(np.int32).copy()).to("cuda")
        room = max(width * height * 4, 4)
        d_rgbe = torch.full((room,), 0x55555555, dtype=torch.int32, device="cuda")      # room for every format; the tail must stay
        d_f16 = torch.full((room,), 0x55555555, dtype=torch.int32, device="cuda")
        d_f32 = torch.full((room,), 0x55555555, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        r.encodeAtlasDevice(d_in.data_ptr(), width, height, "rgbe", d_rgbe.data_ptr(), width * height * 4)
        r.encodeAtlasDevice(d_in.data_ptr(), width, height, "f16", d_f16.data_ptr(), width * height * 8)
        r.encodeAtlasDevice(d_in.data_ptr(), width, height, "f32", d_f32.data_ptr(), width * height * 16)
        r.sync()
        n = width * height
        got = d_rgbe.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[:n], rgbe.ravel()) and (got[n:] == 0x55555555).all(), "RGBE8: words, and nothing behind them"
        got = d_f16.cpu().numpy().view(np.uint32)
        assert eu.same_f16(got[:2 * n].view(np.uint16), f16) and (got[2 * n:] == 0x55555555).all()
        assert np.array_equal(d_f32.cpu().numpy().view(np.uint32), a.view(np.uint32).ravel())
        assert np.array_equal(d_in.cpu().numpy().view(np.uint32), a.view(np.uint32)), "the input was written"
        assert np.array_equal(r.encodeAtlas(a, "rgbe"), rgbe)


def test_refusals(r, cases):
    import torch
    a, rgbe, f16 = cases[(9, 1)]
    out = np.full(9 * 4, 0x77777777, np.uint32)
    L, ctx = r.L, r.ctx

    def host(width=9, height=1, fmt=eu.RGBE8, src=a.ctypes.data, dst=out.ctypes.data, room=out.nbytes):
        return L.rt_encode_atlas(ctx, width, height, fmt, src, dst, room)

    d_in = torch.from_numpy(a.view(np.int32).copy()).to("cuda")
    d_out = torch.full((9 * 4,), 0x77777777, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def dev(width=9, height=1, fmt=eu.RGBE8, src=d_in.data_ptr(), dst=d_out.data_ptr(), room=9 * 16):
        return L.rt_encode_atlas_device(ctx, width, height, fmt, src, dst, room)

    for call in (host, dev):
        bad = [dict(width=0), dict(height=0), dict(width=4097, height=4096), dict(width=1 << 24, height=2),
               dict(width=1 << 31, height=1 << 31), dict(fmt=3), dict(fmt=0xffffffff), dict(src=None), dict(dst=None),
               dict(room=9 * 4 - 1), dict(fmt=eu.F16, room=9 * 8 - 1), dict(fmt=eu.F32, room=9 * 16 - 1), dict(room=0)]
        for kw in bad:
            assert call(**kw) == RT_ERR_INVALID, (call.__name__, kw)
            assert L.rt_last_error(ctx).startswith(b"encode atlas:"), (kw, L.rt_last_error(ctx))
    for kw in (dict(src=d_in.data_ptr() + 8), dict(dst=d_out.data_ptr() + 4), dict(dst=d_in.data_ptr())):   # misaligned, in place
        assert dev(**kw) == RT_ERR_INVALID, kw
        assert L.rt_last_error(ctx).startswith(b"encode atlas:"), (kw, L.rt_last_error(ctx))
    with pytest.raises(ValueError):
        r.encodeAtlas(a, "rgbm")
    with pytest.raises(ValueError):
        r.encodeAtlas(a[:, :, 0:3], "rgbe")
    r.sync()
    assert (out == 0x77777777).all() and (d_out.cpu().numpy().view(np.uint32) == 0x77777777).all(), "a refused call wrote"
    # the context is as usable as before, and the exact sizes are accepted
    assert host() == 0 and np.array_equal(out[:9], rgbe.ravel()) and (out[9:] == 0x77777777).all()
    assert dev(room=9 * 4) == 0
    r.sync()
    assert np.array_equal(d_out.cpu().numpy().view(np.uint32)[:9], rgbe.ravel())
