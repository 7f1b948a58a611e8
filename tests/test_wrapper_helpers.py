"""The Python wrapper's shared helpers (godotoceanwaves_amd/wave_generator.py): device addresses, the device-buffer size check and the host
arrays of a picture call.  No library and no GPU: device buffers are fakes with data_ptr(), numel() and element_size().
"""
import numpy as np
import pytest

from godotoceanwaves_amd import _lib
from godotoceanwaves_amd import wave_generator as wg
from godotoceanwaves_amd.wave_generator import WaveGenerator as W


class FakeBuffer:
    """what the wrapper reads of a torch tensor: `nbytes` bytes of uint8 at `address`"""

    def __init__(self, nbytes, address=0x7000):
        self.nbytes, self.address = nbytes, address

    def data_ptr(self):
        return self.address

    def numel(self):
        return self.nbytes

    def element_size(self):
        return 1


def test_addr_of_a_buffer_an_int_and_none():
    for optional in (False, True):
        assert wg._addr(FakeBuffer(16, 0x1234), optional) == 0x1234
        assert wg._addr(0x5678, optional) == 0x5678
    assert wg._addr(None, True) is None          # a picture call's output that is not asked for
    with pytest.raises(TypeError):
        wg._addr(None)                           # the point calls take no None


def test_ref_and_scales():
    assert wg._ref(None) is None
    cam = W.camera((0, 0, 0), np.eye(3), 60.0, 4, 4, 10.0)
    assert wg._ref(cam)._obj is cam
    sc = wg._scales([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0])
    assert sc.shape == (2, 4) and sc.dtype == np.float32 and sc.flags.c_contiguous


@pytest.mark.parametrize("args,text", [
    ((), "out_device holds fewer than 3 records of 128 bytes"),
    (("points_device",), "points_device holds fewer than 3 records of 128 bytes"),
    (("a device buffer", "pixels"), "a device buffer holds fewer than 3 pixels of 128 bytes"),
])
def test_device_size_check(args, text):
    with pytest.raises(ValueError) as e:
        wg._check_device_size(FakeBuffer(3 * 128 - 1), 3, 128, *args)    # one byte short
    assert str(e.value) == text
    wg._check_device_size(FakeBuffer(3 * 128), 3, 128, *args)            # the exact size
    wg._check_device_size(0x7000, 3, 128, *args)                         # a bare address says nothing about its size


def test_async_methods_raise_the_three_texts():
    """the methods that check their device buffers do so before they touch the library: a generator that was never initialised is enough"""
    gen = W()
    sc = np.ones((1, 4), np.float32)
    with pytest.raises(ValueError, match=f"^out_device holds fewer than 2 records of {W.SURFACE_QUERY.itemsize} bytes$"):
        gen.query_surface_async(FakeBuffer(16), sc, FakeBuffer(2 * W.SURFACE_QUERY.itemsize - 1), count=2)
    with pytest.raises(ValueError, match=f"^points_device holds fewer than 2 records of {W.BUOYANCY_POINT.itemsize} bytes$"):
        gen.buoyancy_async(0x1000, 0x2000, sc, FakeBuffer(W.BUOYANCY_RESULT.itemsize), FakeBuffer(2 * W.BUOYANCY_POINT.itemsize - 1), num_bodies=1,
                           num_points=2)
    cam = W.camera((0, 0, 0), np.eye(3), 60.0, 4, 2, 10.0)
    with pytest.raises(ValueError, match="^a device buffer holds fewer than 8 pixels of 4 bytes$"):
        gen.render_view_async(cam, sc, FakeBuffer(8 * 4 - 1))
    with pytest.raises(ValueError, match=f"^a device buffer holds fewer than 8 pixels of {W.RENDER_PIXEL.itemsize} bytes$"):
        gen.spray_draw_async(None, None, cam, FakeBuffer(8 * 4), FakeBuffer(8 * W.RENDER_PIXEL.itemsize - 1))


def test_picture_arrays():
    cam = W.camera((0, 0, 0), np.eye(3), 60.0, 5, 3, 10.0)     # 5 wide, 3 high
    rgba, rec = W._picture(cam, None, True)
    assert rgba.shape == (3, 5, 4) and rgba.dtype == np.uint8 and rec is None
    rgba, rec = W._picture(cam, None, False)                    # no records: the image is the only output, wanted or not
    assert rgba.shape == (3, 5, 4) and rec is None
    given = np.zeros((3, 5), W.RENDER_PIXEL)
    given["t"] = 7.0
    rgba, rec = W._picture(cam, given, True)
    assert rgba.shape == (3, 5, 4) and rec.shape == (3, 5) and rec.dtype == W.RENDER_PIXEL
    assert rec is not given and rec.flags.c_contiguous and (rec["t"] == 7.0).all()      # a copy: the call rewrites it
    rgba, rec = W._picture(cam, given, False)                   # the one case without an image
    assert rgba is None and rec.shape == (3, 5)
    rgba, rec = W._picture(cam, True, True)                     # fresh records (render_view, mesh_draw)
    assert rgba.shape == (3, 5, 4) and rec.shape == (3, 5) and rec.dtype == W.RENDER_PIXEL and not rec.view(np.uint8).any()
    for shape in ((5, 3), (15,), (3, 4)):
        with pytest.raises(ValueError, match="pixels is"):
            W._picture(cam, np.zeros(shape, W.RENDER_PIXEL), True)
    for w, h in ((_lib.OW_RENDER_MAX_SIDE + 1, 2), (2, _lib.OW_RENDER_MAX_SIDE + 1)):   # refused by the library: nothing that size is allocated
        big = W.camera((0, 0, 0), np.eye(3), 60.0, w, h, 10.0)
        rgba, rec = W._picture(big, True, True)
        assert rgba.shape == (1, 1, 4) and rec.shape == (1, 1)
        rgba, rec = W._picture(big, np.zeros((3, 5), W.RENDER_PIXEL), True)             # ... and the records' shape is the library's to refuse
        assert rgba.shape == (1, 1, 4) and rec.shape == (3, 5)
