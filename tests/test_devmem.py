"""ray_tracer_amd/devmem.py: the owner class every device buffer of the Python side goes through."""
import numpy as np
import pytest

from ray_tracer_amd import devmem, engine

GUARD = 64


@pytest.mark.gpu
@pytest.mark.parametrize("nbytes", [0, 1, 4097])
def test_device_buffer_round_trip(renderer, nbytes):
    """A seeded pattern comes back bit for bit, fill(7) gives sevens, and no copy reaches past `nbytes`: on the host a guard behind
    the destination stays as it was, on the device DeviceBuffer refuses every span that would leave the allocation."""
    pattern = np.random.default_rng(nbytes).integers(0, 256, nbytes, dtype=np.uint8)
    with devmem.DeviceBuffer(nbytes) as b:
        assert b.ptr and b.nbytes == nbytes
        got = b.upload(pattern).download()
        assert got.dtype == np.uint8 and got.shape == (nbytes,) and np.array_equal(got, pattern)
        into = np.full(nbytes + GUARD, 0xEE, np.uint8)
        b.download(into=into[:nbytes])
        assert np.array_equal(into[:nbytes], pattern) and (into[nbytes:] == 0xEE).all()      # nothing written past nbytes on the host
        assert (b.fill(7).download() == 7).all()
        if nbytes >= 4:
            assert b.download((nbytes // 4,), np.uint32)[0] == 0x07070707
        for bad in (lambda: b.upload(np.zeros(nbytes + 1, np.uint8)), lambda: b.download(nbytes + 1),
                    lambda: b.upload(np.zeros(1, np.uint8), offset=nbytes), lambda: b.download(1, offset=nbytes)):
            with pytest.raises(ValueError):
                bad()                                                                        # nothing read or written past nbytes
        assert (b.download() == 7).all()
    assert b.ptr is None
    b.free()                                                                                 # twice is harmless
    with pytest.raises(engine.RtError):
        b.download()


@pytest.mark.gpu
def test_the_renderers_named_buffers_grow_and_go_with_it(built):
    r = engine.Renderer(0)
    p = r._device_buffer("x", 16)
    small = r._owned["x"]
    assert isinstance(p, int) and p == small.ptr and small.nbytes >= 16 and r._device_buffer("x", 8) == p
    q = r._device_buffer("x", 4097)
    big = r._owned["x"]
    assert isinstance(q, int) and q == big.ptr and big.nbytes >= 4097 and small.ptr is None and r._owned == {"x": big}
    pattern = np.arange(4097, dtype=np.uint32).astype(np.uint8)
    assert np.array_equal(big.upload(pattern).download(), pattern)
    r.close()
    assert big.ptr is None and r._owned == {}
