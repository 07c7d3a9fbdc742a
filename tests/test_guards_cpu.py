"""CPU: the guarded outputs of tests/_devpath.py see what the GPU tests rely on them to see: a byte written in front of or behind
an output fails fetch, any written byte ends untouched(), and the pointers, dtypes and shapes follow the spec. DevGuarded runs on
torch's CPU device here; its arithmetic is the same on the GPU."""
import ctypes

import numpy as np
import pytest

from _devpath import FILL, GUARD, DevGuarded, HostGuarded

SPEC = dict(index=(np.int32, (5, 3)), dist=(np.float32, (5, 3)), flag=(np.uint8, (7,)), none=(np.int64, (0, 4)))
KINDS = dict(host=HostGuarded, device=lambda spec, **kw: DevGuarded(spec, device="cpu", **kw))


def _base(g, k):
    """address of the first byte of the buffer behind output k"""
    return g.raw[k].ctypes.data if isinstance(g.raw[k], np.ndarray) else g.raw[k].data_ptr()


def _poke(address):
    """one byte written through the address, as a call writes through the pointers it is given"""
    ctypes.c_uint8.from_address(address).value = 0x11


@pytest.fixture(params=sorted(KINDS))
def make(request):
    return KINDS[request.param]


@pytest.mark.parametrize("guard", [GUARD, 6, 0])
def test_a_fresh_guard_follows_its_spec(make, guard):
    g = make(SPEC, guard=guard)
    assert g.untouched() and g.guard == guard and list(g.spec) == list(SPEC)
    assert g.ptrs() == [g.ptr(k) for k in SPEC]
    for k, (dtype, shape) in SPEC.items():
        nbytes = np.dtype(dtype).itemsize * int(np.prod(shape))
        assert g.ptr(k) == _base(g, k) + guard and len(g.raw[k]) == nbytes + 2 * guard
        a = g.fetch(k)
        assert a.dtype == np.dtype(dtype) and a.shape == tuple(shape) and (a.view(np.uint8) == FILL).all()
    assert [a.shape for a in g.all()] == [tuple(shape) for _, shape in SPEC.values()]
    assert make(SPEC).guard == GUARD == 256 and FILL == 0xA5


@pytest.mark.parametrize("k", ["dist", "none"])
def test_a_byte_in_front_of_or_behind_an_output_fails_fetch(make, k):
    nbytes = np.dtype(SPEC[k][0]).itemsize * int(np.prod(SPEC[k][1]))
    for guard in (GUARD, 6):
        for at in (-1, -guard, nbytes, nbytes + guard - 1):                   # the guard bytes next to the output and the outermost ones
            g = make(SPEC, guard=guard)
            _poke(g.ptr(k) + at)
            assert not g.untouched()
            with pytest.raises(AssertionError, match=k):
                g.fetch(k)
            with pytest.raises(AssertionError):
                g.all()
            for other in SPEC:                                                # the other outputs are still handed out
                if other != k:
                    g.fetch(other)


def test_a_written_output_is_seen_and_handed_out(make):
    g = make(SPEC, guard=8)
    _poke(g.ptr("dist"))
    _poke(g.ptr("flag") + 6)                                                  # the last byte of an output
    assert not g.untouched()
    index, dist, flag, none = g.all()
    assert dist.view(np.uint8)[0, 0] == 0x11 and (dist.view(np.uint8).ravel()[1:] == FILL).all()
    assert list(flag) == [FILL] * 6 + [0x11] and (index.view(np.uint8) == FILL).all() and none.size == 0
    # what fetch hands out is a copy: writing into it is no write into the output
    dist[:] = 0
    assert g.fetch("dist").view(np.uint8)[0, 1] == FILL
