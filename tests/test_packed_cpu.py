"""CPU: the batch cutting of FoldcompDatabase.tensor_batches(packed=True, max_residues=...) as a pure function, and the argument
checks of the packed entry points that answer before anything touches a device."""
import ctypes

import numpy as np
import pytest

from foldcomp_amd import _lib
from foldcomp_amd.api import check_batch_cut, cut_batches
from foldcomp_amd.structure import CAtomsOut, CChainBatch, CDenseIn, CPackedOut

LENS = [350, 20, 700, 64, 64, 1300, 5, 5, 5, 900, 128, 2700, 33, 410, 2]


def flat(batches):
    return [k for b in batches for k in b]


@pytest.mark.parametrize("sort", [False, True])
@pytest.mark.parametrize("budget", [1, 64, 128, 1024, 2048, 2700, 10 ** 9])
@pytest.mark.parametrize("batch_size", [1, 3, 1024])
def test_budget_cap_order_and_oversize(sort, budget, batch_size):
    got = cut_batches(LENS, batch_size, budget, sort)
    order = flat(got)
    assert sorted(order) == list(range(len(LENS)))                                 # every entry once: nothing dropped
    assert order == (sorted(range(len(LENS)), key=lambda k: LENS[k]) if sort else list(range(len(LENS))))
    for b in got:
        assert 1 <= len(b) <= batch_size
        assert sum(LENS[k] for k in b) <= budget or len(b) == 1                   # over budget only alone
    # greedy: a batch closes only because the next entry would not fit or the cap is reached
    for b, nxt in zip(got, got[1:]):
        assert len(b) == batch_size or sum(LENS[k] for k in b) + LENS[nxt[0]] > budget


def test_without_a_budget_and_empty_input():
    assert cut_batches([], 4, 100) == [] and cut_batches([], 4) == []
    assert cut_batches([7] * 10, 4) == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9]]
    assert cut_batches([3, 1, 2], 2, None, True) == [[1, 2], [0]]
    assert cut_batches([5, 5, 5], 8, 10) == [[0, 1], [2]]
    assert cut_batches([0, 0, 11, 0], 8, 10) == [[0, 1], [2], [3]]               # an oversize entry goes alone
    assert cut_batches(np.asarray([4, 4], np.uint16), 8, 8) == [[0, 1]]
    # equal lengths keep their order under the sort
    assert flat(cut_batches([9, 3, 9, 3], 8, None, True)) == [1, 3, 0, 2]
    for bad in (dict(batch_size=0), dict(batch_size=2, max_residues=0)):
        with pytest.raises(ValueError):
            cut_batches([1, 2], **bad)


def test_argument_rules():
    check_batch_cut(False, None, None); check_batch_cut(False, 64, None); check_batch_cut(True, None, None); check_batch_cut(True, None, 4096)
    with pytest.raises(ValueError):
        check_batch_cut(False, None, 4096)                                         # max_residues without packed
    with pytest.raises(ValueError):
        check_batch_cut(True, 64, None)                                            # max_len with packed
    with pytest.raises(ValueError):
        check_batch_cut(True, None, 0)


def test_packed_entry_points_refuse_bad_arguments_without_a_device():
    lib = _lib.load()
    E = -1
    # no device on this path: the checks below answer before the ctx is looked into, so a block of zeros stands in for it
    fake = ctypes.create_string_buffer(4096)
    ctx = ctypes.cast(fake, ctypes.c_void_p)
    buf = np.zeros(1024, np.uint8)
    ptr = buf.ctypes.data
    atoms = CAtomsOut(ptr, ptr, ptr, ptr, ptr, None)
    out = CPackedOut(ptr, ptr, None, None, None, None, None)
    no_pos, no_mask = CPackedOut(None, ptr), CPackedOut(ptr, None)

    def dense(c=ctx, layout=0, o=out):
        return lib.fcz_dense_packed_dev(c, ptr, ptr, 1, ptr, ptr, ctypes.byref(atoms), 0, layout, ctypes.byref(o) if o is not None else None)

    assert dense(c=None) == E and dense(layout=3) == E and dense(layout=-1) == E and dense(o=no_pos) == E and dense(o=no_mask) == E and dense(o=None) == E
    R = ctypes.c_uint32(7)

    def host(c=ctx, layout=0, o=out, r=ctypes.byref(R)):
        return lib.fcz_decompress_dense_packed(c, ptr, ptr, 1, layout, r, None, ctypes.byref(o) if o is not None else None, None)

    assert host(c=None) == E and host(layout=5) == E and host(o=no_pos) == E and host(o=no_mask) == E and host(o=None, r=None) == E
    s = CDenseIn(ptr, ptr, ptr, None)
    counts = np.zeros(3, np.uint32); nbytes = ctypes.c_uint64(0); batch = CChainBatch()

    def encode(c=ctx, sp=s, ro=ptr, layout=0, thr=25):
        spp = ctypes.byref(sp) if sp is not None else None
        r = [f(c, spp, ro, 1, 8, layout, thr, counts.ctypes.data, ctypes.byref(nbytes))
             for f in (lib.fcz_compress_dense_packed_begin_dev, lib.fcz_compress_dense_packed_begin)]
        return r + [lib.fcz_undense_packed_dev(c, spp, ro, 1, 8, layout, thr, ctypes.byref(batch), counts.ctypes.data, None)]

    assert encode(c=None) == [E] * 3 and encode(layout=3) == [E] * 3 and encode(thr=0) == [E] * 3 and encode(ro=None) == [E] * 3 and encode(sp=None) == [E] * 3
    for field in ("pos", "mask", "aatype"):
        s2 = CDenseIn.from_buffer_copy(s)
        setattr(s2, field, None)
        assert encode(sp=s2) == [E] * 3, field
