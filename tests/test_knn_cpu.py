"""CPU: the parts of the neighbour-graph feature that need no device -- the numpy restatement (tests/_knn.py) against a brute-force
sort over Python integers on an integer lattice, the pure-host ABI (fcz_knn_pass, the NULL-ctx refusals, the export list), and the
argument errors of foldcomp.neighbor_graph, raised before torch or a device is touched."""
import ctypes
import math

import numpy as np
import pytest

import _knn as K
from foldcomp_amd import _lib, api, tensors

NEW = ("fcz_knn_pass", "fcz_knn_dev", "fcz_knn_packed_dev", "fcz_knn", "fcz_knn_packed")


def _brute(points, site, k):
    """points: list of integer triples; exact integer d2, sorted by (d2, j) with Python's integers"""
    m = len(points)
    index = np.full((m, k), -1, np.int32)
    dist = np.zeros((m, k), np.float32)
    for i in range(m):
        if not site[i]:
            continue
        cand = sorted((sum((a - b) ** 2 for a, b in zip(points[j], points[i])), j) for j in range(m) if j != i and site[j])
        for c, (d2, j) in enumerate(cand[:k]):
            index[i, c] = j
            dist[i, c] = np.float32(math.sqrt(d2))                   # d2 < 2^24: the double root rounds to the float root
    return index, dist


@pytest.mark.parametrize("k", [1, 3, 8, 64])
def test_restatement_on_an_integer_lattice(k):
    rng = np.random.default_rng(5)
    pts = rng.integers(-4, 5, size=(90, 3))
    pts[10] = pts[3]; pts[11] = pts[3]; pts[80] = pts[79]            # duplicated points: d2 = 0, ties on j
    site = rng.random(90) > 0.1
    site[[3, 10, 11]] = True
    got = K.knn_chain(pts.astype(np.float32), site, k)
    exp = _brute([tuple(int(v) for v in p) for p in pts], site, k)
    K.same(got, exp, f"k={k}")
    assert (got[0][~site] == -1).all() and not got[1][~site].any()
    assert got[0][3, 0] == 10 and got[0][10, 0] == 3 and got[0][11, :2].tolist()[:min(k, 2)] == [3, 10][:min(k, 2)] and got[1][3, 0] == 0


def test_restatement_forms_agree():
    rng = np.random.default_rng(6)
    lens = [0, 1, 2, 5, 30]
    L, A, k = 32, 4, 4
    pos = rng.integers(-3, 4, size=(len(lens), L, A, 3)).astype(np.float32)
    mask = (rng.random((len(lens), L, A)) > 0.1).astype(np.uint8)
    pi, pd = K.knn_padded(pos, mask, np.asarray(lens), 1, k)
    row_off = np.concatenate([[0], np.cumsum(lens)])
    ppos = np.concatenate([pos[e, :n] for e, n in enumerate(lens)])
    pmask = np.concatenate([mask[e, :n] for e, n in enumerate(lens)])
    qi, qd = K.knn_packed(ppos, pmask, row_off, 1, k)
    for e, n in enumerate(lens):
        i = pi[e, :n]
        assert np.array_equal(np.where(i >= 0, i + row_off[e], -1), qi[row_off[e]:row_off[e + 1]])
        assert np.array_equal(K.bits(pd[e, :n]), K.bits(qd[row_off[e]:row_off[e + 1]]))
        assert (pi[e, n:] == -1).all() and not pd[e, n:].any()
    assert (pi[0] == -1).all() and (pi[1] == -1).all()               # no row, and one row: no neighbour


def test_pure_host_abi():
    lib = _lib.load()
    assert set(NEW) <= set(_lib.EXPORTS)
    assert lib.fcz_knn_pass() >= 0
    buf = np.zeros(256, np.uint8)
    p = buf.ctypes.data
    assert lib.fcz_knn_dev(None, p, p, None, 1, 4, 0, 1, 3, p, p) == -1
    assert lib.fcz_knn_packed_dev(None, p, p, p, 1, 4, 0, 1, 3, p, p) == -1
    assert lib.fcz_knn(None, p, p, None, 1, 4, 0, 1, 3, p, p) == -1
    assert lib.fcz_knn_packed(None, p, p, p, 1, 4, 0, 1, 3, p, p) == -1
    # packed rows are int32 in `index`: R above 2^31 - 1 is refused before anything is touched (the ctx is never read)
    fake = ctypes.c_void_p(buf.ctypes.data)
    assert lib.fcz_knn_packed_dev(fake, p, p, p, 1, 2 ** 31, 0, 1, 3, p, p) == -1
    assert lib.fcz_knn_packed(fake, p, p, p, 1, 2 ** 31, 0, 1, 3, p, p) == -1
    assert not buf.any()


def test_neighbor_graph_argument_errors_need_no_device():
    pos37, mask37 = np.zeros((2, 8, 37, 3), np.float32), np.zeros((2, 8, 37), np.uint8)
    pos4, mask4 = np.zeros((2, 8, 4, 3), np.float32), np.zeros((2, 8, 4), np.uint8)
    for kw in (dict(pos=pos37, mask=mask37, k=0), dict(pos=pos37, mask=mask37, k=65), dict(pos=pos4, mask=mask4, atom="CB"),
               dict(pos=pos37, mask=mask37, atom="XX"), dict(pos=pos37, mask=mask37, atom=37), dict(pos=pos4, mask=mask4, atom=4),
               dict(pos=pos37, mask=mask37, k=4.0), dict(pos=pos37, mask=mask37, atom=-1)):
        with pytest.raises(ValueError):
            tensors.neighbor_graph(**kw)
    # decode_tensors raises them before it looks for a device, tensor_batches (a generator: at the first next()) before it reads a record
    class NoRecords(api.FoldcompDatabase):
        def __init__(self):
            pass

        def __len__(self):
            raise AssertionError("tensor_batches read the database before it checked its arguments")

    for kw in (dict(neighbors=0), dict(neighbors=65), dict(neighbors=8, neighbor_atom="CB", layout="backbone4"), dict(neighbors=8, neighbor_atom="XX")):
        with pytest.raises(ValueError):
            tensors.decode_tensors([b"x"], device="cuda:99", **kw)
        with pytest.raises(ValueError):
            next(NoRecords().tensor_batches(4, device="cuda:99", **kw))
        with pytest.raises(ValueError):
            next(NoRecords().tensor_batches(4, packed=True, device="cuda:99", **kw))
