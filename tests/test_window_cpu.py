"""CPU: the parts of the residue-window feature that need no device -- crop_starts on host tensors, the argument rules of
decode_tensors / decode_angles / tensor_batches (raised before any device work), the NULL-ctx refusal of the four entry points."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from foldcomp_amd import _lib, api, tensors
from foldcomp_amd.structure import CAtomsOut, CDenseOut

NEW = ("fcz_dense_window_dev", "fcz_decompress_dense_window", "fcz_angles_window_dev", "fcz_decompress_angles_window")
LENS = [0, 1, 2, 63, 64, 65, 66, 128, 129, 300, 1400, 65535]


def test_crop_starts_formulas_and_range():
    import torch
    L = 64
    length = torch.tensor(LENS, dtype=torch.int32)
    span = np.maximum(np.asarray(LENS) - L, 0)
    for how, exp in (("start", np.zeros(len(LENS), np.int64)), ("center", span // 2)):
        s = tensors.crop_starts(length, L, how)
        assert s.dtype == torch.int32 and s.device.type == "cpu" and tuple(s.shape) == (len(LENS),) and s.is_contiguous()
        assert np.array_equal(s.numpy(), exp), how
    draws = []
    for seed in range(40):
        g = torch.Generator(); g.manual_seed(seed)
        s = tensors.crop_starts(length, L, "random", g).numpy()
        assert s.dtype == np.int32 and (s >= 0).all() and (s <= span).all() and not s[np.asarray(LENS) <= L].any()
        g2 = torch.Generator(); g2.manual_seed(seed)
        assert np.array_equal(s, tensors.crop_starts(length, L, "random", g2).numpy())
        draws.append(s)
    draws = np.stack(draws)
    # len = L + 1 has the two starts 0 and 1, len = L + 2 the three 0 .. 2: 40 seeded draws reach every one of them
    assert set(draws[:, LENS.index(65)]) == {0, 1} and set(draws[:, LENS.index(66)]) == {0, 1, 2}
    assert draws[:, LENS.index(65535)].max() > (65535 - L) // 2 > draws[:, LENS.index(65535)].min()
    # one generator drawn from twice moves on
    g = torch.Generator(); g.manual_seed(0)
    big = torch.full((64,), 1000, dtype=torch.int32)
    assert not np.array_equal(tensors.crop_starts(big, L, "random", g).numpy(), tensors.crop_starts(big, L, "random", g).numpy())
    # no generator: torch's default one
    s = tensors.crop_starts(big, L, "random").numpy()
    assert (s >= 0).all() and (s <= 1000 - L).all()
    # int64 lengths, no entry at all
    assert np.array_equal(tensors.crop_starts(length.to(torch.int64), L, "center").numpy(), span // 2)
    assert tuple(tensors.crop_starts(torch.zeros(0, dtype=torch.int32), L, "random").shape) == (0,)


def test_crop_starts_given_starts():
    import torch
    length = torch.tensor([10, 20, 30], dtype=torch.int32)
    for how in ([0, 5, 40], np.asarray([0, 5, 40], np.uint32), np.asarray([0, 5, 40], np.int64), torch.tensor([0, 5, 40])):
        s = tensors.crop_starts(length, 8, how)
        assert s.dtype == torch.int32 and s.tolist() == [0, 5, 40]
    assert tensors.crop_starts(length, 8, np.asarray([0, 2 ** 32 - 1, 2 ** 31], np.uint32)).tolist() == [0, 2 ** 31 - 1, 2 ** 31 - 1]
    for bad in ([0, 1], [[0, 1, 2]], [0.0, 1.0, 2.0], [0, -1, 2], torch.tensor([0, -1, 2]), torch.tensor([0.5, 1, 2]), "middle"):
        with pytest.raises(ValueError):
            tensors.crop_starts(length, 8, bad)
    with pytest.raises(ValueError):
        tensors.crop_starts(length, 0, "center")


def test_argument_rules_need_no_device():
    api.check_crop(None, None, False); api.check_crop(None, None, True); api.check_crop("random", 64, False); api.check_crop([1, 2], 64, False)
    for crop, max_len, packed in (("random", None, False), ("center", 64, True), ([1, 2], None, False), ("middle", 64, False)):
        with pytest.raises(ValueError):
            api.check_crop(crop, max_len, packed)
    # the public functions raise them before they look for torch's device or a codec (a device that does not exist is never reached)
    for fn in (tensors.decode_tensors, tensors.decode_angles):
        for kw in (dict(crop="random"), dict(crop="center", packed=True), dict(crop="middle", max_len=64), dict(crop=[0], packed=True, max_len=None)):
            with pytest.raises(ValueError):
                fn([b"x"], device="cuda:99", **kw)

    class NoRecords(api.FoldcompDatabase):
        def __init__(self):
            pass

        def __len__(self):
            raise AssertionError("tensor_batches read the database before it checked its arguments")

    for kw in (dict(crop="random"), dict(crop="center", packed=True), dict(crop="middle", max_len=64), dict(crop=[0, 1], max_len=64)):
        with pytest.raises(ValueError):
            next(NoRecords().tensor_batches(4, **kw))


def test_entry_points_refuse_a_null_ctx():
    lib = _lib.load()
    assert set(NEW) <= set(_lib.EXPORTS)
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data
    atoms = CAtomsOut(p, p, p, p, p, None)
    out = CDenseOut(p, p, None, None, None, None)
    w = ctypes.c_uint32(0)
    assert lib.fcz_dense_window_dev(None, p, p, 1, p, p, ctypes.byref(atoms), 0, 0, 8, p, ctypes.byref(out)) == -1
    assert lib.fcz_decompress_dense_window(None, p, p, 1, 0, 0, p, ctypes.byref(w), ctypes.byref(out), None) == -1
    assert lib.fcz_angles_window_dev(None, p, p, 1, p, 8, p, p, p, p) == -1
    assert lib.fcz_decompress_angles_window(None, p, p, 1, 0, p, ctypes.byref(w), p, p, p, None) == -1
    assert not buf.any() and w.value == 0


def test_tensors_module_still_imports_without_torch():
    code = ("import sys; import foldcomp, foldcomp_amd.tensors as t; assert 'torch' not in sys.modules, 'torch imported'; "
            "assert callable(t.crop_starts) and 'crop_starts' in t.__all__")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
