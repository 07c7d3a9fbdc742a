"""GPU: the input checks of the torch-form analysis functions that need tensors on a device -- a mask that is not contiguous, of the
wrong dtype or left on the host, and packed chains whose cu_seqlens decreases or does not end at R. Every defect is refused in Python,
before any launch, with the type and the message pinned here; a valid call behind the refusals gives what it gave in front of them,
so a failed check leaves nothing enqueued. The checks that need no device: tests/test_analysis_errors_cpu.py."""
import pytest
import torch

import foldcomp_amd as foldcomp
from _cases import golden_records
from foldcomp_amd import api

pytestmark = pytest.mark.gpu

L = 8
ON = "every tensor must be on the codec's device"


@pytest.fixture(scope="module")
def batches(codec, golden):
    """two golden records cut to 8 rows as a padded batch, and the same rows packed: made once, never changed"""
    pad = foldcomp.decode_tensors(golden_records(golden)[:2], max_len=L, codec=codec)
    assert pad["pos"].shape == (2, L, 37, 3) and int(pad["length"].min()) >= L
    pad["length"] = pad["length"].clamp(max=L)                                # (encode_tensors refuses a length above L)
    packed = {k: pad[k].reshape((2 * L,) + tuple(pad[k].shape[2:])) for k in ("pos", "mask", "aatype", "plddt", "res_index")}
    packed["cu_seqlens"] = torch.tensor([0, L, 2 * L], dtype=torch.int32, device=pad["pos"].device)
    return dict(padded=pad, packed=packed)


def _pred(b):
    return dict(pos=b["pos"] + 0.25)                                          # (no mask: every atom predicted, so the defect stays true's alone)


def _transforms(b):
    eye = torch.eye(3, device=b["pos"].device).expand(2, 3, 3).contiguous()
    return eye, torch.ones((2, 3), dtype=torch.float32, device=b["pos"].device)


# name -> call(batch, codec): the function on a dict of `true` tensors, every other argument valid
CALLS = dict(
    neighbor_graph=lambda b, c: foldcomp.neighbor_graph(b, k=4, codec=c),
    rigid_frames=lambda b, c: foldcomp.rigid_frames(b, groups="all", codec=c),
    lddt=lambda b, c: foldcomp.lddt(_pred(b), b, codec=c),
    lddt_atoms=lambda b, c: foldcomp.lddt_atoms(_pred(b), b, codec=c),
    superpose=lambda b, c: foldcomp.superpose(_pred(b), b, codec=c),
    tm_score=lambda b, c: foldcomp.tm_score(_pred(b), b, iterations=2, codec=c),
    apply_transform=lambda b, c: foldcomp.apply_transform(b["pos"], *_transforms(b), b, mask=b["mask"], codec=c),
    backbone_hbonds=lambda b, c: foldcomp.backbone_hbonds(b, codec=c),
    secondary_structure=lambda b, c: foldcomp.secondary_structure(b, codec=c),
    solvent_accessibility=lambda b, c: foldcomp.solvent_accessibility(b, n_points=16, codec=c),
    violations=lambda b, c: foldcomp.violations(b, codec=c),
    encode_tensors=lambda b, c: foldcomp.encode_tensors(b, codec=c),
)
NO_CU_RULE = ("rigid_frames", "encode_tensors")          # rigid_frames never reads cu_seqlens; encode_tensors refuses such a chain, not the call


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))
    if isinstance(a, dict):
        return list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    return a == b


def _defects(name, form, b):
    """(defect, the batch with it, type, message)"""
    m = b["mask"]
    other = m.transpose(0, 1).contiguous().transpose(0, 1)
    assert other.shape == m.shape and not other.is_contiguous()
    shape = tuple(m.shape)
    yield "mask not contiguous", dict(b, mask=other), ValueError, f"{name}: mask must be contiguous"
    yield "mask int32", dict(b, mask=m.to(torch.int32)), ValueError, f"mask must be torch.bool / torch.uint8 {shape}, not torch.int32 {shape}"
    yield "mask on the cpu", dict(b, mask=m.cpu()), api.error, f"{name}: mask lies on cpu, pos on cuda:0; {ON}"
    if form == "packed" and name not in NO_CU_RULE:
        cu = b["cu_seqlens"]
        for what, bad in (("decreases", [0, L + 1, L]), ("does not end at R", [0, L, 2 * L - 1])):
            yield f"cu_seqlens {what}", dict(b, cu_seqlens=torch.tensor(bad, dtype=cu.dtype, device=cu.device)), ValueError, \
                f"cu_seqlens must be non-decreasing and end at the {2 * L} rows of pos"


@pytest.mark.parametrize("form", ["padded", "packed"])
@pytest.mark.parametrize("name", list(CALLS))
def test_a_defect_is_refused_and_leaves_nothing_behind(codec, batches, name, form):
    b, call = batches[form], CALLS[name]
    before = call(b, codec)
    for defect, bad, kind, message in _defects(name, form, b):
        with pytest.raises((ValueError, TypeError, api.error)) as e:
            call(bad, codec)
        assert (type(e.value), str(e.value)) == (kind, message), defect
    assert _same(call(b, codec), before)
