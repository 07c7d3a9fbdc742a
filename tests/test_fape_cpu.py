"""CPU: the parts of the backbone FAPE that need no device -- the float64 restatement (tests/_fape.py) against torch's float64 autograd
of a dense transcription of Algorithm 28, the differentiable torch frame builder against tests/_frames.py, the share of rows that lean
on the tie allowance in the very inputs the GPU tests use, the pure-host ABI (exports, refusals), api.check_fape, and the argument
errors of foldcomp.fape, raised before torch or a device is touched."""
import ctypes

import numpy as np
import pytest

import _analysis as AN
import _fape as FP
import _frames as FRM
from foldcomp_amd import _lib, api, tensors

NEW = ("fcz_fape_dev", "fcz_fape_packed_dev", "fcz_fape_grad_dev", "fcz_fape_grad_packed_dev", "fcz_fape", "fcz_fape_packed", "fcz_fape_grad",
       "fcz_fape_grad_packed")
F = np.float32


def _chain(m, seed):
    """one noisy chain of m rows (A = 1, slot 0) -> (the chain dict of fape_chain, frame, point, weights)"""
    inp = FP.walk_frames([m], m, 1, 0, seed)
    c, frame, point = FP._rows(inp, 0)
    return c, frame, point, np.random.default_rng(seed + 100).standard_normal(m)


def _dense_torch(c, frame, point, clamp, eps=1e-4):
    """Algorithm 28 as one dense tensor expression in torch float64 -> (leaves rot, trans, x that require grad, sum [m])"""
    import torch
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64))
    rot, trans, x = (t64(c[k]).requires_grad_() for k in ("rot_p", "trans_p", "pos_p"))
    lp = torch.einsum("fak,fpa->fpk", rot, x[None, :, :] - trans[:, None, :])
    lt = torch.einsum("fak,fpa->fpk", t64(c["rot_t"]), t64(c["pos_t"])[None, :, :] - t64(c["trans_t"])[:, None, :])
    d = torch.sqrt(((lp - lt) ** 2).sum(-1) + float(F(eps)))
    if np.isfinite(clamp):
        d = torch.clamp(d, max=float(F(clamp)))
    pair = torch.tensor(frame)[:, None] & torch.tensor(point)[None, :]
    return rot, trans, x, torch.where(pair, d, torch.zeros((), dtype=torch.float64)).sum(dim=1)


@pytest.mark.parametrize("m,seed,clamp", [(65, 1, 10.0), (257, 2, 10.0), (257, 2, float("inf")), (120, 3, 4.0)])
def test_restatement_against_torch_autograd(m, seed, clamp):
    import torch
    c, frame, point, w = _chain(m, seed)
    for k in ("rot_t", "rot_p", "trans_t", "trans_p", "pos_t", "pos_p"):      # (finite stand-ins where the chain has neither frame nor point)
        c[k] = np.nan_to_num(c[k], nan=1.0)
    ref = FP.fape_chain(c, frame, point, w, clamp)
    rot, trans, x, total = _dense_torch(c, frame, point, clamp)
    assert np.abs(ref["sum"] - total.detach().numpy()).max() <= 1e-9 * np.abs(ref["sum"]).max() and ref["sum"].max() > 10
    assert (ref["points"][frame] == point.sum()).all() and not ref["points"][~frame].any() and not ref["sum"][~frame].any()
    (torch.tensor(w) * total).sum().backward()
    for name, got, leaf in (("grad_rot", ref["grad_rot"], rot), ("grad_trans", ref["grad_trans"], trans), ("grad_pos", ref["grad_pos"], x)):
        g = leaf.grad.numpy()
        assert np.abs(got - g).max() <= 1e-9 * np.abs(g).max() and np.abs(g).max() > 1e-2, (name, np.abs(got - g).max(), np.abs(g).max())
    assert not ref["grad_rot"][~frame].any() and not ref["grad_trans"][~frame].any() and not ref["grad_pos"][~point].any()
    if np.isfinite(clamp):
        assert 0 < ref["clamped"].sum() < ref["terms"].sum()
        free = FP.fape_chain(c, frame, point, w, float("inf"))
        assert free["sum"].sum() > ref["sum"].sum() and not free["clamped"].any()
    else:
        assert not ref["clamped"].any()


def test_restatement_forms_agree():
    lens = [0, 1, 2, 30, 70]
    inp = FP.lattice(lens, 70, 4, 1, 10)
    w = FP.weights((len(lens), 70), 11)
    pad = FP.fape_padded(inp, np.asarray(lens), 1, w, FP.LATTICE_CLAMP)
    pk = FP.fape_packed(FP.pack_inp(inp, lens), AN.row_off_of(lens), 1, AN.pack1(w, lens), FP.LATTICE_CLAMP)
    exp = FP.pack_ref(pad, lens)
    for k in FP.REF_KEYS:
        assert np.array_equal(pk[k], exp[k]), k
        for e, m in enumerate(lens):
            assert not pad[k][e, m:].any(), k
    assert pad["sum"][4].any() and np.abs(pad["grad_pos"][4]).max() > 0 and np.abs(pad["grad_rot"][4]).max() > 0
    # j == i is a term: a chain of one row that is a frame and a point meets itself
    one = pad["frame"][1, 0] and pad["point"][1, 0]
    assert pad["points"][1, 0] == (1 if one else 0)


def _builder_inputs():
    """helices in atom37 with masked, non-finite, coincident and exactly collinear residues -> pos [n, L, 37, 3], mask, the bad rows"""
    rng = np.random.default_rng(5)
    n, L = 2, 40
    pos = np.stack([AN.helix(rng, L, 37) for _ in range(n)])
    mask = np.ones((n, L, 37), np.uint8)
    mask[0, 3, 0] = 0; mask[0, 4, 1] = 0; mask[1, 5, 2] = 0
    pos[0, 6, 1, 1] = np.nan; pos[0, 7, 0, 0] = np.inf; pos[1, 8, 2, 2] = -np.inf
    pos[0, 9, 2] = pos[0, 9, 1]                                               # C on CA
    pos[1, 10, :3] = np.asarray([[-2, 0, 0], [0, 0, 0], [1, 0, 0]], F) + F(3)   # N, CA, C on a line (exactly, in float32)
    pos[1, 11, :3] = np.asarray([[0, 0, 0], [0, 0, 0], [0, 0, 0]], F)
    pos[1, 12, 0, 0] = 3e19                                                   # a norm that overflows float32
    bad = [(0, 3), (0, 4), (1, 5), (0, 6), (0, 7), (1, 8), (0, 9), (1, 10), (1, 11), (1, 12)]
    return pos, mask, bad


def test_torch_frame_builder_against_the_numpy_frames():
    import torch
    pos, mask, bad = _builder_inputs()
    rot, trans, fm = FRM.frames(pos, mask, None, None, 0, 0)
    p = torch.tensor(pos, requires_grad=True)
    trot, ttrans, tfm = tensors.backbone_frames_torch(p, torch.tensor(mask))
    assert tfm.dtype == torch.bool and np.array_equal(tfm.numpy(), fm[..., 0] != 0)
    assert not any(fm[e, r, 0] for e, r in bad) and fm.sum() == fm.size - len(bad)
    assert np.abs(trot.detach().numpy() - rot[..., 0, :, :]).max() <= 1e-5 and np.abs(ttrans.detach().numpy() - trans[..., 0, :]).max() <= 1e-5
    rng = np.random.default_rng(6)
    ((trot * torch.tensor(rng.standard_normal(trot.shape).astype(F))).sum() + (ttrans * torch.tensor(rng.standard_normal(ttrans.shape).astype(F))).sum()).backward()
    g = p.grad.numpy()
    assert np.isfinite(g).all() and np.abs(g).max() > 0.1
    for e, r in bad:
        assert not AN.bits(g[e, r]).any(), ("a gradient at a residue without a frame", e, r)
    assert not AN.bits(np.ascontiguousarray(g[:, :, 3:])).any()              # frames read N, CA, C only
    # without a mask the masked residues are frames again; float64 works as well
    assert int(tensors.backbone_frames_torch(torch.tensor(pos))[2].sum()) == fm.size - len(bad) + 3
    r64 = tensors.backbone_frames_torch(torch.tensor(pos.astype(np.float64)), torch.tensor(mask))[0]
    ok = fm[..., 0] != 0                                                      # (the norm that overflows float32 is finite in float64)
    assert r64.dtype == torch.float64 and np.abs(r64.numpy() - rot[..., 0, :, :])[ok].max() <= 1e-5


def test_the_tie_allowance_stays_rare_in_the_gpu_inputs():
    """the allowance for a term that float32 may honestly put on the other side of the clamp must not become a hiding place for a wrong
    clamp rule: at most 2 % of the rows of a noisy input carry one, and none of the integer lattice"""
    b = FP.walk_batch()
    for clamp, eps in ((10.0, 1e-4), (float("inf"), 1e-4), (10.0, 0.25)):
        ref = FP.fape_padded(b["inp"], b["lens"], 4, b["w"], clamp, eps)
        share = FP.tie_share(ref)
        live = ref["terms"].sum()
        mean_d = ref["sum"].sum() / live
        print(f"walk batch {FP.WALK_LENS}, clamp {clamp}, eps {eps}: tie share {share:.4%}, {ref['clamped'].sum() / live:.2%} of the terms clamped, mean term {mean_d:.2f}")
        assert share <= 0.02 and ref["frame"].sum() > 600 and ref["point"].sum() > 600
        if np.isfinite(clamp):
            assert 0.005 < ref["clamped"].sum() / live < 0.5 and 1.0 < mean_d < 6.0          # both branches of the clamp are exercised
        else:
            assert share == 0 and not ref["clamped"].any()
    s = FP.synthetic_batch(_lib.load().fcz_fape_pass())
    ref = FP.fape_padded(s["inp"], s["lens"], 1, s["w"], FP.LATTICE_CLAMP)
    assert FP.tie_share(ref) == 0 and ref["points"].max() > 2 * _lib.load().fcz_fape_pass() * 0.7
    # the lattice has what it is there for: clamped and free terms, terms without a finite d, rows that are a frame and no point and the
    # other way round, frames refused for a non-finite entry under set masks
    e = len(s["lens"]) - 1
    assert 0 < ref["clamped"][e].sum() < ref["terms"][e].sum() and (ref["terms"][e][ref["frame"][e]] < ref["points"][e][ref["frame"][e]]).all()
    assert (ref["frame"][e] & ~ref["point"][e]).sum() > 100 and (~ref["frame"][e] & ref["point"][e]).sum() > 100
    both = (s["inp"]["fm_t"][e] != 0) & (s["inp"]["fm_p"][e] != 0)
    assert (both[:s["lens"][e]] & ~ref["frame"][e][:s["lens"][e]]).sum() == 4


def test_pure_host_abi():
    lib = _lib.load()
    assert set(NEW) <= set(_lib.EXPORTS) and "fcz_fape_pass" in _lib.EXPORTS and lib.fcz_fape_pass() > 0
    buf = np.zeros(256, np.uint8)
    p = buf.ctypes.data
    ins = [p] * 10
    for name in NEW:
        fn = getattr(lib, name)
        tail = [p, p, p, p] if "grad" in name else [p, p]
        ok = dict(bound=p, n=1, L=4, layout=0, slot=1, clamp=10.0, eps=1e-4)
        assert fn(None, *ins, *ok.values(), *tail) == -1                      # no ctx
        fake = ctypes.c_void_p(p)                                             # refused before anything is touched (the ctx is never read)
        bad = [dict(clamp=0.0), dict(clamp=-1.0), dict(clamp=float("nan")), dict(eps=0.0), dict(eps=-1e-4), dict(eps=float("nan")), dict(eps=float("inf")),
               dict(L=2 ** 29 + 1), dict(slot=37), dict(slot=-1), dict(layout=3), dict(layout=2, slot=4)]
        bad.append(dict(bound=None) if "packed" in name else dict(L=0))       # chains without a row_off; an entry without a row
        for b in bad:
            assert fn(fake, *ins, *dict(ok, **b).values(), *tail) == -1, (name, b)
        for i in (0, 1, 2, 3, 4, 5, 6, 8):                                    # every input but fmask_pred (7) and mask_pred (9) is required
            assert fn(fake, *(None if k == i else p for k in range(10)), *ok.values(), *tail) == -1, (name, i)
        for i in range(len(tail)):
            assert fn(fake, *ins, *ok.values(), *(None if k == i else p for k in range(len(tail)))) == -1, (name, "output", i)
    assert not buf.any()


def test_check_fape():
    assert api.check_fape(10, 10, 1e-4, "CA", 37) == (1, 10.0, 10.0, float(F(1e-4))) and api.check_fape(10.0, 1, 1e-4, "CB", 14)[0] == 4
    assert api.check_fape(None, 10, 1e-4, "CA")[:2] == (None, float("inf")) and api.check_fape(float("inf"), 10, 1e-4, 2, 4)[:2] == (2, float("inf"))
    for kw in (dict(clamp=0), dict(clamp=-1.0), dict(clamp=float("nan")), dict(clamp="10"), dict(clamp=True), dict(scale=0), dict(scale=float("inf")),
               dict(scale=float("nan")), dict(scale=None), dict(eps=0), dict(eps=-1e-4), dict(eps=float("inf")), dict(eps=float("nan")), dict(eps=1e-60),
               dict(atom="XX"), dict(atom="CB", width=4), dict(atom=37, width=37), dict(atom=4, width=4)):
        a = dict(dict(clamp=10.0, scale=10.0, eps=1e-4, atom="CA", width=37), **kw)
        with pytest.raises(ValueError):
            api.check_fape(**a)


def test_argument_errors_need_no_device():
    pos37, mask37 = np.zeros((2, 8, 37, 3), F), np.zeros((2, 8, 37), np.uint8)
    pos4, mask4 = np.zeros((2, 8, 4, 3), F), np.zeros((2, 8, 4), np.uint8)
    true37, true4 = dict(pos=pos37, mask=mask37), dict(pos=pos4, mask=mask4)
    rot, trans = np.zeros((2, 8, 3, 3), F), np.zeros((2, 8, 3), F)
    for pred, true, kw in ((pos37, true37, dict(clamp=0)), (pos37, true37, dict(clamp=float("nan"))), (pos37, true37, dict(scale=0)),
                           (pos37, true37, dict(eps=0)), (pos37, true37, dict(eps=float("inf"))), (pos37, true37, dict(atom="XX")),
                           (pos4, true4, dict(atom="CB")), (pos37, true37, dict(atom=37)), (pos37[:, :7], true37, {}), (pos4, true37, {}),
                           (dict(pos=pos37, mask=mask37[:1]), true37, {}), (dict(rot=rot[:, :7], trans=trans), true37, {}),
                           (dict(rot=rot, trans=trans[:1]), true37, {}), (dict(rot=rot, trans=trans, frame_mask=mask37), true37, {}),
                           (dict(rot=rot, trans=trans, pos=pos4), true37, {}), (pos37, dict(pos=np.zeros((2, 8, 5, 3), F), mask=mask37), {}),
                           (pos37[0], dict(pos=pos37[0, :, :, :2], mask=mask37[0]), {})):
        with pytest.raises(ValueError):
            tensors.fape(pred, true, **kw)
    for pred, true in ((pos37, dict(pos=pos37)), (dict(mask=mask37), true37), (dict(rot=rot), true37), (dict(trans=trans, pos=pos37), true37)):
        with pytest.raises(TypeError):
            tensors.fape(pred, true)
    import foldcomp
    import foldcomp_amd
    assert foldcomp.fape is foldcomp_amd.fape is tensors.fape and "fape" in foldcomp_amd.__all__ and "fape" in tensors.__all__
