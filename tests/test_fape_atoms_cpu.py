"""CPU: the parts of the all-atom FAPE that need no device -- the float64 restatement (tests/_fape_atoms.py) against torch's float64
autograd of a dense transcription, the renaming against a truth whose slots and ambiguous frames were swapped by hand, the padded
against the packed form, the differentiable torch builder of the eight groups against tests/_frames.py, the share of items that lean
on the tie allowance in the very inputs the GPU tests use, the pure-host ABI (exports, refusals), api.check_fape_atoms, and the
argument errors of foldcomp.fape_atoms, raised before torch or a device is touched."""
import ctypes

import numpy as np
import pytest

import _analysis as AN
import _fape_atoms as FA
import _frames as FRM
from foldcomp_amd import _lib, api, tensors

NEW = ("fcz_fape_atoms_dev", "fcz_fape_atoms_packed_dev", "fcz_fape_atoms_grad_dev", "fcz_fape_atoms_grad_packed_dev", "fcz_fape_atoms",
       "fcz_fape_atoms_packed", "fcz_fape_atoms_grad", "fcz_fape_atoms_grad_packed")
F = np.float32


def _chain(m, seed, rename):
    """one noisy atom14 chain of m rows with finite stand-ins where it has neither frame nor point -> (the chain dict, weights)"""
    inp = FA.noisy((m,), 14, seed)
    c = {k: None if v is None else v[0] for k, v in inp.items()}
    if not rename:
        c["swapped"] = None
    for k in ("rot_t", "rot_p", "trans_t", "trans_p", "pos_t", "pos_p"):
        c[k] = np.nan_to_num(c[k], nan=1.0)
    return c, np.random.default_rng(seed + 100).standard_normal((m, FA.GROUPS))


def _dense_torch(c, frame, point, clamp, eps=1e-4):
    """the loss as one dense tensor expression in torch float64 on the renamed truth -> (leaves rot, trans, x, sum [m, 8])"""
    import torch
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64))
    rot_t, pos_t, _ = FA.renamed(c, *FA.tables(14))
    rot, trans, x = (t64(c[k]).requires_grad_() for k in ("rot_p", "trans_p", "pos_p"))
    m = rot.shape[0]
    fl = lambda v: v.reshape((-1,) + tuple(v.shape[2:]))
    lp = torch.einsum("fak,fpa->fpk", fl(rot), fl(x)[None, :, :] - fl(trans)[:, None, :])
    lt = torch.einsum("fak,fpa->fpk", fl(t64(rot_t)), fl(t64(pos_t))[None, :, :] - fl(t64(c["trans_t"]))[:, None, :])
    d = torch.sqrt(((lp - lt) ** 2).sum(-1) + float(F(eps)))
    if np.isfinite(clamp):
        d = torch.clamp(d, max=float(F(clamp)))
    pair = torch.tensor(frame.reshape(-1))[:, None] & torch.tensor(point.reshape(-1))[None, :]
    return rot, trans, x, torch.where(pair, d, torch.zeros((), dtype=torch.float64)).sum(dim=1).reshape(m, FA.GROUPS)


@pytest.mark.parametrize("m,seed,clamp,rename", [(33, 1, 10.0, True), (64, 2, 4.0, False), (64, 2, float("inf"), True), (48, 3, 2.0, True)])
def test_restatement_against_torch_autograd(m, seed, clamp, rename):
    import torch
    c, w = _chain(m, seed, rename)
    ref = FA.chain(c, w, clamp)
    frame, point = ref["frame"], ref["point"]
    rot, trans, x, total = _dense_torch(c, frame, point, clamp)
    assert np.abs(ref["sum"] - total.detach().numpy()).max() <= 1e-9 * np.abs(ref["sum"]).max() and ref["sum"].max() > 10
    assert (ref["points"][frame] == point.sum()).all() and not ref["points"][~frame].any() and not ref["sum"][~frame].any()
    assert frame.sum() > 3 * m and point.sum() > 6 * m and not frame[:, [1, 2, 6, 7]].any()
    (torch.tensor(w) * total).sum().backward()
    for name, got, leaf in (("grad_rot", ref["grad_rot"], rot), ("grad_trans", ref["grad_trans"], trans), ("grad_pos", ref["grad_pos"], x)):
        g = leaf.grad.numpy()
        assert np.abs(got - g).max() <= 1e-9 * np.abs(g).max() and np.abs(g).max() > 1e-2, (name, np.abs(got - g).max(), np.abs(g).max())
    assert not ref["grad_rot"][~frame].any() and not ref["grad_trans"][~frame].any() and not ref["grad_pos"][~point].any()
    if np.isfinite(clamp):
        assert 0 < ref["clamped"].sum() < ref["terms"].sum()
    else:
        assert not ref["clamped"].any()


def test_renaming_is_a_truth_swapped_by_hand():
    """swapped rows read the truth's slots through the table and its ambiguous frames turned: the same numbers as the unrenamed
    restatement on a truth in which exactly that was done by hand, and other numbers than no renaming at all"""
    c, w = _chain(64, 7, True)
    table, alt = FA.tables(14)
    got = FA.chain(c, w, 10.0)
    hand = {k: None if v is None else v.copy() for k, v in c.items()}
    changed = 0
    for r in range(64):
        ty = min(int(c["aatype"][r]), 20)
        if not c["swapped"][r]:
            continue
        for a in range(14):
            b = int(table[ty, a])
            if b > a:
                hand["pos_t"][r, [a, b]] = c["pos_t"][r, [b, a]]
                hand["mask_t"][r, [a, b]] = c["mask_t"][r, [b, a]]
                changed += 1
        for g in range(FA.GROUPS):
            if alt[ty, g]:
                hand["rot_t"][r, g] = c["rot_t"][r, g] @ np.diag([1, -1, -1]).astype(F)
                changed += 1
    hand["swapped"] = None
    exp = FA.chain(hand, w, 10.0)
    for k in FA.REF_KEYS:
        assert np.array_equal(got[k], exp[k]), k
    plain = FA.chain(dict(c, swapped=None), w, 10.0)
    assert changed > 20 and not np.array_equal(plain["sum"], got["sum"]) and not np.array_equal(plain["grad_pos"], got["grad_pos"])
    # a row whose type has no swap and no ambiguous group: swapped or not, the same
    none = ~np.isin(c["aatype"], (FA.ASP, FA.GLU, FA.PHE, FA.TYR))
    assert (c["swapped"][none] != 0).any()
    only = FA.chain(dict(c, swapped=np.where(none, 0, c["swapped"]).astype(np.uint8)), w, 10.0)
    for k in FA.REF_KEYS:
        assert np.array_equal(got[k], only[k]), k
    # the table and the flags the restatement reads are the library's: ASP / PHE / TYR group 5, GLU group 6, two or four partnered slots
    assert [tuple(np.flatnonzero(alt[t])) for t in (FA.ASP, FA.GLU, FA.PHE, FA.TYR)] == [(5,), (6,), (5,), (5,)] and alt.sum() == 4
    assert [(table[t] != np.arange(14)).sum() for t in (FA.ASP, FA.GLU, FA.PHE, FA.TYR)] == [2, 2, 4, 4]
    assert not FA.tables(4)[1].any() and (FA.tables(4)[0] == np.arange(4)).all()


def test_restatement_forms_agree():
    lens = [0, 1, 2, 30, 70]
    inp = FA.lattice(lens, 70, 14, 10)
    w = FA.weights((len(lens), 70, FA.GROUPS), 11)
    pad = FA.ref_padded(inp, np.asarray(lens), w, FA.LATTICE_CLAMP)
    pk = FA.ref_packed(FA.pack_inp(inp, lens), AN.row_off_of(lens), AN.pack1(w, lens), FA.LATTICE_CLAMP)
    exp = FA.pack_ref(pad, lens)
    for k in FA.REF_KEYS:
        assert np.array_equal(pk[k], exp[k]), k
        for e, m in enumerate(lens):
            assert not pad[k][e, m:].any(), k
    assert pad["sum"][4].any() and np.abs(pad["grad_pos"][4]).max() > 0 and np.abs(pad["grad_rot"][4]).max() > 0
    # a residue's own atoms are points of its frames: a chain of one row meets itself
    assert (pad["points"][1, 0][pad["frame"][1, 0]] == pad["point"][1, 0].sum()).all()
    # backbone4: groups 0 and 3 alone, whatever the masks say, and nothing renamed
    b4 = FA.lattice([20], 20, 4, 12, full=(0,))
    r4 = FA.ref_padded(b4, None, None, FA.LATTICE_CLAMP)
    assert r4["frame"][0][:, [0, 3]].all() and not r4["frame"][0][:, [1, 2, 4, 5, 6, 7]].any() and (r4["points"][0][:, 0] == 80).all()
    plain = FA.ref_padded(dict(b4, swapped=None), None, None, FA.LATTICE_CLAMP)
    assert b4["swapped"].any() and all(np.array_equal(plain[k], r4[k]) for k in FA.REF_KEYS)


def _builder_inputs(A):
    """helices with masked, non-finite, coincident and exactly collinear atoms -> pos [n, L, A, 3], mask, aatype"""
    rng = np.random.default_rng(5)
    n, L = 2, 42
    pos = np.stack([AN.helix(rng, L, A) for _ in range(n)])
    mask = (rng.random((n, L, A)) > 0.04).astype(np.uint8)
    aatype = (np.arange(n * L) % 23).astype(np.uint8).reshape(n, L)
    aatype[1, 40] = 255
    pos[0, 6, 1, 1] = np.nan; pos[0, 7, 0, 0] = np.inf; pos[1, 8, 2, 2] = -np.inf
    pos[0, 9, 2] = pos[0, 9, 1]                                               # C on CA
    pos[1, 10, :3] = np.asarray([[-2, 0, 0], [0, 0, 0], [1, 0, 0]], F) + F(3)   # N, CA, C on a line (exactly, in float32)
    pos[1, 12, 0, 0] = 3e19                                                   # a norm that overflows float32
    mask[[0, 0, 1, 0, 1, 1], [6, 7, 8, 9, 10, 12], :3] = 1
    return pos, mask, aatype


@pytest.mark.parametrize("A", [37, 14, 4])
def test_torch_builder_of_the_eight_groups_against_the_numpy_frames(A):
    import torch
    pos, mask, aatype = _builder_inputs(A)
    rot, trans, fm = FRM.frames(pos, mask, aatype, None, FA.LAYOUT[A], 1)
    p = torch.tensor(pos, requires_grad=True)
    trot, ttrans, tfm = tensors.rigid_frames_torch(p, torch.tensor(mask), torch.tensor(aatype))
    assert tfm.dtype == torch.bool and tuple(tfm.shape) == pos.shape[:2] + (8,) and np.array_equal(tfm.numpy(), fm != 0)
    assert not fm[..., 1:3].any() and fm[..., 0].sum() > 60 and (A == 4 or fm[..., 4:].sum() > 80) and not fm[0, 9, 0] and not fm[1, 10, 0] and not fm[1, 12, 0]
    assert np.abs(trot.detach().numpy() - rot).max() <= 1e-5 and np.abs(ttrans.detach().numpy() - trans).max() <= 1e-5
    absent = fm == 0
    assert (trot.detach().numpy()[absent] == np.eye(3, dtype=F)).all() and not ttrans.detach().numpy()[absent].any()
    # every group on its own: the gradient of an absent group is exactly 0, of a present one finite
    rng = np.random.default_rng(6)
    wr, wt = torch.tensor(rng.standard_normal(trot.shape).astype(F)), torch.tensor(rng.standard_normal(ttrans.shape).astype(F))
    off = torch.tensor(absent)
    (((trot * wr).sum((-1, -2)) + (ttrans * wt).sum(-1)) * off).sum().backward(retain_graph=True)
    assert not AN.bits(p.grad.numpy()).any(), "a gradient through a group that does not exist"
    p.grad = None
    ((trot * wr).sum() + (ttrans * wt).sum()).backward()
    g = p.grad.numpy()
    assert np.isfinite(g).all() and np.abs(g).max() > 0.1
    rows_without = ~(fm != 0).any(axis=-1)
    assert rows_without.any() and not AN.bits(np.ascontiguousarray(g[rows_without])).any()
    # the backbone group is backbone_frames_torch's, bit for bit; without aatype only groups 0 and 3 can exist
    brot, btrans, bfm = tensors.backbone_frames_torch(torch.tensor(pos), torch.tensor(mask))
    assert np.array_equal(bfm.numpy(), tfm.numpy()[..., 0]) and np.array_equal(AN.bits(brot.numpy()), AN.bits(trot.detach().numpy()[..., 0, :, :]))
    none = tensors.rigid_frames_torch(torch.tensor(pos), torch.tensor(mask))[2].numpy()
    assert np.array_equal(none[..., [0, 3]], fm[..., [0, 3]] != 0) and not none[..., [1, 2, 4, 5, 6, 7]].any()
    with pytest.raises(ValueError):
        tensors.rigid_frames_torch(torch.tensor(pos), layout="atom37" if A != 37 else "atom14")


def test_the_tie_allowance_stays_rare_in_the_gpu_inputs():
    """the allowance for a term that float32 may honestly put on the other side of the clamp must not become a hiding place for a wrong
    clamp rule: at most 2 % of the items of a noisy input carry one, and none of the integer lattice"""
    lib = _lib.load()
    b = FA.noisy_batch()
    for clamp, eps in ((10.0, 1e-4), (float("inf"), 1e-4), (10.0, 0.25)):
        ref = FA.ref_padded(b["inp"], b["lens"], b["w"], clamp, eps)
        share = FA.tie_share(ref)
        live = ref["terms"].sum()
        mean_d = ref["sum"].sum() / live
        print(f"noisy batch {FA.NOISY_LENS}, clamp {clamp}, eps {eps}: tie share {share:.4%}, {ref['clamped'].sum() / live:.2%} of the terms clamped, mean term {mean_d:.2f}")
        assert share <= FA.TIE_SHARE and ref["frame"].sum() > 700 and ref["point"].sum() > 1500
        if np.isfinite(clamp):
            assert 0.005 < ref["clamped"].sum() / live < 0.9 and 1.0 < mean_d < 10.0   # both branches of the clamp are exercised
        else:
            assert share == 0 and not ref["clamped"].any()
    T, P = lib.fcz_fape_atoms_tile_rows(1), lib.fcz_fape_atoms_pass()
    assert T == FA.fapea_tile_rows(14) and lib.fcz_fape_atoms_tile_rows(2) == FA.fapea_tile_rows(4) and P == FA.FAPEA_PASS
    s = FA.synthetic_batch(T)
    ref = FA.ref_padded(s["inp"], s["lens"], s["w"], FA.LATTICE_CLAMP)
    e = len(s["lens"]) - 1
    assert FA.tie_share(ref) == 0 and ref["points"].max() == 150 * 14 > 2 * P and ref["frame"][e].sum() == 150 * 8
    # the lattice has what it is there for: about half the frame items, clamped and free terms, terms without a finite d, frames
    # refused for a non-finite entry under set masks, swaps on every kind of row, and a swap that lands on a cleared true slot
    k = 5                                                                     # the chain of a tile and a row
    m = int(s["lens"][k])
    inp = {key: v[k, :m] for key, v in s["inp"].items()}
    both = (inp["fm_t"] != 0) & (inp["fm_p"] != 0)
    assert 0.35 < both.mean() < 0.65 and (both & ~ref["frame"][k, :m]).sum() == 4
    assert 0 < ref["clamped"][k].sum() < ref["terms"][k].sum() and (ref["terms"][k][ref["frame"][k]] < ref["points"][k][ref["frame"][k]]).all()
    table, _ = FA.tables(14)
    sw = inp["swapped"] != 0
    assert all((sw & (inp["aatype"] == t)).any() for t in (FA.ASP, FA.GLU, FA.PHE, FA.TYR, 0, 20, 255))
    partner = table[np.minimum(inp["aatype"], 20)]
    moved = sw[:, None] & (partner != np.arange(14))
    landed = moved & (np.take_along_axis(inp["mask_t"], partner.astype(np.int64), axis=1) == 0) & (inp["mask_t"] != 0)
    assert landed.any() and not ref["point"][k, :m][landed].any()
    bb = FA.backbone_batch(P)
    rb = FA.ref_padded(bb["inp"], bb["lens"], bb["w"], FA.LATTICE_CLAMP)
    assert [int(rb["points"][e].max()) for e in range(3)] == [P, P - 1, 2 * P + 12] and FA.tie_share(rb) == 0


def test_pure_host_abi():
    lib = _lib.load()
    assert set(NEW) <= set(_lib.EXPORTS) and {"fcz_fape_atoms_pass", "fcz_fape_atoms_tile_rows"} <= set(_lib.EXPORTS)
    assert lib.fcz_fape_atoms_pass() > 0 and lib.fcz_fape_atoms_tile_rows(0) > 0 and lib.fcz_fape_atoms_tile_rows(3) == -1
    buf = np.zeros(21 * 37, np.uint8)
    p = buf.ctypes.data
    ins = [p] * 12
    bad_table = np.tile(np.arange(14, dtype=np.uint8), (21, 1))
    bad_table[3, 6] = 7                                                       # no involution
    wide_table = np.tile(np.arange(14, dtype=np.uint8), (21, 1))
    wide_table[3, 6] = 14                                                     # outside the row
    for name in NEW:
        fn = getattr(lib, name)
        tail = [p, p, p, p] if "grad" in name else [p, p]
        ok = dict(bound=p, n=1, L=4, layout=1, clamp=10.0, eps=1e-4, table=None)
        assert fn(None, *ins, *ok.values(), *tail) == -1                      # no ctx
        fake = ctypes.c_void_p(p)                                             # refused before anything is touched (the ctx is never read)
        bad = [dict(clamp=0.0), dict(clamp=-1.0), dict(clamp=float("nan")), dict(eps=0.0), dict(eps=-1e-4), dict(eps=float("nan")), dict(eps=float("inf")),
               dict(L=2 ** 29 + 1), dict(layout=0, L=(2 ** 31 - 1) // 37 + 1), dict(layout=3), dict(layout=-1), dict(table=bad_table.ctypes.data),
               dict(table=wide_table.ctypes.data)]
        bad.append(dict(bound=None) if "packed" in name else dict(L=0))       # chains without a row_off; an entry without a row
        for b in bad:
            assert fn(fake, *ins, *dict(ok, **b).values(), *tail) == -1, (name, b)
        for i in (0, 1, 2, 3, 4, 7, 8, 10):                                   # aatype (5), swapped (6), fmask_pred (9) and mask_pred (11) may be NULL
            assert fn(fake, *(None if k == i else p for k in range(12)), *ok.values(), *tail) == -1, (name, i)
        assert fn(fake, *(None if k == 5 else p for k in range(12)), *ok.values(), *tail) == -1, (name, "swapped without aatype")
        for i in range(len(tail)):
            assert fn(fake, *ins, *ok.values(), *(None if k == i else p for k in range(len(tail)))) == -1, (name, "output", i)
    assert not buf.any()


def test_check_fape_atoms():
    ok = dict(clamp=10.0, scale=10.0, eps=1e-4, rename="lddt_atoms", shape=(2, 8, 14, 3))
    assert api.check_fape_atoms(**ok) == (10.0, 10.0, float(F(1e-4)), "lddt_atoms", None)
    assert api.check_fape_atoms(None, 1, 1e-4, None, (9, 37, 3), has_aatype=False)[:4] == (float("inf"), 1.0, float(F(1e-4)), None)
    sw = np.zeros((2, 8), bool)
    assert api.check_fape_atoms(**dict(ok, rename=sw))[3] is sw
    table = np.tile(np.arange(14), (21, 1))
    table[3, [6, 7]] = [7, 6]
    got = api.check_fape_atoms(**dict(ok, swaps=table))[4]
    assert got.dtype == np.uint8 and np.array_equal(got, table)
    bad_table = table.copy()
    bad_table[3, 6] = 8
    for kw in (dict(clamp=0), dict(clamp=float("nan")), dict(clamp="10"), dict(scale=0), dict(scale=float("inf")), dict(eps=0), dict(eps=float("inf")),
               dict(rename="alphafold"), dict(rename=True), dict(rename=np.zeros((2, 7), bool)), dict(rename=np.zeros((2, 8, 14), bool)),
               dict(has_aatype=False), dict(rename=sw, has_aatype=False), dict(shape=(2, 8, 5, 3)), dict(shape=(2, 8, 14, 2)), dict(shape=(8, 14)),
               dict(shape=(1, 2 ** 29 + 1, 4, 3)), dict(shape=((2 ** 31 - 1) // 37 + 1, 37, 3)), dict(swaps="af"), dict(swaps=bad_table), dict(swaps=table[:, :13]),
               dict(swaps=table.astype(np.float32))):
        with pytest.raises(ValueError):
            api.check_fape_atoms(**dict(ok, **kw))
    # lddt_atoms' own check still reads its table the same way
    assert np.array_equal(api.check_lddt_atoms(15.0, None, table, (2, 8, 14, 3), (2, 8, 14, 3))[2], table)
    with pytest.raises(ValueError):
        api.check_lddt_atoms(15.0, None, bad_table, (2, 8, 14, 3), (2, 8, 14, 3))


def test_argument_errors_need_no_device():
    pos, mask, aa = np.zeros((2, 8, 14, 3), F), np.zeros((2, 8, 14), np.uint8), np.zeros((2, 8), np.uint8)
    true = dict(pos=pos, mask=mask, aatype=aa)
    rot, trans = np.zeros((2, 8, 8, 3, 3), F), np.zeros((2, 8, 8, 3), F)
    for pred, tr, kw in ((pos, true, dict(clamp=0)), (pos, true, dict(clamp=float("nan"))), (pos, true, dict(scale=0)), (pos, true, dict(eps=0)),
                         (pos, true, dict(rename="alphafold")), (pos, true, dict(rename=np.zeros((2, 7), bool))), (pos, true, dict(swaps="x")),
                         (pos, dict(pos=pos, mask=mask), {}), (pos, dict(pos=pos, mask=mask), dict(rename=None)), (pos[:, :7], true, {}),
                         (dict(pos=pos, mask=mask[:1]), true, {}), (dict(rot=rot[:, :7], trans=trans, pos=pos), true, {}),
                         (dict(rot=rot, trans=trans[:1], pos=pos), true, {}), (dict(rot=rot[:, :, 0], trans=trans[:, :, 0], pos=pos), true, {}),
                         (dict(rot=rot, trans=trans, pos=pos, frame_mask=aa), true, {}), (pos, dict(pos=np.zeros((2, 8, 5, 3), F), mask=mask, aatype=aa), {})):
        with pytest.raises(ValueError):
            tensors.fape_atoms(pred, tr, **kw)
    for pred, tr in ((pos, dict(pos=pos, aatype=aa)), (dict(mask=mask), true), (dict(rot=rot, trans=trans), true), (dict(rot=rot, pos=pos), true)):
        with pytest.raises(TypeError):
            tensors.fape_atoms(pred, tr)
    import foldcomp
    import foldcomp_amd
    assert foldcomp.fape_atoms is foldcomp_amd.fape_atoms is tensors.fape_atoms and "fape_atoms" in foldcomp_amd.__all__ and "fape_atoms" in tensors.__all__
