"""CPU: the parts of the smooth lDDT that need no device -- the float64 restatement (tests/_lddt_soft.py) against torch's float64
autograd of the dense formulation, its pairs against tests/_lddt.py, its invariances, the share of rows that lean on the tie
allowance in the very inputs the GPU tests use, the pure-host ABI (exports, refusals), and the argument errors of
foldcomp.smooth_lddt, raised before torch or a device is touched."""
import ctypes

import numpy as np
import pytest

import _lddt as Q
import _lddt_soft as S
from foldcomp_amd import _lib, api, tensors

NEW = ("fcz_lddt_soft_dev", "fcz_lddt_soft_packed_dev", "fcz_lddt_soft_grad_dev", "fcz_lddt_soft_grad_packed_dev", "fcz_lddt_soft", "fcz_lddt_soft_packed",
       "fcz_lddt_soft_grad", "fcz_lddt_soft_grad_packed")
F = np.float32


def _chain(m, seed, sigma=0.5):
    """one noisy chain [m, 3] with ~10 % of the rows no site, and weights"""
    t, mt, p = S.walk([m], m, 1, 0, seed, sigma)
    return t[0, :, 0], p[0, :, 0], mt[0, :, 0] != 0, np.random.default_rng(seed + 100).standard_normal(m)


def _dense_torch(t, p, site, cutoff=15.0, thresholds=Q.THRESHOLDS):
    """the dense formulation in torch float64 on the site rows: pred (a leaf that requires grad), soft [sites], pairs [sites]"""
    import torch
    js = np.flatnonzero(site)
    tt = torch.tensor(t[js].astype(np.float64))
    pp = torch.tensor(p[js].astype(np.float64), requires_grad=True)
    inc = torch.tensor(Q._d(t[js], t[js]) < F(cutoff)) & ~torch.eye(len(js), dtype=torch.bool)          # the float32 decision, as the contract has it
    dt = (tt[:, None] - tt[None]).pow(2).sum(-1).sqrt()
    dp = ((pp[:, None] - pp[None]).pow(2).sum(-1) + torch.eye(len(js), dtype=torch.float64)).sqrt()     # (the diagonal is no pair: keep its root differentiable)
    delta = (dt - dp).abs()
    e = 0.25 * sum(torch.sigmoid(float(F(v)) - delta) for v in thresholds)
    return js, pp, (e * inc).sum(dim=1), inc.sum(dim=1)


@pytest.mark.parametrize("m,seed", [(65, 1), (300, 2), (1027, 3)])
def test_restatement_against_torch_autograd(m, seed):
    import torch
    t, p, site, w = _chain(m, seed)
    ref = S.soft_chain(t, p, site, w)
    js, pp, soft, pairs = _dense_torch(t, p, site)
    assert np.array_equal(ref["pairs"][js], pairs.numpy()) and not ref["pairs"][~site].any()
    assert np.allclose(ref["soft"][js], soft.detach().numpy(), rtol=1e-12, atol=1e-12)
    # random row weights
    (torch.tensor(w[js]) * soft).sum().backward(retain_graph=True)
    g = pp.grad.numpy().copy()
    assert np.abs(ref["grad"][js] - g).max() <= 1e-12 * max(1.0, np.abs(g).max()) and np.abs(g).max() > 1e-3 and not ref["grad"][~site].any()
    # the loss: 1 - sum soft / sum pairs, whose row weights are -1 / sum pairs
    pp.grad = None
    (1.0 - soft.sum() / pairs.sum()).backward()
    wl = np.full(m, -1.0 / float(pairs.sum()))
    gl = S.soft_chain(t, p, site, wl)["grad"]
    assert np.abs(gl[js] - pp.grad.numpy()).max() <= 1e-12 * np.abs(gl).max() and np.abs(gl).max() > 0


def test_restatement_against_torch_autograd_on_a_lattice():
    """exact ties (delta == 0, where torch's abs has the subgradient 0) and duplicated predicted points"""
    import torch
    rng = np.random.default_rng(9)
    m = 120
    t = rng.integers(-5, 6, (m, 3)).astype(F)
    p = t + rng.integers(-1, 2, (m, 3)).astype(F)
    site = rng.random(m) > 0.1
    w = rng.standard_normal(m)
    ref = S.soft_chain(t, p, site, w)
    js, pp, soft, pairs = _dense_torch(t, p, site)
    dp = Q._d(p[js], p[js])
    assert ((Q._d(t[js], t[js]) == dp) & ~np.eye(len(js), dtype=bool)).sum() > 100 and not ref["tie"].any()
    # a duplicated predicted point has no gradient by the contract; torch's root has none to give (0 / 0): keep them out of this chain
    keep = ~((dp == 0) & ~np.eye(len(js), dtype=bool)).any(axis=1)
    (torch.tensor(w[js]) * soft).sum().backward()
    g = pp.grad.numpy()
    assert np.array_equal(ref["pairs"][js], pairs.numpy())
    assert np.abs(ref["grad"][js][keep] - g[keep]).max() <= 1e-12 * np.abs(g[keep]).max()


@pytest.mark.parametrize("m,seed", [(64, 4), (257, 5)])
def test_pairs_are_lddt_pairs(m, seed):
    t, p, site, w = _chain(m, seed)
    for cutoff in (15.0, 6.5):
        assert np.array_equal(S.soft_chain(t, p, site, w, cutoff)["pairs"], Q.lddt_chain(t, p, site, cutoff)[1])
    arrays = S.lattice([90, 40], 90, 4, 1, 8)
    ref = S.soft_padded(*arrays, np.asarray([90, 40]), 1)
    assert np.array_equal(ref["pairs"], Q.lddt_padded(*arrays, np.asarray([90, 40]), 1)[1]) and ref["pairs"].sum() > 0


def test_a_structure_against_itself():
    t, _, site, w = _chain(300, 6)
    ref = S.soft_chain(t, t.copy(), site, w)
    e0 = float(S.eps(0.0))
    assert 0.8 < e0 < 0.9 and np.allclose(ref["soft"], ref["pairs"] * e0, rtol=1e-14, atol=0) and ref["pairs"].sum() > 1000
    assert not ref["grad"].any() and not ref["tie"].any() and ref["W"].sum() > 0


def test_translation_and_rotation_invariance():
    """soft depends on distances alone: the gradient has no net force and no net torque"""
    for m, seed in ((65, 7), (400, 8)):
        t, p, site, w = _chain(m, seed)
        ref = S.soft_chain(t, p, site, w)
        g, scale = ref["grad"], np.abs(ref["grad"]).sum()
        assert scale > 1e-2
        assert np.abs(g.sum(axis=0)).max() <= 1e-12 * scale
        assert np.abs(np.cross(p.astype(np.float64), g).sum(axis=0)).max() <= 1e-12 * scale * np.abs(p).max()


def test_restatement_forms_agree():
    lens = [0, 1, 2, 30, 70]
    arrays = S.lattice(lens, 70, 4, 1, 10)
    w = S.weights((len(lens), 70), 11)
    pad = S.soft_padded(*arrays, np.asarray(lens), 1, w)
    pk = S.soft_packed(*[np.concatenate([a[e, :m] for e, m in enumerate(lens)]) for a in arrays], np.concatenate([[0], np.cumsum(lens)]), 1,
                       np.concatenate([w[e, :m] for e, m in enumerate(lens)]))
    exp = S.pack_ref(pad, lens)
    for k in S.KEYS + ("site",):
        assert np.array_equal(pk[k], exp[k]), k
        for e, m in enumerate(lens):
            assert not pad[k][e, m:].any()
    assert not pad["pairs"][:2].any() and pad["pairs"][4].any() and np.abs(pad["grad"][4]).max() > 0
    # without mask_pred more rows are sites (their pred values count)
    filled = arrays[2].copy(); filled[arrays[3] == 0] = 2.0
    assert S.soft_padded(arrays[0], arrays[1], filled, None, np.asarray(lens), 1)["pairs"].sum() > pad["pairs"].sum()


def test_the_tie_allowance_stays_rare_in_the_gpu_inputs():
    """the allowance for a sign that float32 may honestly take the other way must not become a hiding place for a wrong sign rule:
    at most 2 % of the site rows of a noisy input carry one, and none of an integer lattice"""
    b = S.walk_batch()
    t, mt, p = b["arrays"]
    ref = S.soft_padded(t, mt, p, None, b["lens"], 4, b["w"])
    share = S.tie_share(ref)
    print(f"walk batch {S.WALK_LENS}: tie share {share:.4%} of {int(ref['site'].sum())} sites")
    assert share <= 0.02 and ref["site"].sum() > 600 and (ref["pairs"] > 0).sum() > 600
    s = S.synthetic_batch(_lib.load().fcz_lddt_pass())
    ref = S.soft_padded(*s["arrays"], s["lens"], 1, s["w"])
    assert not ref["tie"].any() and ref["pairs"].max() > 1000
    # the lattice has what it is there for: exact ties, duplicated predicted points, pairs without a finite delta
    t, mt, p, mp = s["arrays"]
    e = len(s["lens"]) - 1
    site = ref["site"][e]
    dt, dp = Q._d(t[e, site, 1], t[e, site, 1]), Q._d(p[e, site, 1], p[e, site, 1])
    off = ~np.eye(int(site.sum()), dtype=bool)
    pair = (dt < 15) & off
    assert (pair & (dt == dp)).sum() > 1000 and (pair & (dp == 0)).sum() >= 2 and (pair & np.isinf(dp)).sum() > 100


def test_pure_host_abi():
    lib = _lib.load()
    assert set(NEW) <= set(_lib.EXPORTS)
    buf = np.zeros(256, np.uint8)
    p = buf.ctypes.data
    th = np.asarray(Q.THRESHOLDS, F)
    fns = [getattr(lib, name) for name in NEW]
    for fn in fns:
        assert fn(None, p, p, p, p, p, 1, 4, 0, 1, 15.0, th.ctypes.data, p, p) == -1
    fake = ctypes.c_void_p(buf.ctypes.data)                                   # refused before anything is touched (the ctx is never read)
    for fn in fns:
        for cutoff in (0.0, -1.0, float("nan"), float("inf")):
            assert fn(fake, p, p, p, p, p, 1, 4, 0, 1, cutoff, None, p, p) == -1
        for bad in ((0.5, np.nan, 2, 4), (0.5, 1, 2, np.inf), (-np.inf, 1, 2, 4)):
            assert fn(fake, p, p, p, p, p, 1, 4, 0, 1, 15.0, np.asarray(bad, F).ctypes.data, p, p) == -1, bad
        assert fn(fake, p, p, p, p, p, 1, 2 ** 29 + 1, 0, 1, 15.0, None, p, p) == -1
        assert fn(fake, p, p, p, p, p, 1, 4, 0, 37, 15.0, None, p, p) == -1 and fn(fake, p, p, p, p, p, 1, 4, 3, 1, 15.0, None, p, p) == -1
        assert fn(fake, None, p, p, p, p, 1, 4, 0, 1, 15.0, None, p, p) == -1 and fn(fake, p, None, p, p, p, 1, 4, 0, 1, 15.0, None, p, p) == -1
        assert fn(fake, p, p, None, p, p, 1, 4, 0, 1, 15.0, None, p, p) == -1
        # NULL soft / pairs, NULL weight / grad
        assert fn(fake, p, p, p, p, p, 1, 4, 0, 1, 15.0, None, None, p) == -1 and fn(fake, p, p, p, p, p, 1, 4, 0, 1, 15.0, None, p, None) == -1
    for name in NEW:
        if "packed" in name:
            assert getattr(lib, name)(fake, p, p, p, p, None, 1, 4, 0, 1, 15.0, None, p, p) == -1      # chains without a row_off
        else:
            assert getattr(lib, name)(fake, p, p, p, p, p, 1, 0, 0, 1, 15.0, None, p, p) == -1         # L == 0
    assert not buf.any()


def test_argument_errors_need_no_device():
    pos37, mask37 = np.zeros((2, 8, 37, 3), F), np.zeros((2, 8, 37), np.uint8)
    pos4, mask4 = np.zeros((2, 8, 4, 3), F), np.zeros((2, 8, 4), np.uint8)
    true37, true4 = dict(pos=pos37, mask=mask37), dict(pos=pos4, mask=mask4)
    for pred, true, kw in ((pos37, true37, dict(cutoff=0)), (pos37, true37, dict(cutoff=float("nan"))), (pos37, true37, dict(cutoff=float("inf"))),
                           (pos37, true37, dict(cutoff="15")), (pos37, true37, dict(thresholds=(0.5, 1, 2))),
                           (pos37, true37, dict(thresholds=(0.5, 1, 2, float("nan")))), (pos37, true37, dict(thresholds=(0.5, 1, 2, float("inf")))),
                           (pos37, true37, dict(thresholds=(float("-inf"), 1, 2, 4))), (pos37, true37, dict(thresholds=(0.5, 1, 2, 1e39))),
                           (pos37, true37, dict(atom="XX")), (pos4, true4, dict(atom="CB")), (pos37, true37, dict(atom=37)), (pos37[:, :7], true37, {}),
                           (pos4, true37, {}), (dict(pos=pos37, mask=mask37[:1]), true37, {})):
        with pytest.raises(ValueError):
            tensors.smooth_lddt(pred, true, **kw)
    with pytest.raises(TypeError):
        tensors.smooth_lddt(pos37, dict(pos=pos37))
    with pytest.raises(TypeError):
        tensors.smooth_lddt(dict(mask=mask37), true37)
    assert api.check_lddt_soft(15, None, "CA", 37) == (1, 15.0, (0.5, 1.0, 2.0, 4.0)) and api.check_lddt_soft(6.5, (1, 1, 2, 4), "CB", 14)[0] == 4
    with pytest.raises(ValueError):
        api.check_lddt_soft(15, (0.25, 0.5, 1, np.inf), 2)
    assert api.check_lddt(15, (0.25, 0.5, 1, np.inf), 2)[2][3] == float("inf")                          # lddt's own rule is as it was
    import foldcomp
    import foldcomp_amd
    assert foldcomp.smooth_lddt is foldcomp_amd.smooth_lddt is tensors.smooth_lddt and "smooth_lddt" in foldcomp_amd.__all__
