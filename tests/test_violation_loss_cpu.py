"""CPU: the parts of the violation loss that need no device -- the float32 restatement (tests/_violation_loss.py) against float64 torch
autograd of the dense formulation within the bound derived there from the operation count, its consistency with the metric's
restatement (tests/_violations.py), the pure-host ABI (exports, the pass, refusals) and the argument rules of
api.check_violation_loss. The fixtures are _analysis.helix chains of 60 rows: at tolerance 0 every layout has clashing pairs
(backbone4 has none at the default 1.5), at link factor 0.5 nearly every link violates something."""
import numpy as np
import pytest

import _analysis as AN
import _violation_loss as VL
import _violations as V
from foldcomp_amd import _lib, api

NEW = ("fcz_violation_loss_pass", "fcz_violation_loss_dev", "fcz_violation_loss_packed_dev", "fcz_violation_loss_grad_dev",
       "fcz_violation_loss_grad_packed_dev", "fcz_violation_loss", "fcz_violation_loss_packed", "fcz_violation_loss_grad", "fcz_violation_loss_grad_packed")
F = np.float32
ROWS = 60
PAIRS = {37: 20000, 14: 500, 4: 400}                                         # the 60-row helix at tolerance 0 has more clashing pairs than these


def _helix(A, seed=7):
    """-> (pos [60, A, 3], mask, aatype, table, w_clash, w_link): every mask set, types 0 .. 19 with two PRO"""
    rng = np.random.default_rng(seed)
    pos = AN.helix(rng, ROWS, A)
    mask = np.ones((ROWS, A), np.uint8)
    aa = rng.integers(0, 20, size=ROWS).astype(np.uint8)
    aa[[11, 40]] = V.PRO
    return pos, mask, aa, V.default_table(A), VL.weights((ROWS, A), seed + 1), VL.weights((ROWS, 3), seed + 2)


@pytest.fixture(scope="module", params=[37, 14, 4])
def helix(request):
    """the chain, its float32 restatement at (tolerance 0, link factor 0.5) and the metric's: computed once, never changed"""
    A = request.param
    pos, mask, aa, table, wc, wl = _helix(A)
    clash, link, counts = VL.loss_chain(pos, mask, aa, table, F(0), F(0.5))
    grad = VL.grad_chain(pos, mask, aa, table, wc, wl, F(0), F(0.5))
    metric = V.violations_chain(pos, mask, aa, table, F(0), F(0.5))
    return dict(A=A, inputs=(pos, mask, aa, table), w=(wc, wl), clash=clash, link=link, counts=counts, grad=grad, metric=metric)


def test_the_fixtures_hold_every_term_class(helix):
    h = helix
    per_atom = V.clash_matrix(*h["inputs"][:3], h["inputs"][3], F(0))[1].sum(axis=1)
    print(f"A = {h['A']}: {int(h['metric']['counts'][1])} clashing pairs, up to {int(per_atom.max())} partners an atom, "
          f"{int((h['metric']['link_violation'] != 0).sum())} of {int(h['metric']['link_mask'].sum())} links violate something")
    assert int(h["metric"]["counts"][1]) > PAIRS[h["A"]], h["metric"]["counts"]
    assert (h["clash"] > 0).sum() > 50 and per_atom.max() >= (60 if h["A"] == 37 else 6)
    assert (h["metric"]["link_violation"] != 0).sum() >= 55 and h["metric"]["link_mask"].sum() == 59
    assert all((h["link"][:, k] > 0).any() for k in range(3)), "bond, cos0 and cos1 terms"
    assert all(np.abs(h["grad"][:, s]).max() > 0 for s in (0, 1, 2)) and (h["A"] == 4 or np.abs(h["grad"][:, 4:]).max() > 0)
    # at the defaults backbone4 has no clash
    if h["A"] == 4:
        assert not VL.loss_chain(*h["inputs"])[0].any()


def test_restatement_against_float64_autograd(helix):
    """|float32 - float64| <= the bound of tests/_violation_loss.py for every value and every gradient component"""
    h = helix
    ref = VL.dense64(*h["inputs"], *h["w"], F(0), F(0.5))
    worst = {}
    for key, got in (("clash_loss", h["clash"]), ("link_loss", h["link"]), ("grad", h["grad"])):
        err, bound = np.abs(got.astype(np.float64) - ref[key]), ref["b_" + key]
        assert np.isfinite(ref[key]).all() and (bound[ref[key] != 0] > 0).all(), key
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))
        worst[key] = float(ratio.max())
        print(f"A = {h['A']}, {key}: largest error / bound = {worst[key]:.4f}, largest error {err.max():.3e}, largest value {np.abs(ref[key]).max():.3e}")
    assert all(v <= 1.0 for v in worst.values()), worst
    assert np.abs(ref["grad"]).max() > 1 and ref["clash_loss"].max() > 1 and ref["link_loss"].max() > 0.01


def test_float64_autograd_is_the_plain_formulation():
    """dense64 takes its SETS from float32; on a chain without a boundary case it is the formula one would write down: relu, abs, sqrt"""
    import torch
    pos, mask, aa, table, wc, wl = _helix(4, seed=9)
    ref = VL.dense64(pos, mask, aa, table, wc, wl, F(0), F(0.5))
    P = torch.tensor(pos.astype(np.float64), requires_grad=True)
    R = torch.tensor(table[np.minimum(aa, 20)].astype(np.float64))
    c, rad = P.reshape(-1, 3), R.reshape(-1)
    row, slot = torch.arange(ROWS).repeat_interleave(4), torch.arange(4).repeat(ROWS)
    d = ((c[:, None] - c[None]) ** 2).sum(-1).add(torch.eye(len(c), dtype=torch.float64)).sqrt()
    peptide = (slot[:, None] == 2) & (slot[None] == 0) & (row[None] == row[:, None] + 1)
    pair = (row[:, None] != row[None]) & ~(peptide | peptide.T)
    clash = (torch.relu((rad[:, None] + rad[None]) - 0.0 - d) * pair).sum(1).reshape(ROWS, 4)
    ca, cc, n1, ca1 = P[:-1, 1], P[:-1, 2], P[1:, 0], P[1:, 1]
    cos = lambda a, b, c_: ((a - b) * (c_ - b)).sum(-1) / ((a - b).norm(dim=-1) * (c_ - b).norm(dim=-1))
    pro = torch.tensor(aa[1:] == V.PRO)
    l0, sl = torch.where(pro, float(V.L0_PRO), float(V.L0)), torch.where(pro, float(V.SL_PRO), float(V.SL))
    link = torch.stack([torch.relu(((cc - n1).norm(dim=-1) - l0).abs() - 0.5 * sl), torch.relu((cos(ca, cc, n1) - float(V.COS0)).abs() - 0.5 * float(V.S0)),
                        torch.relu((cos(cc, n1, ca1) - float(V.COS1)).abs() - 0.5 * float(V.S1))], dim=1)
    ((torch.tensor(wc.astype(np.float64)) * clash).sum() + (torch.tensor(wl[:-1].astype(np.float64)) * link).sum()).backward()
    assert np.allclose(ref["clash_loss"], clash.detach().numpy(), rtol=0, atol=1e-6) and np.allclose(ref["link_loss"][:-1], link.detach().numpy(), rtol=0, atol=1e-6)
    assert np.allclose(ref["grad"], P.grad.numpy(), rtol=0, atol=1e-5 * np.abs(ref["grad"]).max())


def test_consistent_with_the_metric(helix):
    h, m = helix, helix["metric"]
    assert not (h["clash"] > 0)[m["clash_atom"] == 0].any()                   # clash_loss > 0 implies clash_atom
    deep = m["clash_depth"] > 0                                               # a row whose deepest overlap is > 0 has an atom with a loss > 0
    assert ((h["clash"] > 0).any(axis=1) >= deep).all() and deep.sum() > 10
    # per atom: where some overlap of the atom is > 0 the sum is
    idx, clash, depth = V.clash_matrix(*h["inputs"][:3], h["inputs"][3], F(0))
    some = (clash & (depth > 0)).any(axis=1)
    assert (h["clash"][idx[:, 0], idx[:, 1]] > 0)[some].all() and not (h["clash"][idx[:, 0], idx[:, 1]] > 0)[~clash.any(axis=1)].any()
    for k in range(3):
        assert np.array_equal(h["link"][:, k] > 0, (m["link_violation"] >> k) & 1 == 1), k
    assert h["counts"][0] == m["counts"][0] and h["counts"][1] == m["link_mask"].sum()


def test_batches_follow_the_chains():
    """padded and packed forms of the restatement give every chain the bytes it has alone"""
    lens = [0, 1, 2, 25, 33]
    rng = np.random.default_rng(5)
    L, A = max(lens), 14
    pos, mask = np.stack([AN.helix(rng, L, A) for _ in lens]), np.ones((len(lens), L, A), np.uint8)
    aa = rng.integers(0, 20, size=(len(lens), L)).astype(np.uint8)
    table, wc, wl = V.default_table(A), VL.weights((len(lens), L, A), 1), VL.weights((len(lens), L, 3), 2)
    ln = np.asarray(lens, np.uint32)
    v = VL.loss(pos, mask, aa, ln, table, F(0), F(0.5))
    g = VL.grad(pos, mask, aa, ln, table, wc, wl, F(0), F(0.5))
    off = AN.row_off_of(lens)
    packed = AN.pack((pos, mask, aa, wc, wl), lens)
    vp = VL.loss(*packed[:3], off, table, F(0), F(0.5), packed=True)
    gp = VL.grad(*packed[:3], off, table, *packed[3:], F(0), F(0.5), packed=True)
    VL.same(vp, dict(clash_loss=AN.pack1(v["clash_loss"], lens), link_loss=AN.pack1(v["link_loss"], lens), counts=v["counts"]), "packed")
    VL.same(gp, AN.pack1(g, lens), "packed grad")
    assert v["counts"][:3, 1].tolist() == [0, 0, 1] and v["counts"][0, 0] == 0 < v["counts"][1, 0] < v["counts"][2, 0] <= 28 and not v["clash_loss"][3, 25:].any() and not g[3, 25:].any() and np.abs(g[3, :25]).max() > 0
    alone = VL.loss_chain(pos[3, :25], mask[3, :25], aa[3, :25], table, F(0), F(0.5))
    VL.same(alone[0], v["clash_loss"][3, :25], "alone")


def test_exports_pass_and_refusals():
    lib = _lib.load()
    assert set(NEW) <= set(_lib.EXPORTS)
    P = lib.fcz_violation_loss_pass()
    assert P > 0 and P % 256 == 0 and P == lib.fcz_violation_loss_pass()
    # refused before the ctx is looked at: a NULL ctx with everything else in order, and every NULL output or weight
    pos, mask, aa = np.zeros((2, 4, 37, 3), F), np.ones((2, 4, 37), np.uint8), np.zeros((2, 4), np.uint8)
    out = [np.full(2 * 4 * 37, 7, F), np.full(2 * 4 * 3, 7, F), np.full(4, 7, np.int64)]
    p = lambda a: a.ctypes.data
    for fn in (lib.fcz_violation_loss, lib.fcz_violation_loss_dev):
        assert fn(None, p(pos), p(mask), p(aa), None, 2, 4, 0, None, 1.5, 12.0, p(out[0]), p(out[1]), p(out[2])) == -1
    for fn in (lib.fcz_violation_loss_grad, lib.fcz_violation_loss_grad_dev):
        assert fn(None, p(pos), p(mask), p(aa), None, 2, 4, 0, None, 1.5, 12.0, p(out[0]), p(out[1]), p(pos)) == -1
    assert all((o == 7).all() for o in out) and not pos.any()


def test_check_violation_loss():
    pos, mask, aa = np.zeros((2, 8, 14, 3), F), np.ones((2, 8, 14), bool), np.zeros((2, 8), np.uint8)
    d = dict(pos=pos, mask=mask, aatype=aa)
    assert api.check_violation_loss("violation_loss", d) == ((2, 8, 14, 3), False, None)
    shape, packed, table = api.check_violation_loss("violation_loss", dict(pos=pos[0], mask=mask[0], aatype=aa[0], cu_seqlens=np.asarray([0, 8])), 0.0, 0.5,
                                                    V.default_table(14))
    assert shape == (8, 14, 3) and packed and table.dtype == np.float32 and table.shape == (21, 14)
    with pytest.raises(ValueError, match="atom14 needs aatype"):
        api.check_violation_loss("violation_loss", dict(pos=pos, mask=mask))
    with pytest.raises(TypeError, match="needs the tensor 'mask'"):
        api.check_violation_loss("violation_loss", dict(pos=pos))
    for kw in (dict(tolerance=-1.0), dict(tolerance=float("nan")), dict(link_factor=float("inf")), dict(link_factor=-0.5), dict(tolerance=True),
               dict(radii="vdw"), dict(radii=np.ones((21, 37), F)), dict(radii=np.full((21, 14), 9.0, F))):
        with pytest.raises(ValueError):
            api.check_violation_loss("violation_loss", d, **kw)
    with pytest.raises(ValueError, match="mask must have the shape"):
        api.check_violation_loss("violation_loss", dict(d, mask=mask[:, :7]))
