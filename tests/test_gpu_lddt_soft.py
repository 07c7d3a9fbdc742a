"""GPU: the smooth lDDT and its fused backward (fcz_lddt_soft_dev, fcz_lddt_soft_grad_dev, their packed and host forms,
Codec.lddt_soft / lddt_soft_grad, foldcomp.smooth_lddt) against the float64 restatement of the contract (tests/_lddt_soft.py) within
the derived bounds given there, `pairs` exactly, determinism on bytes. The device calls write into arrays pre-filled with 0xA5 with
guard bytes on both sides. Every comparison prints the largest observed ratio of the error to its bound."""
import numpy as np
import pytest

import _analysis as AN
import _lddt as Q
import _lddt_soft as S
from _cases import golden_records_raw
from _devpath import DevGuarded, HostGuarded, host_ptr, to_dev
from foldcomp_amd import _lib

pytestmark = pytest.mark.gpu

F = np.float32


def _same_bytes(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(AN.bits(a), AN.bits(b)), (what, np.argwhere(AN.bits(a) != AN.bits(b))[:4])


def _both(codec, dev, bound, n, rows, layout, slot, packed, w, **kw):
    """the value and the gradient of one set of device tensors (pos_true, mask_true, pos_pred, mask_pred or None) -> (soft, pairs, grad)"""
    soft, pairs = S.run_value(codec, *dev, bound, n, rows, layout, slot, packed, **kw)
    return soft, pairs, S.run_grad(codec, *dev, bound, n, rows, layout, slot, packed, w, **kw)


@pytest.fixture(scope="module")
def synthetic():
    """the lattice batch on backbone4 / CA, padded and packed, its weights and the restatement: computed once, never changed"""
    s = S.synthetic_batch(_lib.load().fcz_lddt_pass())
    s["ref"] = S.soft_padded(*s["arrays"], s["lens"], 1, s["w"])
    s["row_off"] = AN.row_off_of(s["lens"])
    s["packed"] = AN.pack(s["arrays"], s["lens"])
    s["w_packed"] = AN.pack1(s["w"], s["lens"])
    s["ref_packed"] = S.pack_ref(s["ref"], s["lens"])
    ref = s["ref"]
    assert ref["pairs"][-1].max() > _lib.load().fcz_lddt_pass() and not ref["pairs"][:3].any() and np.abs(ref["grad"]).max() > 0.1
    return s


def test_synthetic_padded_and_packed(codec, synthetic):
    s = synthetic
    n, L, R = len(s["lens"]), s["L"], int(s["row_off"][-1])
    dev = [to_dev(a) for a in s["arrays"]]
    soft, pairs, grad = _both(codec, dev, to_dev(s["lens"]), n, L, 2, 1, False, to_dev(s["w"]))
    S.check_value((soft, pairs), s["ref"], "lattice, padded")
    S.check_grad(grad, s["ref"], "lattice, padded")
    for e, m in enumerate(s["lens"]):                                         # behind the length: exactly 0
        assert not pairs[e, m:].any() and not AN.bits(soft[e, m:]).any() and not AN.bits(grad[e, m:]).any()
    pdev = [to_dev(a) for a in s["packed"]]
    psoft, ppairs, pgrad = _both(codec, pdev, to_dev(s["row_off"]), n, R, 2, 1, True, to_dev(s["w_packed"]))
    S.check_value((psoft, ppairs), s["ref_packed"], "lattice, packed")
    S.check_grad(pgrad, s["ref_packed"], "lattice, packed")
    # the order of the sums is the chain's alone: padded and packed agree on bytes
    for a, b, what in ((soft, psoft, "soft"), (pairs, ppairs, "pairs"), (grad, pgrad, "grad")):
        _same_bytes(AN.pack1(a, s["lens"]), b, f"padded against packed: {what}")
    # the host-pointer forms through Codec: the bytes of the device forms
    t, mt, p, mp = s["arrays"]
    h = codec.lddt_soft(t, mt, p, mp, 1, length=s["lens"])
    _same_bytes(h["soft"], soft, "Codec.lddt_soft"); _same_bytes(h["pairs"], pairs, "Codec.lddt_soft pairs")
    _same_bytes(codec.lddt_soft_grad(t, mt, p, s["w"], mp, 1, length=s["lens"]), grad, "Codec.lddt_soft_grad")
    t, mt, p, mp = s["packed"]
    h = codec.lddt_soft(t, mt, p, mp, 1, row_off=s["row_off"])
    _same_bytes(h["soft"], psoft, "Codec.lddt_soft, packed"); _same_bytes(h["pairs"], ppairs, "Codec.lddt_soft pairs, packed")
    _same_bytes(codec.lddt_soft_grad(t, mt, p, s["w_packed"], mp, 1, row_off=s["row_off"]), pgrad, "Codec.lddt_soft_grad, packed")


@pytest.fixture(scope="module")
def walk():
    """the noisy random-walk batch on atom14 / CB, no mask_pred, random weights, and the restatement"""
    b = S.walk_batch()
    t, mt, p = b["arrays"]
    b["ref"] = S.soft_padded(t, mt, p, None, b["lens"], 4, b["w"])
    b["dev"] = [to_dev(t), to_dev(mt), to_dev(p), None]
    assert S.tie_share(b["ref"]) <= 0.02
    return b


def test_noisy_walk(codec, walk):
    b = walk
    n, L = len(b["lens"]), b["L"]
    soft, pairs, grad = _both(codec, b["dev"], to_dev(b["lens"]), n, L, 1, 4, False, to_dev(b["w"]))
    S.check_value((soft, pairs), b["ref"], "walk, atom14 CB")
    S.check_grad(grad, b["ref"], "walk, atom14 CB")
    assert (pairs > 0).sum() > 600 and np.abs(grad).max() > 0.01
    # other parameters
    th = (0.25, 1.0, 3.0, 8.0)
    t, mt, p = b["arrays"]
    ref = S.soft_padded(t, mt, p, None, b["lens"], 4, b["w"], 8.0, th)
    soft, pairs, grad = _both(codec, b["dev"], to_dev(b["lens"]), n, L, 1, 4, False, to_dev(b["w"]), cutoff=8.0, thresholds=th)
    S.check_value((soft, pairs), ref, "walk, cutoff 8, other thresholds")
    S.check_grad(grad, ref, "walk, cutoff 8, other thresholds")
    assert ref["pairs"].sum() < b["ref"]["pairs"].sum()


def test_determinism_on_bytes(codec, walk, synthetic):
    b = walk
    n, L = len(b["lens"]), b["L"]
    t, mt, p = b["arrays"]
    w = to_dev(b["w"])
    first = _both(codec, b["dev"], to_dev(b["lens"]), n, L, 1, 4, False, w)
    again = _both(codec, b["dev"], to_dev(b["lens"]), n, L, 1, 4, False, w, guard=4)      # (and outputs that are not 16-byte aligned)
    for a, c, what in zip(first, again, ("soft", "pairs", "grad")):
        _same_bytes(a, c, f"two calls: {what}")
    # pairs are fcz_lddt_dev's
    _same_bytes(first[1], Q.run_dev(codec, *b["dev"], to_dev(b["lens"]), n, L, 1, 4, False)[1], "pairs against fcz_lddt_dev")
    s = synthetic
    sdev = [to_dev(a) for a in s["arrays"]]
    got = S.run_value(codec, *sdev, to_dev(s["lens"]), len(s["lens"]), s["L"], 2, 1, False)[1]
    _same_bytes(got, Q.run_dev(codec, *sdev, to_dev(s["lens"]), len(s["lens"]), s["L"], 2, 1, False)[1], "lattice pairs against fcz_lddt_dev")
    # a chain alone, and the batch permuted: the bytes of the chain inside the batch
    for e in range(n):
        one = [to_dev(a[e:e + 1]) for a in (t, mt, p)] + [None]
        alone = _both(codec, one, to_dev(b["lens"][e:e + 1]), 1, L, 1, 4, False, to_dev(b["w"][e:e + 1]))
        for a, c, what in zip(first, alone, ("soft", "pairs", "grad")):
            _same_bytes(a[e:e + 1], c, f"chain {e} alone: {what}")
    perm = np.asarray([2, 0, 1])
    moved = _both(codec, [to_dev(a[perm]) for a in (t, mt, p)] + [None], to_dev(b["lens"][perm]), n, L, 1, 4, False, to_dev(b["w"][perm]))
    for a, c, what in zip(first, moved, ("soft", "pairs", "grad")):
        _same_bytes(a[perm], c, f"permuted batch: {what}")
    # packed against padded
    lens = b["lens"]
    pk = _both(codec, [to_dev(AN.pack1(a, lens)) for a in (t, mt, p)] + [None], to_dev(AN.row_off_of(lens)), n, int(lens.sum()), 1, 4, True,
               to_dev(AN.pack1(b["w"], lens)))
    for a, c, what in zip(first, pk, ("soft", "pairs", "grad")):
        _same_bytes(AN.pack1(a, lens), c, f"packed: {what}")


def test_length_null_and_clamped(codec):
    lens = [40, 300, 257]
    L = 300
    arrays = S.lattice([L] * 3, L, 14, 4, 12, behind="data")                  # finite rows behind every length below
    w = S.weights((3, L), 13)
    dev, wd = [to_dev(a) for a in arrays], to_dev(w)
    whole = S.soft_padded(*arrays, None, 4, w)
    got = _both(codec, dev, None, 3, L, 1, 4, False, wd)
    S.check_value(got[:2], whole, "length NULL"); S.check_grad(got[2], whole, "length NULL")
    over = _both(codec, dev, to_dev(np.asarray([L + 1, 65535, 0xFFFFFFFF], np.uint32)), 3, L, 1, 4, False, wd)
    for a, c, what in zip(got, over, ("soft", "pairs", "grad")):
        _same_bytes(a, c, f"length > L: {what}")
    ref = S.soft_padded(*arrays, lens, 4, w)
    assert ref["pairs"].sum() < whole["pairs"].sum()
    got = _both(codec, dev, to_dev(np.asarray(lens, np.uint32)), 3, L, 1, 4, False, wd)
    S.check_value(got[:2], ref, "length < L"); S.check_grad(got[2], ref, "length < L")
    # no chain at all: FCZ_OK, and there is no row to write
    g = DevGuarded(S.value_spec((L,)))
    assert codec.lib.fcz_lddt_soft_dev(codec.ctx, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), None, None, 0, L, 1, 4, 15.0, None, *g.ptrs()) == 0
    codec.synchronize()
    assert g.untouched()


def test_hostile_row_off(codec):
    R = 700
    arrays = [a[0] for a in S.lattice([R], R, 4, 1, 13)]
    w = S.weights((R,), 14)
    dev, wd = [to_dev(a) for a in arrays], to_dev(w)
    row_off = AN.HOSTILE_ROW_OFF
    ref = S.soft_packed(*arrays, row_off, 1, w)
    got = _both(codec, dev, to_dev(row_off), 5, R, 2, 1, True, wd)
    S.check_value(got[:2], ref, "hostile row_off"); S.check_grad(got[2], ref, "hostile row_off")
    assert not got[1][:40].any() and not AN.bits(got[0][:40]).any() and not AN.bits(got[2][:40]).any() and got[1][400] == 0
    assert (got[1][40:120] > 0).sum() > 40 and (got[1][401:] > 0).sum() > 200
    # no chain at all: every row is uncovered and filled
    none = _both(codec, dev, to_dev(row_off), 0, R, 2, 1, True, wd)
    assert not none[1].any() and not AN.bits(none[0]).any() and not AN.bits(none[2]).any()
    # the host-pointer forms on the same host arrays, their outputs between guard bytes: what the device forms gave
    for n, dev_form in ((5, got), (0, none)):
        h = HostGuarded(S.value_spec((R,)))
        assert codec.lib.fcz_lddt_soft_packed(codec.ctx, *(host_ptr(a) for a in arrays), host_ptr(row_off), n, R, 2, 1, 15.0, None, *h.ptrs()) == 0
        for a, c in zip(h.all(), dev_form[:2]):
            _same_bytes(a, c, f"fcz_lddt_soft_packed n={n}")
        h = HostGuarded(S.grad_spec((R,)))
        assert codec.lib.fcz_lddt_soft_grad_packed(codec.ctx, *(host_ptr(a) for a in arrays), host_ptr(row_off), n, R, 2, 1, 15.0, None, host_ptr(w), *h.ptrs()) == 0
        _same_bytes(h.all()[0], dev_form[2], f"fcz_lddt_soft_grad_packed n={n}")


def test_refusals_leave_the_outputs_untouched(codec):
    import torch
    n, L, A = 2, 8, 37
    pos, mask, _, off = AN.refusal_inputs(n, L, A)
    wt = torch.zeros((n, L), dtype=torch.float32, device="cuda:0")
    gv, gg = DevGuarded(S.value_spec((n * L,))), DevGuarded(S.grad_spec((n * L,)))
    lib, ctx, P, M, O = codec.lib, codec.ctx, pos.data_ptr(), mask.data_ptr(), off.data_ptr()
    bad_th = [np.asarray(v, F) for v in ((0.5, 1, np.nan, 4), (0.5, 1, 2, np.inf), (-np.inf, 1, 2, 4))]
    torch.cuda.synchronize()
    for padded_fn, packed_fn, o1, o2 in ((lib.fcz_lddt_soft_dev, lib.fcz_lddt_soft_packed_dev, *gv.ptrs()),
                                         (lib.fcz_lddt_soft_grad_dev, lib.fcz_lddt_soft_grad_packed_dev, wt.data_ptr(), gg.ptrs()[0])):
        ok = dict(ctx=ctx, pt=P, mt=M, pp=P, mp=M, bound=None, n=n, L=L, layout=0, slot=1, cutoff=15.0, th=None, o1=o1, o2=o2)
        bad = [dict(ctx=None), dict(pt=None), dict(mt=None), dict(pp=None), dict(o1=None), dict(o2=None), dict(layout=3), dict(layout=-1), dict(slot=37),
               dict(slot=-1), dict(layout=1, slot=14), dict(layout=2, slot=4), dict(cutoff=0.0), dict(cutoff=-1.0), dict(cutoff=float("nan")),
               dict(cutoff=float("inf"))] + [dict(th=t.ctypes.data) for t in bad_th] + [dict(L=2 ** 29 + 1), dict(L=0)]
        for b in bad:
            assert padded_fn(*dict(ok, **b).values()) == -1, b
        for b in bad[:-1]:
            a = dict(ok, bound=O, L=n * L)
            a.update(b)
            assert packed_fn(*a.values()) == -1, b
        assert packed_fn(*dict(ok, L=n * L).values()) == -1                                      # chains without a row_off
        assert padded_fn(*dict(ok, n=0).values()) == 0 and packed_fn(*dict(ok, bound=O, L=0).values()) == 0
    codec.synchronize()
    assert gv.untouched() and gg.untouched()


# ---- Python surface -------------------------------------------------------------------------------------------------------------

def _loss_weights(ref, chains):
    """the row weights of loss = mean over the chains with a pair of 1 - sum soft / sum pairs -> (w of ref's shape, the loss)"""
    w = np.zeros(ref["soft"].shape)
    sums = [(idx, float(ref["soft"][idx].sum()), int(ref["pairs"][idx].sum())) for idx in chains]
    scored = [s for s in sums if s[2] > 0]
    for idx, _, pairs in scored:
        w[idx] = -1.0 / (len(scored) * pairs)
    return w, float(np.mean([1.0 - soft / pairs for _, soft, pairs in scored])) if scored else 0.0


def _check_surface(out, pos_grad, ref0, refw, loss, slot, what):
    """the dict of smooth_lddt and pos.grad after loss.backward() against the restatement (ref0: no weights; refw: the loss' weights)"""
    import torch
    assert set(out) == {"lddt_soft", "lddt_pairs", "lddt_soft_chain", "loss"}, what
    assert out["lddt_soft"].dtype == torch.float32 and out["lddt_pairs"].dtype == torch.int32 and out["lddt_soft_chain"].dtype == torch.float32
    assert out["loss"].dtype == torch.float32 and out["loss"].shape == () and out["lddt_soft"].shape == ref0["soft"].shape
    pairs = out["lddt_pairs"].cpu().numpy()
    assert np.array_equal(pairs, ref0["pairs"]), what
    per_row = out["lddt_soft"].detach().cpu().numpy().astype(np.float64)
    exp = np.where(pairs > 0, ref0["soft"] / np.maximum(pairs, 1), 0.0)
    bound = np.where(pairs > 0, S.soft_bound(ref0) / np.maximum(pairs, 1), 0.0) + 2.0 ** -23        # (the division and the result are float32)
    assert (np.abs(per_row - exp) <= bound).all() and not per_row[pairs == 0].any(), what
    assert abs(float(out["loss"].detach()) - loss) <= float(bound.max()) + 2.0 ** -23, (what, float(out["loss"].detach()), loss)
    g = pos_grad.cpu().numpy()
    ratio = S.check_grad(np.ascontiguousarray(g[..., slot, :]), refw, what)
    others = np.delete(g, slot, axis=-2)
    assert not AN.bits(np.ascontiguousarray(others)).any(), (what, "a gradient at another slot")
    assert np.abs(g).max() > 0
    return ratio


def test_foldcomp_smooth_lddt(codec, golden):
    import torch
    import foldcomp_amd as foldcomp
    records = golden_records_raw(golden)[1]
    lens_all = foldcomp.decode_tensors(records, codec=codec, max_len=8)["length"].cpu().numpy()
    order = np.argsort(lens_all, kind="stable")
    pick = [int(i) for i in order if lens_all[i] >= 40][:4] + [int(order[-1])]       # four short chains and the longest (cropped at 300)
    recs = [records[i] for i in pick]
    n = len(recs)
    rng = np.random.default_rng(29)

    def noisy(t):
        pos = t["pos"].cpu().numpy()
        return (pos + (rng.standard_normal(pos.shape) * 0.5).astype(F)).astype(F)

    # padded, pred as a dict with its mask
    t = foldcomp.decode_tensors(recs, codec=codec, max_len=300)
    L = t["pos"].shape[1]
    assert L == 300 and lens_all[pick[-1]] > 300
    pred_h = noisy(t)
    pred = torch.from_numpy(pred_h).to("cuda:0").requires_grad_()
    out = foldcomp.smooth_lddt(dict(pos=pred, mask=t["mask"]), t, codec=codec)
    assert out["loss"].grad_fn is not None and out["lddt_soft"].grad_fn is not None and out["lddt_soft_chain"].shape == (n,)
    out["loss"].backward()
    mask, lens = t["mask"].cpu().numpy().view(np.uint8), np.minimum(t["length"].cpu().numpy().astype(np.int64), L)
    pos_h = t["pos"].cpu().numpy()
    ref0 = S.soft_padded(pos_h, mask, pred_h, mask, lens, 1)
    w, loss = _loss_weights(ref0, [(e, slice(0, L)) for e in range(n)])
    refw = S.soft_padded(pos_h, mask, pred_h, mask, lens, 1, w)
    assert S.tie_share(refw) <= 0.02
    _check_surface(out, pred.grad, ref0, refw, loss, 1, "smooth_lddt, padded")
    for e, m in enumerate(lens):
        assert not AN.bits(pred.grad[e, m:].cpu().numpy()).any()
    chain = out["lddt_soft_chain"].detach().cpu().numpy()
    assert 0.3 < chain.min() and chain.max() < 0.9 and abs(float(out["loss"].detach()) - (1 - chain.astype(np.float64).mean())) < 1e-6
    # the graph is walked once
    with pytest.raises(RuntimeError):
        out["loss"].backward()
    # no_grad, and a pos that needs no gradient: tensors without a graph, the same values
    with torch.no_grad():
        plain = foldcomp.smooth_lddt(dict(pos=pred, mask=t["mask"]), t, codec=codec)
    still = foldcomp.smooth_lddt(dict(pos=pred.detach(), mask=t["mask"]), t, codec=codec)
    for o in (plain, still):
        assert all(v.grad_fn is None and not v.requires_grad for v in o.values())
        assert AN.teq(o["lddt_soft"], out["lddt_soft"].detach()) and AN.teq(o["loss"], out["loss"].detach()) and AN.teq(o["lddt_pairs"], out["lddt_pairs"])
    assert AN.teq(out["lddt_pairs"], foldcomp.lddt(dict(pos=pred.detach(), mask=t["mask"]), t, codec=codec)["lddt_pairs"])

    # packed, pred a bare tensor, CB
    p = foldcomp.decode_tensors(recs, codec=codec, packed=True)
    ppred_h = noisy(p)
    ppred = torch.from_numpy(ppred_h).to("cuda:0").requires_grad_()
    po = foldcomp.smooth_lddt(ppred, p, atom="CB", codec=codec)
    po["loss"].backward()
    cu = p["cu_seqlens"].cpu().numpy()
    pm = p["mask"].cpu().numpy().view(np.uint8)
    pref0 = S.soft_packed(p["pos"].cpu().numpy(), pm, ppred_h, None, cu, 3)
    w, loss = _loss_weights(pref0, [slice(int(cu[e]), int(cu[e + 1])) for e in range(n)])
    prefw = S.soft_packed(p["pos"].cpu().numpy(), pm, ppred_h, None, cu, 3, w)
    assert S.tie_share(prefw) <= 0.02 and po["lddt_soft"].shape == (int(cu[-1]),) and po["lddt_soft_chain"].shape == (n,)
    _check_surface(po, ppred.grad, pref0, prefw, loss, 3, "smooth_lddt, packed CB")

    # a window: crop_start in the dict, length is not used
    wt = foldcomp.decode_tensors(recs, codec=codec, max_len=64, crop="center", layout="atom14")
    wpred_h = noisy(wt)
    wpred = torch.from_numpy(wpred_h).to("cuda:0").requires_grad_()
    wo = foldcomp.smooth_lddt(dict(pos=wpred), wt, codec=codec)
    wo["loss"].backward()
    wm = wt["mask"].cpu().numpy().view(np.uint8)
    wref0 = S.soft_padded(wt["pos"].cpu().numpy(), wm, wpred_h, None, None, 1)
    w, loss = _loss_weights(wref0, [(e, slice(0, 64)) for e in range(n)])
    wrefw = S.soft_padded(wt["pos"].cpu().numpy(), wm, wpred_h, None, None, 1, w)
    assert S.tie_share(wrefw) <= 0.02
    _check_surface(wo, wpred.grad, wref0, wrefw, loss, 1, "smooth_lddt, window")

    # nothing to score
    e = foldcomp.smooth_lddt(torch.zeros((0, 8, 37, 3), device="cuda:0", requires_grad=True), foldcomp.decode_tensors([], codec=codec, max_len=8), codec=codec)
    assert e["lddt_soft"].shape == (0, 8) and e["lddt_soft_chain"].shape == (0,) and float(e["loss"].detach()) == 0.0
    with pytest.raises(ValueError):
        foldcomp.smooth_lddt(pred[:, :, :14].contiguous(), t, codec=codec)
    with pytest.raises(foldcomp.error):
        foldcomp.smooth_lddt(pred.cpu(), t, codec=codec)


def test_gradient_descent_raises_the_lddt(codec, golden):
    """the sign end to end: a few steps of plain gradient descent on pred lower the loss and raise foldcomp.lddt's lddt_chain"""
    import torch
    import foldcomp_amd as foldcomp
    records = golden_records_raw(golden)[1]
    lens_all = foldcomp.decode_tensors(records, codec=codec, max_len=8)["length"].cpu().numpy()
    # windows of 200 rows of chains that fill them: one step size suits every chain (a row's gradient scales with one over its chain's
    # pairs, and eps has a kink at delta == 0, so a step sized for a long chain makes a chain of a few residues oscillate)
    records = [records[i] for i in np.flatnonzero(lens_all >= 200)[:4]]
    assert len(records) == 4
    t = foldcomp.decode_tensors(records, codec=codec, max_len=200, crop="center")
    gen = torch.Generator(device="cuda:0"); gen.manual_seed(31)
    pred = (t["pos"] + 0.5 * torch.randn(t["pos"].shape, device="cuda:0", generator=gen)).requires_grad_()
    losses, hard, rate = [], [], None
    for step in range(6):
        out = foldcomp.smooth_lddt(pred, t, codec=codec)
        losses.append(float(out["loss"].detach()))
        hard.append(float(foldcomp.lddt(pred.detach(), t, codec=codec)["lddt_chain"].mean()))
        out["loss"].backward()
        if rate is None:
            rate = 0.3 / float(pred.grad.abs().max())                         # the first step moves no atom by more than 0.3 A
        pred = (pred.detach() - rate * pred.grad).requires_grad_()
    print(f"gradient descent, {len(records)} chains: loss {losses[0]:.4f} -> {losses[-1]:.4f}, lddt_chain {hard[0]:.4f} -> {hard[-1]:.4f}")
    assert losses[-1] < losses[0] - 0.02
    assert hard[-1] > hard[0] + 0.02
