"""GPU: the backbone FAPE and its fused backward (fcz_fape_dev, fcz_fape_grad_dev, their packed and host forms, Codec.fape / fape_grad,
foldcomp.fape) against the float64 restatement of the contract (tests/_fape.py) within the derived bounds given there, `points`
exactly, determinism on bytes. The device calls write into arrays pre-filled with 0xA5 with guard bytes on both sides. Every
comparison prints the largest observed ratio of the error to its bound."""
import numpy as np
import pytest

import _analysis as AN
import _fape as FP
import _frames as FRM
from _cases import golden_records_raw
from _devpath import DevGuarded, HostGuarded, host_ptr, to_dev
from foldcomp_amd import _lib

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = ("sum", "points", "grad_rot", "grad_trans", "grad_pos")


def _same_bytes(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(AN.bits(a), AN.bits(b)), (what, np.argwhere(AN.bits(a) != AN.bits(b))[:4])


def _all_same(first, other, what, pick=lambda a: a):
    for a, c, name in zip(first, other, NAMES):
        _same_bytes(pick(a), c, f"{what}: {name}")


def _check(got, ref, what):
    return (FP.check_value(got[:2], ref, what),) + FP.check_grad(got[2:], ref, what)


def _frames_of(inp, side):
    return inp["rot_" + side], inp["trans_" + side], inp["fm_" + side]


@pytest.fixture(scope="module")
def synthetic():
    """the lattice batch on backbone4 / CA, padded and packed, its weights and the restatement: computed once, never changed"""
    P = _lib.load().fcz_fape_pass()
    s = FP.synthetic_batch(P)
    s["ref"] = FP.fape_padded(s["inp"], s["lens"], 1, s["w"], FP.LATTICE_CLAMP)
    assert FP.tie_share(s["ref"]) == 0                                        # before any device result is looked at
    s["row_off"] = AN.row_off_of(s["lens"])
    s["packed"] = FP.pack_inp(s["inp"], s["lens"])
    s["w_packed"] = AN.pack1(s["w"], s["lens"])
    s["ref_packed"] = FP.pack_ref(s["ref"], s["lens"])
    ref = s["ref"]
    assert ref["points"][-1].max() > 2 * P * 0.7 and s["lens"][-1] == 2 * P + 3 and np.abs(ref["grad_pos"]).max() > 0.1 and ref["clamped"].sum() > 1000
    return s


def test_lattice_padded_and_packed(codec, synthetic):
    s = synthetic
    n, L, R = len(s["lens"]), s["L"], int(s["row_off"][-1])
    C = FP.LATTICE_CLAMP
    got = FP.run_both(codec, FP.to_dev(s["inp"]), to_dev(s["lens"]), n, L, 2, 1, False, to_dev(s["w"]), clamp=C)
    _check(got, s["ref"], "lattice, padded")
    for e, m in enumerate(s["lens"]):                                         # behind the length: exactly 0
        assert all(not AN.bits(a[e, m:]).any() for a in got)
    pk = FP.run_both(codec, FP.to_dev(s["packed"]), to_dev(s["row_off"]), n, R, 2, 1, True, to_dev(s["w_packed"]), clamp=C)
    _check(pk, s["ref_packed"], "lattice, packed")
    # the order of the sums is the chain's alone: padded and packed agree on bytes
    _all_same(got, pk, "padded against packed", lambda a: AN.pack1(a, s["lens"]))
    # the host-pointer forms through Codec: the bytes of the device forms
    for inp, w, dev_form, kw, what in ((s["inp"], s["w"], got, dict(length=s["lens"]), "padded"), (s["packed"], s["w_packed"], pk, dict(row_off=s["row_off"]), "packed")):
        a = (_frames_of(inp, "t"), inp["pos_t"], inp["mask_t"], _frames_of(inp, "p"), inp["pos_p"])
        h = codec.fape(*a, inp["mask_p"], 1, clamp=C, **kw)
        _same_bytes(h["sum"], dev_form[0], f"Codec.fape, {what}"); _same_bytes(h["points"], dev_form[1], f"Codec.fape points, {what}")
        g = codec.fape_grad(*a, w, inp["mask_p"], 1, clamp=C, **kw)
        for k, d in zip(("grad_rot", "grad_trans", "grad_pos"), dev_form[2:]):
            _same_bytes(g[k], d, f"Codec.fape_grad {k}, {what}")


@pytest.fixture(scope="module")
def walk():
    """the noisy batch on atom14 / CB, no masks of the prediction, random weights, and the restatement"""
    b = FP.walk_batch()
    b["ref"] = FP.fape_padded(b["inp"], b["lens"], 4, b["w"], 10.0)
    assert FP.tie_share(b["ref"]) <= 0.02
    b["dev"] = FP.to_dev(b["inp"])
    return b


def test_noisy_walk(codec, walk):
    b = walk
    n, L = len(b["lens"]), b["L"]
    lens_t, w = to_dev(b["lens"]), to_dev(b["w"])
    got = FP.run_both(codec, b["dev"], lens_t, n, L, 1, 4, False, w)
    _check(got, b["ref"], "walk, atom14 CB, clamp 10")
    assert (got[1] > 0).sum() > 600 and np.abs(got[4]).max() > 0.01 and 0 < b["ref"]["clamped"].sum() < b["ref"]["terms"].sum()
    free = FP.fape_padded(b["inp"], b["lens"], 4, b["w"], float("inf"))
    assert FP.tie_share(free) == 0 and free["sum"].sum() > b["ref"]["sum"].sum() * 1.01 and np.abs(free["grad_pos"] - b["ref"]["grad_pos"]).max() > 0.1
    _check(FP.run_both(codec, b["dev"], lens_t, n, L, 1, 4, False, w, clamp=float("inf")), free, "walk, unclamped")
    other = FP.fape_padded(b["inp"], b["lens"], 4, b["w"], 10.0, 0.25)
    assert FP.tie_share(other) <= 0.02 and other["sum"].sum() > b["ref"]["sum"].sum()
    _check(FP.run_both(codec, b["dev"], lens_t, n, L, 1, 4, False, w, eps=0.25), other, "walk, eps 0.25")


def test_determinism_on_bytes(codec, walk):
    b = walk
    n, L = len(b["lens"]), b["L"]
    inp, lens = b["inp"], b["lens"]
    w = to_dev(b["w"])
    first = FP.run_both(codec, b["dev"], to_dev(lens), n, L, 1, 4, False, w)
    again = FP.run_both(codec, b["dev"], to_dev(lens), n, L, 1, 4, False, w, guard=4)       # (and outputs that are not 16-byte aligned)
    _all_same(first, again, "two calls")
    # a chain alone, and the batch permuted: the bytes of the chain inside the batch
    cut = lambda idx: {k: None if v is None else v[idx] for k, v in inp.items()}
    for e in range(n):
        alone = FP.run_both(codec, FP.to_dev(cut(slice(e, e + 1))), to_dev(lens[e:e + 1]), 1, L, 1, 4, False, to_dev(b["w"][e:e + 1]))
        _all_same(first, alone, f"chain {e} alone", lambda a: a[e:e + 1])
    perm = np.asarray([2, 0, 1])
    moved = FP.run_both(codec, FP.to_dev(cut(perm)), to_dev(lens[perm]), n, L, 1, 4, False, to_dev(b["w"][perm]))
    _all_same(first, moved, "permuted batch", lambda a: a[perm])
    # packed against padded
    pk = FP.run_both(codec, FP.to_dev(FP.pack_inp(inp, lens)), to_dev(AN.row_off_of(lens)), n, int(lens.sum()), 1, 4, True, to_dev(AN.pack1(b["w"], lens)))
    _all_same(first, pk, "packed", lambda a: AN.pack1(a, lens))


def test_length_null_and_clamped(codec):
    lens = [40, 300, 257]
    L = 300
    C = FP.LATTICE_CLAMP
    inp = FP.lattice([L] * 3, L, 14, 4, 12, behind="data")                    # finite rows behind every length below
    w = FP.weights((3, L), 13)
    dev, wd = FP.to_dev(inp), to_dev(w)
    whole = FP.fape_padded(inp, None, 4, w, C)
    got = FP.run_both(codec, dev, None, 3, L, 1, 4, False, wd, clamp=C)
    _check(got, whole, "length NULL")
    over = FP.run_both(codec, dev, to_dev(np.asarray([L + 1, 65535, 0xFFFFFFFF], np.uint32)), 3, L, 1, 4, False, wd, clamp=C)
    _all_same(got, over, "length > L")
    ref = FP.fape_padded(inp, lens, 4, w, C)
    assert ref["points"].sum() < whole["points"].sum()
    _check(FP.run_both(codec, dev, to_dev(np.asarray(lens, np.uint32)), 3, L, 1, 4, False, wd, clamp=C), ref, "length < L")
    # no chain at all: FCZ_OK, and there is no row to write
    gv, gg = DevGuarded(FP.value_spec((L,))), DevGuarded(FP.grad_spec((L,)))
    ptrs = [AN.ptr(t) for t in dev]
    assert codec.lib.fcz_fape_dev(codec.ctx, *ptrs, None, 0, L, 1, 4, 10.0, 1e-4, *gv.ptrs()) == 0
    assert codec.lib.fcz_fape_grad_dev(codec.ctx, *ptrs, None, 0, L, 1, 4, 10.0, 1e-4, wd.data_ptr(), *gg.ptrs()) == 0
    codec.synchronize()
    assert gv.untouched() and gg.untouched()


def test_hostile_row_off(codec):
    R = 700
    C = FP.LATTICE_CLAMP
    inp = {k: v[0] for k, v in FP.lattice([R], R, 4, 1, 13).items()}
    w = FP.weights((R,), 14)
    dev, wd = FP.to_dev(inp), to_dev(w)
    row_off = AN.HOSTILE_ROW_OFF
    ref = FP.fape_packed(inp, row_off, 1, w, C)
    got = FP.run_both(codec, dev, to_dev(row_off), 5, R, 2, 1, True, wd, clamp=C)
    _check(got, ref, "hostile row_off")
    assert all(not AN.bits(a[:40]).any() for a in got) and got[1][400] in (0, 1)
    assert (got[1][40:120] > 0).sum() > 40 and (got[1][401:] > 0).sum() > 200
    # no chain at all: every row is uncovered and filled
    none = FP.run_both(codec, dev, to_dev(row_off), 0, R, 2, 1, True, wd, clamp=C)
    assert all(not AN.bits(a).any() for a in none)
    # the host-pointer forms on the same host arrays, their outputs between guard bytes: what the device forms gave
    hp = [host_ptr(inp[k]) for k in FP.ORDER]
    for n, dev_form in ((5, got), (0, none)):
        h = HostGuarded(FP.value_spec((R,)))
        assert codec.lib.fcz_fape_packed(codec.ctx, *hp, host_ptr(row_off), n, R, 2, 1, C, 1e-4, *h.ptrs()) == 0
        for a, c in zip(h.all(), dev_form[:2]):
            _same_bytes(a, c, f"fcz_fape_packed n={n}")
        h = HostGuarded(FP.grad_spec((R,)))
        assert codec.lib.fcz_fape_grad_packed(codec.ctx, *hp, host_ptr(row_off), n, R, 2, 1, C, 1e-4, host_ptr(w), *h.ptrs()) == 0
        for a, c in zip(h.all(), dev_form[2:]):
            _same_bytes(a, c, f"fcz_fape_grad_packed n={n}")


def test_refusals_leave_the_outputs_untouched(codec):
    import torch
    n, L, A = 2, 8, 37
    pos, mask, _, off = AN.refusal_inputs(n, L, A)
    rot = torch.eye(3, dtype=torch.float32, device="cuda:0").repeat(n, L, 1, 1).contiguous()
    trans = torch.zeros((n, L, 3), dtype=torch.float32, device="cuda:0")
    fm = torch.ones((n, L), dtype=torch.uint8, device="cuda:0")
    wt = torch.zeros((n, L), dtype=torch.float32, device="cuda:0")
    gv, gg = DevGuarded(FP.value_spec((n * L,))), DevGuarded(FP.grad_spec((n * L,)))
    lib, ctx, O = codec.lib, codec.ctx, off.data_ptr()
    torch.cuda.synchronize()
    for padded_fn, packed_fn, outs in ((lib.fcz_fape_dev, lib.fcz_fape_packed_dev, gv.ptrs()),
                                       (lib.fcz_fape_grad_dev, lib.fcz_fape_grad_packed_dev, [wt.data_ptr()] + gg.ptrs())):
        ok = dict(ctx=ctx, rt=rot.data_ptr(), tt=trans.data_ptr(), ft=fm.data_ptr(), pt=pos.data_ptr(), mt=mask.data_ptr(), rp=rot.data_ptr(), tp=trans.data_ptr(),
                  fp=fm.data_ptr(), pp=pos.data_ptr(), mp=mask.data_ptr(), bound=None, n=n, L=L, layout=0, slot=1, clamp=10.0, eps=1e-4)
        ok.update({f"o{i}": o for i, o in enumerate(outs)})
        bad = [dict(ctx=None)] + [{k: None} for k in ("rt", "tt", "ft", "pt", "mt", "rp", "tp", "pp")] + [{f"o{i}": None} for i in range(len(outs))]
        bad += [dict(layout=3), dict(layout=-1), dict(slot=37), dict(slot=-1), dict(layout=1, slot=14), dict(layout=2, slot=4), dict(clamp=0.0), dict(clamp=-1.0),
                dict(clamp=float("nan")), dict(eps=0.0), dict(eps=-1.0), dict(eps=float("nan")), dict(eps=float("inf")), dict(L=2 ** 29 + 1), dict(L=0)]
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

def _loss_weights(ref, chains, scale):
    """the row weights of loss = mean over the chains with a frame and a point of sum / (frames * points * scale) -> (w, the loss)"""
    w = np.zeros(ref["sum"].shape)
    sums = [(idx, float(ref["sum"][idx].sum()), int(ref["points"][idx].sum())) for idx in chains]
    scored = [s for s in sums if s[2] > 0]
    for idx, _, pts in scored:
        w[idx] = 1.0 / (len(scored) * pts * scale)
    return w, float(np.mean([total / (pts * scale) for _, total, pts in scored])) if scored else 0.0


def _check_values(out, ref0, loss, scale, what):
    import torch
    assert set(out) == {"fape_frame", "fape_points", "frame_mask", "fape_chain", "loss"}, what
    assert out["fape_frame"].dtype == torch.float32 and out["fape_points"].dtype == torch.int32 and out["frame_mask"].dtype == torch.bool
    assert out["fape_chain"].dtype == torch.float32 and out["loss"].dtype == torch.float32 and out["loss"].shape == () and out["fape_frame"].shape == ref0["sum"].shape
    pts = out["fape_points"].cpu().numpy()
    assert np.array_equal(pts, ref0["points"]) and np.array_equal(out["frame_mask"].cpu().numpy(), ref0["frame"]), what
    per_row = out["fape_frame"].detach().cpu().numpy().astype(np.float64)
    exp = np.where(pts > 0, ref0["sum"] / (np.maximum(pts, 1) * scale), 0.0)
    bound = np.where(pts > 0, ref0["b_sum"] / (np.maximum(pts, 1) * scale), 0.0) + 2.0 ** -22 * exp + 2.0 ** -40       # (two float32 operations behind sum)
    assert (np.abs(per_row - exp) <= bound).all() and not per_row[pts == 0].any(), what
    assert abs(float(out["loss"].detach()) - loss) <= float(bound.max()) + 2.0 ** -23 * loss, (what, float(out["loss"].detach()), loss)


def _pick(codec, golden):
    import foldcomp_amd as foldcomp
    records = golden_records_raw(golden)[1]
    lens_all = foldcomp.decode_tensors(records, codec=codec, max_len=8)["length"].cpu().numpy()
    order = np.argsort(lens_all, kind="stable")
    pick = [int(i) for i in order if lens_all[i] >= 40][:4] + [int(order[-1])]       # four short chains and the longest (cropped at 300)
    assert lens_all[pick[-1]] > 300
    return [records[i] for i in pick]


def test_foldcomp_fape_frames_from_coordinates(codec, golden):
    """padded, pred a pos tensor: Algorithm 21 in torch in front of the kernel, autograd carries the gradient on to pos"""
    import torch
    import foldcomp_amd as foldcomp
    from foldcomp_amd import tensors
    recs = _pick(codec, golden)
    n = len(recs)
    rng = np.random.default_rng(47)
    t = foldcomp.decode_tensors(recs, codec=codec, max_len=300)
    L = t["pos"].shape[1]
    pos_h, mask = t["pos"].cpu().numpy(), t["mask"].cpu().numpy().view(np.uint8)
    lens = np.minimum(t["length"].cpu().numpy().astype(np.int64), L)
    pred_h = (pos_h + (rng.standard_normal(pos_h.shape) * 0.5).astype(F)).astype(F)
    pred = torch.from_numpy(pred_h).to("cuda:0").requires_grad_()
    out = foldcomp.fape(dict(pos=pred, mask=t["mask"]), t, codec=codec)
    assert out["loss"].grad_fn is not None and out["fape_frame"].grad_fn is not None and out["fape_chain"].shape == (n,)
    out["loss"].backward()
    # the restatement on the frames the call used: the truth's are fcz_frames_dev's (tests/_frames.py restates them to the bit), the
    # prediction's the builder's on the device
    rt, tt, ft = FRM.frames(pos_h, mask, None, lens, 0, 0)
    with torch.no_grad():
        rp, tp, fp = (v.cpu().numpy() for v in tensors.backbone_frames_torch(pred.detach(), t["mask"]))
    inp = dict(rot_t=rt[..., 0, :, :], trans_t=tt[..., 0, :], fm_t=ft[..., 0], pos_t=pos_h, mask_t=mask, rot_p=rp, trans_p=tp, fm_p=fp.view(np.uint8), pos_p=pred_h,
               mask_p=mask)
    ref0 = FP.fape_padded(inp, lens, 1)
    w, loss = _loss_weights(ref0, [(e, slice(0, L)) for e in range(n)], 10.0)
    refw = FP.fape_padded(inp, lens, 1, w)
    assert FP.tie_share(refw) <= 0.02 and ref0["frame"].sum() > 400
    _check_values(out, ref0, loss, 10.0, "fape, padded, frames from coordinates")
    chain = out["fape_chain"].detach().cpu().numpy()
    # (a term is at most the clamp, so a chain at most clamp / scale = 1; frames built from atoms moved by 0.5 A turn by tens of degrees)
    assert 0.0 < chain.min() and chain.max() <= 1.0 and abs(float(out["loss"].detach()) - chain.astype(np.float64).mean()) < 1e-6
    # pos.grad: the restatement's three gradients carried through the builder in float64 on the host. The builder's Jacobian, with
    # v1 = C - CA, v2 = N - CA, n1 = |v1|, n2 = |v2 - e1 (e1 . v2)|: e1 moves by at most 1 / n1 per Angstrom, e2 by 1 / n2 through v2
    # and 2 |v2| / (n1 n2) through e1, e3 = e1 x e2 by their sum, so no entry of rot moves by more than J = 1 / n1 + 1 / n2 +
    # 2 |v2| / (n1 n2), and the kernel's error reaches a coordinate of pos.grad as at most 9 J b_rot + b_trans + b_pos (nine entries a
    # frame). The float32 builder and its float32 backward add a few 2^-24 relative to each partial sum: 2^-16 max(J, 1) of their
    # absolute sum is allowed.
    p64 = torch.tensor(pred_h.astype(np.float64), requires_grad=True)
    r64, t64, _ = tensors.backbone_frames_torch(p64, torch.tensor(mask))
    ((r64 * torch.tensor(refw["grad_rot"])).sum() + (t64 * torch.tensor(refw["grad_trans"])).sum()).backward()
    exp = p64.grad.numpy().copy()
    exp[:, :, 1] += refw["grad_pos"]
    g = pred.grad.cpu().numpy()
    v1, v2 = pred_h[:, :, 2].astype(np.float64) - pred_h[:, :, 1], pred_h[:, :, 0].astype(np.float64) - pred_h[:, :, 1]
    with np.errstate(all="ignore"):
        n1 = np.linalg.norm(v1, axis=-1)
        n2 = np.linalg.norm(v2 - v1 * ((v1 * v2).sum(-1) / n1 ** 2)[..., None], axis=-1)
        J = np.where(refw["frame"], 1 / n1 + 1 / n2 + 2 * np.linalg.norm(v2, axis=-1) / (n1 * n2), 0.0)
    scale_row = np.abs(refw["grad_rot"]).sum(axis=(-1, -2)) + np.abs(refw["grad_trans"]).sum(axis=-1) + np.abs(refw["grad_pos"]).sum(axis=-1)
    bound = 9.0 * J * refw["b_rot"] + refw["b_trans"] + refw["b_pos"] + 2.0 ** -16 * np.maximum(J, 1.0) * scale_row
    err = np.abs(g.astype(np.float64) - exp).max(axis=(-1, -2))
    ratio = float((err[bound > 0] / bound[bound > 0]).max())
    print(f"fape, padded, frames from coordinates: pos.grad, largest |error| / bound = {ratio:.4f}")
    assert (err <= bound).all() and np.abs(g).max() > 1e-5, (np.argwhere(err > bound)[:4], ratio)
    assert not AN.bits(np.ascontiguousarray(g[:, :, 3:])).any(), "a gradient outside N, CA, C and the atom's slot"
    for e, m in enumerate(lens):
        assert not AN.bits(g[e, m:]).any()
    # the graph is walked once
    with pytest.raises(RuntimeError):
        out["loss"].backward()
    # no_grad, and a pos that needs no gradient: tensors without a graph, the same values
    with torch.no_grad():
        plain = foldcomp.fape(dict(pos=pred, mask=t["mask"]), t, codec=codec)
    still = foldcomp.fape(dict(pos=pred.detach(), mask=t["mask"]), t, codec=codec)
    for o in (plain, still):
        assert all(v.grad_fn is None and not v.requires_grad for v in o.values())
        assert all(AN.teq(o[k], out[k].detach()) for k in out)
    # the truth's frames from the dict, when it carries the backbone ones: the same bytes
    tf = foldcomp.decode_tensors(recs, codec=codec, max_len=300, frames="backbone")
    again = foldcomp.fape(dict(pos=pred.detach(), mask=t["mask"]), tf, codec=codec)
    assert all(AN.teq(again[k], out[k].detach()) for k in out)
    # CB on atom37 (slot 3), unclamped: the gradient reaches N, CA, C and slot 3 only
    pred2 = pred.detach().clone().requires_grad_()
    o2 = foldcomp.fape(pred2, t, atom="CB", clamp=None, codec=codec)
    o2["loss"].backward()
    g2 = pred2.grad.cpu().numpy()
    assert not AN.bits(np.ascontiguousarray(g2[:, :, 4:])).any() and np.abs(g2[:, :, 3]).max() > 1e-6 and float(o2["loss"].detach()) > float(out["loss"].detach()) * 0.5
    # nothing to score, a layout mismatch, a CPU tensor
    e = foldcomp.fape(torch.zeros((0, 8, 37, 3), device="cuda:0", requires_grad=True), foldcomp.decode_tensors([], codec=codec, max_len=8), codec=codec)
    assert e["fape_frame"].shape == (0, 8) and e["fape_chain"].shape == (0,) and float(e["loss"].detach()) == 0.0
    with pytest.raises(ValueError):
        foldcomp.fape(pred[:, :, :14].contiguous(), t, codec=codec)
    with pytest.raises(foldcomp.error):
        foldcomp.fape(pred.cpu(), t, codec=codec)


def test_foldcomp_fape_model_frames(codec, golden):
    """packed, the model's own frames and no pos: the points are trans, and trans.grad holds both contributions; then a window"""
    import torch
    import foldcomp_amd as foldcomp
    recs = _pick(codec, golden)
    n = len(recs)
    rng = np.random.default_rng(53)
    # the padded decode at 300 rows, packed here: the packed decode keeps every residue of the longest chain, and a noisy chain of
    # more than 350 rows leans on the tie allowance in more than 2 % of its rows (tests/_fape.py)
    t = foldcomp.decode_tensors(recs, codec=codec, max_len=300, frames="backbone")
    tl = [min(int(m), 300) for m in t["length"].cpu().numpy()]
    p = {k: torch.cat([t[k][e, :m] for e, m in enumerate(tl)]).contiguous() for k in ("pos", "mask", "rot", "trans", "frame_mask")}
    p["cu_seqlens"] = torch.from_numpy(AN.row_off_of(tl).astype(np.int32)).to("cuda:0")
    cu = p["cu_seqlens"].cpu().numpy()
    R = int(cu[-1])
    rot_t, trans_t, fm_t = p["rot"].cpu().numpy(), p["trans"].cpu().numpy(), p["frame_mask"].cpu().numpy().view(np.uint8)
    rot_h = (FP.small_rotations(rng, (R,), 0.15) @ rot_t.astype(np.float64)).astype(F)
    trans_h = (trans_t + (rng.standard_normal((R, 3)) * 0.5).astype(F)).astype(F)
    rot = torch.from_numpy(rot_h).to("cuda:0").requires_grad_()
    trans = torch.from_numpy(trans_h).to("cuda:0").requires_grad_()
    out = foldcomp.fape(dict(rot=rot, trans=trans), p, codec=codec)
    out["loss"].backward()
    pos_h, mask = p["pos"].cpu().numpy(), p["mask"].cpu().numpy().view(np.uint8)
    pts = np.zeros_like(pos_h)
    pts[:, 1] = trans_h
    inp = dict(rot_t=rot_t, trans_t=trans_t, fm_t=fm_t, pos_t=pos_h, mask_t=mask, rot_p=rot_h, trans_p=trans_h, fm_p=None, pos_p=pts, mask_p=None)
    ref0 = FP.fape_packed(inp, cu, 1)
    w, loss = _loss_weights(ref0, [slice(int(cu[e]), int(cu[e + 1])) for e in range(n)], 10.0)
    refw = FP.fape_packed(inp, cu, 1, w)
    assert FP.tie_share(refw) <= 0.02 and out["fape_frame"].shape == (R,) and out["fape_chain"].shape == (n,)
    _check_values(out, ref0, loss, 10.0, "fape, packed, model frames")
    both = dict(refw, grad_trans=refw["grad_trans"] + refw["grad_pos"], b_trans=refw["b_trans"] + refw["b_pos"] + 2.0 ** -23 * (np.abs(refw["grad_trans"]).max(axis=-1)
                + np.abs(refw["grad_pos"]).max(axis=-1)), grad_pos=np.zeros_like(refw["grad_pos"]), b_pos=np.zeros_like(refw["b_pos"]),
                frame=refw["frame"] | refw["point"])
    rot_ok = FP._ratio(np.abs(rot.grad.cpu().numpy().astype(np.float64) - refw["grad_rot"]).max(axis=(-1, -2)), refw["b_rot"], "model frames", "rot.grad")
    tr_ok = FP._ratio(np.abs(trans.grad.cpu().numpy().astype(np.float64) - both["grad_trans"]).max(axis=-1), both["b_trans"], "model frames", "trans.grad")
    print(f"fape, packed, model frames: rot.grad / trans.grad (both contributions), largest |error| / bound = {rot_ok:.4f} / {tr_ok:.4f}")
    assert np.abs(refw["grad_pos"]).max() > 1e-6 and np.abs(refw["grad_trans"]).max() > 1e-6 and np.abs(rot.grad.cpu().numpy()).max() > 1e-5
    assert not AN.bits(rot.grad.cpu().numpy()[~refw["frame"]]).any()

    # a window: crop_start in the dict, length is not used; the model's frames beside a pos of its own, on atom14
    wt = foldcomp.decode_tensors(recs, codec=codec, max_len=64, crop="center", layout="atom14", frames="backbone")
    wpos_h = wt["pos"].cpu().numpy()
    wpred_h = (wpos_h + (rng.standard_normal(wpos_h.shape) * 0.5).astype(F)).astype(F)
    wrot_t, wtrans_t = wt["rot"].cpu().numpy(), wt["trans"].cpu().numpy()
    wrot_h = (FP.small_rotations(rng, wrot_t.shape[:2], 0.15) @ wrot_t.astype(np.float64)).astype(F)
    wtrans_h = (wtrans_t + (rng.standard_normal(wtrans_t.shape) * 0.5).astype(F)).astype(F)
    wfm_h = (rng.random(wrot_t.shape[:2]) > 0.1)
    leaves = [torch.from_numpy(a).to("cuda:0").requires_grad_() for a in (wrot_h, wtrans_h, wpred_h)]
    wo = foldcomp.fape(dict(rot=leaves[0], trans=leaves[1], pos=leaves[2], frame_mask=torch.from_numpy(wfm_h).to("cuda:0")), wt, atom="CB", clamp=None, codec=codec)
    wo["loss"].backward()
    winp = dict(rot_t=wrot_t, trans_t=wtrans_t, fm_t=wt["frame_mask"].cpu().numpy().view(np.uint8), pos_t=wpos_h, mask_t=wt["mask"].cpu().numpy().view(np.uint8),
                rot_p=wrot_h, trans_p=wtrans_h, fm_p=wfm_h.view(np.uint8), pos_p=wpred_h, mask_p=None)
    wref0 = FP.fape_padded(winp, None, 4, None, float("inf"))
    w, loss = _loss_weights(wref0, [(e, slice(0, 64)) for e in range(n)], 10.0)
    wrefw = FP.fape_padded(winp, None, 4, w, float("inf"))
    _check_values(wo, wref0, loss, 10.0, "fape, window")
    g = leaves[2].grad.cpu().numpy()
    FP.check_grad((leaves[0].grad.cpu().numpy(), leaves[1].grad.cpu().numpy(), np.ascontiguousarray(g[:, :, 4])), wrefw, "fape, window")
    assert not AN.bits(np.ascontiguousarray(np.delete(g, 4, axis=2))).any() and np.abs(g).max() > 1e-6


def test_gradient_descent_lowers_the_fape(codec, golden):
    """the sign end to end: six steps of plain gradient descent on the coordinates, every one of which must lower the loss"""
    import torch
    import foldcomp_amd as foldcomp
    records = golden_records_raw(golden)[1]
    lens_all = foldcomp.decode_tensors(records, codec=codec, max_len=8)["length"].cpu().numpy()
    records = [records[i] for i in np.flatnonzero(lens_all >= 200)[:4]]
    assert len(records) == 4
    t = foldcomp.decode_tensors(records, codec=codec, max_len=200, crop="center")
    gen = torch.Generator(device="cuda:0"); gen.manual_seed(59)
    pred = (t["pos"] + 0.5 * torch.randn(t["pos"].shape, device="cuda:0", generator=gen)).requires_grad_()
    losses, rate = [], None
    for step in range(7):
        out = foldcomp.fape(pred, t, codec=codec)
        losses.append(float(out["loss"].detach()))
        if step == 6:
            break
        out["loss"].backward()
        if rate is None:
            rate = 0.3 / float(pred.grad.abs().max())                         # the first step moves no atom by more than 0.3 A
        pred = (pred.detach() - rate * pred.grad).requires_grad_()
    print("gradient descent on the FAPE, 4 chains of 200 rows: loss " + " -> ".join(f"{v:.5f}" for v in losses))
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
