"""GPU: the all-atom FAPE over the eight rigid groups and its fused backward (fcz_fape_atoms_dev, fcz_fape_atoms_grad_dev, their packed
and host forms, Codec.fape_atoms / fape_atoms_grad, foldcomp.fape_atoms) against the float64 restatement of the contract
(tests/_fape_atoms.py) within the bounds derived in tests/_fape.py, `points` exactly, determinism on bytes. The device calls write
into arrays pre-filled with 0xA5 with guard bytes on both sides. Every comparison prints the largest observed ratio of the error to
its bound."""
import numpy as np
import pytest

import _analysis as AN
import _fape as FP
import _fape_atoms as FA
import _frames as FRM
import _lddt_atoms as LA
from _cases import golden_records_raw
from _devpath import DevGuarded, HostGuarded, host_ptr, to_dev
from foldcomp_amd import _lib

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = FA.OUT_KEYS
C = FA.LATTICE_CLAMP


def _same_bytes(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(AN.bits(a), AN.bits(b)), (what, np.argwhere(AN.bits(a) != AN.bits(b))[:4])


def _all_same(first, other, what, pick=lambda a: a):
    for a, c, name in zip(first, other, NAMES):
        _same_bytes(pick(a), c, f"{what}: {name}")


def _check(got, ref, what):
    return (FA.check_value(got[:2], ref, what),) + FA.check_grad(got[2:], ref, what)


def _frames_of(inp, side):
    return inp["rot_" + side], inp["trans_" + side], inp["fm_" + side]


def _codec_forms(codec, inp, w, dev_form, kw, what, clamp=C):
    """Codec.fape_atoms / fape_atoms_grad (the host-pointer entry points) against the bytes of the device forms"""
    a = (_frames_of(inp, "t"), inp["pos_t"], inp["mask_t"], _frames_of(inp, "p"), inp["pos_p"])
    rest = dict(mask_pred=inp["mask_p"], aatype=inp["aatype"], swapped=inp["swapped"], clamp=clamp, **kw)
    h = codec.fape_atoms(*a, **rest)
    _same_bytes(h["sum"], dev_form[0], f"Codec.fape_atoms, {what}"); _same_bytes(h["points"], dev_form[1], f"Codec.fape_atoms points, {what}")
    g = codec.fape_atoms_grad(*a, w, **rest)
    for k, d in zip(("grad_rot", "grad_trans", "grad_pos"), dev_form[2:]):
        _same_bytes(g[k], d, f"Codec.fape_atoms_grad {k}, {what}")


@pytest.fixture(scope="module")
def synthetic():
    """the atom14 lattice batch, padded and packed, its weights and the restatement: computed once, never changed"""
    lib = _lib.load()
    T, P = lib.fcz_fape_atoms_tile_rows(1), lib.fcz_fape_atoms_pass()
    s = FA.synthetic_batch(T)
    s["ref"] = FA.ref_padded(s["inp"], s["lens"], s["w"], C)
    assert FA.tie_share(s["ref"]) == 0                                        # before any device result is looked at
    s["row_off"] = AN.row_off_of(s["lens"])
    s["packed"] = FA.pack_inp(s["inp"], s["lens"])
    s["w_packed"] = AN.pack1(s["w"], s["lens"])
    s["ref_packed"] = FA.pack_ref(s["ref"], s["lens"])
    ref = s["ref"]
    assert list(s["lens"][:6]) == [0, 1, 2, T - 1, T, T + 1] and ref["points"][-1].max() > 2 * P and ref["frame"][-1].sum() > 2 * 256
    assert np.abs(ref["grad_pos"]).max() > 0.1 and ref["clamped"].sum() > 1000 and 0.3 < ref["frame"][5, :T + 1].mean() < 0.7
    return s


def test_lattice_padded_and_packed(codec, synthetic):
    s = synthetic
    n, L, R = len(s["lens"]), s["L"], int(s["row_off"][-1])
    got = FA.run_both(codec, FA.to_dev(s["inp"]), to_dev(s["lens"]), n, L, 1, False, to_dev(s["w"]), clamp=C)
    _check(got, s["ref"], "lattice atom14, padded")
    for e, m in enumerate(s["lens"]):                                         # behind the length: exactly 0
        assert all(not AN.bits(a[e, m:]).any() for a in got)
    pk = FA.run_both(codec, FA.to_dev(s["packed"]), to_dev(s["row_off"]), n, R, 1, True, to_dev(s["w_packed"]), clamp=C)
    _check(pk, s["ref_packed"], "lattice atom14, packed")
    # the order of the sums is the chain's alone: padded and packed agree on bytes
    _all_same(got, pk, "padded against packed", lambda a: AN.pack1(a, s["lens"]))
    # the host-pointer forms through Codec: the bytes of the device forms
    _codec_forms(codec, s["inp"], s["w"], got, dict(length=s["lens"]), "padded")
    _codec_forms(codec, s["packed"], s["w_packed"], pk, dict(row_off=s["row_off"]), "packed")
    # swapped set on rows whose type has no swap (and cleared there): the same bytes; no swapped at all: other bytes
    inp = s["inp"]
    none = ~np.isin(inp["aatype"], (FA.ASP, FA.GLU, FA.PHE, FA.TYR))
    assert ((inp["swapped"] != 0) & none).any() and ((inp["swapped"] != 0) & ~none).any()
    for sw, what in ((np.where(none, 0, inp["swapped"]).astype(np.uint8), "cleared"), (np.where(none, 1, inp["swapped"]).astype(np.uint8), "set")):
        other = FA.run_both(codec, FA.to_dev(dict(inp, swapped=sw)), to_dev(s["lens"]), n, L, 1, False, to_dev(s["w"]), clamp=C)
        _all_same(got, other, f"swapped {what} where the type has no swap")
    plain = FA.run_both(codec, FA.to_dev(dict(inp, swapped=None)), to_dev(s["lens"]), n, L, 1, False, to_dev(s["w"]), clamp=C)
    _check(plain, FA.ref_padded(dict(inp, swapped=None), s["lens"], s["w"], C), "lattice atom14, no swapped")
    assert not np.array_equal(plain[0], got[0]) and not np.array_equal(plain[2], got[2]) and not np.array_equal(plain[4], got[4])
    # without aatype (and so without swapped) every row is of type 20
    bare = FA.run_both(codec, FA.to_dev(dict(inp, swapped=None, aatype=None)), to_dev(s["lens"]), n, L, 1, False, to_dev(s["w"]), clamp=C)
    _all_same(plain, bare, "no aatype")


def test_backbone4_passes_at_their_fullest(codec):
    """every mask set in backbone4: a chain whose points fill a pass to its last slot, one with a slot less, one of more than two
    passes; groups 0 and 3 alone are frames whatever the masks say"""
    P = codec.lib.fcz_fape_atoms_pass()
    b = FA.backbone_batch(P)
    ref = FA.ref_padded(b["inp"], b["lens"], b["w"], C)
    assert FA.tie_share(ref) == 0 and [int(ref["points"][e].max()) for e in range(3)] == [P, P - 1, 2 * P + 12]
    n, L = 3, b["L"]
    got = FA.run_both(codec, FA.to_dev(b["inp"]), to_dev(b["lens"]), n, L, 2, False, to_dev(b["w"]), clamp=C)
    _check(got, ref, "lattice backbone4, every mask set")
    assert (got[1][..., [0, 3]][ref["frame"][..., [0, 3]]] > 0).all() and not got[1][..., [1, 2, 4, 5, 6, 7]].any()
    lens = b["lens"]
    pk = FA.run_both(codec, FA.to_dev(FA.pack_inp(b["inp"], lens)), to_dev(AN.row_off_of(lens)), n, int(lens.sum()), 2, True, to_dev(AN.pack1(b["w"], lens)), clamp=C)
    _all_same(got, pk, "backbone4 packed", lambda a: AN.pack1(a, lens))


def test_atom37_lattice(codec):
    lens = np.asarray([0, 3, 21, 58], np.uint32)                              # 58 rows with every mask set: 2146 points, three passes
    L = 58
    inp = FA.lattice(lens, L, 37, 61, full=(3,))
    w = FA.weights((4, L, FA.GROUPS), 62)
    ref = FA.ref_padded(inp, lens, w, C)
    assert FA.tie_share(ref) == 0 and ref["points"].max() == 58 * 37
    got = FA.run_both(codec, FA.to_dev(inp), to_dev(lens), 4, L, 0, False, to_dev(w), clamp=C)
    _check(got, ref, "lattice atom37")
    # a swap table of the caller's: GLY's N and CA exchanged as well (nothing chemical, a table is a table)
    table = FA.tables(37)[0].copy()
    table[7, [0, 1]] = [1, 0]
    tref = FA.ref_padded(inp, lens, w, C, table=table, alt=FA.tables(37)[1])
    tgot = FA.run_both(codec, FA.to_dev(inp), to_dev(lens), 4, L, 0, False, to_dev(w), clamp=C, table=table)
    _check(tgot, tref, "lattice atom37, own table")
    assert not np.array_equal(tgot[0], got[0])


@pytest.fixture(scope="module")
def noisy():
    """the noisy atom14 batch of 33, 65 and 128 residues, no masks of the prediction, random weights, and the restatement"""
    b = FA.noisy_batch()
    b["ref"] = FA.ref_padded(b["inp"], b["lens"], b["w"], 10.0)
    assert FA.tie_share(b["ref"]) <= FA.TIE_SHARE
    b["dev"] = FA.to_dev(b["inp"])
    return b


def test_noisy_batch(codec, noisy):
    b = noisy
    n, L = len(b["lens"]), b["L"]
    lens_t, w = to_dev(b["lens"]), to_dev(b["w"])
    got = FA.run_both(codec, b["dev"], lens_t, n, L, 1, False, w)
    _check(got, b["ref"], "noisy, atom14, clamp 10")
    assert (got[1] > 0).sum() > 700 and np.abs(got[4]).max() > 0.01 and 0 < b["ref"]["clamped"].sum() < b["ref"]["terms"].sum()
    free = FA.ref_padded(b["inp"], b["lens"], b["w"], float("inf"))
    assert FA.tie_share(free) == 0 and free["sum"].sum() > b["ref"]["sum"].sum() * 1.01 and np.abs(free["grad_pos"] - b["ref"]["grad_pos"]).max() > 0.1
    _check(FA.run_both(codec, b["dev"], lens_t, n, L, 1, False, w, clamp=float("inf")), free, "noisy, unclamped")
    other = FA.ref_padded(b["inp"], b["lens"], b["w"], 10.0, 0.25)
    assert FA.tie_share(other) <= FA.TIE_SHARE and other["sum"].sum() > b["ref"]["sum"].sum()
    _check(FA.run_both(codec, b["dev"], lens_t, n, L, 1, False, w, eps=0.25), other, "noisy, eps 0.25")


def test_determinism_on_bytes(codec, noisy):
    b = noisy
    n, L = len(b["lens"]), b["L"]
    inp, lens = b["inp"], b["lens"]
    w = to_dev(b["w"])
    first = FA.run_both(codec, b["dev"], to_dev(lens), n, L, 1, False, w)
    again = FA.run_both(codec, b["dev"], to_dev(lens), n, L, 1, False, w, guard=4)          # (and outputs that are not 16-byte aligned)
    _all_same(first, again, "two calls")
    # a chain alone, and the batch permuted: the bytes of the chain inside the batch
    cut = lambda idx: {k: None if v is None else v[idx] for k, v in inp.items()}
    for e in range(n):
        alone = FA.run_both(codec, FA.to_dev(cut(slice(e, e + 1))), to_dev(lens[e:e + 1]), 1, L, 1, False, to_dev(b["w"][e:e + 1]))
        _all_same(first, alone, f"chain {e} alone", lambda a: a[e:e + 1])
    perm = np.asarray([2, 0, 1])
    moved = FA.run_both(codec, FA.to_dev(cut(perm)), to_dev(lens[perm]), n, L, 1, False, to_dev(b["w"][perm]))
    _all_same(first, moved, "permuted batch", lambda a: a[perm])
    # packed against padded
    pk = FA.run_both(codec, FA.to_dev(FA.pack_inp(inp, lens)), to_dev(AN.row_off_of(lens)), n, int(lens.sum()), 1, True, to_dev(AN.pack1(b["w"], lens)))
    _all_same(first, pk, "packed", lambda a: AN.pack1(a, lens))


def test_length_null_and_clamped(codec):
    lens = [40, 130, 65]
    L = 130
    inp = FA.lattice([L] * 3, L, 14, 12, behind="data")                       # finite rows behind every length below
    w = FA.weights((3, L, FA.GROUPS), 13)
    dev, wd = FA.to_dev(inp), to_dev(w)
    whole = FA.ref_padded(inp, None, w, C)
    got = FA.run_both(codec, dev, None, 3, L, 1, False, wd, clamp=C)
    _check(got, whole, "length NULL")
    over = FA.run_both(codec, dev, to_dev(np.asarray([L + 1, 65535, 0xFFFFFFFF], np.uint32)), 3, L, 1, False, wd, clamp=C)
    _all_same(got, over, "length > L")
    ref = FA.ref_padded(inp, lens, w, C)
    assert ref["points"].sum() < whole["points"].sum()
    _check(FA.run_both(codec, dev, to_dev(np.asarray(lens, np.uint32)), 3, L, 1, False, wd, clamp=C), ref, "length < L")
    # no chain at all: FCZ_OK, and there is no row to write
    gv, gg = DevGuarded(FA.value_spec((L,))), DevGuarded(FA.grad_spec((L,), 14))
    ptrs = [AN.ptr(t) for t in dev]
    assert codec.lib.fcz_fape_atoms_dev(codec.ctx, *ptrs, None, 0, L, 1, 10.0, 1e-4, None, *gv.ptrs()) == 0
    assert codec.lib.fcz_fape_atoms_grad_dev(codec.ctx, *ptrs, None, 0, L, 1, 10.0, 1e-4, None, wd.data_ptr(), *gg.ptrs()) == 0
    codec.synchronize()
    assert gv.untouched() and gg.untouched()


def test_hostile_row_off(codec):
    R = 700
    inp = {k: v[0] for k, v in FA.lattice([R], R, 4, 13).items()}
    w = FA.weights((R, FA.GROUPS), 14)
    dev, wd = FA.to_dev(inp), to_dev(w)
    row_off = AN.HOSTILE_ROW_OFF
    ref = FA.ref_packed(inp, row_off, w, C)
    got = FA.run_both(codec, dev, to_dev(row_off), 5, R, 2, True, wd, clamp=C)
    _check(got, ref, "hostile row_off")
    assert all(not AN.bits(a[:40]).any() for a in got) and (got[1][40:120] > 0).sum() > 40 and (got[1][401:] > 0).sum() > 200
    # no chain at all: every row is uncovered and filled
    none = FA.run_both(codec, dev, to_dev(row_off), 0, R, 2, True, wd, clamp=C)
    assert all(not AN.bits(a).any() for a in none)
    # the host-pointer forms on the same host arrays, their outputs between guard bytes: what the device forms gave
    hp = [host_ptr(inp[k]) for k in FA.ORDER]
    for n, dev_form in ((5, got), (0, none)):
        h = HostGuarded(FA.value_spec((R,)))
        assert codec.lib.fcz_fape_atoms_packed(codec.ctx, *hp, host_ptr(row_off), n, R, 2, C, 1e-4, None, *h.ptrs()) == 0
        for a, c in zip(h.all(), dev_form[:2]):
            _same_bytes(a, c, f"fcz_fape_atoms_packed n={n}")
        h = HostGuarded(FA.grad_spec((R,), 4))
        assert codec.lib.fcz_fape_atoms_grad_packed(codec.ctx, *hp, host_ptr(row_off), n, R, 2, C, 1e-4, None, host_ptr(w), *h.ptrs()) == 0
        for a, c in zip(h.all(), dev_form[2:]):
            _same_bytes(a, c, f"fcz_fape_atoms_grad_packed n={n}")


def test_refusals_leave_the_outputs_untouched(codec):
    import torch
    n, L, A = 2, 8, 14
    pos, mask, aa, off = AN.refusal_inputs(n, L, A)
    rot = torch.eye(3, dtype=torch.float32, device="cuda:0").repeat(n, L, 8, 1, 1).contiguous()
    trans = torch.zeros((n, L, 8, 3), dtype=torch.float32, device="cuda:0")
    fm = torch.ones((n, L, 8), dtype=torch.uint8, device="cuda:0")
    wt = torch.zeros((n, L, 8), dtype=torch.float32, device="cuda:0")
    gv, gg = DevGuarded(FA.value_spec((n * L,))), DevGuarded(FA.grad_spec((n * L,), A))
    bad_table = np.tile(np.arange(A, dtype=np.uint8), (21, 1))
    bad_table[3, 6] = 7
    lib, ctx, O = codec.lib, codec.ctx, off.data_ptr()
    torch.cuda.synchronize()
    for padded_fn, packed_fn, outs in ((lib.fcz_fape_atoms_dev, lib.fcz_fape_atoms_packed_dev, gv.ptrs()),
                                       (lib.fcz_fape_atoms_grad_dev, lib.fcz_fape_atoms_grad_packed_dev, [wt.data_ptr()] + gg.ptrs())):
        ok = dict(ctx=ctx, rt=rot.data_ptr(), tt=trans.data_ptr(), ft=fm.data_ptr(), pt=pos.data_ptr(), mt=mask.data_ptr(), aa=aa.data_ptr(), sw=aa.data_ptr(),
                  rp=rot.data_ptr(), tp=trans.data_ptr(), fp=fm.data_ptr(), pp=pos.data_ptr(), mp=mask.data_ptr(), bound=None, n=n, L=L, layout=1, clamp=10.0, eps=1e-4,
                  table=None)
        ok.update({f"o{i}": o for i, o in enumerate(outs)})
        bad = [dict(ctx=None)] + [{k: None} for k in ("rt", "tt", "ft", "pt", "mt", "aa", "rp", "tp", "pp")] + [{f"o{i}": None} for i in range(len(outs))]
        bad += [dict(layout=3), dict(layout=-1), dict(clamp=0.0), dict(clamp=-1.0), dict(clamp=float("nan")), dict(eps=0.0), dict(eps=-1.0), dict(eps=float("nan")),
                dict(eps=float("inf")), dict(table=bad_table.ctypes.data), dict(L=2 ** 29 + 1), dict(layout=0, L=(2 ** 31 - 1) // 37 + 1), dict(L=0)]
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

KEYS = {"fape_frame", "fape_points", "frame_mask", "swapped", "fape_chain", "loss"}


def _loss_weights(ref, chains, scale):
    """the item weights of loss = mean over the chains with a term of sum / (points summed over the frames * scale) -> (w, the loss)"""
    w = np.zeros(ref["sum"].shape)
    sums = [(idx, float(ref["sum"][idx].sum()), int(ref["points"][idx].sum())) for idx in chains]
    scored = [s for s in sums if s[2] > 0]
    for idx, _, pts in scored:
        w[idx] = 1.0 / (len(scored) * pts * scale)
    return w, float(np.mean([total / (pts * scale) for _, total, pts in scored])) if scored else 0.0


def _check_values(out, ref0, loss, scale, what):
    import torch
    assert set(out) == KEYS, what
    assert out["fape_frame"].dtype == torch.float32 and out["fape_points"].dtype == torch.int32 and out["frame_mask"].dtype == torch.bool
    assert out["swapped"].dtype == torch.bool and out["swapped"].shape == ref0["sum"].shape[:-1]
    assert out["fape_chain"].dtype == torch.float32 and out["loss"].dtype == torch.float32 and out["loss"].shape == () and out["fape_frame"].shape == ref0["sum"].shape
    pts = out["fape_points"].cpu().numpy()
    assert np.array_equal(pts, ref0["points"]) and np.array_equal(out["frame_mask"].cpu().numpy(), ref0["frame"]), what
    per = out["fape_frame"].detach().cpu().numpy().astype(np.float64)
    exp = np.where(pts > 0, ref0["sum"] / (np.maximum(pts, 1) * scale), 0.0)
    bound = np.where(pts > 0, ref0["b_sum"] / (np.maximum(pts, 1) * scale), 0.0) + 2.0 ** -22 * exp + 2.0 ** -40           # (two float32 operations behind sum)
    assert (np.abs(per - exp) <= bound).all() and not per[pts == 0].any(), what
    assert abs(float(out["loss"].detach()) - loss) <= float(bound.max()) + 2.0 ** -23 * loss, (what, float(out["loss"].detach()), loss)


def _records(codec, golden, count=4):
    import foldcomp_amd as foldcomp
    records = golden_records_raw(golden)[1]
    lens_all = foldcomp.decode_tensors(records, codec=codec, max_len=8)["length"].cpu().numpy()
    pick = [int(i) for i in np.flatnonzero(lens_all >= 80)[:count]]
    assert len(pick) == count
    return [records[i] for i in pick]


def _truth_inputs(t, lens, pred_frames, pred_h, swapped):
    """the restatement's dict for a decoded atom14 batch `t` (padded), the truth's frames restated by tests/_frames.py to the bit"""
    pos_h, mask, aa = t["pos"].cpu().numpy(), t["mask"].cpu().numpy().view(np.uint8), t["aatype"].cpu().numpy()
    rt, tt, ft = FRM.frames(pos_h, mask, aa, lens, 1, 1)
    rp, tp, fp = pred_frames
    return dict(rot_t=rt, trans_t=tt, fm_t=ft, pos_t=pos_h, mask_t=mask, aatype=aa, swapped=swapped, rot_p=rp, trans_p=tp, fm_p=fp, pos_p=pred_h, mask_p=mask)


def _builder_jacobian(pred_h, aa, frame):
    """J [n, L, 8]: no entry of a group's rot moves by more than J per Angstrom an atom moves (test_gpu_fape.py derives it for the
    backbone group; the other groups are the same construction on their own three atoms): 1 / n1 + 1 / n2 + 2 |v2| / (n1 n2)"""
    tab = FRM.slot_table(1)[np.minimum(aa.astype(np.int64), 20)]              # [n, L, 8, 3]
    idx = np.maximum(tab, 0)
    p64 = pred_h.astype(np.float64)
    a0, a1, a2 = (np.take_along_axis(p64, idx[..., j, None], axis=-2) for j in range(3))
    v1, v2 = a1 - a0, a2 - a1
    with np.errstate(all="ignore"):
        n1 = np.linalg.norm(v1, axis=-1)
        n2 = np.linalg.norm(v2 - v1 * ((v1 * v2).sum(-1) / n1 ** 2)[..., None], axis=-1)
        return np.where(frame, 1 / n1 + 1 / n2 + 2 * np.linalg.norm(v2, axis=-1) / (n1 * n2), 0.0)


def test_foldcomp_fape_atoms_frames_from_coordinates(codec, golden):
    """padded, pred a pos tensor: the eight groups built in torch in front of the kernel, autograd carries the gradient on to pos"""
    import torch
    import foldcomp_amd as foldcomp
    from foldcomp_amd import tensors
    recs = _records(codec, golden)
    n = len(recs)
    rng = np.random.default_rng(47)
    t = foldcomp.decode_tensors(recs, codec=codec, max_len=64, layout="atom14")
    L = t["pos"].shape[1]
    pos_h = t["pos"].cpu().numpy()
    lens = np.minimum(t["length"].cpu().numpy().astype(np.int64), L)
    pred_h = (pos_h + (rng.standard_normal(pos_h.shape) * 0.3).astype(F)).astype(F)
    pred = torch.from_numpy(pred_h).to("cuda:0").requires_grad_()
    out = foldcomp.fape_atoms(dict(pos=pred, mask=t["mask"]), t, codec=codec)
    assert out["loss"].grad_fn is not None and out["fape_frame"].grad_fn is not None and out["fape_chain"].shape == (n,)
    out["loss"].backward()
    with torch.no_grad():
        frames_p = tuple(v.cpu().numpy() for v in tensors.rigid_frames_torch(pred.detach(), t["mask"], t["aatype"]))
    sw = out["swapped"].cpu().numpy()
    inp = _truth_inputs(t, lens, (frames_p[0], frames_p[1], frames_p[2].view(np.uint8)), pred_h, sw.view(np.uint8))
    ref0 = FA.ref_padded(inp, lens)
    w, loss = _loss_weights(ref0, [(e, slice(0, L)) for e in range(n)], 10.0)
    refw = FA.ref_padded(inp, lens, w)
    assert FA.tie_share(refw) <= FA.TIE_SHARE and ref0["frame"].sum() > 3 * lens.sum() and ref0["point"].sum() > 6 * lens.sum()
    _check_values(out, ref0, loss, 10.0, "fape_atoms, padded, frames from coordinates")
    chain = out["fape_chain"].detach().cpu().numpy()
    assert 0.0 < chain.min() and chain.max() <= 1.0 and abs(float(out["loss"].detach()) - chain.astype(np.float64).mean()) < 1e-6
    # the renaming inside the call is lddt_atoms'; a decision handed over gives the same bytes
    la = foldcomp.lddt_atoms(dict(pos=pred.detach(), mask=t["mask"]), t, codec=codec)["swapped"]
    assert AN.teq(la.view(torch.uint8), out["swapped"].view(torch.uint8))
    with torch.no_grad():
        handed = foldcomp.fape_atoms(dict(pos=pred, mask=t["mask"]), t, rename=la, codec=codec)
    assert all(AN.teq(handed[k], out[k].detach()) for k in out)
    # pos.grad: the restatement's three gradients carried through the builder in float64 on the host; the kernel's error reaches a
    # coordinate through every group of its row (nine entries of rot each, moved by at most J per Angstrom: _builder_jacobian) and as
    # its own grad_pos. The float32 builder and its float32 backward add a few 2^-24 relative to each partial sum: 2^-16 max(J, 1) of
    # their absolute sum is allowed, as in test_gpu_fape.py.
    p64 = torch.tensor(pred_h.astype(np.float64), requires_grad=True)
    r64, t64, _ = tensors.rigid_frames_torch(p64, t["mask"].cpu(), t["aatype"].cpu())
    ((r64 * torch.tensor(refw["grad_rot"])).sum() + (t64 * torch.tensor(refw["grad_trans"])).sum()).backward()
    exp = p64.grad.numpy() + refw["grad_pos"]
    g = pred.grad.cpu().numpy()
    J = _builder_jacobian(pred_h, inp["aatype"], refw["frame"])
    scale_row = np.abs(refw["grad_rot"]).sum(axis=(-1, -2, -3)) + np.abs(refw["grad_trans"]).sum(axis=(-1, -2)) + np.abs(refw["grad_pos"]).sum(axis=(-1, -2))
    bound = (9.0 * J * refw["b_rot"] + refw["b_trans"]).sum(axis=-1) + refw["b_pos"].max(axis=-1) + 2.0 ** -16 * np.maximum(J.max(axis=-1), 1.0) * scale_row
    err = np.abs(g.astype(np.float64) - exp).max(axis=(-1, -2))
    ratio = float((err[bound > 0] / bound[bound > 0]).max())
    print(f"fape_atoms, padded, frames from coordinates: pos.grad, largest |error| / bound = {ratio:.4f}; tie share {FA.tie_share(refw):.4f}")
    assert (err <= bound).all() and np.abs(g).max() > 1e-5, (np.argwhere(err > bound)[:4], ratio)
    for e, m in enumerate(lens):
        assert not AN.bits(g[e, m:]).any()
    # the graph is walked once
    with pytest.raises(RuntimeError):
        out["loss"].backward()
    # no_grad, and a pos that needs no gradient: tensors without a graph, the same values
    with torch.no_grad():
        plain = foldcomp.fape_atoms(dict(pos=pred, mask=t["mask"]), t, codec=codec)
    still = foldcomp.fape_atoms(dict(pos=pred.detach(), mask=t["mask"]), t, codec=codec)
    for o in (plain, still):
        assert all(v.grad_fn is None and not v.requires_grad for v in o.values())
        assert all(AN.teq(o[k], out[k].detach()) for k in out)
    # the truth's frames from the dict, when it carries the eight-group ones: the same bytes
    tf = foldcomp.decode_tensors(recs, codec=codec, max_len=64, layout="atom14", frames="all")
    again = foldcomp.fape_atoms(dict(pos=pred.detach(), mask=t["mask"]), tf, codec=codec)
    assert all(AN.teq(again[k], out[k].detach()) for k in out)
    # nothing to score, a layout mismatch, a truth without aatype, a CPU tensor
    e = foldcomp.fape_atoms(torch.zeros((0, 8, 14, 3), device="cuda:0", requires_grad=True), foldcomp.decode_tensors([], codec=codec, max_len=8, layout="atom14"), codec=codec)
    assert e["fape_frame"].shape == (0, 8, 8) and e["fape_chain"].shape == (0,) and e["swapped"].shape == (0, 8) and float(e["loss"].detach()) == 0.0
    with pytest.raises(ValueError):
        foldcomp.fape_atoms(pred[:, :, :4].contiguous(), t, codec=codec)
    with pytest.raises(ValueError):
        foldcomp.fape_atoms(pred.detach(), dict(pos=t["pos"], mask=t["mask"]), rename=None, codec=codec)
    with pytest.raises(foldcomp.error):
        foldcomp.fape_atoms(pred.cpu(), t, codec=codec)


def test_foldcomp_fape_atoms_model_frames(codec, golden):
    """packed, the model's own eight-group frames beside its pos: rot.grad, trans.grad and pos.grad; then a window"""
    import torch
    import foldcomp_amd as foldcomp
    recs = _records(codec, golden)
    n = len(recs)
    rng = np.random.default_rng(53)
    t = foldcomp.decode_tensors(recs, codec=codec, max_len=64, layout="atom14", frames="all")
    tl = [min(int(m), 64) for m in t["length"].cpu().numpy()]
    tl[1] = 37                                                                # (chains of different lengths in the packed form)
    p = {k: torch.cat([t[k][e, :m] for e, m in enumerate(tl)]).contiguous() for k in ("pos", "mask", "aatype", "rot", "trans", "frame_mask")}
    p["cu_seqlens"] = torch.from_numpy(AN.row_off_of(tl).astype(np.int32)).to("cuda:0")
    cu = p["cu_seqlens"].cpu().numpy()
    R = int(cu[-1])
    rot_t, trans_t, fm_t = p["rot"].cpu().numpy(), p["trans"].cpu().numpy(), p["frame_mask"].cpu().numpy().view(np.uint8)
    pos_h, mask, aa = p["pos"].cpu().numpy(), p["mask"].cpu().numpy().view(np.uint8), p["aatype"].cpu().numpy()
    rot_h = (FP.small_rotations(rng, (R, 8), 0.15) @ rot_t.astype(np.float64)).astype(F)
    trans_h = (trans_t + (rng.standard_normal((R, 8, 3)) * 0.5).astype(F)).astype(F)
    pred_h = (pos_h + (rng.standard_normal(pos_h.shape) * 0.5).astype(F)).astype(F)
    leaves = [torch.from_numpy(a).to("cuda:0").requires_grad_() for a in (rot_h, trans_h, pred_h)]
    out = foldcomp.fape_atoms(dict(rot=leaves[0], trans=leaves[1], pos=leaves[2]), p, codec=codec)
    out["loss"].backward()
    sw = out["swapped"].cpu().numpy().view(np.uint8)
    inp = dict(rot_t=rot_t, trans_t=trans_t, fm_t=fm_t, pos_t=pos_h, mask_t=mask, aatype=aa, swapped=sw, rot_p=rot_h, trans_p=trans_h, fm_p=None, pos_p=pred_h, mask_p=None)
    ref0 = FA.ref_packed(inp, cu)
    w, loss = _loss_weights(ref0, [slice(int(cu[e]), int(cu[e + 1])) for e in range(n)], 10.0)
    refw = FA.ref_packed(inp, cu, w)
    assert FA.tie_share(refw) <= FA.TIE_SHARE and out["fape_frame"].shape == (R, 8) and out["fape_chain"].shape == (n,)
    _check_values(out, ref0, loss, 10.0, "fape_atoms, packed, model frames")
    FA.check_grad(tuple(v.grad.cpu().numpy() for v in leaves), refw, "fape_atoms, packed, model frames")
    assert all(np.abs(v.grad.cpu().numpy()).max() > 1e-6 for v in leaves)

    # a window: crop_start in the dict, length is not used; a frame mask of the model's, unclamped, no renaming
    wt = foldcomp.decode_tensors(recs, codec=codec, max_len=48, crop="center", layout="atom14", frames="all")
    wpos_h = wt["pos"].cpu().numpy()
    wpred_h = (wpos_h + (rng.standard_normal(wpos_h.shape) * 0.5).astype(F)).astype(F)
    wrot_t, wtrans_t = wt["rot"].cpu().numpy(), wt["trans"].cpu().numpy()
    wrot_h = (FP.small_rotations(rng, wrot_t.shape[:3], 0.15) @ wrot_t.astype(np.float64)).astype(F)
    wtrans_h = (wtrans_t + (rng.standard_normal(wtrans_t.shape) * 0.5).astype(F)).astype(F)
    wfm_h = (rng.random(wrot_t.shape[:3]) > 0.1)
    leaves = [torch.from_numpy(a).to("cuda:0").requires_grad_() for a in (wrot_h, wtrans_h, wpred_h)]
    wo = foldcomp.fape_atoms(dict(rot=leaves[0], trans=leaves[1], pos=leaves[2], frame_mask=torch.from_numpy(wfm_h).to("cuda:0")), wt, clamp=None, rename=None, codec=codec)
    wo["loss"].backward()
    winp = dict(rot_t=wrot_t, trans_t=wtrans_t, fm_t=wt["frame_mask"].cpu().numpy().view(np.uint8), pos_t=wpos_h, mask_t=wt["mask"].cpu().numpy().view(np.uint8),
                aatype=wt["aatype"].cpu().numpy(), swapped=None, rot_p=wrot_h, trans_p=wtrans_h, fm_p=wfm_h.view(np.uint8), pos_p=wpred_h, mask_p=None)
    wref0 = FA.ref_padded(winp, None, None, float("inf"))
    w, loss = _loss_weights(wref0, [(e, slice(0, 48)) for e in range(n)], 10.0)
    wrefw = FA.ref_padded(winp, None, w, float("inf"))
    _check_values(wo, wref0, loss, 10.0, "fape_atoms, window")
    assert not wo["swapped"].any()
    FA.check_grad(tuple(v.grad.cpu().numpy() for v in leaves), wrefw, "fape_atoms, window")


def test_renaming_a_flipped_ring(codec, golden):
    """a prediction that IS the truth with every PHE / TYR ring and ASP / GLU carboxylate named the other way round: renamed, the loss
    is (nearly) nothing; with rename=None the flipped atoms and the turned frames are punished"""
    import torch
    import foldcomp_amd as foldcomp
    recs = _records(codec, golden, 6)
    t = foldcomp.decode_tensors(recs, codec=codec, max_len=64, layout="atom14", frames="all")
    aa = t["aatype"].cpu().numpy()
    table = FA.tables(14)[0]
    flip = np.isin(aa, (FA.ASP, FA.GLU, FA.PHE, FA.TYR))
    pred_h = np.ascontiguousarray(LA.exchange(t["pos"].cpu().numpy(), aa, flip, table))
    pmask = torch.from_numpy(np.ascontiguousarray(LA.exchange(t["mask"].cpu().numpy()[..., None], aa, flip, table)[..., 0])).to("cuda:0")
    pred = dict(pos=torch.from_numpy(pred_h).to("cuda:0"), mask=pmask)
    renamed = foldcomp.fape_atoms(pred, t, codec=codec)
    plain = foldcomp.fape_atoms(pred, t, rename=None, codec=codec)
    by_hand = foldcomp.fape_atoms(pred, t, rename=renamed["swapped"], codec=codec)
    assert all(AN.teq(by_hand[k], renamed[k]) for k in renamed)
    sw = renamed["swapped"].cpu().numpy()
    assert sw.sum() >= 5 and not (sw & ~flip).any() and not plain["swapped"].any()
    a, b = float(renamed["loss"]), float(plain["loss"])
    print(f"flipped rings: {int(flip.sum())} rows flipped, {int(sw.sum())} renamed; loss renamed {a:.6f}, not renamed {b:.6f}")
    assert b > a + 0.005 and b > 2 * a


def test_gradient_descent_lowers_the_loss(codec, golden):
    """the sign end to end: six steps of plain gradient descent on the coordinates, every one of which must lower the loss"""
    import torch
    import foldcomp_amd as foldcomp
    recs = _records(codec, golden)
    t = foldcomp.decode_tensors(recs, codec=codec, max_len=64, crop="center", layout="atom14")
    gen = torch.Generator(device="cuda:0"); gen.manual_seed(59)
    pred = (t["pos"] + 0.3 * torch.randn(t["pos"].shape, device="cuda:0", generator=gen)).requires_grad_()
    sw = foldcomp.lddt_atoms(dict(pos=pred.detach(), mask=t["mask"]), t, codec=codec)["swapped"]      # one decision for the whole descent
    losses, rate = [], None
    for step in range(7):
        out = foldcomp.fape_atoms(dict(pos=pred, mask=t["mask"]), t, rename=sw, codec=codec)
        losses.append(float(out["loss"].detach()))
        if step == 6:
            break
        out["loss"].backward()
        if rate is None:
            rate = 0.1 / float(pred.grad.abs().max())                         # the first step moves no atom by more than 0.1 A
        pred = (pred.detach() - rate * pred.grad).requires_grad_()
    print("gradient descent on the all-atom FAPE, 4 chains of 64 rows: loss " + " -> ".join(f"{v:.5f}" for v in losses))
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
