"""GPU: the violation loss and its gradient (fcz_violation_loss_dev, fcz_violation_loss_grad_dev, their packed and host forms,
Codec.violation_loss / violation_loss_grad, foldcomp.violation_loss) against the numpy restatement of the contract
(tests/_violation_loss.py). Value and gradient are compared ON BITS; the device calls write into arrays pre-filled with 0xA5 with guard
bytes on both sides. The batch is the shape family of tests/test_gpu_violations.py with the pass of this kernel."""
import numpy as np
import pytest

import _analysis as AN
import _violation_loss as VL
import _violations as V
import test_gpu_violations as TV
from _analysis import NAN_BITS
from _devpath import HostGuarded, host_ptr, to_dev
from foldcomp_amd import _lib

pytestmark = pytest.mark.gpu

F = np.float32
TABLE, TILE = TV.TABLE, TV.TILE
LAYOUT = {37: 0, 14: 1, 4: 2}
TIGHT, DEFAULT = (F(0), F(0.5)), (V.TOL, V.FACTOR)
E = 8                                                                         # the chain of the planted cases


def _nan_where(w, dead):
    w = w.copy()
    w.view(np.uint32)[dead] = NAN_BITS
    return w


@pytest.fixture(scope="module", params=[37, 14, 4])
def batch(request):
    """chains of 0, 1, 2, 3 rows, of one query tile and one row less and more, a chain with every mask set whose atoms exceed the pass
    by one row, and two hostile chains (NaN, +-inf, 3e19 under set masks, NaN patterns under cleared masks and behind the length, aatype
    0 .. 24 and 255). Planted: in the long chain an atom of the last row next to one of the first (a pair across two passes and two
    tiles); in chain 8 two lone CA at exactly d == T of the tight run and two at d == T of the default run (no pair: d2 < T * T is
    strict), two coincident CA (d == 0: a value, no direction), a stretched link, a bent link, two PRO links and a link whose C
    coincides with N' (length 0, both cosines not finite). The weights hold NaN patterns where no atom and no link can be.
    The restatements are computed once per configuration and shared.
    The long chain's first pass closes at 1024 (backbone4), 1008 (atom14) and 936 (atom37) atoms: with every mask set the rule that
    closes a pass is crossed on a whole staging step. The pass at its fullest (1280, 1280, 1267), one slot under it, and a clash
    partner at its last place live in the fuzz (tests/_analysis_fuzz.py, the design group of violation_loss)."""
    A = request.param
    Q = _lib.load().fcz_violation_loss_pass()
    T = TILE[A]
    per_row = {37: 36, 14: 14, 4: 4}[A]
    big = Q // per_row + 1
    lens = [0, 1, 2, 3, T - 1, T, T + 1, big, 60, 130 if A != 37 else 50]
    pos, mask, aa = TV._synthetic(lens, A, 61 + A, full=(7,))
    if A == 14:
        aa[7, :big] = 17                                                      # TRP owns all 14 slots
    pos[7, big - 1, 1] = pos[7, 0, 1] + np.asarray([0.25, 0, 0], F)
    e = E
    lone = [3, 5, 7, 9, 11, 14]                                               # rows that keep their CA only
    mask[e, lone] = 0
    mask[e, lone, 1] = 1
    t_tight, t_default = F(1.7) + F(1.7), (F(1.7) + F(1.7)) - V.TOL
    pos[e, 3, 1], pos[e, 5, 1] = [0, 200, 200], [t_tight, 200, 200]            # (from 0 the difference is the coordinate itself)
    pos[e, 7, 1], pos[e, 9, 1] = [200, 0, 200], [200, t_default, 200]
    pos[e, 11, 1] = pos[e, 14, 1] = [300, 300, 300]
    pos[e, 20:lens[e]] += np.asarray([0.9, 0.3, -0.2], F)                     # link 19 stretched
    pos[e, 30, 1] = pos[e, 30, 0] + (pos[e, 29, 2] - pos[e, 30, 0]) * F(0.9) + F(0.3)   # link 29 bent at N'
    pos[e, 41:44] = AN.helix(np.random.default_rng(3), 3, A) + F(50)          # three clean rows: link 41 has C on N'
    pos[e, 42, 0] = pos[e, 41, 2]
    mask[e, 19:21, :3] = mask[e, 29:31, :3] = mask[e, 41:44, :3] = 1
    aa[e, 25] = aa[e, 26] = V.PRO
    mask[e, 24:27, :3] = 1
    for r in (19, 20, 24, 25, 26, 29, 30):
        assert np.isfinite(pos[e, r, :3]).all(), r
    ln = np.asarray(lens, np.uint32)
    n, L = len(lens), max(lens)
    behind = np.arange(L)[None, :] >= ln[:, None]
    last = np.arange(L)[None, :] + 1 >= ln[:, None]
    w_clash = _nan_where(VL.weights((n, L, A), 5), (mask == 0) | behind[..., None])
    w_link = _nan_where(VL.weights((n, L, 3), 6), np.broadcast_to(last[..., None], (n, L, 3)))
    cache = {}

    def expected(aatype_null=False, table=None, params=TIGHT):
        key = (aatype_null, None if table is None else table.tobytes(), params)
        if key not in cache:
            tab = TABLE[A] if table is None else table
            a = None if aatype_null else aa
            v = VL.loss(pos, mask, a, ln, tab, *params)
            v["grad"] = VL.grad(pos, mask, a, ln, tab, w_clash, w_link, *params)
            for x in v.values():
                x.setflags(write=False)
            cache[key] = v
        return cache[key]

    # the planted cases are what they were planted to be
    tight, default = expected(), expected(params=DEFAULT)
    assert tight["clash_loss"][7, 0, 1] > 0 and tight["clash_loss"][7, big - 1, 1] > 0 and tight["counts"][7, 0] > Q
    assert tight["clash_loss"][e, 3, 1] == 0 and tight["clash_loss"][e, 5, 1] == 0 and tight["clash_loss"][e, 7, 1] > 0       # d == T at tolerance 0
    assert default["clash_loss"][e, 7, 1] == 0 and default["clash_loss"][e, 9, 1] == 0 and default["clash_loss"][e, 5, 1] == 0   # d == T at 1.5
    for v, t in ((tight, t_tight), (default, t_default)):
        assert v["clash_loss"][e, 11, 1] == v["clash_loss"][e, 14, 1] == t and not v["grad"][e, [11, 14], 1].any()          # d == 0
    assert default["link_loss"][e, 19, 0] > 0.5 and default["link_loss"][e, 29, 2] > 0 and tight["link_loss"][e, 24:26].any(axis=1).all()
    assert tight["link_loss"][e, 41].tolist() == [F(V.L0) - F(0.5) * V.SL, 0, 0]                                          # C on N': a value, no gradient of the link
    assert all((tight["link_loss"][..., k] > 0).sum() > 100 for k in range(3)) and (tight["clash_loss"] > 0).sum() > 200
    assert np.isfinite(tight["grad"]).all() and np.isfinite(default["grad"]).all() and np.abs(tight["grad"]).max() > 0.5
    return dict(A=A, layout=LAYOUT[A], lens=ln, L=L, n=n, arrays=(pos, mask, aa), w=(w_clash, w_link), row_off=AN.row_off_of(lens), expected=expected, pass_rows=big)


def _packed(b, v):
    return {k: (x if k == "counts" else AN.pack1(x, b["lens"])) for k, x in v.items()}


def _run(codec, b, arrays, w, bound, n, rows, packed, **kw):
    """value and gradient of one form -> dict(clash_loss, link_loss, counts, grad)"""
    dev = [None if a is None else to_dev(a) for a in arrays]
    out = VL.run_value(codec, *dev, to_dev(bound), n, rows, b["layout"], packed, **kw)
    out["grad"] = VL.run_grad(codec, *dev, to_dev(bound), n, rows, b["layout"], packed, to_dev(w[0]), to_dev(w[1]), **kw)
    return out


@pytest.mark.parametrize("params", [TIGHT, DEFAULT], ids=["tolerance 0, factor 0.5", "defaults"])
def test_value_and_gradient_on_bits(codec, batch, params):
    b = batch
    exp = b["expected"](params=params)
    kw = dict(tol=params[0], factor=params[1])
    got = _run(codec, b, b["arrays"], b["w"], b["lens"], b["n"], b["L"], False, **kw)
    VL.same(got, exp, "padded")
    for e, m in enumerate(b["lens"]):                                         # rows behind the length are exactly 0
        assert not got["clash_loss"][e, m:].view(np.uint32).any() and not got["link_loss"][e, m:].view(np.uint32).any() and not got["grad"][e, m:].view(np.uint32).any()
    again = _run(codec, b, b["arrays"], b["w"], b["lens"], b["n"], b["L"], False, guard=8, **kw)          # two calls, outputs not 16-byte aligned
    VL.same(again, got, "again")
    arrays, w = AN.pack(b["arrays"], b["lens"]), AN.pack(b["w"], b["lens"])
    R = int(b["row_off"][-1])
    gp = _run(codec, b, arrays, w, b["row_off"], b["n"], R, True, guard=8, **kw)
    VL.same(gp, _packed(b, exp), "packed")                                    # padded and packed give the same bytes
    if params is TIGHT:
        # the host-pointer forms against the device forms
        pos, mask, aa = b["arrays"]
        h = codec.violation_loss(pos, mask, aa, length=b["lens"], tolerance=0.0, link_factor=0.5)
        h["grad"] = codec.violation_loss_grad(pos, mask, *b["w"], aatype=aa, length=b["lens"], tolerance=0.0, link_factor=0.5)
        VL.same(h, got, "Codec, padded")
        h = codec.violation_loss(*arrays, row_off=b["row_off"], tolerance=0.0, link_factor=0.5)
        h["grad"] = codec.violation_loss_grad(arrays[0], arrays[1], *w, aatype=arrays[2], row_off=b["row_off"], tolerance=0.0, link_factor=0.5)
        VL.same(h, gp, "Codec, packed")


def test_chain_alone_and_permuted_batch(codec, batch):
    b = batch
    exp = b["expected"]()
    kw = dict(tol=TIGHT[0], factor=TIGHT[1])
    for e in (7, E):
        m = int(b["lens"][e])
        one = _run(codec, b, [a[e:e + 1, :m] for a in b["arrays"]], [w[e:e + 1, :m] for w in b["w"]], b["lens"][e:e + 1], 1, m, False, **kw)
        VL.same(one, {k: (v[e:e + 1] if k == "counts" else v[e:e + 1, :m]) for k, v in exp.items()}, f"chain {e} alone")
    perm = np.asarray([9, 7, 0, 8, 3, 1, 6, 2, 5, 4])
    got = _run(codec, b, [a[perm] for a in b["arrays"]], [w[perm] for w in b["w"]], b["lens"][perm], b["n"], b["L"], False, **kw)
    VL.same(got, {k: v[perm] for k, v in exp.items()}, "permuted")


def test_aatype_null_and_custom_radii(codec, batch):
    """aatype NULL in atom37 and backbone4 (no PRO link, no disulfide, row 0 of the table); a table that zeroes N: N is no clash atom and
    still receives the gradient of its links"""
    b = batch
    pos, mask, aa = b["arrays"]
    kw = dict(tol=TIGHT[0], factor=TIGHT[1])
    if b["A"] != 14:
        exp = b["expected"](aatype_null=True)
        VL.same(_run(codec, b, (pos, mask, None), b["w"], b["lens"], b["n"], b["L"], False, **kw), exp, "aatype NULL")
        assert not np.array_equal(exp["link_loss"][E], b["expected"]()["link_loss"][E])                   # the PRO links differ
    table = TABLE[b["A"]].copy()
    table[:, V.N_SLOT] = 0
    exp = b["expected"](table=table)
    assert not exp["clash_loss"][..., V.N_SLOT].any() and np.abs(exp["grad"][..., V.N_SLOT, :]).max() > 0.1
    got = _run(codec, b, b["arrays"], b["w"], b["lens"], b["n"], b["L"], False, table=table, **kw)
    VL.same(got, exp, "N without a radius")
    arrays, w = AN.pack(b["arrays"], b["lens"]), AN.pack(b["w"], b["lens"])
    VL.same(_run(codec, b, arrays, w, b["row_off"], b["n"], int(b["row_off"][-1]), True, table=table, **kw), _packed(b, exp), "N without a radius, packed")


def test_hostile_row_off(codec):
    R, A = 700, 4
    pos, mask, aa = (a[0] for a in TV._synthetic([R], A, 24))
    pos[350, 1] = pos[130, 1] + np.asarray([0.5, 0, 0], F)                    # a clash inside chain 2 and none with an uncovered row or across chains
    pos[20, 1], pos[60, 1] = pos[500, 1], pos[600, 1]
    mask[[350, 130, 20, 60, 500, 600], 1] = 1
    row_off = AN.HOSTILE_ROW_OFF
    w = VL.weights((R, A), 1), VL.weights((R, 3), 2)
    w[0][:40], w[1][:40] = np.nan, np.nan
    b = dict(layout=2)
    exp = VL.loss(pos, mask, aa, row_off, TABLE[A], packed=True)
    exp["grad"] = VL.grad(pos, mask, aa, row_off, TABLE[A], *w, packed=True)
    assert exp["counts"][0].tolist() == [0, 0] and exp["clash_loss"][350, 1] > 0 and exp["clash_loss"][130, 1] > 0 and not exp["clash_loss"][[20, 60, 500, 600]].any()
    got = _run(codec, b, (pos, mask, aa), w, row_off, 5, R, True, guard=8)
    VL.same(got, exp, "hostile row_off")
    assert all(not got[k][:40].view(np.uint32).any() for k in ("clash_loss", "link_loss", "grad")) and np.abs(got["grad"][40:]).max() > 0
    none = _run(codec, b, (pos, mask, aa), w, row_off, 0, R, True)            # no chain at all: every row is uncovered
    assert all(not none[k].view(np.uint32).any() for k in ("clash_loss", "link_loss", "grad")) and none["counts"].shape == (0, 2)
    # the host form on the same arrays, its outputs between guard bytes
    h = HostGuarded(dict(VL.value_spec((R,), A, 5), grad=(np.float32, (R, A, 3))))
    p = [host_ptr(a) for a in (pos, mask, aa, row_off)]
    assert codec.lib.fcz_violation_loss_packed(codec.ctx, *p, 5, R, 2, None, float(V.TOL), float(V.FACTOR), h.ptr("clash_loss"), h.ptr("link_loss"), h.ptr("counts")) == 0
    assert codec.lib.fcz_violation_loss_grad_packed(codec.ctx, *p, 5, R, 2, None, float(V.TOL), float(V.FACTOR), host_ptr(w[0]), host_ptr(w[1]), h.ptr("grad")) == 0
    VL.same({k: h.fetch(k) for k in got}, got, "host forms")
    # chains without a row (R = 0): their counters are 0 and nothing else has an element
    zeros = np.zeros(4, np.uint32)
    form = VL.run_value(codec, *(to_dev(a[:1]) for a in (pos, mask, aa)), to_dev(zeros), 3, 0, 2, True)
    assert form["counts"].shape == (3, 2) and not form["counts"].any()


def test_refusals_leave_the_outputs_untouched(codec):
    import torch
    from _devpath import DevGuarded
    n, L, A = 2, 8, 37
    pos, mask, aa, off = AN.refusal_inputs(n, L, A)
    o = DevGuarded(dict(VL.value_spec((n * L,), A, n), grad=(np.float32, (n * L, A, 3))))
    wc, wl = torch.ones((n * L, A), dtype=torch.float32, device="cuda:0"), torch.ones((n * L, 3), dtype=torch.float32, device="cuda:0")
    big, nan_tab = TABLE[37].copy(), TABLE[37].copy()
    big[3, 5], nan_tab[20, 0] = 8.0, np.nan
    lib, ctx = codec.lib, codec.ctx

    def call(fn, grad, **kw):
        a = dict(ctx=ctx, pos=pos.data_ptr(), mask=mask.data_ptr(), aa=aa.data_ptr(), bound=None, n=n, rows=L, layout=0, table=None, tol=1.5, factor=12.0,
                 x=wc.data_ptr() if grad else o.ptr("clash_loss"), y=wl.data_ptr() if grad else o.ptr("link_loss"), z=o.ptr("grad") if grad else o.ptr("counts"))
        a.update(kw)
        return fn(a["ctx"], a["pos"], a["mask"], a["aa"], a["bound"], a["n"], a["rows"], a["layout"], a["table"], a["tol"], a["factor"], a["x"], a["y"], a["z"])

    bad = [dict(ctx=None), dict(pos=None), dict(mask=None), dict(x=None), dict(y=None), dict(z=None), dict(layout=3), dict(layout=-1), dict(rows=2 ** 31),
           dict(tol=float("nan")), dict(tol=float("inf")), dict(tol=-0.5), dict(factor=float("nan")), dict(factor=float("inf")), dict(factor=-12.0),
           dict(table=big.ctypes.data), dict(table=nan_tab.ctypes.data), dict(layout=1, aa=None)]
    torch.cuda.synchronize()
    for grad, padded, packed in ((False, lib.fcz_violation_loss_dev, lib.fcz_violation_loss_packed_dev),
                                 (True, lib.fcz_violation_loss_grad_dev, lib.fcz_violation_loss_grad_packed_dev)):
        for k in bad:
            assert call(padded, grad, **k) == -1, (grad, k)
            assert call(packed, grad, **dict(dict(bound=off.data_ptr(), rows=n * L), **k)) == -1, (grad, k)
        assert call(padded, grad, rows=0) == -1                               # L == 0
        assert call(packed, grad, rows=n * L) == -1                           # chains without a row_off
        assert call(padded, grad, n=0) == 0 and call(packed, grad, bound=off.data_ptr(), n=0, rows=0) == 0
    codec.synchronize()
    assert o.untouched()


# ---- Python surface -------------------------------------------------------------------------------------------------------------

def _compose(v, lens=None):
    """what the docstring of foldcomp.violation_loss says, in float64 -> (the four per-chain values and the loss, w_clash, w_link)"""
    atoms, links = v["counts"][:, 0], v["counts"][:, 1]
    n = len(atoms)
    if lens is None:
        rows = [slice(None)] * n
        sums = lambda x: np.asarray([x[e].astype(np.float64).sum() for e in range(n)])
    else:
        off = np.concatenate([[0], np.cumsum(lens)])
        sums = lambda x: np.asarray([x[off[e]:off[e + 1]].astype(np.float64).sum() for e in range(n)])
    per_atom, per_link = np.maximum(atoms, 1).astype(np.float64), np.maximum(links, 1).astype(np.float64)
    clash, bond = sums(v["clash_loss"]) / per_atom, sums(v["link_loss"][..., 0]) / per_link
    angle = sums(v["link_loss"][..., 1]) / per_link + sums(v["link_loss"][..., 2]) / per_link
    chain = clash + bond + angle
    has = atoms > 0
    share = 1.0 / max(int(has.sum()), 1)
    return dict(clash_chain=clash, bond_chain=bond, angle_chain=angle, violation_chain=chain, loss=np.where(has, chain, 0).sum() / max(int(has.sum()), 1)), \
        np.where(has, share / per_atom, 0).astype(F), np.where(has, share / per_link, 0).astype(F)


def test_foldcomp_violation_loss(codec, batch, monkeypatch):
    import torch
    import foldcomp_amd as foldcomp
    b = batch
    pos, mask, aa = b["arrays"]
    n, L, A = b["n"], b["L"], b["A"]
    exp = b["expected"]()
    chains, wc, wl = _compose(exp)
    true = dict(mask=to_dev(mask).bool(), aatype=to_dev(aa), length=to_dev(b["lens"]).to(torch.int32))
    close = lambda t, e: np.allclose(t.detach().cpu().numpy().astype(np.float64), e, rtol=2.0 ** -22, atol=0)
    x = to_dev(pos).requires_grad_(True)
    out = foldcomp.violation_loss(x, true, tolerance=0.0, link_factor=0.5, codec=codec)
    assert set(out) == {"clash_loss", "link_loss", "clash_chain", "bond_chain", "angle_chain", "violation_chain", "loss"}
    VL.same(dict(clash_loss=out["clash_loss"].detach().cpu().numpy(), link_loss=out["link_loss"].detach().cpu().numpy()),
            dict(clash_loss=exp["clash_loss"], link_loss=exp["link_loss"]), "foldcomp.violation_loss")
    assert all(out[k].dtype == torch.float32 and out[k].shape == (n,) and close(out[k], chains[k]) for k in ("clash_chain", "bond_chain", "angle_chain", "violation_chain"))
    assert out["loss"].shape == () and close(out["loss"], chains["loss"]) and float(out["loss"].detach()) > 0.1 and out["loss"].requires_grad
    out["loss"].backward()
    w_clash, w_link = np.broadcast_to(wc[:, None, None], (n, L, A)), np.broadcast_to(wl[:, None, None], (n, L, 3))
    VL.same(x.grad.cpu().numpy(), VL.grad(pos, mask, aa, b["lens"], TABLE[A], w_clash, w_link, *TIGHT), "pos.grad, padded")
    # pred as a dict with a mask of its own: a slot is used when it is set in both
    pm = mask.copy()
    pm[E, 20:40, 1] = 0
    both = foldcomp.violation_loss(dict(pos=x.detach(), mask=to_dev(pm)), true, tolerance=0.0, link_factor=0.5, codec=codec)
    VL.same(both["clash_loss"].cpu().numpy(), VL.loss(pos, mask & pm, aa, b["lens"], TABLE[A], *TIGHT)["clash_loss"], "both masks")
    assert not both["loss"].requires_grad
    # packed, with true's pos left out
    arrays = AN.pack(b["arrays"], b["lens"])
    xp = to_dev(arrays[0]).requires_grad_(True)
    cu = torch.from_numpy(b["row_off"].astype(np.int32)).cuda()
    outp = foldcomp.violation_loss(xp, dict(mask=to_dev(arrays[1]), aatype=to_dev(arrays[2]), cu_seqlens=cu), tolerance=0.0, link_factor=0.5, codec=codec)
    VL.same(outp["clash_loss"].detach().cpu().numpy(), AN.pack1(exp["clash_loss"], b["lens"]), "packed")
    assert all(close(outp[k], chains[k]) for k in chains)
    outp["loss"].backward()
    VL.same(xp.grad.cpu().numpy(), AN.pack1(x.grad.cpu().numpy(), b["lens"]), "pos.grad, packed against padded")
    # no_grad, or a pos that needs no gradient: the value kernel only
    calls = []
    real = foldcomp.tensors._call
    monkeypatch.setattr(foldcomp.tensors, "_call", lambda c, name, *a: (calls.append(name), real(c, name, *a))[1])
    with torch.no_grad():
        quiet = foldcomp.violation_loss(x, true, tolerance=0.0, link_factor=0.5, codec=codec)
    plain = foldcomp.violation_loss(x.detach(), true, tolerance=0.0, link_factor=0.5, codec=codec)
    assert calls == ["fcz_violation_loss", "fcz_violation_loss"] and not quiet["loss"].requires_grad and AN.teq(quiet["loss"], out["loss"].detach())
    assert AN.teq(plain["clash_loss"], quiet["clash_loss"])
    # the defaults, and what is refused before a device is touched
    d = foldcomp.violation_loss(x.detach(), true, codec=codec)
    VL.same(d["link_loss"].cpu().numpy(), b["expected"](params=DEFAULT)["link_loss"], "defaults")
    with pytest.raises(ValueError):
        foldcomp.violation_loss(x.detach(), true, tolerance=-1.0, codec=codec)
    with pytest.raises(TypeError):
        foldcomp.violation_loss(x.detach(), dict(aatype=true["aatype"]), codec=codec)
    with pytest.raises(foldcomp.error):
        foldcomp.violation_loss(x.detach().cpu(), dict(true, mask=true["mask"].cpu(), aatype=true["aatype"].cpu(), length=None), codec=codec)


def test_backward_from_one_output_alone(codec):
    """every other backward here goes through out["loss"], whose upstream gradients are constant along a chain. Here the backward is
    taken from clash_loss alone and from link_loss alone, under arbitrary elementwise weights, as a product and as an expanded
    (stride 0 along the rows) gradient handed to backward() itself, so that what reaches the gradient kernel's wrapper is not
    contiguous; each against the restatement with those weights and zeros for the other output, on bits"""
    import torch
    import foldcomp_amd as foldcomp
    A, lens = 14, np.asarray([40, 23], np.uint32)
    n, L = len(lens), int(lens.max())
    rng = np.random.default_rng(77)
    pos = np.stack([AN.helix(rng, L, A) for _ in range(n)])
    mask = (rng.random((n, L, A)) > 0.03).astype(np.uint8)
    aa = rng.integers(0, 21, size=(n, L)).astype(np.uint8)
    aa[0, 5] = aa[1, 7] = V.PRO
    true = dict(mask=to_dev(mask).bool(), aatype=to_dev(aa), length=to_dev(lens).to(torch.int32))
    row = dict(clash_loss=VL.weights((n, 1, A), 78), link_loss=VL.weights((n, 1, 3), 79))
    full = dict(clash_loss=VL.weights((n, L, A), 80), link_loss=VL.weights((n, L, 3), 81))
    zeros = dict(clash_loss=np.zeros((n, L, A), F), link_loss=np.zeros((n, L, 3), F))
    for key in ("clash_loss", "link_loss"):
        for how in ("product", "expanded product", "expanded gradient"):
            W = full[key] if how == "product" else np.ascontiguousarray(np.broadcast_to(row[key], full[key].shape))
            x = to_dev(pos).requires_grad_(True)
            out = foldcomp.violation_loss(x, true, tolerance=0.0, link_factor=0.5, codec=codec)
            if how == "product":
                (out[key] * to_dev(W)).sum().backward()
            else:
                Wt = to_dev(row[key]).expand(*full[key].shape)
                assert Wt.stride(1) == 0 and not Wt.is_contiguous()
                if how == "expanded product":
                    (out[key] * Wt).sum().backward()
                else:
                    out[key].backward(gradient=Wt)
            w = dict(zeros, **{key: W})
            exp = VL.grad(pos, mask, aa, lens, TABLE[A], w["clash_loss"], w["link_loss"], *TIGHT)
            assert np.abs(exp).max() > 0.1 and not exp[1, 23:].any()
            VL.same(x.grad.cpu().numpy(), exp, f"pos.grad from {key} alone, {how}")


def test_gradient_descent_lowers_the_loss(codec):
    """ten steps of plain gradient descent on a clashing helix: every step strictly lowers the loss"""
    import torch
    import foldcomp_amd as foldcomp
    A, m = 14, 40
    rng = np.random.default_rng(12)
    pos = AN.helix(rng, m, A)[None]
    true = dict(mask=torch.ones((1, m, A), dtype=torch.bool, device="cuda:0"), aatype=to_dev(rng.integers(0, 20, size=(1, m)).astype(np.uint8)))
    x = to_dev(pos).requires_grad_(True)
    losses = []
    for _ in range(11):
        out = foldcomp.violation_loss(x, true, codec=codec)
        losses.append(float(out["loss"].detach()))
        out["loss"].backward()
        with torch.no_grad():
            x -= DESCENT_STEP * x.grad
        x.grad = None
    print("descent:", [round(v, 5) for v in losses])
    assert losses[0] > 0.05 and all(b < a for a, b in zip(losses, losses[1:])), losses


DESCENT_STEP = 1.0
