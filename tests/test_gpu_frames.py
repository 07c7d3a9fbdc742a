"""GPU: the rigid frames (fcz_frames_dev, its host form, foldcomp.rigid_frames, decode_tensors(frames=), tensor_batches(frames=))
against the numpy restatement of the contract (tests/_frames.py). Every comparison is on bits; the device calls write into arrays
pre-filled with 0xA5 with guard bytes on both sides, so a byte the call leaves unwritten fails the comparison."""
import numpy as np
import pytest

import _analysis as AN
import _dense as D
import _frames as F
from _cases import db_cases, golden_records_raw
from _devpath import DevGuarded, HostGuarded, host_ptr, to_dev

pytestmark = pytest.mark.gpu

L_GOLD = 1400
BACKBONE, ALL = 0, 1
TILE_ALL, TILE_BACKBONE = 32, 256                                    # rows per tile of k_frames<A, 8> / <A, 1>


@pytest.fixture(scope="module")
def records(golden):
    return golden_records_raw(golden)[1]


@pytest.fixture(scope="module")
def gold(codec, records):
    """the 56 golden records as atom37 / atom14 / backbone4 at L = 1400 (host and device) and the restatement with groups = all on
    each: computed once, never changed"""
    host, dev = AN.decoded_layouts(codec, records, L_GOLD, ("pos", "mask", "aatype", "length"))
    assert host["atom37"]["length"].max() == L_GOLD
    exp = {lay: F.frames(h["pos"], h["mask"], h["aatype"], h["length"], D.LAYOUTS[lay], ALL) for lay, h in host.items()}
    return dict(host=host, dev=dev, n=len(records), exp=exp)


def _gold_dev(codec, gold, layout, groups, guard=F.GUARD, aatype=True):
    d = gold["dev"][layout]
    return F.run_dev(codec, d["pos"], d["mask"], d["aatype"] if aatype else None, d["length"], gold["n"], L_GOLD, D.LAYOUTS[layout], groups, guard)


def _col0(exp):
    return exp[0][..., :1, :, :], exp[1][..., :1, :], exp[2][..., :1]


def test_golden_all_layouts(codec, gold):
    e37, e14, e4 = (gold["exp"][lay] for lay in ("atom37", "atom14", "backbone4"))
    F.same(_gold_dev(codec, gold, "atom37", ALL), e37, "atom37 all")
    F.same(_gold_dev(codec, gold, "atom14", ALL), e14, "atom14 all")
    F.same(_gold_dev(codec, gold, "backbone4", ALL), e4, "backbone4 all")
    F.same(e14, e37, "the layouts hold the same atoms")
    assert e37[2][..., 4:].sum() > 5000 and not e4[2][..., 4:].any() and not e4[2][..., 1:3].any()
    F.same((e4[0][..., [0, 3], :, :], e4[1][..., [0, 3], :], e4[2][..., [0, 3]]),
           (e37[0][..., [0, 3], :, :], e37[1][..., [0, 3], :], e37[2][..., [0, 3]]), "backbone4 groups 0 and 3")
    lens = gold["host"]["atom37"]["length"]
    assert all(e37[2][e, :m, 0].all() and not e37[2][e, m:].any() for e, m in enumerate(lens))


def test_golden_backbone_is_column_0(codec, gold):
    for lay in D.LAYOUTS:
        F.same(_gold_dev(codec, gold, lay, BACKBONE, aatype=False), _col0(gold["exp"][lay]), f"{lay} backbone")
    F.same(_gold_dev(codec, gold, "atom37", BACKBONE), _col0(gold["exp"]["atom37"]), "backbone with an aatype")


def test_golden_packed(codec, gold):
    h = gold["host"]["atom37"]
    lens = np.minimum(h["length"].astype(np.int64), L_GOLD)
    cat = lambda a: AN.pack1(a, lens)
    pos, mask, aa = cat(h["pos"]), cat(h["mask"]), cat(h["aatype"])
    R = len(pos)
    exp = tuple(cat(x)[None] for x in gold["exp"]["atom37"])
    F.same(F.run_dev(codec, to_dev(pos), to_dev(mask), to_dev(aa), None, 1, R, 0, ALL), exp, "packed all")
    F.same(F.run_dev(codec, to_dev(pos), to_dev(mask), None, None, 1, R, 0, BACKBONE), _col0(exp), "packed backbone")


# ---- synthetic rows ---------------------------------------------------------------------------------------------------------------

def _pool(layout, seed):
    """rows [R, A, 3] built from one residue of every type 0 .. 20 and aatype 200 (every slot set, lattice coordinates that keep
    every triple well conditioned): the plain row; every slot's mask cleared in turn; NaN, +inf, -inf and -0.0 in every slot in
    turn (defining and other atoms alike); per group a coincident and a collinear triple; shuffled"""
    A = F.WIDTH[layout]
    rng = np.random.default_rng(seed)
    tab = F.slot_table(layout)
    pos, mask, aa = [], [], []

    def add(p, m, ty):
        pos.append(p); mask.append(m); aa.append(ty)

    for ty in list(range(21)) + [200]:
        p0 = rng.integers(-9, 10, size=(A, 3)).astype(np.float32) + np.arange(A, dtype=np.float32)[:, None] * np.float32(0.25)
        m0 = np.ones(A, np.uint8)
        add(p0, m0, ty)
        for a in range(A):
            m = m0.copy(); m[a] = 0; add(p0, m, ty)
            for c, v in enumerate((np.nan, np.inf, -np.inf)):
                p = p0.copy(); p[a, c] = v; add(p, m0, ty)
            p = p0.copy(); p[a] = np.float32(-0.0); add(p, m0, ty)
        for g in range(8):
            a0, a1, a2 = tab[min(ty, 20), g]
            if a0 < 0:
                continue
            p = p0.copy(); p[a0] = p[a1]; add(p, m0, ty)
            p = p0.copy(); p[a2] = p[a1]; add(p, m0, ty)
            p = p0.copy(); p[a0] = p[a1] + np.asarray([3, 0, 0], np.float32); p[a2] = p[a1] - np.asarray([6, 0, 0], np.float32); add(p, m0, ty)
    order = rng.permutation(len(pos))
    return np.stack(pos)[order], np.stack(mask)[order], np.asarray(aa, np.uint8)[order]


@pytest.fixture(scope="module")
def pools():
    out = {}
    for layout in (0, 1, 2):
        pos, mask, aa = _pool(layout, 20 + layout)
        exp = F.frames(pos, mask, aa, None, layout, ALL)
        assert not np.isnan(exp[0]).any() and not np.isnan(exp[1]).any()
        out[layout] = dict(pos=pos, mask=mask, aa=aa, exp=exp, dev=(to_dev(pos), to_dev(mask), to_dev(aa)))
    fm = out[0]["exp"][2]
    assert fm[:, 4:].any(axis=0).all() and (fm[:, [0, 3, 4]] == 0).sum() > 300 and len(out[0]["pos"]) > 3 * TILE_BACKBONE
    return out


@pytest.mark.parametrize("layout", [0, 1, 2])
def test_synthetic_pool(codec, pools, layout):
    s = pools[layout]
    R = len(s["pos"])
    F.same(F.run_dev(codec, *s["dev"], None, 1, R, layout, ALL), tuple(x[None] for x in s["exp"]), "all")
    F.same(F.run_dev(codec, s["dev"][0], s["dev"][1], None, None, 1, R, layout, BACKBONE), _col0(tuple(x[None] for x in s["exp"])), "backbone")


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 255, 256, 257, TILE_ALL + 3, TILE_BACKBONE + 3])
def test_synthetic_row_counts(codec, pools, rows):
    s = pools[0]
    pos, mask, aa = (to_dev(np.ascontiguousarray(s[k][:rows])) for k in ("pos", "mask", "aa"))
    exp = tuple(x[None, :rows] for x in s["exp"])
    F.same(F.run_dev(codec, pos, mask, aa, None, 1, rows, 0, ALL), exp, "packed form")
    F.same(F.run_dev(codec, pos, mask, aa, None, rows, 1, 0, ALL), tuple(x[0][:, None] for x in exp), "one row per entry")
    F.same(F.run_dev(codec, pos, mask, None, None, 1, rows, 0, BACKBONE), _col0(exp), "backbone")


def test_no_entries(codec, pools):
    pos, mask, aa = pools[0]["dev"]
    g = DevGuarded(F.out_spec((8,), 8))
    rp, tp, fp = g.ptrs()
    assert codec.lib.fcz_frames_dev(codec.ctx, pos.data_ptr(), mask.data_ptr(), aa.data_ptr(), None, 0, 8, 0, ALL, rp, tp, fp) == 0
    codec.synchronize()
    assert g.untouched()
    h = HostGuarded(F.out_spec((8,), 8))
    host = [host_ptr(np.ascontiguousarray(pools[0][k])) for k in ("pos", "mask", "aa")]
    assert codec.lib.fcz_frames(codec.ctx, *host, None, 0, 8, 0, ALL, *h.ptrs()) == 0
    assert h.untouched()


# ---- length and outputs -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", [0, 2])
def test_length_and_unaligned_arrays(codec, pools, layout):
    import torch
    s = pools[layout]
    n, L, A = 4, 70, F.WIDTH[layout]
    pos, mask, aa = (np.ascontiguousarray(s[k][:n * L]).reshape((n, L) + s[k].shape[1:]) for k in ("pos", "mask", "aa"))
    dev = [to_dev(x) for x in (pos, mask, aa)]
    whole = F.frames(pos, mask, aa, None, layout, ALL)
    F.same(F.run_dev(codec, *dev, None, n, L, layout, ALL), whole, "NULL")
    F.same(F.run_dev(codec, *dev, to_dev(np.asarray([L, L + 1, 65535, 0xFFFFFFFF], np.uint32)), n, L, layout, ALL), whole, "length >= L")
    blank = F.run_dev(codec, *dev, to_dev(np.zeros(n, np.uint32)), n, L, layout, ALL)
    F.same(blank, F.frames(pos, mask, aa, np.zeros(n, np.uint32), layout, ALL), "length 0")
    assert not blank[2].any() and not F.bits(blank[1]).any()
    # rows behind the length hold 0xA5 bytes in pos, mask and aatype: none of them reaches the output
    lens = np.asarray([0, 1, 33, 69], np.uint32)
    live = F.live_rows(n, L, lens)
    gp, gm, ga = pos.copy(), mask.copy(), aa.copy()
    gp.view(np.uint8)[~live] = 0xA5; gm[~live] = 0xA5; ga[~live] = 0xA5
    exp = F.frames(pos, mask, aa, lens, layout, ALL)
    for guard in (F.GUARD, 4):                                        # 4: no output begins on 16 bytes
        got = F.run_dev(codec, to_dev(gp), to_dev(gm), to_dev(ga), to_dev(lens), n, L, layout, ALL, guard)
        F.same(got, exp, f"length < L, guard {guard}")
        F.same(F.run_dev(codec, to_dev(gp), to_dev(gm), None, to_dev(lens), n, L, layout, BACKBONE, guard), _col0(exp), f"backbone, guard {guard}")
    assert not exp[2][~live].any() and exp[2][live][:, 0].sum() > 20
    # inputs that do not begin on 16 bytes: pos 4 bytes in, mask and aatype 1 byte in
    raw_p = torch.zeros(pos.size + 1, dtype=torch.float32, device="cuda:0"); raw_p[1:] = dev[0].reshape(-1)
    raw_m = torch.zeros(mask.size + 1, dtype=torch.uint8, device="cuda:0"); raw_m[1:] = dev[1].reshape(-1)
    raw_a = torch.zeros(aa.size + 1, dtype=torch.uint8, device="cuda:0"); raw_a[1:] = dev[2].reshape(-1)
    F.same(F.run_dev(codec, raw_p[1:], raw_m[1:], raw_a[1:], None, n, L, layout, ALL), whole, "unaligned inputs")


def test_refusals_leave_the_outputs_untouched(codec):
    import torch
    n, L, A = 2, 8, 37
    pos, mask, aa, _ = AN.refusal_inputs(n, L, A)
    g = DevGuarded(F.out_spec((n, L), 8))
    rp, tp, fp = g.ptrs()
    lib, ctx, P, M, T = codec.lib, codec.ctx, pos.data_ptr(), mask.data_ptr(), aa.data_ptr()
    bad = [(None, P, M, T, None, n, L, 0, ALL, rp, tp, fp), (ctx, None, M, T, None, n, L, 0, ALL, rp, tp, fp), (ctx, P, None, T, None, n, L, 0, ALL, rp, tp, fp),
           (ctx, P, M, None, None, n, L, 0, ALL, rp, tp, fp), (ctx, P, M, T, None, n, L, 0, ALL, None, tp, fp), (ctx, P, M, T, None, n, L, 0, ALL, rp, None, fp),
           (ctx, P, M, T, None, n, L, 0, ALL, rp, tp, None), (ctx, P, M, T, None, n, L, 3, ALL, rp, tp, fp), (ctx, P, M, T, None, n, L, -1, ALL, rp, tp, fp),
           (ctx, P, M, T, None, n, L, 0, 2, rp, tp, fp), (ctx, P, M, T, None, n, L, 0, -1, rp, tp, fp), (ctx, P, M, T, None, n, 0, 0, ALL, rp, tp, fp)]
    torch.cuda.synchronize()
    for a in bad:
        assert lib.fcz_frames_dev(*a) == -1, a
    assert lib.fcz_frames_dev(ctx, P, M, T, None, 0, L, 0, ALL, rp, tp, fp) == 0
    codec.synchronize()
    assert g.untouched()


def test_host_forms(codec, pools):
    s = pools[1]
    n, L = 5, 41
    pos, mask, aa = (np.ascontiguousarray(s[k][:n * L]).reshape((n, L) + s[k].shape[1:]) for k in ("pos", "mask", "aa"))
    lens = np.asarray([41, 0, 7, 100, 40], np.uint32)
    exp = F.frames(pos, mask, aa, lens, 1, ALL)
    h = codec.frames(pos, mask, aa, length=lens, groups="all")
    assert h["frame_mask"].dtype == np.bool_ and h["rot"].shape == (n, L, 8, 3, 3)
    F.same((h["rot"], h["trans"], h["frame_mask"]), exp, "Codec.frames all")
    h = codec.frames(pos, mask, length=lens, layout="atom14")
    assert h["rot"].shape == (n, L, 3, 3) and h["trans"].shape == (n, L, 3) and h["frame_mask"].shape == (n, L)
    F.same((h["rot"][..., None, :, :], h["trans"][..., None, :], h["frame_mask"][..., None]), _col0(exp), "Codec.frames backbone")
    R = n * L
    h = codec.frames(pos.reshape(R, 14, 3), mask.reshape(R, 14).view(np.bool_), aa.reshape(R), groups="all")
    F.same((h["rot"], h["trans"], h["frame_mask"]), F.frames(pos.reshape(R, 14, 3), mask.reshape(R, 14), aa.reshape(R), None, 1, ALL), "Codec.frames packed")
    with pytest.raises(ValueError):
        codec.frames(pos, mask, groups="all")
    with pytest.raises(ValueError):
        codec.frames(pos, mask, aa, layout="atom37")


# ---- Python surface -------------------------------------------------------------------------------------------------------------

KEYS = ("rot", "trans", "frame_mask")


def _np3(d):
    return AN.to_numpy(d, KEYS)


def test_rigid_frames_and_decode_tensors(codec, gold, records):
    import torch
    import foldcomp_amd as foldcomp
    plain = foldcomp.decode_tensors(records, codec=codec)
    assert foldcomp.decode_tensors(records, codec=codec, frames=None).keys() == plain.keys() and not set(KEYS) & set(plain)
    t = foldcomp.decode_tensors(records, codec=codec, frames="all")
    assert set(t) == set(plain) | set(KEYS) and t["rot"].dtype == torch.float32 and t["frame_mask"].dtype == torch.bool
    assert t["rot"].shape == (56, L_GOLD, 8, 3, 3) and t["trans"].shape == (56, L_GOLD, 8, 3) and t["frame_mask"].shape == (56, L_GOLD, 8)
    F.same(_np3(t), gold["exp"]["atom37"], "decode_tensors all")
    r = foldcomp.rigid_frames(plain, groups="all", codec=codec)
    assert all(AN.teq(r[k], t[k]) for k in KEYS)
    b = foldcomp.decode_tensors(records, codec=codec, frames="backbone", layout="backbone4")
    assert b["rot"].shape == (56, L_GOLD, 3, 3) and b["trans"].shape == (56, L_GOLD, 3) and b["frame_mask"].shape == (56, L_GOLD)
    e = _col0(gold["exp"]["atom37"])
    F.same(_np3(b), (e[0][..., 0, :, :], e[1][..., 0, :], e[2][..., 0]), "decode_tensors backbone")
    r = foldcomp.rigid_frames(pos=b["pos"], mask=b["mask"], length=b["length"], codec=codec)                 # keywords, no aatype
    assert all(AN.teq(r[k], b[k]) for k in KEYS)
    # the alternative frames of the ambiguity table are one multiply away and exist only where the table says
    amb = torch.from_numpy(foldcomp.frame_ambiguous()).to(t["aatype"].device)[t["aatype"].long()]
    assert amb.shape == t["frame_mask"].shape and bool((amb & t["frame_mask"]).any()) and not bool(amb[..., :5].any())
    # packed
    pp = foldcomp.decode_tensors(records, codec=codec, packed=True)
    p = foldcomp.decode_tensors(records, codec=codec, packed=True, frames="all", layout="atom14")
    p37 = foldcomp.decode_tensors(records, codec=codec, packed=True, frames="all")
    assert set(p37) == set(pp) | set(KEYS) and p["rot"].shape == (p["pos"].shape[0], 8, 3, 3) and p["frame_mask"].shape == (p["pos"].shape[0], 8)
    assert all(AN.teq(p[k], p37[k]) for k in KEYS)
    lens = np.minimum(gold["host"]["atom37"]["length"].astype(np.int64), L_GOLD)
    F.same(_np3(p37), AN.pack(gold["exp"]["atom37"], lens), "decode_tensors packed")
    r = foldcomp.rigid_frames(p37, groups="all", codec=codec)
    assert all(AN.teq(r[k], p37[k]) for k in KEYS)
    r = foldcomp.rigid_frames(p37, codec=codec)
    assert r["rot"].shape == (p37["pos"].shape[0], 3, 3) and AN.teq(r["rot"], p37["rot"][:, 0].contiguous())
    # a window: the restatement on the returned rows only (crop_start in the dict: length is not used)
    w = foldcomp.decode_tensors(records, codec=codec, max_len=64, crop="center", frames="all", layout="atom14")
    exp = F.frames(w["pos"].cpu().numpy(), w["mask"].cpu().numpy().view(np.uint8), w["aatype"].cpu().numpy(), None, 1, ALL)
    F.same(_np3(w), exp, "window")
    assert exp[2][gold["host"]["atom37"]["length"] > 64][:, :, 0].all()
    r = foldcomp.rigid_frames(w, groups="all", codec=codec)
    assert all(AN.teq(r[k], w[k]) for k in KEYS)
    e = foldcomp.decode_tensors([], codec=codec, max_len=8, frames="all")
    assert e["rot"].shape == (0, 8, 8, 3, 3) and e["frame_mask"].shape == (0, 8, 8)
    assert foldcomp.decode_tensors([], codec=codec, packed=True, frames="backbone")["trans"].shape == (0, 3)
    with pytest.raises(ValueError):
        foldcomp.rigid_frames(pos=plain["pos"], mask=plain["mask"][:, :-1].contiguous(), codec=codec)
    with pytest.raises(ValueError):
        foldcomp.rigid_frames(pos=plain["pos"], mask=plain["mask"], aatype=plain["aatype"].to(torch.int64), groups="all", codec=codec)
    with pytest.raises(ValueError):
        foldcomp.rigid_frames(pos=plain["pos"].transpose(0, 1), mask=plain["mask"].transpose(0, 1), codec=codec)


def test_tensor_batches_frames(codec, golden, tmp_path):
    import foldcomp_amd as foldcomp
    from foldcomp_amd import api
    from foldcomp_amd.database import DatabaseWriter
    z, index = golden
    entries = [z[f"{n}/fcz"].tobytes() for n in db_cases(index)[:8]]
    path = str(tmp_path / "db")
    w = DatabaseWriter(path)
    for i, e in enumerate(entries):
        w.append(e, i, f"entry_{i:02d}")
    w.close()
    api.set_codec(codec)
    try:
        with foldcomp.open(path) as db:
            old = set(next(iter(db.tensor_batches(5))))
            for kw in (dict(), dict(packed=True, max_residues=2000)):
                seen = 0
                for b in db.tensor_batches(5, frames="backbone", **kw):
                    assert set(b) >= set(KEYS) and b["rot"].shape == b["pos"].shape[:-2] + (3, 3) and b["frame_mask"].shape == b["pos"].shape[:-2]
                    ref = foldcomp.rigid_frames(b)
                    assert all(AN.teq(ref[k], b[k]) for k in KEYS)
                    seen += len(b["names"])
                assert seen == 8
            assert set(next(iter(db.tensor_batches(5)))) == old and not set(KEYS) & old
    finally:
        api.set_codec(None)
