"""The maximised GDT counts (include/fcz_hip.h, fcz_gdt_dev) without a device: the properties of the definition on the numpy reference
of tests/_gdt.py, the gain on hinged chains, the padded and the packed form, a chain against its sites alone, the conditions under
which that reference may judge the kernel, the new ABI symbols' refusals and the argument errors of foldcomp.gdt."""
import ctypes

import numpy as np
import pytest

import _gdt as G
import _superpose as SP
import _tmscore as T
from foldcomp_amd import _lib, api, tensors
from foldcomp_amd.structure import CGdtOut

F = np.float32
NEW = ("fcz_gdt_dev", "fcz_gdt_packed_dev", "fcz_gdt", "fcz_gdt_packed")


def _batch():
    lens, hinged, pos_t, mask, pos_p = T.tm_batch()
    n, ref, traces = G.gdt_batch_reference()
    return n, lens[:n], hinged[:n], pos_t[:n], mask[:n], pos_p[:n], ref, traces


def test_the_properties_of_the_definition():
    n, lens, hinged, pos_t, mask, pos_p, ref, _ = _batch()
    kab = SP.superpose_padded(pos_t, mask, pos_p, None, lens, 1)
    tm, _ = T.tm_batch_reference()
    assert (ref["gdt_counts"] >= kab["gdt_counts"]).all()
    assert (ref["gdt_counts"] >= tm["gdt_counts"][:n]).all()
    assert (np.diff(ref["gdt_counts"], axis=1) >= 0).all() and (ref["gdt_counts"] <= lens[:, None]).all()
    assert np.array_equal(ref["sites"], lens) and (ref["run"] >= 0).all() and (ref["run"] < 6).all()
    assert (ref["selected"] <= lens[:, None]).all() and (ref["selected"][lens >= 3] >= 3).all()
    for k in range(5):                                                        # the popcount of bit k is the count
        assert np.array_equal((ref["within"] >> k & 1).sum(axis=1), ref["gdt_counts"][:, k]), k
    assert not ref["within"][np.arange(pos_t.shape[1])[None, :] >= lens[:, None]].any()
    # the TM run alone: between tm_score's counts and all runs'
    sub = lens <= 65
    only = G.gdt_padded(pos_t[sub], mask[sub], pos_p[sub], None, lens[sub], 1, runs=G.RUNS_TM)
    assert (only["gdt_counts"] >= tm["gdt_counts"][:n][sub]).all() and (only["gdt_counts"] <= ref["gdt_counts"][sub]).all()
    assert not only["run"].any()
    # a single constant-cut run never wins under another run's name
    one = G.gdt_padded(pos_t[sub], mask[sub], pos_p[sub], None, lens[sub], 1, runs=1 << 3)
    assert (one["run"][lens[sub] > 0] == 3).all() and (one["gdt_counts"] >= kab["gdt_counts"][sub]).all()


def test_one_level_and_no_iteration_is_the_kabsch_fit():
    n, lens, _, pos_t, mask, pos_p, _, _ = _batch()
    one = G.gdt_padded(pos_t, mask, pos_p, None, lens, 1, iterations=0, levels=1)
    kab = SP.superpose_padded(pos_t, mask, pos_p, None, lens, 1)
    assert np.array_equal(one["gdt_counts"], kab["gdt_counts"]) and np.array_equal(one["sites"], kab["sites"])
    for k in range(5):
        assert np.array_equal(one["rot"][:, k], kab["rot"]) and np.array_equal(one["trans"][:, k], kab["trans"])
        assert np.array_equal(one["within"] >> k & 1, (kab["dev"] <= G.CUTOFFS[k]) & (np.arange(pos_t.shape[1])[None, :] < lens[:, None]))
    assert not one["seed"].any() and not one["run"].any() and np.array_equal(one["selected"], np.repeat(lens[:, None], 5, axis=1))


def test_the_gain_on_hinged_chains():
    n, lens, hinged, pos_t, mask, pos_p, ref, _ = _batch()
    kab = SP.superpose_padded(pos_t, mask, pos_p, None, lens, 1)
    tm, _ = T.tm_batch_reference()
    ts = lambda c: SP.gdt_scores(np.asarray(c), lens)[0].astype(np.float64)
    gain, over_tm = ts(ref["gdt_counts"]) - ts(kab["gdt_counts"]), ts(ref["gdt_counts"]) - ts(tm["gdt_counts"][:n])
    assert (gain >= 0).all() and (over_tm >= 0).all()
    # the hinged chains of 63 residues and more: the nine of the batch up to 257 rows and the one of 1027 rows, searched in full
    all_lens, all_hinged, all_t, all_mask, all_p = T.tm_batch()
    e, long, traces = G.gdt_long_reference()
    a, b, c = G.assert_fair(all_t[e:e + 1], all_p[e:e + 1], 1, traces, "1027 rows")
    ts1 = lambda counts: float(SP.gdt_scores(np.asarray(counts), all_lens[e:e + 1])[0][0])
    kab_long = SP.superpose_padded(all_t[e:e + 1], all_mask[e:e + 1], all_p[e:e + 1], None, all_lens[e:e + 1], 1)
    big = hinged & (lens >= 63)
    gains = np.concatenate([gain[big], [ts1(long["gdt_counts"]) - ts1(kab_long["gdt_counts"])]])
    over = np.concatenate([over_tm[big], [ts1(long["gdt_counts"]) - ts1(tm["gdt_counts"][e:e + 1])]])
    print("GDT-TS gains on the hinged chains of 63 .. 1027 residues over the Kabsch fit:", np.round(np.sort(gains), 3), "over tm_score:", np.round(np.sort(over), 3))
    print(f"1027 rows, hinged: counts {long['gdt_counts'][0]} against the Kabsch fit's {kab_long['gdt_counts'][0]}, {traces[0]['fits']} fits, (a) {a:.3g} (b) {b:.3g} (c) {c:.3g}")
    assert len(gains) == 10 == (all_hinged & (all_lens >= 63)).sum() and (gains > 0).all() and (over >= 0).all()
    assert (long["gdt_counts"] >= kab_long["gdt_counts"]).all() and (long["gdt_counts"] >= tm["gdt_counts"][e:e + 1]).all()


def test_padded_against_packed_and_the_site_rules():
    rng = np.random.default_rng(6)
    lens = [0, 1, 2, 5, 30]
    L, A = 32, 4
    pos = rng.uniform(-20, 20, (len(lens), L, A, 3)).astype(F)
    pred = (pos + rng.standard_normal(pos.shape)).astype(F)
    mask = (rng.random((len(lens), L, A)) > 0.1).astype(np.uint8)
    pmask = (rng.random((len(lens), L, A)) > 0.1).astype(np.uint8)
    pos[4, 3, 1, 0] = np.nan; pred[4, 7, 1, 2] = np.inf; mask[4, [3, 7], 1] = 1; pmask[4, [3, 7], 1] = 1
    pad = G.gdt_padded(pos, mask, pred, pmask, np.asarray(lens), 1)
    row_off = np.concatenate([[0], np.cumsum(lens)])
    pk = G.gdt_packed(*SP.pack((pos, mask, pred, pmask), lens), row_off, 1)
    for k in G.KEYS[:-1]:
        assert np.array_equal(pad[k], pk[k]), k
    assert np.array_equal(SP.pack((pad["within"],), lens)[0], pk["within"])
    site = SP.site_of(pos, mask, pred, pmask, 1)
    assert not site[4, 3] and not site[4, 7] and pad["within"][4, 3] == 0 and pad["within"][4, 7] == 0
    assert pad["sites"][4] == site[4, :30].sum() < 30 and pad["sites"][0] == 0 and np.array_equal(pad["rot"][0], np.tile(np.eye(3), (5, 1, 1)))
    assert not pad["gdt_counts"][0].any() and not pad["seed"][0].any() and not pad["selected"][0].any() and not pad["within"][0].any()
    # the fragments count SITES, not rows: the search of a chain equals the search of its sites alone
    js = np.flatnonzero(site[4, :30])
    alone = G.search_chain(pos[4, js, 1], pred[4, js, 1], np.ones(len(js), bool))
    for k in ("gdt_counts", "seed", "run", "selected", "rot", "trans"):
        assert np.array_equal(alone[k], pad[k][4]), k
    assert np.array_equal(alone["within"], pad["within"][4, js])


def test_the_cuts_of_the_runs():
    assert G.cuts_of(0, 300, 3) == [T.d_search_of(300) - 1.0, T.d_search_of(300) + 1.0, T.d_search_of(300) + 1.0]
    assert [G.cuts_of(1 + k, 300, 2) for k in range(5)] == [[c, c] for c in (0.5, 1.0, 2.0, 4.0, 8.0)] and G.cuts_of(4, 9, 0) == []
    assert api.GDT_CUTOFFS == G.CUTOFFS == (0.5, 1.0, 2.0, 4.0, 8.0)


def test_the_gpu_tests_seeded_inputs_meet_its_conditions():
    """A float64 judge with another solver is fair to a search over thresholds only if, for EVERY chain of the GPU test's batch, (a) no
    deviation lies within 1e-8 A of a cut in any selection step (two implementations differ by ~1e-10 A in dev, so both select the
    same sets), (b) at every fit whose count at a cutoff reaches the chain's maximum - 1 no deviation lies within 1e-8 A of that
    cutoff (so the counts that decide, and with them the winning seed, run and round, are exact), and (c) Horn's largest eigenvalue
    is well separated for every winning selection (section 6.11's condition for the transform tolerance)."""
    n, lens, _, pos_t, mask, pos_p, _, traces = _batch()
    a, b, c = G.fair(pos_t, pos_p, 1, traces)
    fits = sum(t["fits"] for t in traces)
    winners = np.isfinite(c).sum()
    print(f"generator seed {T.TM_SEED}: (a) {a.min():.3g} A, (b) {b.min():.3g} A, (c) {c.min():.3g} over {winners} winners of >= 3 sites, {fits} fits")
    assert (a >= G.MARGIN).all() and (b >= G.MARGIN).all() and (c >= G.GAP).all()
    assert winners == 5 * (lens >= 3).sum() == 125


def test_pure_host_abi():
    lib = _lib.load()
    assert set(NEW) <= set(_lib.EXPORTS)
    assert [f for f, _ in CGdtOut._fields_] == list(G.KEYS)
    buf = np.zeros(256, np.uint8)
    p = buf.ctypes.data
    out = CGdtOut(p, p, p, p, p, p, p, p)
    fns = (lib.fcz_gdt_dev, lib.fcz_gdt_packed_dev, lib.fcz_gdt, lib.fcz_gdt_packed)
    for fn in fns:
        assert fn(None, p, p, p, p, p, 1, 4, 0, 1, 0, 20, 63, ctypes.byref(out)) == -1
    fake = ctypes.c_void_p(buf.ctypes.data)                                  # refused before anything is touched (the ctx is never read)
    for fn in fns:
        assert fn(fake, p, p, p, p, p, 1, 4, 0, 37, 0, 20, 63, ctypes.byref(out)) == -1 and fn(fake, p, p, p, p, p, 1, 4, 3, 1, 0, 20, 63, ctypes.byref(out)) == -1
        assert fn(fake, p, p, p, p, p, 1, 4, 2, 4, 0, 20, 63, ctypes.byref(out)) == -1 and fn(fake, p, p, p, p, p, 1, 4, 0, -1, 0, 20, 63, ctypes.byref(out)) == -1
        assert fn(fake, None, p, p, p, p, 1, 4, 0, 1, 0, 20, 63, ctypes.byref(out)) == -1 and fn(fake, p, None, p, p, p, 1, 4, 0, 1, 0, 20, 63, ctypes.byref(out)) == -1
        assert fn(fake, p, p, None, p, p, 1, 4, 0, 1, 0, 20, 63, ctypes.byref(out)) == -1 and fn(fake, p, p, p, p, p, 1, 4, 0, 1, 0, 20, 63, None) == -1
        assert fn(fake, p, p, p, p, p, 1, 4, 0, 1, 0, 20, 63, ctypes.byref(CGdtOut(None, p, p, p, p, p, p, p))) == -1   # NULL gdt_counts
        assert fn(fake, p, p, p, p, p, 1, 2 ** 31, 0, 1, 0, 20, 63, ctypes.byref(out)) == -1
        assert fn(fake, p, p, p, p, p, 1, 4, 0, 1, 0, 65, 63, ctypes.byref(out)) == -1            # iterations > 64
        assert fn(fake, p, p, p, p, p, 1, 4, 0, 1, 0, 20, 0, ctypes.byref(out)) == -1             # no run
        assert fn(fake, p, p, p, p, p, 1, 4, 0, 1, 0, 20, 64, ctypes.byref(out)) == -1            # a seventh run
        assert fn(fake, p, p, p, p, p, 1, 4, 0, 1, 0, 20, 2 ** 32 - 1, ctypes.byref(out)) == -1
    for fn in (lib.fcz_gdt_dev, lib.fcz_gdt):
        assert fn(fake, p, p, p, p, p, 1, 0, 0, 1, 0, 20, 63, ctypes.byref(out)) == -1            # L == 0
    for fn in (lib.fcz_gdt_packed_dev, lib.fcz_gdt_packed):
        assert fn(fake, p, p, p, p, None, 1, 4, 0, 1, 0, 20, 63, ctypes.byref(out)) == -1         # chains without a row_off
    assert not buf.any()


def test_argument_errors_need_no_device():
    pos37, mask37 = np.zeros((2, 8, 37, 3), F), np.zeros((2, 8, 37), np.uint8)
    pos4, mask4 = np.zeros((2, 8, 4, 3), F), np.zeros((2, 8, 4), np.uint8)
    true37, true4 = dict(pos=pos37, mask=mask37), dict(pos=pos4, mask=mask4)
    for pred, true, kw in ((pos37, true37, dict(atom="XX")), (pos4, true4, dict(atom="CB")), (pos37, true37, dict(atom=37)), (pos37, true37, dict(atom=-1)),
                           (pos37[:, :7], true37, {}), (pos4, true37, {}), (dict(pos=pos37, mask=mask37[:1]), true37, {}),
                           (pos37, true37, dict(iterations=65)), (pos37, true37, dict(iterations=True)), (pos37, true37, dict(levels=0)),
                           (pos37, true37, dict(levels=1.0)), (pos37, true37, dict(runs="none")), (pos37, true37, dict(runs=())),
                           (pos37, true37, dict(runs=(3.0,))), (pos37, true37, dict(runs=("tm", "all"))), (pos37, true37, dict(runs=63)),
                           (pos37, true37, dict(runs=None)), (pos37, true37, dict(runs=(True,)))):
        with pytest.raises(ValueError):
            tensors.gdt(pred, true, **kw)
    with pytest.raises(TypeError):
        tensors.gdt(pos37, dict(pos=pos37))
    with pytest.raises(TypeError):
        tensors.gdt(pos37, true37, apply=True)                                # there is no apply
    assert api.check_gdt("CA", pos37.shape, pos37.shape, mask37.shape) == (1, 20, 0, 63)
    assert api.check_gdt("CB", (9, 14, 3), (9, 14, 3), None, 0, 3, "tm") == (4, 0, 3, 1)
    assert api.check_gdt_runs(("tm", 8)) == 33 and api.check_gdt_runs([0.5, 1, 2.0, np.float32(4)]) == 30 and api.check_gdt_runs(iter((0.5,))) == 2
    assert api.check_gdt_runs("all") == api.GDT_RUNS_ALL == 63 and api.check_gdt_runs("tm") == api.GDT_RUNS_TM == 1
    import foldcomp
    import foldcomp_amd
    assert foldcomp.gdt is foldcomp_amd.gdt is tensors.gdt and foldcomp.GDT_CUTOFFS == (0.5, 1.0, 2.0, 4.0, 8.0)
    assert "gdt" in foldcomp.__all__ and "gdt" in foldcomp_amd.__all__ and "GDT_CUTOFFS" in foldcomp.__all__
    assert "apply_transform" in tensors.gdt.__doc__
