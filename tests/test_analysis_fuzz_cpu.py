"""CPU: what the case list of tests/_analysis_fuzz.py is, without a device. The list is a pure function of its seed; the comparators'
margins are met by few redraws; the list holds the chains the fuzz exists for, asserted on the built inputs through the mirror of
chain_stage_slots' pass split; and that mirror agrees with a line-by-line transcription of the device function on random masks."""
import collections
import dataclasses
import os
import re

import numpy as np
import pytest

import _analysis_fuzz as FZ
import _fape_atoms as FA
import _sweep_grids as G
import _violation_loss as VL
import _violations as V

CASES = FZ.cases()
BY = collections.defaultdict(list)
for _c in CASES:
    BY[_c.analysis].append(_c)


def _bytes(inp):
    return b"".join(k.encode() + (b"-" if v is None else v.tobytes()) for k, v in sorted(inp.items()))


def _inputs(c):
    """the arrays a case is built into (a TM-align case: its two sets and its pairs)"""
    if c.analysis != "tmalign":
        return FZ.build(c).inp
    b = FZ.build_tmalign(c)
    return dict({"a_" + k: v for k, v in b.sa.items()}, **{"b_" + k: v for k, v in b.sb.items()}, pairs=b.pairs)


def test_the_list_is_a_pure_function_of_the_seed():
    again = FZ.cases()
    assert repr(again).encode() == repr(CASES).encode() and again == CASES
    assert FZ.cases(1) != CASES and len({c.id for c in CASES}) == len(CASES)
    for c in CASES[::7]:
        assert FZ.Case(*dataclasses.astuple(c)) == c
        assert _bytes(_inputs(c)) == _bytes(_inputs(FZ.Case(*dataclasses.astuple(c)))), c.id


def test_the_cases_of_the_analyses_before_fape_atoms_are_unchanged():
    """the 250 cases the list held before the all-atom FAPE joined it, as tuples, at seeds 0 and 1: a checksum of their repr"""
    for seed, crc in ((0, 2045179907), (1, 3364877883)):
        old = tuple(dataclasses.astuple(c) for c in FZ.cases(seed) if c.analysis != "fape_atoms")
        assert len(old) == 250 and FZ.crc(repr(old)) == crc, seed


@pytest.mark.parametrize("name", FZ.NEED_MARGIN)
def test_few_cases_are_redrawn(name):
    """at most one case in eight of an analysis whose comparator needs a margin is redrawn, and every case finds a seed (realise raises
    when four seeds in a row miss the margin, so no profile is lost silently)"""
    built = [FZ.realise(c) for c in BY[name]]
    redrawn = [b.case.id for b in built if b.redrawn]
    print(f"{name}: {len(redrawn)} of {len(built)} cases redrawn {redrawn}; loose chains {sum(len(b.loose) for b in built)}")
    assert len(redrawn) * 8 <= len(built), redrawn
    assert all(b.redrawn < FZ.REDRAWS for b in built)


def _axis(cases, i):
    return {p.split("/")[i] for c in cases for p in c.profile[:-1]}


@pytest.mark.parametrize("name", list(FZ.SPECS))
def test_every_axis_occurs(name):
    spec, cases = FZ.SPECS[name], BY[name]
    assert set(spec.geoms) <= _axis(cases, 0), set(spec.geoms) - _axis(cases, 0)
    assert set(spec.masks) <= _axis(cases, 1), set(spec.masks) - _axis(cases, 1)
    assert set(spec.rates) <= _axis(cases, 2) and set(FZ.COMPS) <= _axis(cases, 3) and set(spec.noises) <= _axis(cases, 4)
    forms = {c.form[0] for c in cases}
    assert {"padded", "clamped", "null"} <= forms and (("packed" in forms) == spec.packed)
    assert {c.profile[-1].split("/")[2] for c in cases} == {"wide", "small"}                  # outputs on 256 bytes and at unaligned offsets
    assert {(c.A, c.slot, c.param) for c in cases} >= set(spec.variants) and {c.A for c in cases} == {4, 14, 37}
    assert {len(c.lens) for c in cases} >= {1, 2, 3} and max(len(c.lens) for c in cases) >= 9
    lens = {m for c in cases for m in c.lens}
    T = spec.tile(spec.variants[0][0])
    assert {0, 1, 2, 3} <= lens and ({T - 1, T, T + 1, 2 * T, 2 * T + 1} <= lens or spec.waves)
    assert any(c.lens[0] == 0 for c in cases) and any(c.lens[-1] == 0 for c in cases)
    assert any(a == b == 0 for c in cases for a, b in zip(c.lens, c.lens[1:]))                # empty chains first, last and adjacent
    if name in FZ.PAIRED:
        assert {c.profile[-1].split("/")[0] for c in cases} == {"null", "mask"} and set(FZ.MPREDS) <= _axis(cases, 5)
    if name in FZ.WITH_AATYPE:
        assert {c.profile[-1].split("/")[1] for c in cases} == {"aatype", "noaatype"}
    # Uncovered packed rows: in front of row_off[0] and behind row_off[n] (R beyond it). Rows BETWEEN two chains, which the issue also names,
    # do not exist in this ABI: chain_range gives chain e the rows row_off[e] .. row_off[e + 1], so neighbours share their edge, and a
    # row_off that runs backwards in the middle makes ranges overlap, which the ABI forbids. There is nothing to assert for them.
    if spec.packed:
        assert any(c.form[0] == "packed" and c.form[1] > 0 and c.form[2] > 0 for c in cases) and any(c.form == ("packed", 0, 0) for c in cases)
    if name == "knn":                                                                          # k above and below the site count of a compact globule
        sites = [(c.param, s) for c in cases for s, p in zip(FZ.sites_of(FZ.build(c)), c.profile[:-1]) if p.startswith("globule") and s >= 2]
        assert any(k > s - 1 for k, s in sites) and any(k < s - 1 for k, s in sites), sites
    if name == "sasa":
        assert {c.param for c in cases} == {1, 92} and sum(c.param == 92 for c in cases) == 1


@pytest.mark.parametrize("name", [n for n, s in FZ.SPECS.items() if s.row_pass])
def test_row_pass_edges(name):
    for P in FZ.SPECS[name].row_pass:
        lens = {m for c in BY[name] if c.form[0] != "clamped" for m in c.lens}
        assert {P - 1, P, P + 1, 2 * P, 2 * P + 1} <= lens, (name, P)
        whole = [c for c in BY[name] for m, p in zip(c.lens, c.profile[:-1]) if m == P and p.split("/")[1:3] == ["all", "0"] and p.endswith("/equal")]
        assert {c.form[0] for c in whole} >= {"packed", "null"}, "a chain of exactly P rows whose every row, the last too, is a site"


@pytest.mark.parametrize("name", [n for n, s in FZ.SPECS.items() if s.atom_pass])
def test_atom_pass_edges(name):
    """for every layout: a chain whose first pass closes holding the most a pass of the layout can hold, one whose pass closes one slot
    under it, a chain that ends on that pass edge, one that goes on for a row, and one whose final pass stages nothing"""
    spec = FZ.SPECS[name]
    PASS, STEP = spec.pass_step
    seen = collections.defaultdict(set)
    top = {}
    for c in BY[name]:
        b = FZ.build(c)
        cand = FZ.candidate_slots(b.an)
        for e, m in enumerate(b.eff):
            if m == 0:
                continue
            atom = FZ.candidates(b, e)
            passes = FZ.pass_split(atom.sum(axis=1), c.A, PASS, STEP)
            kind = c.profile[e].split("/")[1]
            if kind.startswith("design"):
                c_row = int(cand[min(int(b.inp["aatype"][e, 0]), 20)].sum())
                top[c.A] = FZ.fullest_pass(c.A, c_row, PASS, STEP)
                assert passes == FZ.stage_slots_transcribed(atom, PASS, STEP), c.id
            first = passes[0][2]
            seen[c.A] |= {("staged", first)} | ({"ends on the edge"} if len(passes) == 1 and first > PASS - FZ.step_rows(c.A, STEP) * c.A else set())
            if len(passes) > 1:
                seen[c.A] |= {("behind", passes[1][1] - passes[1][0], passes[-1][2])}
    assert top == ({4: 1280, 14: 1280, 37: 1267} if name == "violation_loss" else {4: 1024, 14: 1024, 37: 1024} if name == "fape_atoms" else {4: G.ATOM_PASS, 14: G.ATOM_PASS, 37: G.ATOM_PASS if name == "lddt_atoms" else 1523}), top
    # chains that are NOT designed, through the mirror on the built inputs (the profile's name proves nothing): three passes and more, a
    # cleared run longer than any pass of the chain at its start and at its end with two staged passes beside it, a cleared run longer
    # than a staging step inside a chain, and a non-finite coordinate under a set mask in a pass' last row and in the next pass' first
    for A in (4, 14, 37):
        wild = set()
        for c in BY[name]:
            if c.A != A or c.group == "design":
                continue
            b = FZ.build(c)
            for e, m in enumerate(b.eff):
                if m == 0:
                    continue
                atom = FZ.candidates(b, e)
                per_row = atom.sum(axis=1)
                passes = FZ.pass_split(per_row, A, PASS, STEP)
                full = [p for p in passes if p[2]]
                live = np.flatnonzero(per_row)
                span = max(int(live[live < q][-1]) - int(live[live >= p][0]) + 1 for p, q, _ in full) if full else m      # rows from a pass' first atom to its last
                head, tail = (int(live[0]), m - 1 - int(live[-1])) if len(live) else (m, 0)
                gaps = np.diff(live) - 1 if len(live) > 1 else np.zeros(0, int)
                wild |= {("passes", min(len(full), 3))} | ({"head"} if len(full) >= 2 and head > span else set()) | ({"tail"} if len(full) >= 2 and tail > span else set())
                wild |= {"inner run"} if len(gaps) and gaps.max() > FZ.step_rows(A, STEP) else set()
                pos, mask = (b.inp["pt"], b.inp["mt"]) if "pt" in b.inp else (b.inp["pos_p"], b.inp["mask_p"]) if "pos_p" in b.inp else (b.inp["pos"], b.inp["mask"])
                mask = np.ones(pos.shape[:-1], np.uint8) if mask is None else mask
                with np.errstate(invalid="ignore"):                                          # (the all-atom FAPE: its family spoils a point's prediction there)
                    bad = ((mask[e, :m] != 0) & ~np.isfinite(pos[e, :m]).all(axis=-1)).any(axis=1)
                for _, end, _ in passes[:-1]:
                    wild |= ({"bad last row"} if bad[end - 1] else set()) | ({"bad first row"} if bad[end] else set())
        assert {("passes", 3), "head", "tail", "inner run", "bad last row", "bad first row"} <= wild, (name, A, sorted(map(str, wild)))
    for A in (4, 14, 37):
        assert {("staged", top[A]), ("staged", top[A] - 1), "ends on the edge"} <= seen[A], (A, sorted(map(str, seen[A])))
        assert any(s[0] == "behind" and s[1] == 1 for s in seen[A] if isinstance(s, tuple)), "a chain that goes on one row behind the pass edge"
        assert any(s[0] == "behind" and s[2] == 0 for s in seen[A] if isinstance(s, tuple)), "a final pass that stages nothing"


@pytest.mark.parametrize("name", [n for n, s in FZ.SPECS.items() if s.waves])
def test_wave_per_chain_chains(name):
    """chains of 0, 1, 2 and 3 sites with 200 rows at least, a coincident and a collinear chain of three sites or more"""
    few, geoms = set(), set()
    for c in BY[name]:
        b = FZ.build(c)
        for s, m, p in zip(FZ.sites_of(b), b.eff, c.profile[:-1]):
            if m >= 200:
                few.add(int(s))
            if s >= 3:
                geoms.add(p.split("/")[0])
    assert {0, 1, 2, 3} <= few and {"coincident", "collinear"} <= geoms, (few, geoms)
    if name == "tmscore":
        assert {FZ.TM_LDS_ROWS - 1, FZ.TM_LDS_ROWS, FZ.TM_LDS_ROWS + 1} <= {m for c in BY[name] for m in c.lens}


def test_the_mirror_is_the_transcription():
    """pass_split against chain_stage_slots line by line, on random masks of every density, for the three widths and for a pass and a
    step of other sizes"""
    rng = np.random.default_rng(5)
    for A in (4, 14, 37):
        for PASS, STEP in ((G.ATOM_PASS, FZ.ATOM_STEP), (G.VLOSS_PASS, FZ.VLOSS_STEP), (FA.FAPEA_PASS, FZ.FAPEA_STEP), (FZ.FAPEA_FRAME_PASS, FZ.FAPEA_FRAME_STEP), (1024, 256), (512, 512)):     # (1280, 512): a step that does not divide the pass
            for m in (0, 1, STEP // A - 1, STEP // A, STEP // A + 1, 3 * (PASS // A) + 7, int(rng.integers(1, 400))):
                for density in (0.0, 0.05, 0.5, 0.97, 1.0):
                    atom = rng.random((m, A)) < density
                    if m > 20:
                        r = int(rng.integers(m - 10))
                        atom[r:r + int(rng.integers(1, 200))] = bool(rng.integers(2))         # a run of empty or of full rows
                    got = FZ.pass_split(atom.sum(axis=1), A, PASS, STEP)
                    assert got == FZ.stage_slots_transcribed(atom, PASS, STEP), (A, PASS, STEP, m, density)
                    assert all(s <= PASS for _, _, s in got) and [a for a, _, _ in got[1:]] == [b for _, b, _ in got[:-1]]
                    assert sum(s for _, _, s in got) == int(atom.sum()) and (not got or (got[0][0] == 0 and got[-1][1] == m))


def test_the_mirror_is_the_transcription_of_the_frame_staging():
    """k_fape_atoms_grad_points stages FRAMES: rows of 8 groups (the divider fapea_div_groups), a pass of 256 and a step of 256, so a
    pass closes behind the first step that stages anything. Runs of empty rows of every length about a step make passes of several steps"""
    rng = np.random.default_rng(6)
    P = (FZ.FAPEA_FRAME_PASS, FZ.FAPEA_FRAME_STEP)
    assert FZ.step_rows(FA.GROUPS, P[1]) == 32
    for m in (0, 1, 31, 32, 33, 64, 65, 320, 333):
        for density in (0.0, 0.02, 0.5, 0.97, 1.0):
            for run in (0, 31, 32, 33, 64, 97):
                frame = rng.random((m, FA.GROUPS)) < density
                if run and m > run:
                    r = int(rng.integers(m - run + 1)) if rng.integers(2) else (m - run) // 32 * 32
                    frame[r:r + run] = False
                got = FZ.pass_split(frame.sum(axis=1), FA.GROUPS, *P)
                assert got == FZ.stage_slots_transcribed(frame, *P), (m, density, run)
                assert all(s <= P[0] and (s or q == m) for _, q, s in got) and sum(s for _, _, s in got) == int(frame.sum())
    assert FZ.pass_split([8] * 32 + [0] * 64 + [8] * 32, 8, *P) == [(0, 32, 256), (32, 128, 256)]


def test_a_designed_pass_closes_where_it_was_aimed():
    assert [FZ.fullest_pass(A, A, FA.FAPEA_PASS, FZ.FAPEA_STEP) for A in (4, 14, 37)] == [1024, 1024, 1024]           # (a point needs no radius: OXT counts)
    assert [len(FZ.design_counts(A, A, False, FA.FAPEA_PASS, FZ.FAPEA_STEP)[0]) for A in (4, 14, 37)] == [256, 108, 39]
    assert [FZ.pass_split([A] * 600, A, FA.FAPEA_PASS, FZ.FAPEA_STEP)[0][2] for A in (4, 14, 37)] == [1024, 1008, 962]     # what every mask set reaches
    for A in (4, 14, 37):                                                                     # the spread step keeps its total
        for short in (False, True):
            counts, target = FZ.design_counts(A, A, short, FA.FAPEA_PASS, FZ.FAPEA_STEP)
            spread = FZ.respread(counts, A, FZ.step_rows(A, FZ.FAPEA_STEP))
            assert FZ.pass_split(spread, A, FA.FAPEA_PASS, FZ.FAPEA_STEP) == [(0, len(counts), target)] and max(spread) <= A
    for P in ((G.ATOM_PASS, FZ.ATOM_STEP), (G.VLOSS_PASS, FZ.VLOSS_STEP), (FA.FAPEA_PASS, FZ.FAPEA_STEP)):
        for A, c_row in ((4, 4), (14, 14), (37, 36), (37, 37)):
            for short in (False, True):
                counts, target = FZ.design_counts(A, c_row, short, *P)
                assert target == FZ.fullest_pass(A, c_row, *P) - short and max(counts) <= c_row
                assert FZ.pass_split(counts, A, *P) == [(0, len(counts), target)]
                assert FZ.pass_split(counts + [c_row], A, *P) == [(0, len(counts), target), (len(counts), len(counts) + 1, c_row)]
                assert FZ.pass_split(counts + [0] * 50, A, *P)[-1][2] == 0
    assert [FZ.fullest_pass(A, c, G.VLOSS_PASS, FZ.VLOSS_STEP) for A, c in ((4, 4), (14, 14), (37, 36))] == [1280, 1280, 1267]


def test_the_mirrored_constants_are_the_headers_():
    """every constant the generator places an edge by, read from the kernels' headers (the GPU test asks the library for those it exports)"""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "foldcomp_amd", "csrc")

    def const(header, name):
        """`constexpr uint32_t NAME = <integer>;` or `= <integer> * BLOCK;`, with or without the u suffix"""
        text = open(os.path.join(csrc, header)).read()
        m = re.search(r"constexpr\s+uint32_t\s+" + name + r"\s*=\s*(?:(\d+)u?)?\s*\*?\s*(BLOCK)?\s*;", text)
        assert m and (m.group(1) or m.group(2)), (header, name)
        return int(m.group(1) or 1) * (G.BLOCK if m.group(2) else 1)

    def tile_rows(header, name):
        """`A == 37u ? 20u : A == 14u ? 18u : 64u` or `A == 4u ? 128u : 64u` behind the function's name -> {A: rows}"""
        text = open(os.path.join(csrc, header)).read()
        body = text[text.index("uint32_t " + name + "("):].split("}")[0]
        pairs = re.findall(r"A == (\d+)u \? (\d+)u", body)
        rest = int(re.search(r": (\d+)u;", body).group(1))
        return {A: dict((int(a), int(r)) for a, r in pairs).get(A, rest) for A in (4, 14, 37)}

    assert const("fcz_fape.h", "FAPE_FRAME_PASS") == G.FAPE_FRAME_PASS and const("fcz_fape.h", "FAPE_PASS") == G.FAPE_PASS
    assert const("fcz_tmscore.h", "TM_LDS_ROWS") == FZ.TM_LDS_ROWS
    assert const("fcz_sasa.h", "SASA_STEP") == const("fcz_violations.h", "VIOL_STEP") == const("fcz_lddt_atoms.h", "LDDTA_STEP") == FZ.ATOM_STEP
    assert const("fcz_sasa.h", "SASA_PASS") == const("fcz_violations.h", "VIOL_PASS") == const("fcz_lddt_atoms.h", "LDDTA_PASS") == G.ATOM_PASS
    assert (const("fcz_knn.h", "KNN_PASS"), const("fcz_lddt.h", "LDDT_PASS"), const("fcz_dssp.h", "HBOND_PASS")) == (G.KNN_PASS, G.LDDT_PASS, G.HBOND_PASS)
    assert const("fcz_violation_loss.h", "VLOSS_PASS") == G.VLOSS_PASS == FZ.SPECS["violation_loss"].pass_atoms
    assert const("fcz_violation_loss.h", "VLOSS_STEP") == FZ.VLOSS_STEP == FZ.SPECS["violation_loss"].step and G.VLOSS_PASS % FZ.VLOSS_STEP != 0
    spec = FZ.SPECS["fape_atoms"]
    assert const("fcz_fape_atoms.h", "FAPEA_PASS") == FA.FAPEA_PASS == spec.pass_atoms and const("fcz_fape_atoms.h", "FAPEA_STEP") == FZ.FAPEA_STEP == spec.step
    assert (const("fcz_fape_atoms.h", "FAPEA_FRAME_PASS"), const("fcz_fape_atoms.h", "FAPEA_FRAME_STEP")) == (FZ.FAPEA_FRAME_PASS, FZ.FAPEA_FRAME_STEP)
    assert const("fcz_fape_atoms.h", "FAPEA_GROUPS") == FA.GROUPS and FA.MAX_ITEMS == spec.max_items
    assert tile_rows("fcz_fape_atoms.h", "fapea_tile_rows") == {A: FA.fapea_tile_rows(A) for A in (4, 14, 37)} == {A: spec.tile(A) for A in (4, 14, 37)}
    assert tile_rows("fcz_lddt_atoms.h", "lddta_tile_rows") == {A: G.lddta_tile_rows(A, False) for A in (4, 14, 37)}           # the point tile of k_fape_atoms_grad_points
    assert const("fcz_sasa.h", "SASA_TILE_ROWS") == G.SASA_TILE_ROWS and const("fcz_lddt_atoms.h", "LDDTA_DECIDE_ROWS") == G.LDDTA_DECIDE_ROWS


# ---- the violation loss: a sweep that SUMS, so where a partner is staged matters -----------------------------------------------------------
VLOSS_TOPS = {4: 1280, 14: 1280, 37: 1267}
_PAIRS = {}


def _vloss_chain(c, e):
    """chain e of a violation-loss case through the restatement's dense matrices and the mirror -> dict: idx [N, 2] the atoms in
    ascending (row, slot), clash bool [N, N] (exclusions struck out), T and d [N, N], and of every atom the pass that stages it, its
    place in that pass and the staging step of the pass"""
    if (c, e) not in _PAIRS:
        b, spec = FZ.build(c), FZ.SPECS[c.analysis]
        m = b.eff[e]
        aa = None if b.inp["aatype"] is None else b.inp["aatype"][e, :m]
        idx, _, clash, T, d = VL._pairs(b.inp["pos"][e, :m], b.inp["mask"][e, :m], aa, V.default_table(c.A), b.an.params[0])
        assert np.array_equal(idx, np.argwhere(FZ.candidates(b, e)))
        passes = FZ.pass_split(np.bincount(idx[:, 0], minlength=m), c.A, *spec.pass_step)
        ends = np.asarray([q for _, q, _ in passes])
        in_pass = np.searchsorted(ends, idx[:, 0], side="right")
        first = np.searchsorted(idx[:, 0], [p for p, _, _ in passes])          # the atoms in front of every pass
        place = np.arange(len(idx)) - first[in_pass]
        step = (idx[:, 0] - np.asarray([p for p, _, _ in passes])[in_pass]) // FZ.step_rows(c.A, spec.step)
        assert all(place[in_pass == k].tolist() == list(range(s)) for k, (_, _, s) in enumerate(passes))
        _PAIRS[(c, e)] = dict(idx=idx, clash=clash, T=T, d=d, passes=passes, in_pass=in_pass, place=place, step=step)
    return _PAIRS[(c, e)]


def test_violation_loss_pairs_at_the_last_place():
    """for every layout, in the chain whose first pass closes at the fullest it can be and in the one that closes one slot under it: a
    clashing pair (no exclusion, a direction) whose partner is staged at the LAST place of that pass, and one whose partner sits at a
    place of 1024 or more; the hand-picked tests of the loss stage 1024 atoms a pass at the most"""
    seen = collections.defaultdict(set)
    for c in BY["violation_loss"]:
        if c.group != "design":
            continue
        ref = FZ.realise(c).ref
        for e in range(len(c.lens)):
            p = _vloss_chain(c, e)
            staged = p["passes"][0][2]
            last, other = staged - 1, FZ.PLANT_PLACE
            assert staged in (VLOSS_TOPS[c.A], VLOSS_TOPS[c.A] - 1) and 1024 <= other < last
            for j in (last, other):
                assert p["in_pass"][j] == 0 and p["place"][j] == j
                with np.errstate(invalid="ignore"):
                    moves = p["clash"][:, j] & (p["d"][:, j] != 0) & ((p["T"][:, j] - p["d"][:, j]) != 0)
                assert moves.any(), (c.id, e, j, "no clashing pair has its partner at this place")
                i = int(np.flatnonzero(moves)[0])
                assert p["idx"][i][0] != p["idx"][j][0] and ref["clash_loss"][(e,) + tuple(p["idx"][i])] > 0 and ref["grad"][(e,) + tuple(p["idx"][i])].any()
            seen[c.A].add(staged)
            print(f"A = {c.A}, {c.profile[e].split('/')[1]}: the pass stages {staged}, a partner at place {last} (row {p['idx'][last][0]}, slot {p['idx'][last][1]}) and at {other}")
    assert {A: s for A, s in seen.items()} == {A: {t, t - 1} for A, t in VLOSS_TOPS.items()}, dict(seen)


def test_violation_loss_sums_live_across_a_pass_edge():
    """for every layout, in a long chain: a query atom whose clash partners are staged by two passes at least (its sum register lives
    across the barrier that closes a pass), and a query atom with three partners and more inside one staging step"""
    for A in (4, 14, 37):
        across = within = 0
        for c in BY["violation_loss"]:
            if c.A != A or not c.group.startswith("long"):
                continue
            for e in range(len(c.lens)):
                p = _vloss_chain(c, e)
                in_passes = np.stack([p["clash"][:, p["in_pass"] == k].any(axis=1) for k in range(len(p["passes"]))])
                across += int((in_passes.sum(axis=0) >= 2).sum())
                key = p["in_pass"] * 1000 + p["step"]
                within += sum(int((p["clash"][:, key == k].sum(axis=1) >= 3).sum()) for k in np.unique(key))
        print(f"A = {A}: {across} query atoms with partners in two passes and more, {within} (atom, step) with three partners and more")
        assert across and within, (A, across, within)


def _sg_pairs(b, e):
    """the SG - SG pairs of two CYS rows of chain e that pass the distance test and are struck out as disulfides"""
    A, m = b.case.A, b.eff[e]
    if A == 4 or b.inp["aatype"] is None or m < 2:
        return 0
    aa, pos = b.inp["aatype"][e, :m], b.inp["pos"][e, :m]
    atom, radius = VL.atoms_of(pos, b.inp["mask"][e, :m], aa, V.default_table(A))
    rows = np.flatnonzero(atom[:, V.SG_SLOT[A]] & (aa == V.CYS))
    sg, R = pos[rows, V.SG_SLOT[A]], radius[rows, V.SG_SLOT[A]]
    T = (R[:, None] + R[None, :]) - b.an.params[0]
    with np.errstate(over="ignore", invalid="ignore"):
        return int(((T > 0) & (V._d2(sg[:, None], sg[None, :]) < T * T) & ~np.eye(len(rows), dtype=bool)).sum()) // 2


def test_violation_loss_term_classes():
    """over the list, at tolerance 0 and factor 0.5: clash terms and each of the three link terms above 0 in every layout, a PRO link
    with a term above 0, a coincident chain (every pair at d == 0: the value is the sum of the T in sequence, the gradient 0), and in
    atom14 and atom37 an SG - SG pair of two CYS rows inside the clash distance, which is struck out. Every restated value and
    gradient of every case, at either parameter set, is finite: the comparison on bits never rests on the payload of a NaN"""
    terms, pro, sg, still = collections.defaultdict(set), 0, collections.Counter(), 0
    assert {c.param for c in BY["violation_loss"]} == {0, 1}
    for c in BY["violation_loss"]:
        b = FZ.realise(c)
        assert b.redrawn == 0 and all(np.isfinite(v).all() for v in b.ref.values()), c.id
        if c.param:
            continue
        terms[c.A] |= ({"clash"} if (b.ref["clash_loss"] > 0).any() else set()) | {k for k in range(3) if (b.ref["link_loss"][..., k] > 0).any()}
        for e, m in enumerate(b.eff):
            sg[c.A] += _sg_pairs(b, e)
            if b.inp["aatype"] is not None and m > 1:
                pro += int(((b.inp["aatype"][e, 1:m] == V.PRO) & (b.ref["link_loss"][e, :m - 1] > 0).any(axis=-1)).sum())
            if c.profile[e].startswith("coincident/") and b.ref["counts"][e, 0] >= 2:
                p = _vloss_chain(c, e)
                if p["clash"].any():
                    assert (p["d"][p["clash"]] == 0).all() and not b.ref["grad"][e].any()
                    want = VL._seq_sum(np.where(p["clash"], p["T"], np.float32(0)))
                    assert np.array_equal(b.ref["clash_loss"][e][p["idx"][:, 0], p["idx"][:, 1]], want) and (want > 0).any()
                    still += 1
    print(f"PRO links with a term: {pro}; SG - SG pairs struck out: {dict(sg)}; coincident chains: {still}")
    assert all(terms[A] == {"clash", 0, 1, 2} for A in (4, 14, 37)), dict(terms)
    assert pro and still and sg[14] and sg[37], (pro, still, dict(sg))


def test_violation_loss_weights():
    """w_clash and w_link: exact zeros, both signs, one value of 1e15 in magnitude each in a case with atoms and links, and a NaN bit
    pattern exactly where the restatement has no atom and no link; packed, the uncovered rows are finite"""
    for c in BY["violation_loss"]:
        b = FZ.build(c)
        inp = b.inp
        for e, m in enumerate(b.eff):
            atom = FZ.candidates(b, e)
            assert np.array_equal(np.isnan(inp["w_clash"][e, :m]), ~atom) and np.isnan(inp["w_clash"][e, m:]).all()
            exist = VL._links(inp["pos"][e, :m], inp["mask"][e, :m], None if inp["aatype"] is None else inp["aatype"][e, :m], b.an.params[1])["exist"] if m > 1 else np.zeros(0, bool)
            assert np.array_equal(~np.isnan(inp["w_link"][e, :max(m - 1, 0)]).any(axis=-1), exist) and np.isnan(inp["w_link"][e, max(m - 1, 0):]).all()
        for k in ("w_clash", "w_link"):
            w = inp[k][~np.isnan(inp[k])]
            if len(w) > 100:
                assert (w == 0).any() and (w > 0).any() and (w < 0).any() and (np.abs(w) == FZ.BIG_WEIGHT).sum() == 1, (c.id, k)
            if b.packed:
                assert all(np.isfinite(a).all() for a in (lambda f: (f[:c.form[1]], f[len(f) - c.form[2]:]))(FZ.form_arrays(b, {k: inp[k]})[k]))


def test_tmalign_pairs():
    """two fuzzed sets of chains of 120 rows or under in both forms, with chains of 0 to 3 rows and of 0 to 3 sites, related and unrelated
    partners, and every pair alone in the list of its case"""
    cases = BY["tmalign"]
    assert {c.form[0] for c in cases} == {"padded", "packed"} and any(c.form[0] == "packed" and c.form[1] and c.form[2] for c in cases)
    lens = {m for c in cases for m in c.lens}
    assert {0, 1, 2, 3, 120} <= lens and max(lens) <= 120
    assert {p.split("/")[5] for c in cases for p in c.profile[:-1]} == {"related", "unrelated"}
    sites = set()
    for c in cases:
        b = FZ.realise(c)
        assert b.wb <= 125 and len(b.pairs) > len(c.lens) and (b.ref["status"] == 0).all()
        sites |= set(b.ref["sites_a"].tolist()) | set(b.ref["sites_b"].tolist())
    assert {0, 1, 2, 3} <= sites and max(sites) >= 100 and sum(int((FZ.realise(c).ref["aligned"] >= 3).sum()) for c in cases) >= 12


# ---- the all-atom FAPE: two stagings (points in passes of 1024, frames in passes of 256) and rounds of BLOCK over a tile's list -------------
FA_PASS = (FA.FAPEA_PASS, FZ.FAPEA_STEP)
FA_FRAME_PASS = (FZ.FAPEA_FRAME_PASS, FZ.FAPEA_FRAME_STEP)


def _fa_chains(head, groups=("design",)):
    """(case, Built with its restatement, chain, rows) of every chain of the all-atom FAPE whose mask kind begins with `head`"""
    for c in BY["fape_atoms"]:
        if c.group in groups:
            for e, p in enumerate(c.profile[:-1]):
                if p.split("/")[1].split("-")[0] == head:
                    b = FZ.realise(c)
                    yield c, b, e, b.eff[e]


def _fa_alone(b, e, m, **changed):
    """the restatement of chain e alone with some of its arrays replaced"""
    c = dict(FZ.fapea_chain(b.inp, e, m), **{k: v for k, v in changed.items() if k != "w"})
    return FA.chain(c, changed.get("w", b.inp["w"][e, :m]), b.an.clamp)


def test_fape_atoms_designed_point_passes():
    """for every layout: the first pass of the designed chains stages exactly 1024 and 1023 of the restatement's points (never the
    masks: a swapped row reads the truth through the partner table), the second begins where designed, with the four tails. Clearing
    the point at the LAST place of that pass moves the restated sum of every frame of the chain by more than the frame's bound, a
    gradient of one frame at least by more than its bound, and takes away a grad_pos above its b_pos"""
    seen = collections.defaultdict(set)
    for c, b, e, m in _fa_chains("design"):
        _, short, tail = c.profile[e].split("/")[1].split("-")
        ref, inp = b.ref, b.inp
        point, frame = ref["point"][e, :m], ref["frame"][e, :m]
        assert np.array_equal(point, FZ.candidates(b, e)) and b.redrawn == 0
        rows, target = len(FZ.design_counts(c.A, c.A, short == "short", *FA_PASS)[0]), 1024 - (short == "short")
        passes = FZ.pass_split(point.sum(axis=1), c.A, *FA_PASS)
        assert passes == FZ.stage_slots_transcribed(point, *FA_PASS) and passes[0] == (0, rows, target), (c.id, passes)
        assert m == rows + FZ.DESIGN_TAILS[tail]
        if tail == "end":
            assert len(passes) == 1
        elif tail == "plus1":
            assert passes[1:] == [(rows, rows + 1, c.A)]
        elif tail == "empty":
            assert passes[1:] == [(rows, m, 0)]
        else:
            assert passes[1][0] == rows and passes[1][2] > 0
        if c.A != 4:                                                                           # in the step that is spread: swapped rows whose points are not the slots the truth's mask has set
            sw = (inp["swapped"][e, :m] != 0) & np.isin(inp["aatype"][e, :m], FZ.SWAP_TYPES)
            renamed = sw & (point != (inp["mask_t"][e, :m] != 0)).any(axis=1) & (point.sum(axis=1) == (inp["mask_t"][e, :m] != 0).sum(axis=1))
            assert renamed[:rows].sum() >= 2, (c.id, int(renamed.sum()))
        r, a = np.argwhere(point)[target - 1]
        assert r < rows and np.argwhere(point)[target - 1:target + 1].tolist()[-1][0] >= r
        mp = inp["mask_p"][e, :m].copy()
        mp[r, a] = 0
        less = _fa_alone(b, e, m, mask_p=mp)
        assert int(less["point"].sum()) == int(point.sum()) - 1 and frame.sum() >= 100
        assert (np.abs(less["sum"] - ref["sum"][e, :m])[frame] > ref["b_sum"][e, :m][frame]).all(), (c.id, "a frame's sum does not show the last place")
        moved = (np.abs(less["grad_rot"] - ref["grad_rot"][e, :m]).max(axis=(-1, -2)) > ref["b_rot"][e, :m]) | (np.abs(less["grad_trans"] - ref["grad_trans"][e, :m]).max(axis=-1) > ref["b_trans"][e, :m])
        assert (moved & frame).any() and np.abs(ref["grad_pos"][e, r, a]).max() > ref["b_pos"][e, r, a] > 0, (c.id, "no gradient shows the last place")
        seen[c.A].add((target, tail))
        print(f"A = {c.A}, {short}-{tail}: the pass stages {target}, the last place is row {r} slot {a}; {int(moved.sum())} of {int(frame.sum())} frames' gradients show it")
    assert dict(seen) == {A: {(1024, "end"), (1024, "empty"), (1023, "plus1"), (1023, "more")} for A in (4, 14, 37)}, dict(seen)


def test_fape_atoms_designed_frame_passes():
    """for every layout, through the mirror at (256, 256) on the restatement's frames: a full pass (256; backbone4 64: 32 rows x groups 0
    and 3) right behind two steps that stage nothing, at the chain's start and again in its middle, a pass one frame short of full, a
    pass of one frame, and a final pass that stages nothing. The weight of the frame at the last place of every pass moves grad_pos of
    a point by more than its b_pos (grad_pos is linear in w: the restatement of that frame alone is its share)"""
    done = set()
    for c, b, e, m in _fa_chains("fpass"):
        ref, top = b.ref, 64 if c.A == 4 else 256
        frame, point = ref["frame"][e, :m], ref["point"][e, :m]
        per_row = frame.sum(axis=1)
        passes = FZ.pass_split(per_row, FA.GROUPS, *FA_FRAME_PASS)
        assert passes == FZ.stage_slots_transcribed(frame, *FA_FRAME_PASS)
        assert passes == [(0, 96, top), (96, 128, top - 1), (128, 160, 1), (160, 256, top), (256, 320, 0)] and m == 320, (c.id, passes)
        assert [int(per_row[s:s + 32].sum()) for s in range(0, m, 32)] == list(FZ.frame_steps(c.A))
        at, first = np.argwhere(frame), 0
        for _, _, staged in passes[:-1]:
            first += staged
            r, g = at[first - 1]
            only = np.zeros((m, FA.GROUPS), np.uint8)
            only[r, g] = 1
            share = _fa_alone(b, e, m, fm_t=only)
            assert share["frame"].sum() == 1 and b.inp["w"][e, r, g] != 0
            shows = (np.abs(share["grad_pos"]).max(axis=-1) > ref["b_pos"][e, :m]) & point
            assert shows.any(), (c.id, "the frame at place", staged - 1, "moves no point")
        done.add(c.A)
    assert done == {4, 14, 37}


def test_fape_atoms_rounds():
    """chains of ONE tile whose list ends on the edges of a wavefront and of a round of BLOCK: frames in a frame tile of atom14, points
    in a point tile of atom37, 256 of each in backbone4; counted on the restatement"""
    frames = {(c.A, int(b.ref["frame"][e].sum())) for c, b, e, m in _fa_chains("rndf") if m == FA.fapea_tile_rows(c.A)}
    points = {(c.A, int(b.ref["point"][e].sum())) for c, b, e, m in _fa_chains("rndp") if m == G.lddta_tile_rows(c.A, False)}
    assert frames == {(14, q) for q in (1, 63, 64, 65, 255, 256, 257, 512)} | {(4, 256)}, frames
    assert points == {(37, q) for q in (1, 64, 65, 256, 257, 512, 513, 740)} | {(4, 256)}, points
    assert G.lddta_tile_rows(37, False) * 37 == 740 and FA.fapea_tile_rows(14) * FA.GROUPS == 512 and G.BLOCK == 256


def test_fape_atoms_inputs():
    """over the list: the weights hold a NaN pattern exactly where the restatement has no frame and behind every length, zeros, both
    signs and one 3e19 outside the designed chains; cases without aatype (and so without swapped), with aatype and without swapped,
    without mask_pred and fmask_pred; non-finite values under set masks in trans, rot and both pos; no tie on an integer chain and a
    share of 0.02 at the most; every chain within MAX_ITEMS (the restatement asserts it); a swapped row of a type with partners whose
    points are not its mask's slots next to a pass edge"""
    kinds, bad, big, at_edge = set(), set(), 0, 0
    for c in BY["fape_atoms"]:
        b = FZ.realise(c)
        inp, ref = b.inp, b.ref
        assert FA.tie_share(ref) <= FZ.TIE_SHARE
        kinds.add(("aatype", inp["aatype"] is not None, "swapped", inp["swapped"] is not None, "pred masks", inp["mask_p"] is not None))
        assert (inp["mask_p"] is None) == (inp["fm_p"] is None) and not (inp["swapped"] is not None and inp["aatype"] is None)
        for e, m in enumerate(b.eff):
            assert np.array_equal(np.isnan(inp["w"][e, :m]), ~ref["frame"][e, :m]) and np.isnan(inp["w"][e, m:]).all()
            if m == 0:
                continue
            if c.profile[e].split("/")[0] in FZ.EXACT:
                assert not ref["tie_f"][e].any() and not ref["tie_p"][e].any(), (c.id, e)
            with np.errstate(invalid="ignore"):
                fm = (inp["fm_t"][e, :m] != 0) & (True if inp["fm_p"] is None else inp["fm_p"][e, :m] != 0)
                for k in ("trans_t", "trans_p", "rot_t", "rot_p"):
                    bad |= {k[:-2]} if (fm & ~np.isfinite(inp[k][e, :m]).reshape(m, FA.GROUPS, -1).all(axis=-1)).any() else set()
                for k, mk in (("pos_t", "mask_t"), ("pos_p", "mask_p")):
                    bad |= {k} if inp[mk] is not None and ((inp[mk][e, :m] != 0) & ~np.isfinite(inp[k][e, :m]).all(axis=-1)).any() else set()
            if inp["swapped"] is not None and c.A != 4 and m:
                point, mask = ref["point"][e, :m], inp["mask_t"][e, :m] != 0
                renamed = (inp["swapped"][e, :m] != 0) & np.isin(inp["aatype"][e, :m], FZ.SWAP_TYPES) & (point & ~mask).any(axis=1)
                for _, end, _ in FZ.pass_split(point.sum(axis=1), c.A, *FA_PASS)[:-1]:
                    at_edge += int(renamed[max(end - 2, 0):end + 2].any())
        w = inp["w"][~np.isnan(inp["w"])]
        big += int((np.abs(w) == np.float32(3e19)).sum())
        assert (np.abs(w) == np.float32(3e19)).sum() <= 1
        if len(w) > 100:
            assert (w == 0).any() and (w > 0).any() and (w < 0).any(), c.id
    print(f"kinds {sorted(kinds)}; non-finite under set masks in {sorted(bad)}; cases with a 3e19 weight {big}; renamed rows at a pass edge {at_edge}")
    got = {k[1::2] for k in kinds}
    assert (True, True, True) in got and any(not k[0] for k in got) and any(k[0] and not k[1] for k in got) and any(not k[2] for k in got), sorted(kinds)
    assert bad == {"trans", "rot", "pos_t", "pos_p"} and big >= 8 and at_edge >= 3, (bad, big, at_edge)
