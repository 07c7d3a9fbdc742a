"""A seeded differential fuzz of the dense-tensor analyses over what their kernels' control flow depends on: masks,
residue types, non-finite values, geometry, lengths about every tile and pass edge, and the padded / packed forms. The generator is
here; tests/test_gpu_analysis_fuzz.py runs it on the device, tests/test_analysis_fuzz_cpu.py asserts what the list covers, and
tools/dbg/analysis_fuzz.py runs it at any seed and case count.

A CASE is (analysis, A, slot, param, form, lens, profile, seed, group): `Case(*tuple)` rebuilds it and `build` draws its inputs from
nothing else. `profile` holds one string a chain, "geometry/mask/non-finite rate/composition/noise/mask_pred kind", and a last one
for the case: "null" or "mask" (is mask_pred passed), "aatype" or "noaatype", and the guard, "wide" (outputs on 256 bytes) or
"small" (at unaligned offsets). The inputs come from `Analysis.fuzz_pool` (tests/_sweep_grids.py), which calls `draw` below. The
restatement, the device call and the comparator with its bounds are the analysis' own (`ref`, `run`, tests/_*.py).

What a case asserts on the device (`drive`):
  WRITTEN    no output unit keeps its 0xA5 fill, the guards survive (the run_* helpers), and every row outside every chain holds the
             restatement's empty-row value on bytes;
  ALONE      every non-empty chain run alone in the same form gives the bytes it gave in the batch (packed indices rebased);
  REFERENCE  the batch against the restatement under the analysis' comparator.
A comparator that needs a margin of its inputs gets it by redrawing the case with the next seed, on the CPU, from the restatement
alone (`realise`): the Horn gap and threshold margins of _superpose.py / _tmscore.py / _gdt.py, the conditions of
_tmalign.fairness, the tie share (<= 0.02) of _lddt_soft.py / _fape.py. No comparator is loosened.

The pass split of chain_stage_slots (fcz_chains.h) is mirrored in `pass_split` and transcribed line by line in
`stage_slots_transcribed`; the CPU test holds the two together on random masks.
  * `design_counts` uses the arithmetic to build chains whose pass closes at the fullest it can be, one slot under it, on the
    chain's last row, and with a final pass that stages nothing.
  * Chains that are NOT designed take three passes and more in the long4 / long14 / long37 groups. There atom_inputs clears, through
    pass_split on the chain's own candidates, a run longer than any of its passes at its start or end, and puts a non-finite value
    into the last row of every pass and the first row of the next.
  * 1 to 3 sites "either side of a pass edge" exist for the row-pass sweeps only: a pass of chain_stage_slots closes on a staged
    count, so a chain of three atoms has one pass whatever rows they sit in.

The fullest pass by layout. PASS is 1536, a step examines step_rows = 512 / A rows, and the pass closes when another step might
not fit (staged + step_rows * A > PASS). backbone4 and atom14 reach 1536 (every slot of a TRP row is an atom). All-atom lDDT
reaches it on atom37 too (a candidate needs no radius). SASA and violations on atom37 reach 1055 + 13 * 36 = 1523, because OXT
holds no radius. `design_counts` aims at that maximum and the CPU test asserts it through the mirror.

The violation loss (fcz_violation_loss.h) has a pass of its own, `Spec.pass_atoms` = VLOSS_PASS = 1280 with the same step of 512,
which does not divide it, and stages through chain_stage_slots_ordered: the same steps and the same rule that closes a pass, the
places handed out in ascending (row, slot) by a ballot and a scan, because its outputs are float32 sums in that order. The mirror and
the transcription take PASS and STEP and are held together at (1280, 512) as well. Its fullest passes are 1280 (backbone4), 1280
(atom14, TRP rows) and 1280 - 13 * 37 + 13 * 36 = 1267 (atom37). With every mask set a pass closes at 1024 / 1008 / 936, so places
1024 to 1279 of the staging arrays are reached by designed masks only. A sweep that sums can also go wrong by WHERE a partner is
staged, so the designed chains of this analysis get two planted pairs (`plant_last_place`): the atom at the last place of the first
pass (1279 / 1279 / 1266, one less in the chains that close one slot under the top) and the atom at place 1100 are moved next to
atoms of row 0. Its family (`vloss_inputs`) adds the upstream weights: normal, a tenth zeros, one +-1e15 each, and NaN bit patterns
wherever the contract reads no weight, the sets taken from the restatement. It runs at two parameter sets, `Case.param` 0 (tolerance
0, factor 0.5: every term class occurs) and 1 (the defaults 1.5, 12.0); the comparator is _violation_loss.same, integers equal and
floats on bits, with nothing redrawn. It keeps the `coincident` geometry that `violations` drops: the loss defines a value (T) and
the gradient 0 at d == 0. The CPU test asserts through the restatement: the planted partners' places, a query atom whose partners
lie in two passes and one with three partners in a staging step in every layout's long chains, every term class, a PRO link, a
disulfide struck out (`plant_disulfide`), and that every restated number is finite.

The all-atom FAPE (fcz_fape_atoms.h: k_fape_atoms, k_fape_atoms_grad_frames, k_fape_atoms_grad_points) has TWO stagings through
chain_stage_slots_ordered and takes both through the mirror.
  * POINTS: FAPEA_PASS = 1024 with the step of 512 (`Spec.pass_atoms`, `Spec.step`). A point needs no radius and OXT counts, so the
    fullest pass is 1024 in all three layouts. With every mask set a pass closes at 1024 (backbone4), 2 * 36 * 14 = 1008 (atom14) and
    2 * 13 * 37 = 962 (atom37), so places 1008 / 962 to 1023 of the six staging arrays are reached by designed masks only:
    design_counts(A, A, short, 1024, 512) gives 256, 108 and 39 rows. Its one step that is neither whole nor empty is spread over
    the step's rows (`respread`), and every second row of it is a swapped ASP / GLU / PHE / TYR row that holds one slot of a partnered
    pair and lacks the other: which slot is a point then rests on the partner's mask, and the CPU test takes the points from the
    restatement's `point`, never from the masks. The point at the pass' last place (1023, or 1022 one slot under the top) is planted
    (`plant_last_point`): its prediction sits on the lattice where its term with every frame of the chain is 3 at least, above every
    b_sum a chain within the item cap can have, and below the clamp with one frame at least, whose weight is set.
  * FRAMES of k_fape_atoms_grad_points: FAPEA_FRAME_PASS = 256 with a step of 256 items (32 rows of 8 groups, the divider
    fapea_div_groups), mirrored as pass_split(counts, 8, 256, 256). A pass closes behind the first step that stages anything, so it
    spans more than a step only behind steps that stage nothing. `frame_steps` lays out: two such steps, a full pass (256; backbone4
    64, 32 rows of groups 0 and 3), a pass one frame short, a pass of ONE frame, two empty steps and a full pass again, and two
    empty steps that leave a final pass of nothing. The frame at every pass' last place carries a set weight.
  * ROUNDS: a tile's frames or points are compacted into a list and taken in rounds of BLOCK, a wavefront without an item skipping
    the sweep. Chains of one tile hold 1, 63, 64, 65, 255, 256, 257 and 512 frames (atom14: 64 rows of 8) and 1, 64, 65, 256, 257,
    512, 513 and 740 points (atom37: 20 rows of 37), backbone4 256 of each.
Its family (`fape_atoms_inputs`) draws the points as the all-atom lDDT's family does and the frames as the backbone FAPE's, with
aatype / swapped / mask_pred / fmask_pred each NULL somewhere, non-finite values either side of every pass edge of the chain's own
points, a swapped row that lacks a partner slot there too, and weights with NaN patterns at every item that is no frame. The item cap:
the bounds of _fape.py rest on at most _fape_atoms.MAX_ITEMS = 2181 points and as many frames a chain (the restatement asserts it), so
`Spec.max_items` keeps a chain of a MIX at 2181 / A rows (58 in atom37) and the long chains are sized for it: a cleared run of a pass
and a row and then some 2 050 points (780 / 220 / 82 rows), a chain under a subset mask_pred (1 000 / 300 / 110 rows) and one that
keeps half its rows (900 / 260 / 90). Chains of more than 128 rows are on the lattice (no tie); `restate` asks a tie share of 0 of every
chain on an integer geometry and of 0.02 at the most of the case.

What the packed ABI cannot express: rows BETWEEN two chains that no chain covers. Chain e is row_off[e] .. row_off[e + 1], so two
neighbours share their edge, and a row_off that runs backwards in the middle makes ranges overlap, which the ABI forbids. Uncovered
rows are in front of row_off[0] and behind row_off[n] (k_chain_fill writes both); the fuzz has both and R beyond row_off[n].

Profiles dropped by name, with the reason:
  fape_atoms x rate 0.05  fape's reason below; 1 % stays, with the first and last row and both sides of every pass edge besides.
  fape_atoms x +-3e19 in rot
                          fape's reason below.
  fape_atoms x +-3e19 on the integer geometries
                          a +-3e19 origin and a +-3e19 point cancel to a finite term whose bound is huge, a tie, and an integer chain
                          is asked a tie share of exactly 0. The noisy geometries keep all five values in trans and in both pos.
  fape_atoms x long noisy chains
                          head_pass, tail_pass and iid50 of long4 / long14 / long37 and the designed chains are on the lattice, not
                          on a helix: _fape_atoms.py measured the tie share of noisy chains up to 128 rows only.
  fape_atoms x no aatype with swapped
                          the ABI refuses swapped without aatype; no aatype and no swapped, and aatype without swapped, both run.
  fape x rate 0.05        a +-3e19 origin and a +-3e19 point cancel in e = l - l' to a finite term whose bound is huge: an honest tie
                          allowance (_fape.py), and at 5 % of the rows the share of such rows passes 0.02 at every seed. 1 % stays.
  fape x +-3e19 in rot    a finite entry that is no rotation's: _fape.py derives its bounds for columns of unit length. rot takes NaN
                          and +-inf (no frame), trans takes all five.
  lddt_soft x noise 0     a rigid motion of the truth leaves every delta at about 1e-6, inside the sign-tie band: at noise 0 the
                          prediction is the truth itself (delta exactly 0) for this analysis.
  tmscore, gdt x noise 0  every seed then reaches the same score on another selection, so the winner is not unique (condition b).
  superpose, tmscore, gdt, tmalign x +-3e19
                          a finite site whose square overflows float32; their pools hold NaN and +-inf only.
  superpose, tmscore, gdt x a trans component that cancels to 0
                          (an integer motion with a zero shift) 2 ulps of a value that is 0 but for rounding are no bound: the case
                          is redrawn, and the exact motions shift by non-zero integers.
  superpose, tmscore, gdt x coincident, collinear and line chains of three sites or more
                          the minimiser is not unique (Horn gap 0), so such a chain is `loose`: its rot and trans, and the seed and
                          selection a search won with, are not compared; a proper rotation is asserted, and rmsd, dev, tm and the
                          counts of the minimum are held to the restatement as ever.
  superpose, tmscore, gdt x helix
                          a long ideal helix is nearly a line (Horn gap under 1e-3 from some 150 rows): their chains walk.
  tmalign x geometry      the integer and degenerate geometries tie exactly or have a Horn gap of 0 at every seed, a long ideal helix
                          is nearly a line, and a plane of 120 rows misses the gap one seed in two: its chains walk or fill a globule.
  frames x no aatype      with groups = all the ABI refuses a NULL aatype; the backbone group runs without.
  sasa, violations, violation_loss x no aatype on atom14
                          refused too (a slot's atom depends on the type there); atom37 and backbone4 run without.
  apply x non-finite      the payload of a NaN result is not part of the contract and the comparison is on bytes (Apply's docstring).
  violations x coincident link_cos of a link of coincident atoms is 0 / 0, a NaN whose sign bit is no part of the contract, and
                          same_violations compares bits.
  frames x form, geometry padded only (the ABI has no packed form); geometry beyond the helix and the lattice adds nothing to a
                          per-row kernel and is left out.

Sizing. `an.ref` measured on the build machine's CPU, seconds for one chain of the stated rows with every mask set:
  knn 4097: 0.25          lddt 2049: 0.07         lddt_soft 2049: 0.99       hbond 961: 0.06       fape 1025: 0.88, 2049: 3.4
  sasa 150 x atom14: 0.06         violations 150 x atom14: 0.04         lddt_atoms 120 x atom14: 0.07         superpose 300: < 0.01
  tmscore 300: 0.16, 1025: 0.8    gdt 120: 0.35 (a coincident or collinear chain of 30 rows: 20 s, so GDT's take 12 rows)
Building the inputs costs as much again (an ideal helix of 4 097 rows: 1.0 s). The counts that follow, as cases (seconds of build
and restatement of an (analysis, group) test), 275 cases in all:
  knn 18 (passes 2.5, the rest 0.3)      lddt 17 (passes 0.8)      lddt_soft 17 (passes 2.5)      hbond 17 (0.6)      labels 10 (0.7)
  apply 12 (0.7)      frames 12 (0.8)      fape 24 (passes256 1, passes1024 5 with seven cases to 2 049 rows, the rest 0.5)
  sasa 20, violations 19, lddt_atoms 19 (design 1.4, mix 0.8, each of long4 / long14 / long37 0.5 to 1.6 with four chains of
  1 250, 640 and 150 rows at the most)      superpose 13 (< 0.1)      tmscore 16 (long 1.7)      gdt 13 (0.5)      tmalign 4 (3.0)
  violation_loss 19: its restatement holds dense atoms x atoms matrices of a whole chain, so the long chains are those of the other
  sweeps times 1280 / 1536 (1 050, 540 and 125 rows at the most; each still takes three passes and more) and the six designed cases
  run at parameter set 0 only: edges 0.1, design 3.5, long4 3.6, long14 3.4, long37 3.5, mix 4.7
  fape_atoms 25: a restatement costs frames x points, so the designed point chains keep some 150 frames and the designed frame chains
  some 600 points: edges 2.2 (a chain of 129 rows with every mask set), design 2.6 (twelve cases), long4 2.1, long14 1.9, long37 0.8,
  mix 1.3
Every test stays under about 5 s of restatement. A MIX case has up to 9 chains of at most `cap` rows."""
import dataclasses
import zlib

import numpy as np

import _analysis as AN
import _dssp as DS
import _fape as FP
import _fape_atoms as FA
import _gdt as GD
import _lddt_atoms as LA
import _lddt_soft as S
import _sasa as SA
import _superpose as SP
import _sweep_grids as G
import _tmalign as TA
import _tmscore as TM
import _violation_loss as VL
import _violations as V
from _devpath import FILL, GUARD, to_dev

F = np.float32
ATOM_STEP = 2 * G.BLOCK         # fcz_sasa.h SASA_STEP = fcz_violations.h VIOL_STEP = fcz_lddt_atoms.h LDDTA_STEP = 2 * BLOCK
VLOSS_STEP = 2 * G.BLOCK        # fcz_violation_loss.h VLOSS_STEP = 2 * BLOCK: it does not divide VLOSS_PASS = 1280
FAPEA_STEP = 2 * G.BLOCK        # fcz_fape_atoms.h FAPEA_STEP = 2 * BLOCK: the points, two slots a lane; FAPEA_PASS = 1024 = _fape_atoms.FAPEA_PASS
FAPEA_FRAME_PASS = 256          # fcz_fape_atoms.h: constexpr uint32_t FAPEA_FRAME_PASS = 256, the frames k_fape_atoms_grad_points stages a pass
FAPEA_FRAME_STEP = G.BLOCK      # fcz_fape_atoms.h FAPEA_FRAME_STEP = BLOCK: 32 rows of 8 groups a step, so a pass closes once a step has staged anything
TM_LDS_ROWS = 1024              # fcz_tmscore.h: constexpr uint32_t TM_LDS_ROWS = 1024
TIE_SHARE = 0.02                # _lddt_soft.py / _fape.py: tie_share() must stay at or below 0.02 on every noisy input
GLY, LEU, TRP, ALA = 7, 10, 17, 0

GEOMS = ("helix", "lattice", "globule", "line", "coincident", "collinear", "coplanar")
WAVE_GEOMS = ("walk",) + GEOMS[1:]        # a long ideal helix is nearly a line (Horn gap under 1e-3 from some 150 rows): the superpositions walk
MASKS = ("all", "iid1", "iid10", "iid50", "iid99", "runs1", "runs8", "runs64", "runs400", "head", "tail", "none", "one_first", "two_last", "three_edge",
         "bb_only", "side_only", "no_slot")
LIVE = ("all", "iid1", "iid10", "runs8", "iid50", "runs64", "head", "tail")
FEW = ("zero_long", "one_first", "one_last", "two_last", "three_edge", "three_any")
RATES = ("0", "0.01", "0.05")
COMPS = ("gly", "big", "mid", "unknown", "255", "mix", "alternate")
NOISES = ("0", "0.05", "1.5")
MPREDS = ("equal", "subset", "disjoint")           # per chain; the case says whether mask_pred is passed at all ("mask") or NULL ("null")


def crc(s):
    return zlib.crc32(s.encode())


# ---- chain_stage_slots, mirrored and transcribed ---------------------------------------------------------------------------------------

def step_rows(A, STEP=ATOM_STEP):
    """chain_stage_slots: step_rows = chain_div_a(STEP, A): 13, 36, 128"""
    return STEP // A


def pass_split(counts, A, PASS=G.ATOM_PASS, STEP=ATOM_STEP):
    """the mirror: counts int [m], the candidates of every row of one chain -> [(first row, the row behind the last, staged)] a pass,
    as the callers' `for (r0 = 0; r0 < len;)` loops over chain_stage_slots produce them"""
    cum = np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))])
    m, sr = len(counts), STEP // A
    out, r0 = [], 0
    while r0 < m:
        ends = np.arange(r0 + sr, m + sr, sr).clip(max=m)                      # where the steps of this pass would end
        staged = cum[ends] - cum[r0]
        closes = np.flatnonzero((ends >= m) | (staged + sr * A > PASS))
        out.append((r0, int(ends[closes[0]]), int(staged[closes[0]])))
        r0 = int(ends[closes[0]])
    return out


def stage_slots_transcribed(atom, PASS=G.ATOM_PASS, STEP=ATOM_STEP, BLOCK=G.BLOCK):
    """chain_stage_slots line by line for one chain's candidates, bool [len, A]: every lane, both halves of a step, the two exits"""
    length, A = atom.shape
    out, r0 = [], 0
    while r0 < length:
        first, s_count, rows = r0, 0, STEP // A
        while True:
            nr = length - r0 if length - r0 < rows else rows
            for h in range(STEP // BLOCK):
                for tid in range(BLOCK):
                    x = tid + h * BLOCK
                    if x < nr * A:
                        rr = x // A
                        if atom[r0 + rr, x - rr * A]:
                            s_count += 1
            r0 += nr
            staged = s_count
            if r0 >= length or staged + rows * A > PASS:
                break
        out.append((first, r0, s_count))
    return out


def fullest_pass(A, c_row, PASS=G.ATOM_PASS, STEP=ATOM_STEP):
    """the most a pass can hold when a row has at most c_row candidates: the last step starts at PASS - step_rows * A at the most"""
    return min(PASS, PASS - step_rows(A, STEP) * A + step_rows(A, STEP) * c_row)


def design_counts(A, c_row, short, PASS=G.ATOM_PASS, STEP=ATOM_STEP):
    """candidates to keep in each row so that the first pass closes holding fullest_pass (short: one less): whole steps, one step that
    brings the count to target - a step's worth, and a last whole step -> (counts, target)"""
    sr = step_rows(A, STEP)
    s, th = sr * c_row, PASS - sr * A
    target = fullest_pass(A, c_row, PASS, STEP) - (1 if short else 0)
    before = target - s
    assert 0 <= before <= th < target
    q, rem = divmod(before, s)
    counts = [c_row] * (q * sr)
    if rem:
        full, part = divmod(rem, c_row)
        step = [c_row] * full + ([part] if part else [])
        counts += step + [0] * (sr - len(step))
    return counts + [c_row] * sr, target


DESIGN_TAILS = dict(end=0, plus1=1, empty=50, more=40)       # rows behind the designed pass: none, one, a cleared run, ordinary rows


# ---- the pieces the families draw from --------------------------------------------------------------------------------------------------

def row_keep(rng, m, kind, edges):
    """bool [m]: the rows of a chain that keep their masks. edges = (rows of a staging step, of a query tile, of a pass). head / tail
    clear a run one row longer than one of the edges that fit into the chain (half the chain where none does); head_pass / tail_pass
    are cleared by atom_inputs, which knows through pass_split how many rows the chain's own passes span"""
    keep = np.ones(m, bool)
    if m == 0 or kind in ("all", "bb_only", "side_only", "no_slot", "head_pass", "tail_pass") or kind.startswith("design"):
        return keep
    if kind.startswith("iid"):
        return rng.random(m) >= float(kind[3:]) / 100
    if kind.startswith("runs"):
        r, on = 0, bool(rng.integers(2))
        while r < m:
            k = int(rng.geometric(1.0 / int(kind[4:])))
            keep[r:r + k] = on
            r, on = r + k, not on
        return keep
    if kind == "gap_step":                                                     # a cleared run longer than a staging step inside the chain, a tenth cleared beside it
        keep = rng.random(m) >= 0.1
        keep[m // 3:m // 3 + int(edges[0]) + 1] = False
        return keep
    if kind in ("head", "tail"):                                               # a cleared run longer than a step, a tile or a pass, at an end of the chain
        fits = [int(x) + 1 for x in edges if int(x) + 1 < m]
        k = fits[int(rng.integers(len(fits)))] if fits else m // 2
        keep[:k if kind == "head" else 0] = False
        keep[m - k if kind == "tail" else m:] = False
        return keep
    keep[:] = False
    edge = edges[2] if m > edges[2] else edges[1] if m > edges[1] else m - 1   # the rows either side of a pass edge, of a tile edge in a shorter chain
    rows = dict(none=[], zero_long=[], one_first=[0], one_last=[m - 1], two_last=[m - 1, int(rng.integers(max(m - 1, 1)))], three_edge=[0, edge - 1, edge],
                three_any=list(rng.choice(m, size=min(3, m), replace=False)))[kind]
    keep[[r for r in rows if 0 <= r < m]] = True
    return keep


def slot_kind(mask, kind, slot):
    """per-slot clearing of mask [m, A]: only N, CA, C; only side chains; the analysis' own slot absent"""
    if kind == "bb_only":
        mask[:, 3:] = 0
    elif kind == "side_only":
        mask[:, :3] = 0
    elif kind == "no_slot" and slot is not None:
        mask[:, slot] = 0


def site_chain(rng, m, geom):
    """the sites of one chain, float64 [m, 3]"""
    if geom == "helix":
        return AN.helix(rng, m, 4)[:, 1].astype(np.float64) + rng.uniform(-40, 40, 3)
    if geom == "walk":
        return SP.walk_chain(rng, m) if m else np.zeros((0, 3))
    if geom == "lattice":
        return rng.integers(-6, 7, size=(m, 3)).astype(np.float64)
    if geom == "globule":                                                      # every site within the cutoff of every other
        v = rng.normal(size=(m, 3))
        return v * (6.0 * rng.random(m) ** (1 / 3) / np.maximum(np.linalg.norm(v, axis=1), 1e-9))[:, None] + 11.0
    if geom == "line":                                                         # spacing beyond the cutoff of 15: no pair
        return np.stack([np.arange(m) * 16.0, rng.normal(size=m) * 0.1, rng.normal(size=m) * 0.1], axis=1)
    if geom == "coincident":
        return np.tile(rng.integers(-9, 10, size=3).astype(np.float64), (m, 1))
    if geom == "collinear":
        return rng.integers(-9, 10, size=3) + np.arange(m)[:, None] * np.asarray([1.0, 2.0, -1.0])
    if geom == "coplanar":
        return np.concatenate([rng.uniform(-12, 12, (m, 2)), np.full((m, 1), 3.0)], axis=1)
    raise AssertionError(geom)


EXACT = ("lattice", "coincident", "collinear")


def pred_chain(rng, x, geom, noise, still=False):
    """a rigid motion of x plus noise; the integer geometries move by a signed permutation and an integer shift, so they stay exact (and the
    degenerate ones degenerate: they take no noise)"""
    if geom in EXACT:
        shift = rng.integers(1, 10, size=3) * rng.choice([-1, 1], size=3)        # (no component 0: the exact trans would be 0, which has no ulp to be held to)
        y = x @ FP.signed_permutations()[int(rng.integers(24))].astype(np.float64).T + shift
        return y + (rng.integers(-2, 3, size=x.shape) if geom == "lattice" and noise else 0)
    if still and not noise:                                                    # the prediction IS the truth: every delta is exactly 0
        return x.copy()
    return x @ SP.random_rotation(rng).T + rng.uniform(-30, 30, 3) + noise * rng.standard_normal(x.shape)


def atoms_chain(rng, m, A, geom):
    """the atoms of one chain, float32 [m, A, 3]"""
    if m == 0:
        return np.zeros((0, A, 3), F)
    if geom == "lattice":
        return rng.integers(-3, 4, size=(m, A, 3)).astype(F)
    if geom == "globule":
        return SA.globule(rng, m, A, spread=6.0)
    if geom == "coincident":
        return np.tile(rng.integers(-9, 10, size=3).astype(F), (m, A, 1))
    if geom == "collinear":
        return (rng.integers(-9, 10, size=3) + np.arange(m * A).reshape(m, A, 1) * np.asarray([1.0, 2.0, -1.0])).astype(F)
    pos = AN.helix(rng, m, A)
    if geom == "line":                                                         # every residue 20 A from the next
        pos = pos - pos[:, 1:2] + (np.arange(m, dtype=F) * F(20))[:, None, None] * np.asarray([1, 0, 0], F)
    if geom == "coplanar":
        pos[..., 2] = 3.0
    return np.ascontiguousarray(pos, F)


BAD = (np.nan, np.inf, -np.inf, 3e19, -3e19)


def spoil(rng, arrays, ok, rate, edges, bad=None):
    """NaN, +-inf and +-3e19 under set masks: in the rows of `ok` (bool [m]) at `rate`, and, where the rate is not 0, in the first and last
    row of the chain and of its first pass; arrays: [m, 3] or [m, k, 3] views, one of them takes the value"""
    m = len(ok)
    if rate == 0 or m == 0:
        return
    rows = set(np.flatnonzero(rng.random(m) < rate)) | {0, m - 1} | ({edges[2] - 1, edges[2]} if m > edges[2] else set())
    for r in sorted(rows):
        if ok[r]:
            a = arrays[int(rng.integers(len(arrays)))][r]
            a.reshape(-1)[int(rng.integers(a.size))] = (bad or BAD)[int(rng.integers(len(bad or BAD)))]


def payload(pos, mask):
    pos.view(np.uint32)[np.asarray(mask) == 0] = AN.NAN_BITS


def aatype_of(rng, m, comp, A):
    big = G.biggest_type(A if A != 4 else 14)
    if comp == "mix":
        aa = rng.integers(0, 25, size=m).astype(np.uint8)
        aa[rng.random(m) < 0.05] = 255
        return aa
    if comp == "alternate":
        return np.where(np.arange(m) % 2 == 0, GLY, big).astype(np.uint8)
    if comp == "unknown":
        return rng.integers(20, 25, size=m).astype(np.uint8)
    return np.full(m, dict(gly=GLY, big=big, mid=LEU, ala=ALA)[comp] if comp != "255" else 255, np.uint8)


def edges_of(an):
    return an.fz.edges(an.A)


def fuzz_weights(rng, lens, L):
    """upstream weights: normal, a tenth zeros, and one +-3e19 in a row of the first chain that has rows"""
    w = rng.standard_normal((len(lens), L)).astype(F)
    w[rng.random(w.shape) < 0.1] = 0
    for e, m in enumerate(lens):
        if m:
            w[e, int(rng.integers(m))] = F(3e19) * (1 if rng.integers(2) else -1)
            break
    return w


# ---- the families: padded inputs [n, L, ..] for any lengths ------------------------------------------------------------------------------

def _split(profile):
    return [p.split("/") for p in profile[:-1]], profile[-1].split("/")


def pair_inputs(an, rng, lens, L, profile):
    """the one-slot analyses: truth and prediction at `slot`, other numbers in the other slots and behind every length"""
    chains, (mpred, _, _) = _split(profile)
    n, A, slot = len(lens), an.A, an.slot
    pt, pp = (rng.standard_normal((n, L, A, 3)) * 30).astype(F), (rng.standard_normal((n, L, A, 3)) * 30).astype(F)
    mt, mp = (rng.random((n, L, A)) < 0.8).astype(np.uint8), (rng.random((n, L, A)) < 0.8).astype(np.uint8)
    for e, m in enumerate(lens):
        geom, mask, rate, _, noise, kind = chains[e]
        x = site_chain(rng, m, geom)
        pt[e, :m, slot], pp[e, :m, slot] = x, pred_chain(rng, x, geom, float(noise), an.fz.still)
        keep = row_keep(rng, m, mask, edges_of(an))
        mt[e, :m, slot] = keep
        slot_kind(mt[e, :m], mask, slot)
        sub = mt[e, :m, slot] & (rng.random(m) < 0.5)
        mp[e, :m, slot] = 1 if mpred == "null" else dict(equal=mt[e, :m, slot], disjoint=1 - mt[e, :m, slot], subset=sub)[kind]
        spoil(rng, [pt[e, :m, slot], pp[e, :m, slot]], (mt[e, :m, slot] != 0) & (mp[e, :m, slot] != 0), float(rate), edges_of(an), an.fz.bad)
    payload(pt, mt)
    if mpred == "null":
        return dict(pt=pt, mt=mt, pp=pp, mp=None)
    payload(pp, mp)
    return dict(pt=pt, mt=mt, pp=pp, mp=mp)


def site_inputs(an, rng, lens, L, profile):
    d = pair_inputs(an, rng, lens, L, tuple(p.rsplit("/", 1)[0] + "/equal" for p in profile[:-1]) + ("mask/" + profile[-1].split("/", 1)[1],))
    return dict(pos=d["pt"], mask=d["mt"])


def soft_inputs(an, rng, lens, L, profile):
    return dict(pair_inputs(an, rng, lens, L, profile), w=fuzz_weights(rng, lens, L))


def fape_inputs(an, rng, lens, L, profile):
    """the points as pair_inputs draws them; frames exact (signed permutations, integer origins) for the integer geometries and noisy
    rotations about an origin near the point for the others; the frame masks drawn afresh by the chain's mask kind"""
    chains, (mpred, _, _) = _split(profile)
    p = pair_inputs(an, rng, lens, L, profile)
    n, slot = len(lens), an.slot
    perms = FP.signed_permutations()
    d = dict(rot_t=FP.random_rotations(rng, (n, L)).astype(F), rot_p=FP.random_rotations(rng, (n, L)).astype(F),
             trans_t=(rng.standard_normal((n, L, 3)) * 30).astype(F), trans_p=(rng.standard_normal((n, L, 3)) * 30).astype(F),
             fm_t=np.ones((n, L), np.uint8), fm_p=np.ones((n, L), np.uint8), pos_t=p["pt"], mask_t=p["mt"], pos_p=p["pp"], mask_p=p["mp"])
    for e, m in enumerate(lens):
        geom, mask, rate, _, noise, kind = chains[e]
        if geom in EXACT:
            d["rot_t"][e, :m], d["rot_p"][e, :m] = perms[rng.integers(0, 24, size=m)], perms[rng.integers(0, 24, size=m)]
            d["trans_t"][e, :m] = rng.integers(-6, 7, size=(m, 3))
            d["trans_p"][e, :m] = d["trans_t"][e, :m] + rng.integers(-2, 3, size=(m, 3))
        else:
            rt = FP.random_rotations(rng, (m,))
            d["rot_t"][e, :m], d["rot_p"][e, :m] = rt, FP.small_rotations(rng, (m,), 0.15) @ rt
            site = np.nan_to_num(p["pt"][e, :m, slot].astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0).clip(-1e3, 1e3)
            d["trans_t"][e, :m] = site + rng.standard_normal((m, 3)) * 1.5 / FP.SQ3
            d["trans_p"][e, :m] = d["trans_t"][e, :m] + (rng.standard_normal((m, 3)) * max(float(noise), 0.05)).astype(F)
        keep = row_keep(rng, m, mask, edges_of(an)).astype(np.uint8)
        d["fm_t"][e, :m] = keep
        d["fm_p"][e, :m] = 1 if mpred == "null" else dict(equal=keep, disjoint=1 - keep, subset=keep & (rng.random(m) < 0.5))[kind]
        both = (d["fm_t"][e, :m] != 0) & (d["fm_p"][e, :m] != 0)
        spoil(rng, [d[k][e, :m] for k in ("trans_t", "trans_p")], both, float(rate), edges_of(an))
        spoil(rng, [d[k][e, :m] for k in ("rot_t", "rot_p")], both, float(rate) / 2, edges_of(an), BAD[:3])
    for side in "tp":
        d["rot_" + side].view(np.uint32)[d["fm_" + side] == 0] = AN.NAN_BITS
        d["trans_" + side].view(np.uint32)[d["fm_" + side] == 0] = AN.NAN_BITS
    if mpred == "null":
        d["fm_p"] = None
    return dict({k: (None if d[k] is None else np.ascontiguousarray(d[k])) for k in FP.ORDER}, w=fuzz_weights(rng, lens, L))


def candidate_slots(an):
    """bool [21, A]: the slots of a row of every type that can be a candidate of the analysis' staging (the mask permitting)"""
    if an.family in ("atom_pair", "fape_atoms"):                               # (a candidate needs no radius: OXT counts)
        return np.ones((21, an.A), bool)
    return SA.default_table(an.A) != 0


def atom_inputs(an, rng, lens, L, profile, slots=None):
    """the all-slot analyses: pos [n, L, A, 3], mask [n, L, A], aatype [n, L] (or None); a designed chain (mask kind design-*) holds in
    every row the candidates design_counts asks for"""
    chains, (_, aakind, _) = _split(profile)
    n, A = len(lens), an.A
    pos = (rng.standard_normal((n, L, A, 3)) * 30).astype(F)
    mask = np.ones((n, L, A), np.uint8)
    aatype = rng.integers(0, 25, size=(n, L)).astype(np.uint8)
    for e, m in enumerate(lens):
        geom, kind, rate, comp = chains[e][:4]
        pos[e, :m] = atoms_chain(rng, m, A, geom)
        aatype[e, :m] = aatype_of(rng, m, comp, A)
        if kind.startswith("design"):
            cand = candidate_slots(an)[min(int(aatype[e, 0]), 20)] if m else None
            counts, _ = design_counts(A, int(cand.sum()), kind.split("-")[1] == "short", *an.fz.pass_step)
            tail = kind.split("-")[2]
            assert m == len(counts) + DESIGN_TAILS[tail], (m, len(counts), tail)
            for r, c in enumerate(counts):
                mask[e, r, np.flatnonzero(cand)[c:]] = 0
            if tail == "empty":
                mask[e, len(counts):m] = 0
            continue
        keep = row_keep(rng, m, kind, edges_of(an))
        mask[e, :m] = keep[:, None] & (rng.random((m, A)) >= 0.01)
        slot_kind(mask[e, :m], kind, None)
        spoil(rng, [pos[e, :m]], mask[e, :m].any(axis=1), float(rate), edges_of(an))
        if an.fz.atom_pass and m:                                              # what depends on where the chain's own passes close
            ty = np.zeros(m, np.int64) if aakind == "noaatype" else np.minimum(aatype[e, :m], 20)
            staged = lambda: (mask[e, :m] != 0) & candidate_slots(an)[ty] & np.isfinite(pos[e, :m]).all(axis=-1)
            if kind in ("head_pass", "tail_pass"):                             # a cleared run longer than any pass of the chain, with two passes left
                span = max(b - a for a, b, _ in pass_split(staged().sum(axis=1), A, *an.fz.pass_step)) + 1
                assert 3 * span < m, (m, span, "the chain is too short for a run of a pass and two passes")
                mask[e, :span if kind == "head_pass" else 0] = 0
                mask[e, m - span if kind == "tail_pass" else m:m] = 0
            if float(rate):                                                    # a non-finite value in the last row of every pass and in the first of the next
                for _, end, _ in pass_split(staged().sum(axis=1), A, *an.fz.pass_step)[:-1]:
                    for r in (end - 1, end):
                        slots = np.flatnonzero(staged()[r])
                        if len(slots):
                            pos[e, r, int(slots[int(rng.integers(len(slots)))]), int(rng.integers(3))] = BAD[int(rng.integers(len(BAD)))]
    payload(pos, mask)
    return dict(pos=pos, mask=mask, aatype=None if aakind == "noaatype" else aatype)


def atom_pair_inputs(an, rng, lens, L, profile):
    """all-atom lDDT: the truth as atom_inputs draws it, the prediction the truth plus the chain's noise with the partnered slots of every
    second row that has some exchanged; mask_pred by the case's kind"""
    chains, (mpred, _, _) = _split(profile)
    t = atom_inputs(an, rng, lens, L, profile)
    pt, mt, aa = t["pos"], t["mask"], t["aatype"]
    pp = pt.copy()
    mp = np.ones(mt.shape, np.uint8)
    for e, m in enumerate(lens):
        _, kind, _, _, noise, mkind = chains[e]
        with np.errstate(invalid="ignore"):
            pp[e, :m] = pt[e, :m] + (rng.standard_normal((m, an.A, 3)) * float(noise)).astype(F)
        if not kind.startswith("design"):
            sub = mt[e, :m] & (rng.random((m, an.A)) < 0.5)
            mp[e, :m] = 1 if mpred == "null" else dict(equal=mt[e, :m], disjoint=1 - mt[e, :m], subset=sub)[mkind]
    if aa is not None:
        table = LA.default_table(an.A)
        capable = (table != np.arange(an.A))[np.minimum(aa, 20)].any(axis=-1)
        rows = np.zeros(capable.size, bool)
        rows[np.flatnonzero(capable.ravel())[::2]] = True
        pp = np.ascontiguousarray(LA.exchange(pp, aa, rows.reshape(capable.shape), table))
    pp.view(np.uint32)[np.isnan(pp) & (mp == 0)[..., None]] = AN.NAN_BITS
    return dict(pt=pt, mt=mt, pp=pp, mp=None if mpred == "null" else mp, aatype=aa)


PLANT_PLACE = 1100               # a place of a designed pass behind every pass the hand-picked tests of the loss stage (1024 at the most)
BIG_WEIGHT = F(1e15)             # finite through (w_i + w_j) * unit and a sum of a pass' worth of terms: 2e15 * 1280 < 3.4e38


def plant_last_place(pos, atom, PASS, STEP):
    """a designed chain of the violation loss, pos [m, A, 3] and its atoms bool [m, A]: the atom at the LAST place of the first pass is
    moved next to the chain's first atom, the one at PLANT_PLACE next to its second, both of row 0 and so of another residue. A finite
    move of an atom changes nothing that is staged; the places are those of the ascending (row, slot) order, np.argwhere's"""
    idx = np.argwhere(atom)
    staged = pass_split(atom.sum(axis=1), atom.shape[1], PASS, STEP)[0][2]
    assert staged > PLANT_PLACE and idx[1][0] == 0 and idx[PLANT_PLACE][0] > 0
    for place, near, shift in ((staged - 1, 0, (0.25, 0, 0)), (PLANT_PLACE, 1, (0, 0.25, 0))):
        pos[tuple(idx[place])] = pos[tuple(idx[near])] + np.asarray(shift, F)


def plant_disulfide(pos, atom, aatype, A):
    """a chain that is not designed: the SG of its second CYS row that has one is moved next to the SG of the first (a helix brings no two
    SG inside the clash distance), so that a pair passes the distance test and is struck out as a disulfide. Only ordinary coordinates
    move: a +-3e19 placed at a pass edge stays"""
    if A == 4 or aatype is None:
        return
    sg = V.SG_SLOT[A]
    rows = np.flatnonzero(atom[:, sg] & (aatype == V.CYS) & (np.abs(pos[:, sg]) < 1e6).all(axis=-1))
    if len(rows) >= 2:
        pos[rows[1], sg] = pos[rows[0], sg] + np.asarray((0.25, 0, 0), F)


def vloss_inputs(an, rng, lens, L, profile):
    """the violation loss: atom_inputs and the upstream weights w_clash [n, L, A] and w_link [n, L, 3]: normal values of both signs, a
    tenth of them exact zeros, one +-1e15 on an atom and one on a link of the first chain that has one, and NaN bit patterns wherever
    the contract says that no weight is read: a slot that is no atom (atoms_of), a row whose link does not exist (_links), every row
    behind a length. Both sets come from the restatement. A designed chain gets its two planted pairs (plant_last_place), every other
    chain with two CYS a disulfide (plant_disulfide); neither changes what is staged"""
    chains, _ = _split(profile)
    d = atom_inputs(an, rng, lens, L, profile)
    pos, mask, aatype = d["pos"], d["mask"], d["aatype"]
    n, A = len(lens), an.A
    atom, link = np.zeros((n, L, A), bool), np.zeros((n, L), bool)
    for e, m in enumerate(lens):
        aa = None if aatype is None else aatype[e, :m]
        if m:
            atom[e, :m] = SA.atoms_of(pos[e, :m], mask[e, :m], aa, SA.default_table(A))[0]
        if chains[e][1].startswith("design"):
            plant_last_place(pos[e, :m], atom[e, :m], *an.fz.pass_step)
        elif m:
            plant_disulfide(pos[e, :m], atom[e, :m], aa, A)
        if m > 1:
            link[e, :m - 1] = VL._links(pos[e, :m], mask[e, :m], aa, an.params[1])["exist"]
    w = dict(w_clash=rng.standard_normal((n, L, A)).astype(F), w_link=rng.standard_normal((n, L, 3)).astype(F))
    for k, live in (("w_clash", atom), ("w_link", np.repeat(link[..., None], 3, axis=-1))):
        w[k][rng.random(w[k].shape) < 0.1] = 0
        for e in range(n):
            at = np.argwhere(live[e])
            if len(at):
                w[k][e][tuple(at[int(rng.integers(len(at)))])] = BIG_WEIGHT * (1 if rng.integers(2) else -1)
                break
        w[k].view(np.uint32)[~live] = AN.NAN_BITS
    return dict(d, **w)


# ---- the all-atom FAPE: points as the all-atom lDDT has them, frames of eight groups as the backbone FAPE has them ---------------------------
SWAP_TYPES = (FA.ASP, FA.GLU, FA.PHE, FA.TYR)
FAPEA_OWN = ("design", "fpass", "rndf", "rndp")        # the mask kinds whose masks this family lays out itself, slot by slot and item by item
FAPEA_ROUND_FRAMES = (1, 63, 64, 65, 255, 256, 257, 512)       # frames of one frame tile of atom14 (64 rows x 8): wavefront and round edges
FAPEA_ROUND_POINTS = (1, 64, 65, 256, 257, 512, 513, 740)      # points of one point tile of atom37 (20 rows x 37)
FAPEA_DESIGN_FRAMES, FAPEA_SPARSE_POINTS = 150, 600            # frames of a designed point chain, points of a designed frame chain: the restatement's time


def frame_groups(A):
    """the groups of a row that can be frames: backbone4 holds the atoms of groups 0 and 3 alone"""
    return (0, 3) if A == 4 else tuple(range(FA.GROUPS))


def frame_steps(A):
    """the frames of every staging step (32 rows) of the designed frame chain: two steps that stage nothing at the chain's start, a
    full pass right behind them, a pass one frame short of full, a pass of one frame, a frame-free run of two steps in the middle with
    a full pass behind it, and two steps at the end that leave a final pass of nothing"""
    top = FAPEA_FRAME_STEP // FA.GROUPS * len(frame_groups(A))
    return (0, 0, top, top - 1, 1, 0, 0, top, 0, 0)


def frame_design_rows(A):
    return len(frame_steps(A)) * (FAPEA_FRAME_STEP // FA.GROUPS)


def respread(counts, A, sr):
    """design_counts' one step that is neither whole nor empty, its total spread evenly over its rows: where the pass closes rests on
    the step's total alone, and every row of the step then holds some slots and lacks others"""
    counts = list(counts)
    for s0 in range(0, len(counts) - sr + 1, sr):
        total = sum(counts[s0:s0 + sr])
        if 0 < total < sr * A:
            q, r = divmod(total, sr)
            counts[s0:s0 + sr] = [q + (i < r) for i in range(sr)]
    return counts


def fapea_chain(inp, e, m):
    return {k: None if inp.get(k) is None else inp[k][e, :m] for k in FA.ORDER}


def fapea_items(inp, e, m):
    """(frame bool [m, 8], point bool [m, A]) of chain e: the restatement's own predicate (_fape_atoms.items)"""
    return FA.items(fapea_chain(inp, e, m))[3:]


def _subset(rng, shape, count):
    out = np.zeros(int(np.prod(shape)), np.uint8)
    out[rng.permutation(out.size)[:count]] = 1
    return out.reshape(shape)


def plant_last_point(rng, d, e, m, target):
    """a designed point chain: the point at the LAST place of its first pass (ascending (row, slot): np.argwhere's order) gets a
    prediction on the lattice such that its term with EVERY frame of the chain is 3 at least (above any b_sum of a chain within
    MAX_ITEMS: 2181 * 2^-24 * 2181 * 10.25 = 2.9) and below the clamp with one frame at least -> that frame's (row, group)"""
    c = fapea_chain(d, e, m)
    rot_t, pos_t, _, frame, point = FA.items(c)
    r, a = np.argwhere(point)[target - 1]
    fi = np.argwhere(frame)
    Rt, tt = rot_t[frame].astype(np.float64), c["trans_t"][frame].astype(np.float64)
    Rp, tp = c["rot_p"][frame].astype(np.float64), c["trans_p"][frame].astype(np.float64)
    lt = np.einsum("fak,fa->fk", Rt, pos_t[r, a].astype(np.float64) - tt)
    cube = np.stack(np.meshgrid(*[np.arange(-5, 6)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    xp = pos_t[r, a].astype(np.float64) + cube                                                   # [K, 3]
    e2 = ((np.einsum("fak,cfa->cfk", Rp, xp[:, None, :] - tp[None]) - lt[None]) ** 2).sum(axis=-1)   # [offsets, frames]
    ok = np.flatnonzero((e2.min(axis=1) >= 9) & ((e2 < FA.LATTICE_CLAMP ** 2 - 1).sum(axis=1) > 0))
    assert len(ok), "no lattice offset keeps the planted point's term above every b_sum"
    k = int(ok[np.argmax((e2[ok] < FA.LATTICE_CLAMP ** 2 - 1).sum(axis=1))])
    d["pos_p"][e, r, a] = xp[k]
    return tuple(fi[int(np.argmin(e2[k]))])


def fape_atoms_inputs(an, rng, lens, L, profile):
    """the all-atom FAPE. POINTS: the truth as atom_inputs draws it, the prediction the truth plus the chain's noise (integer steps on the
    integer geometries, so that every e stays exact) with the partnered slots of every second capable row exchanged, mask_pred by the
    chain's kind. FRAMES of all eight groups as fape_inputs draws them: signed permutations about integer origins on the integer
    geometries, noisy rotations about origins near the row's atoms otherwise; the frame masks drawn afresh by the chain's mask kind,
    groups 1 and 2 included, fmask_pred equal, a subset, disjoint or NULL. aatype by the chain's composition with a quarter of the
    rows ASP, GLU, PHE or TYR, a third of the rows of every kind swapped; a case without aatype has no swapped, and one case in five
    with aatype has none either. Non-finite values under set masks in trans, rot and both pos at the chain's first and last row, at
    the chain's rate, and either side of every pass edge of the chain's own points (pass_split on the restatement's `point`); the
    integer geometries take NaN and +-inf only. Weights [n, L, 8]: normal, a tenth zeros, one +-3e19 outside the designed chains (whose
    sensitivities are measured against bounds that grow with |w|), NaN bit patterns at every item that is no frame and behind every
    length. The kinds of FAPEA_OWN lay their masks out slot by slot: design-* (the point pass), fpass (frame_steps), rndf-N / rndp-N
    (N frames / points in a chain of one tile)"""
    chains, (mpred, aakind, _) = _split(profile)
    n, A, NG = len(lens), an.A, FA.GROUPS
    PASS, STEP = an.fz.pass_step
    edges = edges_of(an)
    head = [c[1].split("-")[0] for c in chains]
    plain = tuple("/".join([c[0], "all" if h in FAPEA_OWN + ("head_pass", "tail_pass") else c[1], "0"] + c[3:]) for c, h in zip(chains, head))
    t = atom_inputs(an, rng, lens, L, plain + (profile[-1],))
    pt, mt, aa = t["pos"], t["mask"], t["aatype"]
    designed = [h in FAPEA_OWN for h in head]
    swapped = None
    if aa is not None:
        rows = rng.random((n, L)) < 0.25
        aa[rows] = np.asarray(SWAP_TYPES, np.uint8)[rng.integers(0, 4, size=int(rows.sum()))]
        swapped = (rng.random((n, L)) < 0.35).astype(np.uint8)
        if rng.random() < 0.2 and not any(designed):
            swapped = None
    perms = FP.signed_permutations()
    d = dict(rot_t=FP.random_rotations(rng, (n, L, NG)).astype(F), rot_p=FP.random_rotations(rng, (n, L, NG)).astype(F),
             trans_t=(rng.standard_normal((n, L, NG, 3)) * 30).astype(F), trans_p=(rng.standard_normal((n, L, NG, 3)) * 30).astype(F),
             fm_t=(rng.random((n, L, NG)) < 0.7).astype(np.uint8), fm_p=(rng.random((n, L, NG)) < 0.7).astype(np.uint8),
             pos_t=pt, mask_t=mt, aatype=aa, swapped=swapped, pos_p=(rng.standard_normal(pt.shape) * 30).astype(F), mask_p=np.ones(mt.shape, np.uint8))
    planted = {}
    for e, m in enumerate(lens):
        geom, kind, rate, _, noise, mkind = chains[e]
        exact, h = geom in EXACT, head[e]
        if m == 0:
            continue
        # ---- the masks of the points and of the frames
        if designed[e]:                                                        # (atom_inputs left NaN patterns under the masks it cleared)
            pt[e, :m], mt[e, :m] = atoms_chain(rng, m, A, geom), 1
        keepf = row_keep(rng, m, "iid50" if h in FAPEA_OWN + ("head_pass", "tail_pass") else kind, edges)
        d["fm_t"][e, :m] = keepf[:, None] & (rng.random((m, NG)) < 0.7)
        fkind = MPREDS[int(rng.integers(3 if m <= edges[2] else 2))]           # (a chain of more than a pass keeps frames: not disjoint)
        d["fm_p"][e, :m] = 1 if mpred == "null" else dict(equal=d["fm_t"][e, :m], disjoint=1 - d["fm_t"][e, :m], subset=d["fm_t"][e, :m] & (rng.random((m, NG)) < 0.5))[fkind]
        sub = mt[e, :m] & (rng.random((m, A)) < 0.5)
        d["mask_p"][e, :m] = 1 if mpred == "null" else dict(equal=mt[e, :m], disjoint=1 - mt[e, :m], subset=sub)[mkind]
        if designed[e]:
            d["fm_p"][e, :m], d["mask_p"][e, :m] = 1, 1
            allowed = np.zeros((m, NG), np.uint8)
            allowed[:, list(frame_groups(A))] = 1
        if h == "design":                                                      # the truth's mask holds the counts: a swapped row reads it through the partner table
            counts = respread(design_counts(A, A, kind.split("-")[1] == "short", PASS, STEP)[0], A, step_rows(A, STEP))
            tail = kind.split("-")[2]
            assert m == len(counts) + DESIGN_TAILS[tail], (m, len(counts), tail)
            for r, c in enumerate(counts):
                mt[e, r] = _subset(rng, (A,), c)
            mt[e, len(counts):m] = 0 if tail == "empty" else (rng.random((m - len(counts), A)) < 0.5) if tail == "more" else 1
            d["fm_t"][e, :m] = allowed & (rng.random((m, NG)) < FAPEA_DESIGN_FRAMES / allowed.sum())
            if aa is not None and A != 4:                                      # the rows of the spread step: every second one a swapped row of a type with partners
                part = [r for r, c in enumerate(counts) if 0 < c < A][::2]
                aa[e, part], swapped[e, part] = np.asarray(SWAP_TYPES, np.uint8)[np.arange(len(part)) % 4], 1
                table = LA.default_table(A)
                for r in part:                                                 # ... that holds one slot of a partnered pair and lacks the other
                    a = int(rng.choice(np.flatnonzero(table[aa[e, r]] != np.arange(A))))
                    rest = np.setdiff1d(np.arange(A), [a, table[aa[e, r], a]])
                    mt[e, r] = 0
                    mt[e, r, [a] + list(rng.permutation(rest)[:counts[r] - 1])] = 1
        elif h == "fpass":
            sr = FAPEA_FRAME_STEP // NG
            assert m == frame_design_rows(A)
            for s, c in enumerate(frame_steps(A)):
                top = sr * len(frame_groups(A))
                fm = allowed[s * sr:(s + 1) * sr].copy()
                if c == 1:
                    fm = _one_of(rng, fm)
                elif c == top - 1:
                    fm = fm & (1 - _one_of(rng, fm))
                elif c == 0:
                    fm[:] = 0
                d["fm_t"][e, s * sr:(s + 1) * sr] = fm
            mt[e, :m] = rng.random((m, A)) < FAPEA_SPARSE_POINTS / (m * A)
        elif h == "rndf":
            d["fm_t"][e, :m] = 0
            at = np.argwhere(allowed)
            pick = at[rng.permutation(len(at))[:int(kind.split("-")[1])]]
            d["fm_t"][e, pick[:, 0], pick[:, 1]] = 1
            mt[e, :m] = rng.random((m, A)) < min(1.0, FAPEA_SPARSE_POINTS / 2 / (m * A))
        elif h == "rndp":                                                      # the truth's mask all set, so the count is mask_pred's whatever the row's naming
            d["mask_p"][e, :m] = _subset(rng, (m, A), int(kind.split("-")[1]))
            d["fm_t"][e, :m] = allowed & (rng.random((m, NG)) < 0.5)
        # ---- the prediction's points and the frames' geometry
        x = pt[e, :m]
        hole = np.isnan(x).any(axis=-1)
        with np.errstate(invalid="ignore"):
            y = x + (rng.integers(-2, 3, size=x.shape) if exact else rng.standard_normal(x.shape) * float(noise)).astype(F)
        y[hole] = (rng.standard_normal((int(hole.sum()), 3)) * 30).astype(F)
        if aa is not None and not designed[e]:                                 # a prediction under the other naming, as atom_pair_inputs has it
            table = LA.default_table(A)
            capable = (table != np.arange(A))[np.minimum(aa[e, :m], 20)].any(axis=-1)
            rows = np.zeros(m, bool)
            rows[np.flatnonzero(capable)[::2]] = True
            y = LA.exchange(y[None], aa[e, :m][None], rows[None], table)[0]
        d["pos_p"][e, :m] = y
        with np.errstate(invalid="ignore"):
            site = np.nan_to_num(np.where(hole[..., None], 0, x).sum(axis=1) / np.maximum((~hole).sum(axis=1), 1)[:, None]).astype(np.float64)
        if exact:
            d["rot_t"][e, :m], d["rot_p"][e, :m] = perms[rng.integers(0, 24, size=(m, NG))], perms[rng.integers(0, 24, size=(m, NG))]
            d["trans_t"][e, :m] = np.rint(site)[:, None, :] + rng.integers(-6, 7, size=(m, NG, 3))
            d["trans_p"][e, :m] = d["trans_t"][e, :m] + rng.integers(-2, 3, size=(m, NG, 3))
        else:
            rt = FP.random_rotations(rng, (m, NG))
            d["rot_t"][e, :m], d["rot_p"][e, :m] = rt, FP.small_rotations(rng, (m, NG), 0.15) @ rt
            d["trans_t"][e, :m] = site[:, None, :] + rng.standard_normal((m, NG, 3)) * 1.5 / FP.SQ3
            d["trans_p"][e, :m] = d["trans_t"][e, :m] + (rng.standard_normal((m, NG, 3)) * max(float(noise), 0.05)).astype(F)
        per_row = lambda: fapea_items(d, e, m)[1].sum(axis=1)
        if h in ("head_pass", "tail_pass"):                                    # a cleared run longer than any pass of the chain's points, with two passes left
            span = max(b - a for a, b, _ in pass_split(per_row(), A, PASS, STEP)) + 1
            assert 3 * span < m, (m, span, "the chain is too short for a run of a pass and two passes")
            mt[e, :span if h == "head_pass" else 0] = 0
            mt[e, m - span if h == "tail_pass" else m:m] = 0
        # ---- non-finite values under set masks
        if float(rate) and not designed[e]:
            at_edge = {r for _, end, _ in pass_split(per_row(), A, PASS, STEP)[:-1] for r in (end - 1, end)}
            if swapped is not None and A != 4:                                 # either side of a pass edge: a swapped row of a type with partners that lacks one slot of a pair
                table = LA.default_table(A)
                for i, r in enumerate(sorted(at_edge)):
                    aa[e, r], swapped[e, r] = SWAP_TYPES[i % 4], 1
                    mt[e, r, int(rng.choice(np.flatnonzero(table[aa[e, r]] != np.arange(A))))] = 0
            frame, point = fapea_items(d, e, m)
            for r in sorted(set(np.flatnonzero(rng.random(m) < float(rate)).tolist()) | {0, m - 1} | at_edge):
                bad = BAD[:3] if exact or r in at_edge else BAD
                what = int(rng.integers(2, 4)) if r in at_edge else int(rng.integers(4))
                value = bad[int(rng.integers(len(bad)))]
                if what < 2 and frame[r].any():
                    g = int(rng.choice(np.flatnonzero(frame[r])))
                    side = "tp"[int(rng.integers(2))]
                    if what == 0:
                        d["trans_" + side][e, r, g, int(rng.integers(3))] = value
                    else:                                                      # (a finite entry that is no rotation's has no bound: _fape.py)
                        d["rot_" + side][e, r, g, int(rng.integers(3)), int(rng.integers(3))] = BAD[int(rng.integers(3))]
                elif point[r].any():                                           # a point's prediction, or the truth's slot the point reads
                    a = int(rng.choice(np.flatnonzero(point[r])))
                    if what == 3 or swapped is None or not swapped[e, r]:
                        d["pos_p" if what == 3 else "pos_t"][e, r, a, int(rng.integers(3))] = value
                    else:
                        d["pos_p"][e, r, a, int(rng.integers(3))] = value
        if h == "design":
            planted[e] = plant_last_point(rng, d, e, m, pass_split(per_row(), A, PASS, STEP)[0][2])
    # ---- the weights, by the restatement's frames
    frame = np.zeros((n, L, NG), bool)
    for e, m in enumerate(lens):
        if m:
            frame[e, :m] = fapea_items(d, e, m)[0]
    w = rng.standard_normal((n, L, NG)).astype(F)
    w[rng.random(w.shape) < 0.1] = 0
    for e in range(n):
        at = np.argwhere(frame[e])
        if len(at) and not designed[e]:
            w[e][tuple(at[int(rng.integers(len(at)))])] = F(3e19) * (1 if rng.integers(2) else -1)
            break
    for e, m in enumerate(lens):
        if head[e] == "fpass":                                                 # the frame at the last place of every pass carries a weight
            at = np.argwhere(frame[e, :m])
            first = 0
            for _, _, staged in pass_split(frame[e, :m].sum(axis=1), NG, FAPEA_FRAME_PASS, FAPEA_FRAME_STEP):
                first += staged
                if staged:
                    w[e][tuple(at[first - 1])] = F(1.5)
        if e in planted:
            w[e][planted[e]] = F(-1.25)
    w.view(np.uint32)[~frame] = AN.NAN_BITS
    # ---- NaN patterns under every cleared mask, the NULL forms
    payload(d["pos_t"], d["mask_t"])
    payload(d["pos_p"], d["mask_p"])
    for side in "tp":
        d["rot_" + side].view(np.uint32)[d["fm_" + side] == 0] = AN.NAN_BITS
        d["trans_" + side].view(np.uint32)[d["fm_" + side] == 0] = AN.NAN_BITS
    if mpred == "null":
        d["fm_p"] = d["mask_p"] = None
    return dict({k: (None if d[k] is None else np.ascontiguousarray(d[k])) for k in FA.ORDER}, w=w)


def _one_of(rng, allowed):
    """uint8 like `allowed` with one of its set items set"""
    at = np.argwhere(allowed)
    out = np.zeros_like(allowed)
    out[tuple(at[int(rng.integers(len(at)))])] = 1
    return out


def backbone_inputs(an, rng, lens, L, profile):
    d = atom_inputs(an, rng, lens, L, profile)
    if d["aatype"] is not None:
        d["aatype"] = np.minimum(d["aatype"], 20)
        d["aatype"][rng.random(d["aatype"].shape) < 0.1] = DS.PRO
    return d


def labels_inputs(an, rng, lens, L, profile):
    d = backbone_inputs(an, rng, lens, L, profile)
    acc_index, acc_energy, _, _ = DS.hbonds(d["pos"], d["mask"], d["aatype"], np.asarray(lens, np.uint32))
    return dict(d, acc_index=acc_index, acc_energy=acc_energy)


def apply_inputs(an, rng, lens, L, profile):
    d = atom_inputs(an, rng, lens, L, tuple("/".join(p.split("/")[:2] + ["0"] + p.split("/")[3:]) for p in profile[:-1]) + profile[-1:])
    n = len(lens)
    return dict(pos=d["pos"], mask=d["mask"], rot=rng.uniform(-2, 2, (n, 3, 3)).astype(F), trans=rng.uniform(-100, 100, (n, 3)).astype(F))


FAMILIES = dict(pair=pair_inputs, site=site_inputs, soft=soft_inputs, fape=fape_inputs, atoms=atom_inputs, atom_pair=atom_pair_inputs, backbone=backbone_inputs,
                labels=labels_inputs, apply=apply_inputs, vloss=vloss_inputs, fape_atoms=fape_atoms_inputs)


def draw(an, rng, lens, L, profile):
    return FAMILIES[an.family](an, rng, [int(m) for m in lens], int(L), profile)


# ---- the analyses ---------------------------------------------------------------------------------------------------------------------

class SoftF(G.LddtSoft):
    """LddtSoft with the prediction's mask passed on (the sweep-grid pool has none)"""
    family = "soft"

    def ref(self, inp, lens):
        return S.soft_padded(inp["pt"], inp["mt"], inp["pp"], inp["mp"], lens, self.slot, inp["w"])

    def run(self, codec, dev, bound_t, n, rows, packed):
        a = (dev["pt"], dev["mt"], dev["pp"], dev["mp"], bound_t, n, rows, self.layout, self.slot, packed)
        soft, pairs = S.run_value(codec, *a, guard=self.guard)
        return dict(soft=soft, pairs=pairs, grad=S.run_grad(codec, *a, dev["w"], guard=self.guard))


def _with(an, A, slot, name):
    an.A, an.slot, an.name = A, slot, name
    return an


def _sasa(A, slot, param):
    an = G.Sasa(A)
    an.N_POINTS = param
    return an


def _frames(A, slot, param):
    an = G.Frames(param)
    an.A = A
    return an


def _labels(A, slot, param):
    return _with(G.Labels(), A, 1, "dssp labels")


LONG_LENS = ((4, (1250, 1250, 900, 700)), (14, (640, 640, 420, 300)), (37, (150, 150, 110, 90)))
VLOSS_LONG_LENS = ((4, (1050, 1050, 750, 590)), (14, (540, 540, 350, 250)), (37, (125, 125, 92, 75)))       # the same chains at a pass of 1280 for 1536
# the all-atom FAPE: at most _fape_atoms.MAX_ITEMS points (and frames) a chain, and still three passes of 1024 points. head_pass / tail_pass: a
# cleared run of one pass and a row, then some 2 050 points; the third chain passes a subset mask_pred (half its slots), the fourth keeps half its rows
FAPEA_LONG_LENS = ((4, (780, 780, 1000, 900)), (14, (220, 220, 300, 260)), (37, (82, 82, 110, 90)))


@dataclasses.dataclass(frozen=True)
class Spec:
    make: object                # (A, slot, param) -> Analysis
    variants: tuple             # (A, slot, param) the cases cycle through
    tile: object                # A -> rows of a query tile
    row_pass: tuple = ()        # rows a candidate pass of a row-pass sweep
    atom_pass: bool = False     # stages through chain_stage_slots
    waves: bool = False         # a wavefront a chain
    packed: bool = True
    cap: int = 300              # the longest chain of a mix case
    mixes: int = 4              # mix cases
    n_max: int = 9              # chains a mix case at the most
    geoms: tuple = GEOMS
    masks: tuple = MASKS
    rates: tuple = RATES
    noises: tuple = NOISES
    bad: tuple = None           # the non-finite values under set masks, None: BAD
    still: bool = False         # at noise 0 the prediction is the truth itself, not a rigid motion of it
    pass_atoms: int = G.ATOM_PASS   # the atoms of a pass of an atom-pass sweep
    step: int = ATOM_STEP           # the slots its staging step examines
    long_lens: tuple = LONG_LENS    # the rows of the four chains of the long4 / long14 / long37 cases, by layout
    max_items: int = 0              # where the comparator's bounds rest on it: the slots a chain may hold, so A * rows stays at or below it

    @property
    def pass_step(self):
        return self.pass_atoms, self.step

    def edges(self, A):
        return (step_rows(A, self.step) if self.atom_pass else 64, self.tile(A),
                max(self.row_pass) if self.row_pass else (self.pass_atoms // A if self.atom_pass else 256))


SLOTS = ((4, 1, 0), (14, 4, 0), (37, 36, 0), (14, 1, 0), (37, 3, 0), (4, 3, 0), (14, 13, 0), (37, 1, 0))     # CA, CB and the layout's last slot
LAYOUTS3 = ((14, 0, 0), (4, 0, 0), (37, 0, 0))
tile256 = lambda A: G.CHAIN_TILE
SPECS = dict(
    knn=Spec(lambda A, s, k: G.Knn(A, s, k), tuple((A, s, k) for (A, s, _), k in zip(SLOTS, (5, 17, 1, 17, 5, 3, 16, 2))), tile256, (G.KNN_PASS,), mixes=8),
    lddt=Spec(lambda A, s, p: G.Lddt(A, s), SLOTS, tile256, (G.LDDT_PASS,), mixes=8),
    lddt_soft=Spec(lambda A, s, p: _with(SoftF(), A, s, "lddt_soft"), SLOTS, tile256, (G.LDDT_PASS,), mixes=8, still=True),
    hbond=Spec(lambda A, s, p: _with(G.Hbond(), A, 1, "hbond"), LAYOUTS3, tile256, (G.HBOND_PASS,), mixes=8),
    labels=Spec(_labels, LAYOUTS3, tile256, mixes=8),
    apply=Spec(lambda A, s, p: _with(G.Apply(), A, 1, "superpose_apply"), LAYOUTS3, tile256, mixes=10, rates=("0",)),
    fape=Spec(lambda A, s, p: _with(G.Fape(), A, s, "fape"), SLOTS, tile256, (G.FAPE_FRAME_PASS, G.FAPE_PASS), mixes=8, cap=200, rates=RATES[:2]),
    sasa=Spec(_sasa, ((14, 0, 1), (4, 0, 1), (37, 0, 1)), lambda A: G.SASA_TILE_ROWS, atom_pass=True, mixes=8, cap=80),
    violations=Spec(lambda A, s, p: G.Violations(A), LAYOUTS3, G.viol_tile_rows, atom_pass=True, mixes=8, cap=80,
                    geoms=tuple(g for g in GEOMS if g != "coincident")),
    violation_loss=Spec(lambda A, s, p: G.ViolationLoss(A, p), LAYOUTS3 + tuple((A, s, 1) for A, s, _ in LAYOUTS3), G.viol_tile_rows, atom_pass=True, mixes=8, cap=80,
                        pass_atoms=G.VLOSS_PASS, step=VLOSS_STEP, long_lens=VLOSS_LONG_LENS),
    lddt_atoms=Spec(lambda A, s, p: G.LddtAtoms(A), LAYOUTS3, lambda A: G.lddta_tile_rows(A, False), atom_pass=True, mixes=8, cap=80),
    frames=Spec(_frames, ((14, 0, 1), (37, 0, 1), (4, 0, 0), (14, 0, 0)), lambda A: 32, packed=False, mixes=10, geoms=("helix", "lattice")),
    superpose=Spec(lambda A, s, p: _with(G.Superpose(), A, s, "superpose"), SLOTS, lambda A: 64, waves=True, geoms=WAVE_GEOMS, bad=BAD[:3], mixes=8),
    tmscore=Spec(lambda A, s, p: _with(G.TmScore(), A, s, "tmscore"), SLOTS, lambda A: 64, waves=True, geoms=WAVE_GEOMS, bad=BAD[:3], noises=NOISES[1:], mixes=8, cap=150),
    gdt=Spec(lambda A, s, p: _with(G.Gdt(), A, s, "gdt"), SLOTS, lambda A: 64, waves=True, geoms=WAVE_GEOMS, bad=BAD[:3], noises=NOISES[1:], mixes=8, cap=80),
    fape_atoms=Spec(lambda A, s, p: FA.FapeAtoms(A), LAYOUTS3, FA.fapea_tile_rows, atom_pass=True, mixes=8, cap=80, rates=RATES[:2], pass_atoms=FA.FAPEA_PASS, step=FAPEA_STEP,
                    long_lens=FAPEA_LONG_LENS, max_items=FA.MAX_ITEMS),
)
PAIRED = ("lddt", "lddt_soft", "fape", "lddt_atoms", "superpose", "tmscore", "gdt", "fape_atoms")            # the analyses that take mask_pred
WITH_AATYPE = ("hbond", "labels", "sasa", "violations", "violation_loss", "lddt_atoms", "frames", "fape_atoms")              # the ABI takes NULL for aatype
NEED_MARGIN = ("lddt_soft", "fape", "superpose", "tmscore", "gdt", "tmalign", "fape_atoms")                              # their comparators need a margin of the inputs: redrawn


@dataclasses.dataclass(frozen=True)
class Case:
    analysis: str
    A: int
    slot: int
    param: int
    form: tuple                 # ("padded", extra rows of L) | ("clamped", L) | ("null", 0) | ("packed", rows in front, rows behind)
    lens: tuple
    profile: tuple              # a string a chain, "geometry/mask/rate/composition/noise/mask_pred kind", and one for the case, "null|mask/aatype/guard"
    seed: int
    group: str = "mix"

    @property
    def id(self):
        return f"{self.analysis}-{self.group}-{self.seed}"


def _chain_profile(spec, c, cm, geom=None, mask=None, rate=None, comp=None, noise=None, mpred=None):
    """chain number c of an analysis takes the c-th value of every axis (the axes' lengths are coprime enough that all values meet);
    the masks go by cm, the chains so far whose mask was theirs to choose, and every second of those keeps most of its sites"""
    own = spec.masks[(cm // 2) % len(spec.masks)] if cm % 2 else LIVE[(cm // 2) % len(LIVE)]
    return "/".join([geom or spec.geoms[c % len(spec.geoms)], mask or own, rate or spec.rates[c % len(spec.rates)], comp or COMPS[c % len(COMPS)],
                     noise or spec.noises[(c // 2) % len(spec.noises)], mpred or ("disjoint" if c % 9 == 4 else MPREDS[c % 2])])


def _case_profile(name, k):
    mpred = ("null" if k % 3 == 0 else "mask") if name in PAIRED else "mask"
    aa = "noaatype" if name in WITH_AATYPE and k % 4 == 3 else "aatype"
    return f"{mpred}/{aa}/{'small' if k % 2 else 'wide'}"


def _forms(spec, k, lens, rng):
    kind = k % (5 if spec.packed else 3)
    longest = max(list(lens) + [1])
    if kind == 0:
        return ("padded", int(rng.integers(0, 6)))
    if kind == 1 and len(set(lens)) > 1 and sorted(lens)[-2] > 0:
        return ("clamped", int(sorted(lens)[-2]))                             # L below the longest length[e]
    if kind == 2:
        return ("null", 0)
    if kind in (3, 4):
        return ("packed", int(rng.integers(0, 8)) if kind == 4 else 0, int(rng.integers(1, 8)) if kind == 4 else 0)
    return ("padded", 0)


def cases(seed=0, per=None):
    """the list: a pure function of `seed` (and of `per`, mix cases an analysis, None: the specs' own counts)"""
    out = []
    for name, spec in SPECS.items():
        rng = np.random.default_rng([crc(name), seed])
        c = cm = k = 0                                                         # chains, chains with a mask of their own, and cases drawn so far

        def add(group, lens, profs, form=None, variant=None, case_profile=None):
            nonlocal k
            A, slot, param = variant or spec.variants[k % len(spec.variants)]
            form = form or _forms(spec, k, lens, rng)
            case_profile = case_profile or _case_profile(name, k)
            if (name == "frames" and param == 1) or (name in ("sasa", "violations", "violation_loss") and A == 14):     # (the ABI refuses a NULL aatype there)
                case_profile = case_profile.replace("noaatype", "aatype")
            if form[0] == "null":                                             # length NULL: every chain has L rows
                lens = [max(list(lens) + [1])] * len(lens)
            out.append(Case(name, A, slot, param, form, tuple(int(m) for m in lens), tuple(profs) + (case_profile,),
                            seed * 1000 + k, group))
            k += 1

        def profs(count, **fixed):
            nonlocal c, cm
            free = 0 if "mask" in fixed else 1
            got = [_chain_profile(spec, c + i, cm + i * free, **fixed) for i in range(count)]
            c, cm = c + count, cm + count * free
            return got

        # 1. the tile edges and the shortest chains, padded and packed, with empty chains first, last and adjacent
        T = spec.tile(spec.variants[0][0])
        edge = [0, 0, 1, 2, 3, T - 1, T, T + 1, 2 * T, 2 * T + 1, 0]
        if spec.waves:
            edge = [0, 0, 1, 2, 3, 4, 63, 64, 65, 0]
        add("edges", edge, profs(len(edge), mask="all", rate="0"), ("padded", 2), spec.variants[0])
        add("edges", edge, profs(len(edge)), ("packed", 3, 5) if spec.packed else ("padded", 0), spec.variants[1])
        # 2. the pass edges of the row-pass sweeps, a chain or two a case
        for P in spec.row_pass:
            geom = "lattice" if name in ("fape", "lddt_soft") else None      # (a long dense noisy chain has a sign tie in most rows: _lddt_soft.py, _fape.py)
            # P rows, every one a site, the last too, on a helix (or the lattice), where the last row has neighbours and hydrogen bonds
            full = profs(1, mask="all", rate="0", mpred="equal", geom=geom or "helix")
            group = "passes" if len(spec.row_pass) == 1 else f"passes{P}"     # (FAPE's two passes are a test each: 1 s and 5 s of restatement)
            add(group, [P], full, ("packed", 2, 1), spec.variants[0])
            add(group, [P, P], full + profs(1, mask="iid1"), ("null", 0), spec.variants[0])
            for lens, masks, form in (([P - 1, P], ("tail", "all"), ("padded", 1)), ([P + 1], ("three_edge",), ("packed", 0, 0)),
                                      ([2 * P, 0, 7], ("iid10", "all", "all"), ("packed", 6, 3)), ([2 * P + 1], ("iid1",), ("null", 0)), ([2 * P + 1], ("head",), ("padded", 0))):
                add(group, lens, [p for m in masks for p in profs(1, mask=m, geom=geom)], form, spec.variants[0] if name == "fape" else None)
        # 3. the atom-pass sweeps: for every layout a chain whose pass closes at its fullest, one slot under it, and what lies behind
        if spec.atom_pass:
            for v in spec.variants[:3]:                                        # (a layout each; the variants behind them repeat the layouts at other parameters)
                an = spec.make(*v)
                comp = "ala" if an.family == "atom_pair" else "big"
                c_row = int(candidate_slots(an)[ALA if comp == "ala" else G.biggest_type(v[0] if v[0] != 4 else 14)].sum())
                for short, tails in ((False, ("end", "empty")), (True, ("plus1", "more"))):
                    rows = len(design_counts(v[0], c_row, short, *spec.pass_step)[0])
                    lens = [rows + DESIGN_TAILS[t] for t in tails]
                    ps = profs(2, geom="lattice" if name == "fape_atoms" else "helix", rate="0", comp=comp)      # (a long noisy chain has a tie in most rows: _fape_atoms.py)
                    ps = ["/".join(p.split("/")[:1] + [f"design-{'short' if short else 'full'}-{t}"] + p.split("/")[2:5] + ["equal"]) for p, t in zip(ps, tails)]
                    add("design", lens, ps, ("packed", 2, 3) if short else ("padded", 1), v, "mask/aatype/wide")
                if name == "fape_atoms":
                    # the frame staging of k_fape_atoms_grad_points (frame_steps), and chains of ONE tile whose frames / points end on the
                    # edges of a wavefront and of a round of BLOCK: frames in atom14 (a tile of 64 rows x 8), points in atom37 (20 rows x 37)
                    own = lambda kind: profs(1, geom="lattice", mask=kind, rate="0", comp="mix", mpred="equal")
                    add("design", [frame_design_rows(v[0])], own("fpass"), ("packed", 1, 2) if v[0] == 14 else ("padded", 0), v, "mask/aatype/small")
                    rounds = {14: [(f"rndf-{q}", FA.fapea_tile_rows(14)) for q in FAPEA_ROUND_FRAMES], 37: [(f"rndp-{q}", G.lddta_tile_rows(37, False)) for q in FAPEA_ROUND_POINTS],
                              4: [(f"rndf-{G.BLOCK}", FA.fapea_tile_rows(4)), (f"rndp-{G.BLOCK}", G.lddta_tile_rows(4, False))]}[v[0]]
                    add("design", [m for _, m in rounds], [p for kind, _ in rounds for p in own(kind)], ("packed", 0, 0) if v[0] == 37 else ("padded", 2), v, "mask/aatype/wide")
            # chains of several passes that are NOT designed: mixed types, runs, independent clearing, non-finite values at the pass edges
            # (placed through pass_split), a cleared run longer than any of the chain's passes at its start and at its end
            for v, form in zip(spec.variants, (("packed", 3, 2), ("padded", 1), ("packed", 0, 0))):
                lens = list(dict(spec.long_lens)[v[0]])
                lg = "lattice" if name == "fape_atoms" else "helix"           # (the all-atom FAPE: noisy chains stay at 128 rows or under, _fape_atoms.py)
                ps = (profs(1, geom=lg, mask="head_pass", rate="0.01", comp="mix", mpred="equal") + profs(1, geom=lg, mask="tail_pass", rate=spec.rates[-1], comp="alternate", mpred="equal")
                      + profs(1, geom="lattice", mask="gap_step" if v[0] == 4 else "runs64", rate="0.01", comp="mix", mpred="subset") + profs(1, geom=lg, mask="iid50", rate=spec.rates[-1], comp="mix", mpred="equal"))
                add(f"long{v[0]}", lens, ps, form, v, "mask/aatype/small")
        # 4. the wave-per-chain kernels: 0 to 3 sites anywhere in a long chain, coincident and collinear chains in an ordinary batch
        if spec.waves:
            few = [200 + int(rng.integers(0, 60)) for _ in FEW]
            add("few", few, [p for m in FEW for p in profs(1, mask=m, rate="0", geom="walk", mpred="equal")], ("padded", 1), case_profile="mask/aatype/wide")
            add("few", few, [p for m in FEW for p in profs(1, mask=m, rate="0", geom="walk")], ("packed", 4, 2), case_profile="null/aatype/small")
            lens = [40, 33, 25, 30] if name != "gdt" else [40, 12, 12, 30]
            add("few", lens, profs(1, geom="walk", mask="all", mpred="equal") + profs(1, geom="coincident", mask="all", rate="0", mpred="equal")
                + profs(1, geom="collinear", mask="all", rate="0", mpred="subset")
                + profs(1, geom="walk", mask="iid10", mpred="equal"), ("padded", 0), case_profile="mask/aatype/wide")
            if name == "tmscore":
                for m in (TM_LDS_ROWS - 1, TM_LDS_ROWS, TM_LDS_ROWS + 1):
                    add("long", [m], profs(1, geom="walk", mask="iid1", rate="0", noise="1.5"), ("padded", 0), case_profile="null/aatype/wide")
        # 5. the mixes: n from 1 to 9, lengths uniform and from the edges, every axis by the chain's number
        for i in range(spec.mixes if per is None else per):
            n = 1 + (i * 7 + 2) % spec.n_max
            pool = [0, 1, 2, 3, T - 1, T, T + 1]
            lens = [int(pool[int(rng.integers(len(pool)))]) if rng.random() < 0.3 else int(rng.integers(4, spec.cap + 1)) for _ in range(n)]
            lens = [min(m, spec.cap) for m in lens]
            if spec.max_items:                                                 # (a chain of the mix may have every mask set)
                lens = [min(m, spec.max_items // spec.variants[k % len(spec.variants)][0]) for m in lens]
            add("mix", lens, profs(n))
        if name == "knn":                                                      # compact globules of fewer sites than k + 1 and of more
            add("mix", [3, 6, 12, 40, 0], profs(5, geom="globule", mask="all", rate="0"), ("packed", 1, 1), spec.variants[1])
        if name == "sasa":                                                     # one case at a larger point set
            add("mix", [20, 0, 33], profs(3), ("padded", 1), (14, 0, 92))
    return tuple(out) + tmalign_cases(seed)


# ---- TM-align: pairs of chains of two fuzzed sets, 120 rows or under, through drive_tmalign's comparator -----------------------------------
TMALIGN_GEOMS = ("walk", "globule")
TMALIGN_SETS = (((0, 1, 2, 3, 17, 40, 64, 0), ("all", "all", "all", "all", "iid10", "runs8", "all", "all"), ("padded", 0)),
                ((33, 0, 65, 24, 120), ("iid10", "none", "runs8", "tail", "iid1"), ("packed", 2, 3)),
                ((50, 30, 12, 80, 5, 0, 0), ("one_first", "two_last", "three_any", "iid50", "all", "all", "all"), ("padded", 2)),
                ((96, 63, 9), ("head", "all", "iid10"), ("packed", 0, 0)))
TMALIGN_EDGES = (8, 16, 32)


def tmalign_cases(seed=0):
    """set a by the lengths and masks above, set b a related chain a chain (_tmalign.related: a deletion, an insertion, a hinge, a rigid
    motion, noise) or an unrelated one; the pairs are every chain with its partner and with its partner's neighbour"""
    out = []
    for k, (lens, masks, form) in enumerate(TMALIGN_SETS):
        A, slot, _ = SLOTS[(k + seed) % len(SLOTS)]
        profs = [f"{TMALIGN_GEOMS[(k + i) % 2]}/{m}/{('0', '0.05')[(i + k) % 2]}/-/{('0.4', '1.5')[i % 2]}/{'unrelated' if i % 4 == 3 else 'related'}" for i, m in enumerate(masks)]
        out.append(Case("tmalign", A, slot, 0, form, lens, tuple(profs) + ("mask/aatype/wide",), seed * 1000 + k, "pairs"))
    return tuple(out)


@dataclasses.dataclass
class BuiltAlign:
    case: Case
    sa: dict
    sb: dict
    pairs: np.ndarray
    wa: int
    wb: int
    ref: dict = None
    redrawn: int = 0
    loose: tuple = ()
    why: tuple = ()


def _align_set(rng, case, chains, keeps):
    """the chains [m, 3] with their kept rows as a set in the case's form: other numbers in the other slots, behind the lengths and in
    the uncovered packed rows, NaN payloads under cleared masks"""
    A, slot = case.A, case.slot
    if case.form[0] == "packed":
        _, front, back = case.form
        off = (AN.row_off_of([len(c) for c in chains]).astype(np.int64) + front).astype(np.uint32)
        R = int(off[-1]) + back
        pos, mask = (rng.standard_normal((R, A, 3)) * 30).astype(F), np.ones((R, A), np.uint8)
        for c, k, lo in zip(chains, keeps, off):
            pos[lo:lo + len(c), slot], mask[lo:lo + len(c), slot] = c, k
        payload(pos, mask)
        return dict(pos=pos, mask=mask, length=None, row_off=off)
    L = max([len(c) for c in chains] + [1]) + case.form[1]
    pos, mask = (rng.standard_normal((len(chains), L, A, 3)) * 30).astype(F), np.ones((len(chains), L, A), np.uint8)
    for e, (c, k) in enumerate(zip(chains, keeps)):
        pos[e, :len(c), slot], mask[e, :len(c), slot] = c, k
    payload(pos, mask)
    return dict(pos=pos, mask=mask, length=np.asarray([len(c) for c in chains], np.uint32), row_off=None)


def build_tmalign(case):
    rng = np.random.default_rng([crc("tmalign"), case.seed, 1])
    ca, cb, ka, kb = [], [], [], []
    for m, p in zip(case.lens, case.profile[:-1]):
        geom, mask, rate, _, noise, rel = p.split("/")
        x = site_chain(rng, m, geom)
        y = TA.related(rng, x, float(noise)) if rel == "related" and m else site_chain(rng, max(m + int(rng.integers(-2, 3)), 0), geom)
        x, y = x.astype(F), y.astype(F)
        for c, chains, keeps in ((x, ca, ka), (y, cb, kb)):
            keep = row_keep(rng, len(c), mask, TMALIGN_EDGES)
            spoil(rng, [c], keep, float(rate), TMALIGN_EDGES, BAD[:3])
            chains.append(c)
            keeps.append(keep)
    n = len(ca)
    pairs = np.asarray([(i, i) for i in range(n)] + [(i, (i + 1) % n) for i in range(0, n, 2)], np.int32)
    return BuiltAlign(case, _align_set(rng, case, ca, ka), _align_set(rng, case, cb, kb), pairs, max([len(c) for c in ca] + [1]), max([len(c) for c in cb] + [1]))


def restate_tmalign(b):
    traces = []
    b.ref = TA.align_sets(b.sa, b.sb, b.pairs, b.wa, b.wb, b.case.slot, traces)
    for e, tr in enumerate(traces):                                            # the conditions _sweep_grids.tmalign_pool asserts of its pairs
        margin, gap, dps_ok, lead, shared, _, exact_ties = TA.fairness(tr)
        if not (margin >= 1e-8 and shared and gap >= 1e-3 and dps_ok and exact_ties and lead >= 1e-9):
            b.why = (e, margin, gap, dps_ok, lead, shared, exact_ties)
            return False
    return True


def drive_tmalign(codec, case):
    """written / alone / reference for the pairs of one case, the last through _sweep_grids.tmalign_check"""
    b = realise(case)
    what = repr(dataclasses.astuple(case))
    da, db = TA.to_device(b.sa), TA.to_device(b.sb)
    run = lambda pairs: TA.run_dev(codec, da, db, to_dev(pairs), b.wa, b.wb, G.LAYOUT[case.A], case.slot)
    got = run(b.pairs)
    for k, g in got.items():
        left = (G._raw(g) == FILL).all(axis=1)
        assert not left.any(), (what, k, "pairs still 0xA5", np.flatnonzero(left)[:4])
    for e in range(len(b.pairs)):
        alone = run(b.pairs[e:e + 1])
        for k, a in alone.items():
            assert a.tobytes() == np.ascontiguousarray(got[k][e:e + 1]).tobytes(), (what, k, "pair", e, "alone differs from the batch on bytes")
    G.tmalign_check(got, b.ref, what)
    return b


# ---- a case's arrays ---------------------------------------------------------------------------------------------------------------------

@dataclasses.dataclass
class Built:
    case: Case
    an: object
    inp: dict
    eff: list                   # the rows of every chain that exist (min(length, L))
    L: int
    ref: dict = None
    loose: tuple = ()
    redrawn: int = 0
    why: tuple = ()             # what margin the last refused draw missed

    @property
    def packed(self):
        return self.case.form[0] == "packed"

    @property
    def n(self):
        return len(self.eff)

    @property
    def bound(self):
        f = self.case.form
        if f[0] == "null":
            return None
        if f[0] == "packed":
            return (AN.row_off_of(self.eff).astype(np.int64) + f[1]).astype(np.uint32)
        return np.asarray(self.case.lens, np.uint32)

    @property
    def rows(self):
        f = self.case.form
        return int(np.sum(self.eff)) + f[1] + f[2] if f[0] == "packed" else self.L


def build(case):
    spec = SPECS[case.analysis]
    an = spec.make(case.A, case.slot, case.param)
    an.fz = spec
    an.guard = GUARD if case.profile[-1].endswith("wide") else 8 if case.analysis in ("violations", "violation_loss") else 4      # (chain_counts and counts are int64: 8)
    lens = list(case.lens)
    L = case.form[1] if case.form[0] == "clamped" else max(lens + [1]) + (case.form[1] if case.form[0] == "padded" else 0)
    eff = [min(m, L) for m in lens]
    inp = an.fuzz_pool(np.random.default_rng([crc(case.analysis), case.seed, 1]), eff, L, case.profile)
    return Built(case, an, inp, eff, L)


def restate(b):
    """the restatement of a built case, its fairness and its loose chains -> whether the comparator's margins hold"""
    an, inp, eff = b.an, b.inp, np.asarray(b.eff, np.uint32)
    name = b.case.analysis
    geoms = [p.split("/")[0] for p in b.case.profile[:-1]]
    if name in ("tmscore", "gdt"):
        traces = []
        b.ref = (TM.tm_padded if name == "tmscore" else GD.gdt_padded)(inp["pt"], inp["mt"], inp["pp"], inp["mp"], eff, an.slot, traces=traces)
    else:
        b.ref = an.ref(inp, eff)
    if name in ("lddt_soft", "fape"):
        return (S if name == "lddt_soft" else FP).tie_share(b.ref) <= TIE_SHARE
    if name == "fape_atoms":                                                   # no tie at all on the integer geometries, few on the noisy ones
        exact = [e for e, g in enumerate(geoms) if g in EXACT and (b.ref["tie_f"][e].any() or b.ref["tie_p"][e].any())]
        b.why = (FA.tie_share(b.ref), "integer chains with a tie", exact)
        return FA.tie_share(b.ref) <= TIE_SHARE and not exact
    if name not in ("superpose", "tmscore", "gdt"):
        return True
    loose, site = [], SP.site_of(inp["pt"], inp["mt"], inp["pp"], inp["mp"], an.slot)
    gdt_fair = GD.fair(inp["pt"], inp["pp"], an.slot, traces) if name == "gdt" else None
    for e, m in enumerate(b.eff):
        s = site[e, :m]
        if geoms[e] in ("coincident", "collinear", "line"):                      # (line: collinear but for a jitter of 0.1 A)
            if s.sum() >= 3:
                loose.append(e)
            continue
        t, p = inp["pt"][e, :m, an.slot], inp["pp"][e, :m, an.slot]
        if s.sum() >= 3 and np.abs(b.ref["trans"][e]).min() < 1e-6:              # a component that cancels to 0: 2 ulps of it are no bound (_superpose.close)
            b.why = (e, "trans", b.ref["trans"][e])
            return False
        if name == "superpose":
            if SP.threshold_margin(b.ref["dev"][e, :m][s]) < 1e-4 or (s.sum() >= 3 and SP.horn_gap(t, p, s) < 1e-3):
                b.why = (e, "margin", SP.threshold_margin(b.ref["dev"][e, :m][s]), "gap", SP.horn_gap(t, p, s) if s.sum() >= 3 else None)
                return False
        elif name == "tmscore":
            a, shared, gap, _ = TM.fairness(t, p, traces[e])
            if not (a >= 1e-8 and shared and gap >= 1e-3):
                b.why = (e, "margin", a, "shared", shared, "gap", gap)
                return False
        elif not (gdt_fair[0][e] >= GD.MARGIN and gdt_fair[1][e] >= GD.MARGIN and (gdt_fair[2][e] >= GD.GAP).all()):
            b.why = (e, "a", gdt_fair[0][e], "b", gdt_fair[1][e], "gaps", gdt_fair[2][e])
            return False
    b.loose = tuple(loose)
    return True


_REALISED = {}
REDRAWS = 4


def realise(case):
    """build, restate, and redraw with the next seed while the comparator's margin is not met -> Built with ref, loose and redrawn;
    computed once a case and never changed"""
    if case not in _REALISED:
        align = case.analysis == "tmalign"
        for tries in range(REDRAWS):
            b = (build_tmalign if align else build)(dataclasses.replace(case, seed=case.seed + tries * 100000))
            if (restate_tmalign if align else restate)(b):
                b.redrawn = tries
                for v in list(b.ref.values()) + ([] if align else list(b.inp.values())):
                    if v is not None:
                        v.setflags(write=False)
                _REALISED[case] = b
                break
        else:
            raise AssertionError(("no seed meets the comparator's margin", case, b.why))
    return _REALISED[case]


def _filler(rng, k, v):
    """what the uncovered rows of a packed INPUT hold: set masks over finite numbers, so that a kernel that read them would show"""
    shape = v.shape[2:]
    if k in ("acc_index",):
        return lambda r: np.full((r,) + shape, -1, v.dtype)
    if v.dtype == np.uint8 and k != "aatype":
        return lambda r: np.ones((r,) + shape, np.uint8)
    if v.dtype == np.uint8:
        return lambda r: rng.integers(0, 21, size=(r,) + shape).astype(np.uint8)
    return lambda r: (rng.standard_normal((r,) + shape) * 10).astype(v.dtype)


def form_arrays(b, arrays, empty=None):
    """the padded dict `arrays` [n, L, ..] of a case in its form. Packed: the chains' rows behind one another from row `front`, the
    uncovered rows from `empty` (outputs: the empty-row value) or, for inputs, set masks over finite numbers; index keys get the chain's
    first row added"""
    if not b.packed:
        return dict(arrays)
    _, front, back = b.case.form
    off = b.bound.astype(np.int64)
    rng = np.random.default_rng([crc(b.case.analysis), b.case.seed, 2])
    out = {}
    for k, v in arrays.items():
        if v is None or k in b.an.chain_keys:
            out[k] = v
            continue
        fill = (lambda r, k=k, v=v: np.tile(np.asarray(empty[k], v.dtype), (r,) + (1,) * (v.ndim - 2))) if empty is not None else _filler(rng, k, v)
        parts = [fill(front)]
        for e, m in enumerate(b.eff):
            rows = v[e, :m]
            parts.append(np.where(rows >= 0, rows + off[e], -1).astype(v.dtype) if k in b.an.index_keys else rows)
        out[k] = np.ascontiguousarray(np.concatenate(parts + [fill(back)]))
    return out


def empty_rows(b):
    """the restatement's value of a row outside every chain, a key: the analysis on one chain of no row"""
    sub = {k: None if v is None else np.ascontiguousarray(v[:1] if k in b.an.chain_keys else v[:1, :1]) for k, v in b.inp.items()}
    zero = np.zeros(1, np.uint32)
    if b.case.analysis == "tmscore":
        ref = TM.tm_padded(sub["pt"], sub["mt"], sub["pp"], sub["mp"], zero, b.an.slot)
    elif b.case.analysis == "gdt":
        ref = GD.gdt_padded(sub["pt"], sub["mt"], sub["pp"], sub["mp"], zero, b.an.slot)
    else:
        ref = b.an.ref(sub, zero)
    return {k: v[0, 0] for k, v in ref.items() if k not in b.an.chain_keys}


# ---- the device side ----------------------------------------------------------------------------------------------------------------------

def _dev(arrays):
    return {k: None if v is None else to_dev(v) for k, v in arrays.items()}


def run_form(codec, b, arrays, bound, n, rows):
    return b.an.run(codec, _dev(arrays), None if bound is None else to_dev(bound), n, rows, b.packed)


def assert_written(b, got, empty, what):
    for k, g in got.items():
        lead = 1 if (k in b.an.chain_keys or b.packed) else 2
        raw = G._raw(np.ascontiguousarray(g).reshape((-1,) + g.shape[lead:]))
        left = (raw == FILL).all(axis=1) if raw.size else np.zeros(0, bool)
        assert not left.any(), (what, k, "units still 0xA5", int(left.sum()), np.flatnonzero(left)[:4])
        if k in b.an.chain_keys or k not in empty:
            continue
        want = np.asarray(empty[k]).astype(g.dtype)
        want = (want[..., :g.shape[-1]] if want.ndim else want).tobytes()        # (k-NN restates K_REF columns, the device writes k)
        if b.packed:
            _, front, back = b.case.form
            outside = [g[:front], g[len(g) - back:]]
        else:
            outside = [g[e, m:] for e, m in enumerate(b.eff)]
        for o in outside:
            o = np.ascontiguousarray(o)
            assert o.tobytes() == want * o.shape[0], (what, k, "a row outside every chain does not hold the empty-row value")


def assert_alone(codec, b, arrays, got, what):
    """every non-empty chain alone in the same form gives the bytes it gave in the batch"""
    an = b.an
    off = b.bound.astype(np.int64) if b.packed else None
    for e, m in enumerate(b.eff):
        if m == 0:
            continue
        sub = {}
        for k, v in arrays.items():
            if v is None:
                sub[k] = None
            elif k in an.chain_keys or not b.packed:
                sub[k] = np.ascontiguousarray(v[e:e + 1])
            else:
                rows = v[off[e]:off[e] + m]
                sub[k] = np.ascontiguousarray(np.where(rows >= 0, rows - off[e], -1).astype(v.dtype) if k in an.index_keys else rows)
        if b.packed:
            bound, rows = np.asarray([0, m], np.uint32), m
        else:
            bound, rows = (None if b.bound is None else b.bound[e:e + 1]), b.L
        alone = run_form(codec, b, sub, bound, 1, rows)
        for k, a in alone.items():
            if k in an.chain_keys or not b.packed:
                mine = got[k][e:e + 1]
            else:
                mine = got[k][off[e]:off[e] + m]
                if k in an.index_keys:
                    mine = np.where(mine >= 0, mine - off[e], -1).astype(mine.dtype)
            assert a.shape == mine.shape and a.tobytes() == np.ascontiguousarray(mine).tobytes(), \
                (what, k, "chain", e, "alone differs from the batch on bytes", np.argwhere(AN.bits(a) != AN.bits(np.ascontiguousarray(mine)))[:4])


def _loosen(b, got, exp):
    """what is not unique about a loose chain (a minimiser that is not unique: its rot and trans, and which seed and selection of a
    search reached the optimum) takes the restatement's value; rmsd, dev, tm, the counts and `within` of the minimum are unique and stay
    the device's, held to the restatement under the comparator's bounds"""
    if not b.loose:
        return got
    out = {k: v.copy() for k, v in got.items()}
    off = b.bound.astype(np.int64) if b.packed else None
    for e in b.loose:
        for k, v in out.items():
            if k not in ("rot", "trans", "seed", "selected", "run"):
                continue
            if k in b.an.chain_keys:
                v[e] = np.asarray(exp[k][e]).astype(v.dtype)
            elif b.packed:
                v[off[e]:off[e] + b.eff[e]] = np.asarray(exp[k][off[e]:off[e] + b.eff[e]]).astype(v.dtype)
            else:
                v[e] = np.asarray(exp[k][e]).astype(v.dtype)
    return out


EYE = np.eye(3, dtype=F)


def check(b, got, exp, what):
    """the analysis' comparator with its bounds; the three wave-per-chain analyses through the comparators their check() calls, without
    its demand that the batch holds a chain of no site (the coverage test asserts that of the list)"""
    name = b.case.analysis
    if name == "violations":
        return V.same_violations(got, exp, what)
    if name not in ("superpose", "tmscore", "gdt"):
        return b.an.check(got, exp, what)
    g = _loosen(b, got, exp)
    sites = exp["sites"]
    few, none = sites < 2, sites == 0
    if name == "gdt":
        solved = sites >= 3
        GD.close(g, exp, what, compare=np.repeat(solved[:, None], 5, axis=1))
        SP.proper(got["rot"][solved], what)
        assert (got["rot"][none] == EYE).all() and not got["trans"][none].any() and not got["gdt_counts"][none].any(), what
        return None
    if name == "tmscore":
        for k in ("seed", "selected"):
            assert g[k].dtype == np.int32 and np.array_equal(g[k], exp[k]), (what, k, np.argwhere(g[k] != exp[k])[:4])
    SP.close(g, exp, what, compare_rot=(exp["selected"] if name == "tmscore" else sites) >= 3)
    SP.proper(got["rot"], what)
    assert (got["rot"][few] == EYE).all() and not got["trans"][none].any() and not got["rmsd"][few].any(), what
    assert not got["gdt_counts"][none].any() and (got["gdt_counts"][sites == 1] == 1).all() and not got["tm"][none].any(), what
    if name == "tmscore":
        assert (got["tm"][sites == 1] == 1).all() and not got["seed"][sites < 3].any(), what
    return None


def drive(codec, case):
    """the three assertions of one case on the device -> the Built"""
    if case.analysis == "tmalign":
        return drive_tmalign(codec, case)
    b = realise(case)
    what = repr(dataclasses.astuple(case))
    empty = empty_rows(b)
    arrays = form_arrays(b, b.inp)
    got = run_form(codec, b, arrays, b.bound, b.n, b.rows)
    assert_written(b, got, empty, what)
    assert_alone(codec, b, arrays, got, what)
    check(b, got, form_arrays(b, b.ref, empty), what)
    return b


# ---- what the list covers, through the mirrors -------------------------------------------------------------------------------------------

def candidates(b, e):
    """bool [m, A]: the slots of chain e that its analysis stages as candidates (the score launch of the all-atom lDDT, where no row of
    the chain has a partnered slot)"""
    m, inp, an = b.eff[e], b.inp, b.an
    if an.family == "fape_atoms":                                              # the restatement's own predicate: the renaming decides which slot is a point
        return fapea_items(inp, e, m)[1]
    if an.family == "atom_pair":
        with np.errstate(invalid="ignore"):
            ok = (inp["mt"][e, :m] != 0) & np.isfinite(inp["pt"][e, :m]).all(axis=-1) & np.isfinite(inp["pp"][e, :m]).all(axis=-1)
        return ok if inp["mp"] is None else ok & (inp["mp"][e, :m] != 0)
    return SA.atoms_of(inp["pos"][e, :m], inp["mask"][e, :m], None if inp["aatype"] is None else inp["aatype"][e, :m], SA.default_table(an.A))[0]


def sites_of(b):
    """int [n]: the sites of every chain of a one-slot case"""
    inp = b.inp
    if "pos" in inp:
        from _knn import _site
        site = _site(inp["pos"], inp["mask"], b.an.slot)
    else:
        site = SP.site_of(inp["pt"], inp["mt"], inp["pp"], inp["mp"], b.an.slot)
    return np.asarray([int(site[e, :m].sum()) for e, m in enumerate(b.eff)])
