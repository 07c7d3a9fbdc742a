"""CPU: the exception every analysis function raises for an input with ONE defect, torch form (foldcomp_amd.tensors) and numpy form
(Codec.*), pinned as literals: the type and the whole message. The functions share their input checks, so a change to a shared check
shows here as the rows of every function it reaches. No case needs a device: the torch forms refuse before a codec is made (a stand-in
with `device = 0` serves where a valid input must reach the torch checks), the numpy forms before they touch the library (an instance
made without __init__). Run as a script, the file prints the table of the code it is run against."""
import numpy as np
import pytest

from foldcomp_amd import api, tensors
from foldcomp_amd.codec import Codec

F = np.float32


class _Standin:
    """a codec that is never called: the checks read its device only"""
    device = 0


def _batch(A=37, packed=False):
    """2 chains x 8 rows of zeros with a full mask, padded beside length or packed beside cu_seqlens = [0, 8, 16]"""
    lead = (16,) if packed else (2, 8)
    d = dict(pos=np.zeros(lead + (A, 3), F), mask=np.ones(lead + (A,), np.uint8), aatype=np.zeros(lead, np.uint8))
    d.update(cu_seqlens=np.asarray([0, 8, 16], np.int32)) if packed else d.update(length=np.asarray([8, 8], np.int32))
    return d


def _short(a, packed):
    return a[:15] if packed else a[:, :7]


def _torch(d):
    import torch
    return {k: torch.from_numpy(v) for k, v in d.items()}


def _without(d, *keys):
    return {k: v for k, v in d.items() if k not in keys}


def _shape_defects(d, packed):
    """(defect, the dict with it) for the rules on pos, mask and aatype"""
    chains = _without(d, "pos", "mask", "aatype")
    yield "pos rank 2", dict(chains, pos=np.zeros((37, 3), F), mask=np.ones(37, np.uint8))
    yield "last axis 2", dict(d, pos=d["pos"][..., :2])
    yield "A = 5", dict(d, pos=d["pos"][..., :5, :], mask=d["mask"][..., :5])
    yield "mask one row short", dict(d, mask=_short(d["mask"], packed))
    yield "aatype one column short", dict(d, aatype=_short(d["aatype"], packed))


SINGLE = dict(neighbor_graph={}, rigid_frames={}, backbone_hbonds={}, secondary_structure={}, solvent_accessibility={}, violations={})
PAIR = dict(lddt={}, lddt_atoms={}, superpose={}, tm_score={})
FORMS = (("padded", False), ("packed", True))
# rules that come behind the torch checks: a defect of that kind cannot be reached without a device (tests/test_gpu_analysis_inputs.py)
_BEHIND = ("pos rank 2", "last axis 2", "mask one row short", "aatype one column short")
BEHIND_TORCH = dict(neighbor_graph=_BEHIND, lddt=_BEHIND, superpose=_BEHIND, tm_score=_BEHIND, rigid_frames=_BEHIND[2:], lddt_atoms=_BEHIND[2:])
# defects that read no shape: one row, in the padded form, pins them
ANY_FORM = ("no pos", "no mask", "no aatype", "numpy arrays", "tensors on the cpu", "true without pos", "true without mask", "pred without pos",
            "atom14 without aatype", "all without aatype", "CB in backbone4", "swaps without aatype", "a threshold that is no integer", "slot = A",
            "mask_true None", "a layout of another width")


def _cases():
    """id -> a call that must raise"""
    cases = {}
    for form, packed in FORMS:
        d = _batch(37, packed)
        pred = dict(pos=d["pos"] + F(1), mask=d["mask"].copy())
        for name, kw in SINGLE.items():
            fn = getattr(tensors, name)
            inputs = [("no pos", _without(d, "pos")), ("no mask", _without(d, "mask"))] + list(_shape_defects(d, packed))
            inputs += [("numpy arrays", d), ("tensors on the cpu", _torch(d))]
            for defect, x in inputs:
                if defect not in BEHIND_TORCH.get(name, ()):
                    cases[f"{name} / {form} / {defect}"] = lambda fn=fn, x=x, kw=kw: fn(x, codec=_Standin(), **kw)
        d14 = _without(_batch(14, packed), "aatype")
        for name in ("solvent_accessibility", "violations"):
            cases[f"{name} / {form} / atom14 without aatype"] = lambda fn=getattr(tensors, name), x=d14: fn(x, codec=_Standin())
        cases[f"rigid_frames / {form} / all without aatype"] = lambda x=_without(d, "aatype"): tensors.rigid_frames(x, groups="all", codec=_Standin())
        cases[f"neighbor_graph / {form} / CB in backbone4"] = lambda x=_batch(4, packed): tensors.neighbor_graph(x, atom="CB", codec=_Standin())
        for name, kw in PAIR.items():
            fn = getattr(tensors, name)
            inputs = [("true without pos", pred, _without(d, "pos")), ("true without mask", pred, _without(d, "mask")), ("pred without pos", _without(pred, "pos"), d)]
            cut = {"pos rank 2": dict(pos=np.zeros((37, 3), F)), "last axis 2": dict(pred, pos=pred["pos"][..., :2]),
                   "A = 5": dict(pos=pred["pos"][..., :5, :], mask=pred["mask"][..., :5])}   # (pred follows true; the other two are defects of true alone)
            inputs += [(defect, cut.get(defect, pred), x) for defect, x in _shape_defects(d, packed)]
            p14 = _batch(14, packed)
            inputs += [("pred pos of another width", dict(pos=p14["pos"]), d), ("pred mask of another shape", dict(pred, mask=_short(pred["mask"], packed)), d),
                       ("numpy arrays", pred, d), ("tensors on the cpu", _torch(pred), _torch(d))]
            for defect, p, t in inputs:
                if defect not in BEHIND_TORCH.get(name, ()):
                    cases[f"{name} / {form} / {defect}"] = lambda fn=fn, p=p, t=t, kw=kw: fn(p, t, codec=_Standin(), **kw)
        cases[f"lddt_atoms / {form} / swaps without aatype"] = lambda p=pred, t=_without(d, "aatype"): tensors.lddt_atoms(p, t, codec=_Standin())
        # apply_transform(pos, rot, trans, batch, mask=)
        chains = _without(d, "pos", "mask", "aatype")
        rot, trans = np.zeros((2, 3, 3), F), np.zeros((2, 3), F)
        inputs = [("no pos", None, None, rot, trans), ("pos rank 2", np.zeros((37, 3), F), None, rot, trans), ("last axis 2", d["pos"][..., :2], None, rot, trans),
                  ("A = 5", d["pos"][..., :5, :], None, rot, trans), ("mask one row short", d["pos"], _short(d["mask"], packed), rot, trans),
                  ("rot of the wrong shape", d["pos"], d["mask"], rot[:1], trans), ("trans of the wrong shape", d["pos"], d["mask"], rot, trans[:, :2]),
                  ("numpy arrays", d["pos"], d["mask"], rot, trans)]
        for defect, pos, mask, r, t in inputs:
            cases[f"apply_transform / {form} / {defect}"] = lambda pos=pos, mask=mask, r=r, t=t, b=chains: tensors.apply_transform(pos, r, t, b, mask=mask, codec=_Standin())
        td, tb = _torch(d), _torch(chains)
        cases[f"apply_transform / {form} / tensors on the cpu"] = lambda td=td, tb=tb, r=_torch(dict(r=rot, t=trans)): tensors.apply_transform(
            td["pos"], r["r"], r["t"], tb, mask=td["mask"], codec=_Standin())
        # encode_tensors: its shape rules come behind the device's, so only what is missing and where the tensors lie shows here
        for key in ("pos", "mask", "aatype", "cu_seqlens" if packed else "length"):
            cases[f"encode_tensors / {form} / no {key}"] = lambda x=_without(d, key): tensors.encode_tensors(x, codec=_Standin())
        cases[f"encode_tensors / {form} / numpy arrays"] = lambda x=d: tensors.encode_tensors(x, codec=_Standin())
        cases[f"encode_tensors / {form} / tensors on the cpu"] = lambda x=_torch(d): tensors.encode_tensors(x, codec=_Standin())
        cases[f"encode_tensors / {form} / a threshold that is no integer"] = lambda x=d: tensors.encode_tensors(x, anchor_residue_threshold=25.0, codec=_Standin())
        cases.update(_numpy_cases(form, packed, d, pred))
    return {k: v for k, v in cases.items() if not (" / packed / " in k and k.rsplit(" / ", 1)[1] in ANY_FORM)}


def _numpy_cases(form, packed, d, pred):
    """the numpy forms, on a Codec made without __init__: every case is refused before the library is touched"""
    c = Codec.__new__(Codec)
    cases = {}
    chains = dict(row_off=np.asarray([0, 8, 16], np.uint32)) if packed else dict(length=np.asarray([8, 8], np.uint32))
    bad_chains = dict(row_off=np.zeros((1, 3), np.uint32)) if packed else dict(length=np.asarray([8, 8, 8], np.uint32))
    bad_name = "row_off of rank 2" if packed else "length of the wrong size"
    pos, mask, aa = d["pos"], d["mask"], d["aatype"]
    shapes = [("pos rank 2", np.zeros((37, 3), F), np.ones(37, np.uint8), None),
              ("last axis 2", pos[..., :2], mask, aa), ("A = 5", pos[..., :5, :], mask[..., :5], aa), ("mask one row short", pos, _short(mask, packed), aa),
              ("aatype one column short", pos, mask, _short(aa, packed))]
    single = dict(neighbors=lambda p, m, a, **kw: c.neighbors(p, m, 4, 1, **kw), secondary_structure=c.secondary_structure, solvent_accessibility=c.solvent_accessibility,
                  violations=c.violations)
    for name, fn in single.items():
        for defect, p, m, a in shapes:
            if name == "neighbors" and defect.startswith("aatype"):
                continue                                                         # (neighbors reads no aatype)
            call = (lambda fn=fn, p=p, m=m, a=a: fn(p, m, a, **chains))
            cases[f"Codec.{name} / {form} / {defect}"] = call
        cases[f"Codec.{name} / {form} / {bad_name}"] = lambda fn=fn: fn(pos, mask, aa, **bad_chains)
    p14 = _without(_batch(14, packed), "aatype")
    for name in ("solvent_accessibility", "violations"):
        cases[f"Codec.{name} / {form} / atom14 without aatype"] = lambda fn=single[name]: fn(p14["pos"], p14["mask"], None, **chains)
    pp, pm = pred["pos"], pred["mask"]
    pair = dict(lddt=c.lddt, superpose=c.superpose, tm_score=c.tm_score, lddt_atoms=lambda pt, mt, pp, mp, **kw: c.lddt_atoms(pt, mt, pp, mp, aa, **kw))
    for name, fn in pair.items():
        inputs = [("mask_true None", pos, None, pp, pm), ("pos rank 2", np.zeros((37, 3), F), np.ones(37, np.uint8), np.zeros((37, 3), F), None),
                  ("last axis 2", pos[..., :2], mask, pp[..., :2], pm), ("A = 5", pos[..., :5, :], mask[..., :5], pp[..., :5, :], pm[..., :5]),
                  ("mask_true one row short", pos, _short(mask, packed), pp, pm), ("pos_pred of another width", pos, mask, _batch(14, packed)["pos"], None),
                  ("mask_pred of another shape", pos, mask, pp, _short(pm, packed))]
        for defect, a, b, e, f in inputs:
            cases[f"Codec.{name} / {form} / {defect}"] = lambda fn=fn, a=a, b=b, e=e, f=f: fn(a, b, e, f, **chains)
        cases[f"Codec.{name} / {form} / {bad_name}"] = lambda fn=fn: fn(pos, mask, pp, pm, **bad_chains)
        if name != "lddt_atoms":
            cases[f"Codec.{name} / {form} / slot = A"] = lambda fn=fn: fn(pos, mask, pp, pm, slot=37, **chains)
    cases[f"Codec.lddt_atoms / {form} / aatype one column short"] = lambda: c.lddt_atoms(pos, mask, pp, pm, _short(aa, packed), **chains)
    cases[f"Codec.lddt_atoms / {form} / swaps without aatype"] = lambda: c.lddt_atoms(pos, mask, pp, pm, None, **chains)
    rot, trans = np.zeros((2, 3, 3), F), np.zeros((2, 3), F)
    inputs = [("pos rank 2", np.zeros((37, 3), F), rot, trans, None), ("last axis 2", pos[..., :2], rot, trans, mask),
              ("A = 5", pos[..., :5, :], rot, trans, mask[..., :5]), ("mask one row short", pos, rot, trans, _short(mask, packed)),
              ("rot of the wrong shape", pos, rot[:1], trans, mask), ("trans of the wrong shape", pos, rot, trans[:, :2], mask)]
    for defect, p, r, t, m in inputs:
        cases[f"Codec.apply_transform / {form} / {defect}"] = lambda p=p, r=r, t=t, m=m: c.apply_transform(p, r, t, m, **chains)
    cases[f"Codec.apply_transform / {form} / {bad_name}"] = lambda: c.apply_transform(pos, rot, trans, mask, **bad_chains)
    # frames: the packed form is a pos of rank 3, and takes no length
    for defect, p, m, a in shapes:
        cases[f"Codec.frames / {form} / {defect}"] = lambda p=p, m=m, a=a: c.frames(p, m, a)
    cases[f"Codec.frames / {form} / " + ("a length" if packed else "length of the wrong size")] = lambda: c.frames(pos, mask, aa, np.asarray([8, 8, 8], np.uint32))
    cases[f"Codec.frames / {form} / a layout of another width"] = lambda: c.frames(pos, mask, aa, layout="atom14")
    cases[f"Codec.frames / {form} / all without aatype"] = lambda: c.frames(pos, mask, None, groups="all")
    return cases


CASES = _cases()
E, T, V = api.error, TypeError, ValueError

POS4 = "pos must be float32 [n, L, A, 3], or [R, A, 3] beside cu_seqlens, with A = 37, 14 or 4, not "

TABLE = {
    'neighbor_graph / padded / no pos': (T, "neighbor_graph needs the tensor 'pos'"),
    'neighbor_graph / padded / no mask': (T, "neighbor_graph needs the tensor 'mask'"),
    'neighbor_graph / padded / A = 5': (V, 'a layout of 5 slots per residue has no CA'),
    'neighbor_graph / padded / numpy arrays': (E, 'neighbor_graph takes torch tensors on the GPU (numpy arrays: Codec.neighbors)'),
    'neighbor_graph / padded / tensors on the cpu': (E, 'neighbor_graph: pos lies on cpu, the codec works on cuda:0; there is no CPU path'),
    'rigid_frames / padded / no pos': (T, "rigid_frames needs the tensor 'pos'"),
    'rigid_frames / padded / no mask': (T, "rigid_frames needs the tensor 'mask'"),
    'rigid_frames / padded / pos rank 2': (V, 'pos must be float32 [n, L, A, 3] or [R, A, 3] with A = 37, 14 or 4, not (37, 3)'),
    'rigid_frames / padded / last axis 2': (V, 'pos must be float32 [n, L, A, 3] or [R, A, 3] with A = 37, 14 or 4, not (2, 8, 37, 2)'),
    'rigid_frames / padded / A = 5': (V, 'pos must be float32 [n, L, A, 3] or [R, A, 3] with A = 37, 14 or 4, not (2, 8, 5, 3)'),
    'rigid_frames / padded / numpy arrays': (E, 'rigid_frames takes torch tensors on the GPU (numpy arrays: Codec.frames)'),
    'rigid_frames / padded / tensors on the cpu': (E, 'rigid_frames: pos lies on cpu, the codec works on cuda:0; there is no CPU path'),
    'backbone_hbonds / padded / no pos': (T, "backbone_hbonds needs the tensor 'pos'"),
    'backbone_hbonds / padded / no mask': (T, "backbone_hbonds needs the tensor 'mask'"),
    'backbone_hbonds / padded / pos rank 2': (V, POS4 + '(37, 3)'),
    'backbone_hbonds / padded / last axis 2': (V, POS4 + '(2, 8, 37, 2)'),
    'backbone_hbonds / padded / A = 5': (V, POS4 + '(2, 8, 5, 3)'),
    'backbone_hbonds / padded / mask one row short': (V, 'mask must have the shape (2, 8, 37), not (2, 7, 37)'),
    'backbone_hbonds / padded / aatype one column short': (V, 'aatype must have the shape (2, 8), not (2, 7)'),
    'backbone_hbonds / padded / numpy arrays': (E, 'backbone_hbonds takes torch tensors on the GPU (numpy arrays: Codec.secondary_structure)'),
    'backbone_hbonds / padded / tensors on the cpu': (E, 'backbone_hbonds: pos lies on cpu, the codec works on cuda:0; there is no CPU path'),
    'secondary_structure / padded / no pos': (T, "secondary_structure needs the tensor 'pos'"),
    'secondary_structure / padded / no mask': (T, "secondary_structure needs the tensor 'mask'"),
    'secondary_structure / padded / pos rank 2': (V, POS4 + '(37, 3)'),
    'secondary_structure / padded / last axis 2': (V, POS4 + '(2, 8, 37, 2)'),
    'secondary_structure / padded / A = 5': (V, POS4 + '(2, 8, 5, 3)'),
    'secondary_structure / padded / mask one row short': (V, 'mask must have the shape (2, 8, 37), not (2, 7, 37)'),
    'secondary_structure / padded / aatype one column short': (V, 'aatype must have the shape (2, 8), not (2, 7)'),
    'secondary_structure / padded / numpy arrays': (E, 'secondary_structure takes torch tensors on the GPU (numpy arrays: Codec.secondary_structure)'),
    'secondary_structure / padded / tensors on the cpu': (E, 'secondary_structure: pos lies on cpu, the codec works on cuda:0; there is no CPU path'),
    'solvent_accessibility / padded / no pos': (T, "solvent_accessibility needs the tensor 'pos'"),
    'solvent_accessibility / padded / no mask': (T, "solvent_accessibility needs the tensor 'mask'"),
    'solvent_accessibility / padded / pos rank 2': (V, POS4 + '(37, 3)'),
    'solvent_accessibility / padded / last axis 2': (V, POS4 + '(2, 8, 37, 2)'),
    'solvent_accessibility / padded / A = 5': (V, POS4 + '(2, 8, 5, 3)'),
    'solvent_accessibility / padded / mask one row short': (V, 'mask must have the shape (2, 8, 37), not (2, 7, 37)'),
    'solvent_accessibility / padded / aatype one column short': (V, 'aatype must have the shape (2, 8), not (2, 7)'),
    'solvent_accessibility / padded / numpy arrays': (E, 'solvent_accessibility takes torch tensors on the GPU (numpy arrays: Codec.solvent_accessibility)'),
    'solvent_accessibility / padded / tensors on the cpu': (E, 'solvent_accessibility: pos lies on cpu, the codec works on cuda:0; there is no CPU path'),
    'violations / padded / no pos': (T, "violations needs the tensor 'pos'"),
    'violations / padded / no mask': (T, "violations needs the tensor 'mask'"),
    'violations / padded / pos rank 2': (V, POS4 + '(37, 3)'),
    'violations / padded / last axis 2': (V, POS4 + '(2, 8, 37, 2)'),
    'violations / padded / A = 5': (V, POS4 + '(2, 8, 5, 3)'),
    'violations / padded / mask one row short': (V, 'mask must have the shape (2, 8, 37), not (2, 7, 37)'),
    'violations / padded / aatype one column short': (V, 'aatype must have the shape (2, 8), not (2, 7)'),
    'violations / padded / numpy arrays': (E, 'violations takes torch tensors on the GPU (numpy arrays: Codec.violations)'),
    'violations / padded / tensors on the cpu': (E, 'violations: pos lies on cpu, the codec works on cuda:0; there is no CPU path'),
    'solvent_accessibility / padded / atom14 without aatype': (V, 'solvent_accessibility: atom14 needs aatype (which atom a slot holds depends on the residue type)'),
    'violations / padded / atom14 without aatype': (V, 'violations: atom14 needs aatype (which atom a slot holds depends on the residue type)'),
    'rigid_frames / padded / all without aatype': (V, "groups='all' needs aatype: the chi groups depend on the residue type"),
    'neighbor_graph / padded / CB in backbone4': (V, 'a layout of 4 slots per residue has no CB'),
    'lddt / padded / true without pos': (T, "lddt needs the tensor 'pos' of true"),
    'lddt / padded / true without mask': (T, "lddt needs the tensor 'mask' of true"),
    'lddt / padded / pred without pos': (T, "lddt needs the tensor 'pos' of pred"),
    'lddt / padded / A = 5': (V, 'a layout of 5 slots per residue has no CA'),
    'lddt / padded / pred pos of another width': (V, 'pred pos must have the shape of true pos, (2, 8, 37, 3), not (2, 8, 14, 3)'),
    'lddt / padded / pred mask of another shape': (V, 'pred mask must have the shape of true mask, (2, 8, 37), not (2, 7, 37)'),
    'lddt / padded / numpy arrays': (E, 'lddt takes torch tensors on the GPU (numpy arrays: Codec.lddt)'),
    'lddt / padded / tensors on the cpu': (E, 'lddt: pos lies on cpu, the codec works on cuda:0; there is no CPU path'),
    'lddt_atoms / padded / true without pos': (T, "lddt_atoms needs the tensor 'pos' of true"),
    'lddt_atoms / padded / true without mask': (T, "lddt_atoms needs the tensor 'mask' of true"),
    'lddt_atoms / padded / pred without pos': (T, "lddt_atoms needs the tensor 'pos' of pred"),
    'lddt_atoms / padded / pos rank 2': (V, 'pos must be float32 [n, L, A, 3] or [R, A, 3] with A = 37, 14 or 4, not (37, 3)'),
    'lddt_atoms / padded / last axis 2': (V, 'pos must be float32 [n, L, A, 3] or [R, A, 3] with A = 37, 14 or 4, not (2, 8, 37, 2)'),
    'lddt_atoms / padded / A = 5': (V, 'pos must be float32 [n, L, A, 3] or [R, A, 3] with A = 37, 14 or 4, not (2, 8, 5, 3)'),
    'lddt_atoms / padded / pred pos of another width': (V, 'pred pos must have the shape of true pos, (2, 8, 37, 3), not (2, 8, 14, 3)'),
    'lddt_atoms / padded / pred mask of another shape': (V, 'pred mask must have the shape of true mask, (2, 8, 37), not (2, 7, 37)'),
    'lddt_atoms / padded / numpy arrays': (E, 'lddt_atoms takes torch tensors on the GPU (numpy arrays: Codec.lddt_atoms)'),
    'lddt_atoms / padded / tensors on the cpu': (E, 'lddt_atoms: pos lies on cpu, the codec works on cuda:0; there is no CPU path'),
    'superpose / padded / true without pos': (T, "superpose needs the tensor 'pos' of true"),
    'superpose / padded / true without mask': (T, "superpose needs the tensor 'mask' of true"),
    'superpose / padded / pred without pos': (T, "superpose needs the tensor 'pos' of pred"),
    'superpose / padded / A = 5': (V, 'a layout of 5 slots per residue has no CA'),
    'superpose / padded / pred pos of another width': (V, 'pred pos must have the shape of true pos, (2, 8, 37, 3), not (2, 8, 14, 3)'),
    'superpose / padded / pred mask of another shape': (V, 'pred mask must have the shape of true mask, (2, 8, 37), not (2, 7, 37)'),
    'superpose / padded / numpy arrays': (E, 'superpose takes torch tensors on the GPU (numpy arrays: Codec.superpose)'),
    'superpose / padded / tensors on the cpu': (E, 'superpose: pos lies on cpu, the codec works on cuda:0; there is no CPU path'),
    'tm_score / padded / true without pos': (T, "tm_score needs the tensor 'pos' of true"),
    'tm_score / padded / true without mask': (T, "tm_score needs the tensor 'mask' of true"),
    'tm_score / padded / pred without pos': (T, "tm_score needs the tensor 'pos' of pred"),
    'tm_score / padded / A = 5': (V, 'a layout of 5 slots per residue has no CA'),
    'tm_score / padded / pred pos of another width': (V, 'pred pos must have the shape of true pos, (2, 8, 37, 3), not (2, 8, 14, 3)'),
    'tm_score / padded / pred mask of another shape': (V, 'pred mask must have the shape of true mask, (2, 8, 37), not (2, 7, 37)'),
    'tm_score / padded / numpy arrays': (E, 'tm_score takes torch tensors on the GPU (numpy arrays: Codec.tm_score)'),
    'tm_score / padded / tensors on the cpu': (E, 'tm_score: pos lies on cpu, the codec works on cuda:0; there is no CPU path'),
    'lddt_atoms / padded / swaps without aatype': (V, 'lddt_atoms needs aatype in `true` to rename side chains (swaps=None: no renaming)'),
    'apply_transform / padded / no pos': (T, "apply_transform needs the tensor 'pos'"),
    'apply_transform / padded / pos rank 2': (V, POS4 + '(37, 3)'),
    'apply_transform / padded / last axis 2': (V, POS4 + '(2, 8, 37, 2)'),
    'apply_transform / padded / A = 5': (V, POS4 + '(2, 8, 5, 3)'),
    'apply_transform / padded / mask one row short': (V, 'mask must have the shape (2, 8, 37), not (2, 7, 37)'),
    'apply_transform / padded / rot of the wrong shape': (V, 'rot must be float32 (2, 3, 3), one transform per chain, not (1, 3, 3)'),
    'apply_transform / padded / trans of the wrong shape': (V, 'trans must be float32 (2, 3), one transform per chain, not (2, 2)'),
    'apply_transform / padded / numpy arrays': (E, 'apply_transform takes torch tensors on the GPU (numpy arrays: Codec.apply_transform)'),
    'apply_transform / padded / tensors on the cpu': (E, 'apply_transform: pos lies on cpu, the codec works on cuda:0; there is no CPU path'),
    'encode_tensors / padded / no pos': (T, "encode_tensors needs the tensor 'pos'"),
    'encode_tensors / padded / no mask': (T, "encode_tensors needs the tensor 'mask'"),
    'encode_tensors / padded / no aatype': (T, "encode_tensors needs the tensor 'aatype'"),
    'encode_tensors / padded / no length': (T, "encode_tensors needs the tensor 'length'"),
    'encode_tensors / padded / numpy arrays': (E, 'encode_tensors takes torch tensors on the GPU (numpy arrays: Codec.compress_dense)'),
    'encode_tensors / padded / tensors on the cpu': (E, 'encode_tensors: pos lies on cpu, the codec works on cuda:0; the records are built where the tensors are and there is no CPU path'),
    'encode_tensors / padded / a threshold that is no integer': (T, 'anchor_residue_threshold must be an integer'),
    'Codec.neighbors / padded / pos rank 2': (V, 'pos must be float32 [n, L, A, 3] with A = 37, 14 or 4, not (37, 3)'),
    'Codec.neighbors / padded / last axis 2': (V, 'pos must be float32 [n, L, A, 3] with A = 37, 14 or 4, not (2, 8, 37, 2)'),
    'Codec.neighbors / padded / A = 5': (V, 'pos must be float32 [n, L, A, 3] with A = 37, 14 or 4, not (2, 8, 5, 3)'),
    'Codec.neighbors / padded / mask one row short': (V, 'mask must be bool / uint8 (2, 8, 37), not uint8 (2, 7, 37)'),
    'Codec.neighbors / padded / length of the wrong size': (V, 'length must be [2], not (3,)'),
    'Codec.secondary_structure / padded / pos rank 2': (V, 'pos must be float32 [n, L, A, 3] with A = 37, 14 or 4, not (37, 3)'),
    'Codec.secondary_structure / padded / last axis 2': (V, 'pos must be float32 [n, L, A, 3] with A = 37, 14 or 4, not (2, 8, 37, 2)'),
    'Codec.secondary_structure / padded / A = 5': (V, 'pos must be float32 [n, L, A, 3] with A = 37, 14 or 4, not (2, 8, 5, 3)'),
    'Codec.secondary_structure / padded / mask one row short': (V, 'mask must be bool / uint8 (2, 8, 37), not uint8 (2, 7, 37)'),
    'Codec.secondary_structure / padded / aatype one column short': (V, 'aatype must be uint8 (2, 8), not uint8 (2, 7)'),
    'Codec.secondary_structure / padded / length of the wrong size': (V, 'length must be [2], not (3,)'),
    'Codec.solvent_accessibility / padded / pos rank 2': (V, 'pos must be float32 [n, L, A, 3] with A = 37, 14 or 4, not (37, 3)'),
    'Codec.solvent_accessibility / padded / last axis 2': (V, 'pos must be float32 [n, L, A, 3] with A = 37, 14 or 4, not (2, 8, 37, 2)'),
    'Codec.solvent_accessibility / padded / A = 5': (V, 'pos must be float32 [n, L, A, 3] with A = 37, 14 or 4, not (2, 8, 5, 3)'),
    'Codec.solvent_accessibility / padded / mask one row short': (V, 'mask must be bool / uint8 (2, 8, 37), not uint8 (2, 7, 37)'),
    'Codec.solvent_accessibility / padded / aatype one column short': (V, 'aatype must be uint8 (2, 8), not uint8 (2, 7)'),
    'Codec.solvent_accessibility / padded / length of the wrong size': (V, 'length must be [2], not (3,)'),
    'Codec.violations / padded / pos rank 2': (V, 'pos must be float32 [n, L, A, 3] with A = 37, 14 or 4, not (37, 3)'),
    'Codec.violations / padded / last axis 2': (V, 'pos must be float32 [n, L, A, 3] with A = 37, 14 or 4, not (2, 8, 37, 2)'),
    'Codec.violations / padded / A = 5': (V, 'pos must be float32 [n, L, A, 3] with A = 37, 14 or 4, not (2, 8, 5, 3)'),
    'Codec.violations / padded / mask one row short': (V, 'mask must be bool / uint8 (2, 8, 37), not uint8 (2, 7, 37)'),
    'Codec.violations / padded / aatype one column short': (V, 'aatype must be uint8 (2, 8), not uint8 (2, 7)'),
    'Codec.violations / padded / length of the wrong size': (V, 'length must be [2], not (3,)'),
    'Codec.solvent_accessibility / padded / atom14 without aatype': (V, 'Codec.solvent_accessibility: atom14 needs aatype (which atom a slot holds depends on the residue type)'),
    'Codec.violations / padded / atom14 without aatype': (V, 'Codec.violations: atom14 needs aatype (which atom a slot holds depends on the residue type)'),
    'Codec.lddt / padded / mask_true None': (V, 'mask_true is needed'),
    'Codec.lddt / padded / pos rank 2': (V, 'pos_true must be float32 [n, L, A, 3] with A = 37, 14 or 4, not (37, 3)'),
    'Codec.lddt / padded / last axis 2': (V, 'pos_true must be float32 [n, L, A, 3] with A = 37, 14 or 4, not (2, 8, 37, 2)'),
    'Codec.lddt / padded / A = 5': (V, 'pos_true must be float32 [n, L, A, 3] with A = 37, 14 or 4, not (2, 8, 5, 3)'),
    'Codec.lddt / padded / mask_true one row short': (V, 'mask_true must be bool / uint8 (2, 8, 37), not uint8 (2, 7, 37)'),
    'Codec.lddt / padded / pos_pred of another width': (V, 'pos_pred must have the shape of pos_true, (2, 8, 37, 3), not (2, 8, 14, 3)'),
    'Codec.lddt / padded / mask_pred of another shape': (V, 'mask_pred must be bool / uint8 (2, 8, 37), not uint8 (2, 7, 37)'),
    'Codec.lddt / padded / length of the wrong size': (V, 'length must be [2], not (3,)'),
    'Codec.lddt / padded / slot = A': (V, 'slot must be 0 .. 36'),
    'Codec.superpose / padded / mask_true None': (V, 'mask_true is needed'),
    'Codec.superpose / padded / pos rank 2': (V, 'pos_true must be float32 [n, L, A, 3] with A = 37, 14 or 4, not (37, 3)'),
    'Codec.superpose / padded / last axis 2': (V, 'pos_true must be float32 [n, L, A, 3] with A = 37, 14 or 4, not (2, 8, 37, 2)'),
    'Codec.superpose / padded / A = 5': (V, 'pos_true must be float32 [n, L, A, 3] with A = 37, 14 or 4, not (2, 8, 5, 3)'),
    'Codec.superpose / padded / mask_true one row short': (V, 'mask_true must be bool / uint8 (2, 8, 37), not uint8 (2, 7, 37)'),
    'Codec.superpose / padded / pos_pred of another width': (V, 'pos_pred must have the shape of pos_true, (2, 8, 37, 3), not (2, 8, 14, 3)'),
    'Codec.superpose / padded / mask_pred of another shape': (V, 'mask_pred must be bool / uint8 (2, 8, 37), not uint8 (2, 7, 37)'),
    'Codec.superpose / padded / length of the wrong size': (V, 'length must be [2], not (3,)'),
    'Codec.superpose / padded / slot = A': (V, 'slot must be 0 .. 36'),
    'Codec.tm_score / padded / mask_true None': (V, 'mask_true is needed'),
    'Codec.tm_score / padded / pos rank 2': (V, 'pos_true must be float32 [n, L, A, 3] with A = 37, 14 or 4, not (37, 3)'),
    'Codec.tm_score / padded / last axis 2': (V, 'pos_true must be float32 [n, L, A, 3] with A = 37, 14 or 4, not (2, 8, 37, 2)'),
    'Codec.tm_score / padded / A = 5': (V, 'pos_true must be float32 [n, L, A, 3] with A = 37, 14 or 4, not (2, 8, 5, 3)'),
    'Codec.tm_score / padded / mask_true one row short': (V, 'mask_true must be bool / uint8 (2, 8, 37), not uint8 (2, 7, 37)'),
    'Codec.tm_score / padded / pos_pred of another width': (V, 'pos_pred must have the shape of pos_true, (2, 8, 37, 3), not (2, 8, 14, 3)'),
    'Codec.tm_score / padded / mask_pred of another shape': (V, 'mask_pred must be bool / uint8 (2, 8, 37), not uint8 (2, 7, 37)'),
    'Codec.tm_score / padded / length of the wrong size': (V, 'length must be [2], not (3,)'),
    'Codec.tm_score / padded / slot = A': (V, 'slot must be 0 .. 36'),
    'Codec.lddt_atoms / padded / mask_true None': (V, 'mask_true is needed'),
    'Codec.lddt_atoms / padded / pos rank 2': (V, 'pos_true must be float32 [n, L, A, 3] with A = 37, 14 or 4, not (37, 3)'),
    'Codec.lddt_atoms / padded / last axis 2': (V, 'pos must be float32 [n, L, A, 3] or [R, A, 3] with A = 37, 14 or 4, not (2, 8, 37, 2)'),
    'Codec.lddt_atoms / padded / A = 5': (V, 'pos must be float32 [n, L, A, 3] or [R, A, 3] with A = 37, 14 or 4, not (2, 8, 5, 3)'),
    'Codec.lddt_atoms / padded / mask_true one row short': (V, 'mask_true must be bool / uint8 (2, 8, 37), not uint8 (2, 7, 37)'),
    'Codec.lddt_atoms / padded / pos_pred of another width': (V, 'pred pos must have the shape of true pos, (2, 8, 37, 3), not (2, 8, 14, 3)'),
    'Codec.lddt_atoms / padded / mask_pred of another shape': (V, 'mask_pred must be bool / uint8 (2, 8, 37), not uint8 (2, 7, 37)'),
    'Codec.lddt_atoms / padded / length of the wrong size': (V, 'length must be [2], not (3,)'),
    'Codec.lddt_atoms / padded / aatype one column short': (V, 'aatype must be uint8 (2, 8), not uint8 (2, 7)'),
    'Codec.lddt_atoms / padded / swaps without aatype': (V, 'lddt_atoms needs aatype in `true` to rename side chains (swaps=None: no renaming)'),
    'Codec.apply_transform / padded / pos rank 2': (V, 'pos must be float32 [n, L, A, 3] with A = 37, 14 or 4, not (37, 3)'),
    'Codec.apply_transform / padded / last axis 2': (V, 'pos must be float32 [n, L, A, 3] with A = 37, 14 or 4, not (2, 8, 37, 2)'),
    'Codec.apply_transform / padded / A = 5': (V, 'pos must be float32 [n, L, A, 3] with A = 37, 14 or 4, not (2, 8, 5, 3)'),
    'Codec.apply_transform / padded / mask one row short': (V, 'mask must be bool / uint8 (2, 8, 37), not uint8 (2, 7, 37)'),
    'Codec.apply_transform / padded / rot of the wrong shape': (V, 'rot must be [2, 3, 3] and trans [2, 3], one transform per chain, not (1, 3, 3) and (2, 3)'),
    'Codec.apply_transform / padded / trans of the wrong shape': (V, 'rot must be [2, 3, 3] and trans [2, 3], one transform per chain, not (2, 3, 3) and (2, 2)'),
    'Codec.apply_transform / padded / length of the wrong size': (V, 'length must be [2], not (3,)'),
    'Codec.frames / padded / pos rank 2': (V, 'pos must be float32 [n, L, A, 3] or [R, A, 3] with A = 37, 14 or 4, not (37, 3)'),
    'Codec.frames / padded / last axis 2': (V, 'pos must be float32 [n, L, A, 3] or [R, A, 3] with A = 37, 14 or 4, not (2, 8, 37, 2)'),
    'Codec.frames / padded / A = 5': (V, 'pos must be float32 [n, L, A, 3] or [R, A, 3] with A = 37, 14 or 4, not (2, 8, 5, 3)'),
    'Codec.frames / padded / mask one row short': (V, 'mask must be bool / uint8 (2, 8, 37), not uint8 (2, 7, 37)'),
    'Codec.frames / padded / aatype one column short': (V, 'aatype must be uint8 (2, 8), not (2, 7)'),
    'Codec.frames / padded / length of the wrong size': (V, 'length must be [2], not (3,)'),
    'Codec.frames / padded / a layout of another width': (V, "layout 'atom14' does not have 37 slots per residue"),
    'Codec.frames / padded / all without aatype': (V, "groups='all' needs aatype: the chi groups depend on the residue type"),
    'neighbor_graph / packed / A = 5': (V, 'a layout of 5 slots per residue has no CA'),
    'rigid_frames / packed / pos rank 2': (V, 'pos must be float32 [n, L, A, 3] or [R, A, 3] with A = 37, 14 or 4, not (37, 3)'),
    'rigid_frames / packed / last axis 2': (V, 'pos must be float32 [n, L, A, 3] or [R, A, 3] with A = 37, 14 or 4, not (16, 37, 2)'),
    'rigid_frames / packed / A = 5': (V, 'pos must be float32 [n, L, A, 3] or [R, A, 3] with A = 37, 14 or 4, not (16, 5, 3)'),
    'backbone_hbonds / packed / pos rank 2': (V, POS4 + '(37, 3)'),
    'backbone_hbonds / packed / last axis 2': (V, POS4 + '(16, 37, 2)'),
    'backbone_hbonds / packed / A = 5': (V, POS4 + '(16, 5, 3)'),
    'backbone_hbonds / packed / mask one row short': (V, 'mask must have the shape (16, 37), not (15, 37)'),
    'backbone_hbonds / packed / aatype one column short': (V, 'aatype must have the shape (16,), not (15,)'),
    'secondary_structure / packed / pos rank 2': (V, POS4 + '(37, 3)'),
    'secondary_structure / packed / last axis 2': (V, POS4 + '(16, 37, 2)'),
    'secondary_structure / packed / A = 5': (V, POS4 + '(16, 5, 3)'),
    'secondary_structure / packed / mask one row short': (V, 'mask must have the shape (16, 37), not (15, 37)'),
    'secondary_structure / packed / aatype one column short': (V, 'aatype must have the shape (16,), not (15,)'),
    'solvent_accessibility / packed / pos rank 2': (V, POS4 + '(37, 3)'),
    'solvent_accessibility / packed / last axis 2': (V, POS4 + '(16, 37, 2)'),
    'solvent_accessibility / packed / A = 5': (V, POS4 + '(16, 5, 3)'),
    'solvent_accessibility / packed / mask one row short': (V, 'mask must have the shape (16, 37), not (15, 37)'),
    'solvent_accessibility / packed / aatype one column short': (V, 'aatype must have the shape (16,), not (15,)'),
    'violations / packed / pos rank 2': (V, POS4 + '(37, 3)'),
    'violations / packed / last axis 2': (V, POS4 + '(16, 37, 2)'),
    'violations / packed / A = 5': (V, POS4 + '(16, 5, 3)'),
    'violations / packed / mask one row short': (V, 'mask must have the shape (16, 37), not (15, 37)'),
    'violations / packed / aatype one column short': (V, 'aatype must have the shape (16,), not (15,)'),
    'lddt / packed / A = 5': (V, 'a layout of 5 slots per residue has no CA'),
    'lddt / packed / pred pos of another width': (V, 'pred pos must have the shape of true pos, (16, 37, 3), not (16, 14, 3)'),
    'lddt / packed / pred mask of another shape': (V, 'pred mask must have the shape of true mask, (16, 37), not (15, 37)'),
    'lddt_atoms / packed / pos rank 2': (V, 'pos must be float32 [n, L, A, 3] or [R, A, 3] with A = 37, 14 or 4, not (37, 3)'),
    'lddt_atoms / packed / last axis 2': (V, 'pos must be float32 [n, L, A, 3] or [R, A, 3] with A = 37, 14 or 4, not (16, 37, 2)'),
    'lddt_atoms / packed / A = 5': (V, 'pos must be float32 [n, L, A, 3] or [R, A, 3] with A = 37, 14 or 4, not (16, 5, 3)'),
    'lddt_atoms / packed / pred pos of another width': (V, 'pred pos must have the shape of true pos, (16, 37, 3), not (16, 14, 3)'),
    'lddt_atoms / packed / pred mask of another shape': (V, 'pred mask must have the shape of true mask, (16, 37), not (15, 37)'),
    'superpose / packed / A = 5': (V, 'a layout of 5 slots per residue has no CA'),
    'superpose / packed / pred pos of another width': (V, 'pred pos must have the shape of true pos, (16, 37, 3), not (16, 14, 3)'),
    'superpose / packed / pred mask of another shape': (V, 'pred mask must have the shape of true mask, (16, 37), not (15, 37)'),
    'tm_score / packed / A = 5': (V, 'a layout of 5 slots per residue has no CA'),
    'tm_score / packed / pred pos of another width': (V, 'pred pos must have the shape of true pos, (16, 37, 3), not (16, 14, 3)'),
    'tm_score / packed / pred mask of another shape': (V, 'pred mask must have the shape of true mask, (16, 37), not (15, 37)'),
    'apply_transform / packed / pos rank 2': (V, POS4 + '(37, 3)'),
    'apply_transform / packed / last axis 2': (V, POS4 + '(16, 37, 2)'),
    'apply_transform / packed / A = 5': (V, POS4 + '(16, 5, 3)'),
    'apply_transform / packed / mask one row short': (V, 'mask must have the shape (16, 37), not (15, 37)'),
    'apply_transform / packed / rot of the wrong shape': (V, 'rot must be float32 (2, 3, 3), one transform per chain, not (1, 3, 3)'),
    'apply_transform / packed / trans of the wrong shape': (V, 'trans must be float32 (2, 3), one transform per chain, not (2, 2)'),
    'encode_tensors / packed / no cu_seqlens': (T, "encode_tensors needs the tensor 'length'"),
    'Codec.neighbors / packed / pos rank 2': (V, 'pos must be float32 [R, A, 3] with A = 37, 14 or 4, not (37, 3)'),
    'Codec.neighbors / packed / last axis 2': (V, 'pos must be float32 [R, A, 3] with A = 37, 14 or 4, not (16, 37, 2)'),
    'Codec.neighbors / packed / A = 5': (V, 'pos must be float32 [R, A, 3] with A = 37, 14 or 4, not (16, 5, 3)'),
    'Codec.neighbors / packed / mask one row short': (V, 'mask must be bool / uint8 (16, 37), not uint8 (15, 37)'),
    'Codec.neighbors / packed / row_off of rank 2': (V, 'row_off must be [n + 1]'),
    'Codec.secondary_structure / packed / pos rank 2': (V, 'pos must be float32 [R, A, 3] with A = 37, 14 or 4, not (37, 3)'),
    'Codec.secondary_structure / packed / last axis 2': (V, 'pos must be float32 [R, A, 3] with A = 37, 14 or 4, not (16, 37, 2)'),
    'Codec.secondary_structure / packed / A = 5': (V, 'pos must be float32 [R, A, 3] with A = 37, 14 or 4, not (16, 5, 3)'),
    'Codec.secondary_structure / packed / mask one row short': (V, 'mask must be bool / uint8 (16, 37), not uint8 (15, 37)'),
    'Codec.secondary_structure / packed / aatype one column short': (V, 'aatype must be uint8 (16,), not uint8 (15,)'),
    'Codec.secondary_structure / packed / row_off of rank 2': (V, 'row_off must be [n + 1]'),
    'Codec.solvent_accessibility / packed / pos rank 2': (V, 'pos must be float32 [R, A, 3] with A = 37, 14 or 4, not (37, 3)'),
    'Codec.solvent_accessibility / packed / last axis 2': (V, 'pos must be float32 [R, A, 3] with A = 37, 14 or 4, not (16, 37, 2)'),
    'Codec.solvent_accessibility / packed / A = 5': (V, 'pos must be float32 [R, A, 3] with A = 37, 14 or 4, not (16, 5, 3)'),
    'Codec.solvent_accessibility / packed / mask one row short': (V, 'mask must be bool / uint8 (16, 37), not uint8 (15, 37)'),
    'Codec.solvent_accessibility / packed / aatype one column short': (V, 'aatype must be uint8 (16,), not uint8 (15,)'),
    'Codec.solvent_accessibility / packed / row_off of rank 2': (V, 'row_off must be [n + 1]'),
    'Codec.violations / packed / pos rank 2': (V, 'pos must be float32 [R, A, 3] with A = 37, 14 or 4, not (37, 3)'),
    'Codec.violations / packed / last axis 2': (V, 'pos must be float32 [R, A, 3] with A = 37, 14 or 4, not (16, 37, 2)'),
    'Codec.violations / packed / A = 5': (V, 'pos must be float32 [R, A, 3] with A = 37, 14 or 4, not (16, 5, 3)'),
    'Codec.violations / packed / mask one row short': (V, 'mask must be bool / uint8 (16, 37), not uint8 (15, 37)'),
    'Codec.violations / packed / aatype one column short': (V, 'aatype must be uint8 (16,), not uint8 (15,)'),
    'Codec.violations / packed / row_off of rank 2': (V, 'row_off must be [n + 1]'),
    'Codec.lddt / packed / pos rank 2': (V, 'pos_true must be float32 [R, A, 3] with A = 37, 14 or 4, not (37, 3)'),
    'Codec.lddt / packed / last axis 2': (V, 'pos_true must be float32 [R, A, 3] with A = 37, 14 or 4, not (16, 37, 2)'),
    'Codec.lddt / packed / A = 5': (V, 'pos_true must be float32 [R, A, 3] with A = 37, 14 or 4, not (16, 5, 3)'),
    'Codec.lddt / packed / mask_true one row short': (V, 'mask_true must be bool / uint8 (16, 37), not uint8 (15, 37)'),
    'Codec.lddt / packed / pos_pred of another width': (V, 'pos_pred must have the shape of pos_true, (16, 37, 3), not (16, 14, 3)'),
    'Codec.lddt / packed / mask_pred of another shape': (V, 'mask_pred must be bool / uint8 (16, 37), not uint8 (15, 37)'),
    'Codec.lddt / packed / row_off of rank 2': (V, 'row_off must be [n + 1]'),
    'Codec.superpose / packed / pos rank 2': (V, 'pos_true must be float32 [R, A, 3] with A = 37, 14 or 4, not (37, 3)'),
    'Codec.superpose / packed / last axis 2': (V, 'pos_true must be float32 [R, A, 3] with A = 37, 14 or 4, not (16, 37, 2)'),
    'Codec.superpose / packed / A = 5': (V, 'pos_true must be float32 [R, A, 3] with A = 37, 14 or 4, not (16, 5, 3)'),
    'Codec.superpose / packed / mask_true one row short': (V, 'mask_true must be bool / uint8 (16, 37), not uint8 (15, 37)'),
    'Codec.superpose / packed / pos_pred of another width': (V, 'pos_pred must have the shape of pos_true, (16, 37, 3), not (16, 14, 3)'),
    'Codec.superpose / packed / mask_pred of another shape': (V, 'mask_pred must be bool / uint8 (16, 37), not uint8 (15, 37)'),
    'Codec.superpose / packed / row_off of rank 2': (V, 'row_off must be [n + 1]'),
    'Codec.tm_score / packed / pos rank 2': (V, 'pos_true must be float32 [R, A, 3] with A = 37, 14 or 4, not (37, 3)'),
    'Codec.tm_score / packed / last axis 2': (V, 'pos_true must be float32 [R, A, 3] with A = 37, 14 or 4, not (16, 37, 2)'),
    'Codec.tm_score / packed / A = 5': (V, 'pos_true must be float32 [R, A, 3] with A = 37, 14 or 4, not (16, 5, 3)'),
    'Codec.tm_score / packed / mask_true one row short': (V, 'mask_true must be bool / uint8 (16, 37), not uint8 (15, 37)'),
    'Codec.tm_score / packed / pos_pred of another width': (V, 'pos_pred must have the shape of pos_true, (16, 37, 3), not (16, 14, 3)'),
    'Codec.tm_score / packed / mask_pred of another shape': (V, 'mask_pred must be bool / uint8 (16, 37), not uint8 (15, 37)'),
    'Codec.tm_score / packed / row_off of rank 2': (V, 'row_off must be [n + 1]'),
    'Codec.lddt_atoms / packed / pos rank 2': (V, 'pos_true must be float32 [R, A, 3] with A = 37, 14 or 4, not (37, 3)'),
    'Codec.lddt_atoms / packed / last axis 2': (V, 'pos must be float32 [n, L, A, 3] or [R, A, 3] with A = 37, 14 or 4, not (16, 37, 2)'),
    'Codec.lddt_atoms / packed / A = 5': (V, 'pos must be float32 [n, L, A, 3] or [R, A, 3] with A = 37, 14 or 4, not (16, 5, 3)'),
    'Codec.lddt_atoms / packed / mask_true one row short': (V, 'mask_true must be bool / uint8 (16, 37), not uint8 (15, 37)'),
    'Codec.lddt_atoms / packed / pos_pred of another width': (V, 'pred pos must have the shape of true pos, (16, 37, 3), not (16, 14, 3)'),
    'Codec.lddt_atoms / packed / mask_pred of another shape': (V, 'mask_pred must be bool / uint8 (16, 37), not uint8 (15, 37)'),
    'Codec.lddt_atoms / packed / row_off of rank 2': (V, 'row_off must be [n + 1]'),
    'Codec.lddt_atoms / packed / aatype one column short': (V, 'aatype must be uint8 (16,), not uint8 (15,)'),
    'Codec.apply_transform / packed / pos rank 2': (V, 'pos must be float32 [R, A, 3] with A = 37, 14 or 4, not (37, 3)'),
    'Codec.apply_transform / packed / last axis 2': (V, 'pos must be float32 [R, A, 3] with A = 37, 14 or 4, not (16, 37, 2)'),
    'Codec.apply_transform / packed / A = 5': (V, 'pos must be float32 [R, A, 3] with A = 37, 14 or 4, not (16, 5, 3)'),
    'Codec.apply_transform / packed / mask one row short': (V, 'mask must be bool / uint8 (16, 37), not uint8 (15, 37)'),
    'Codec.apply_transform / packed / rot of the wrong shape': (V, 'rot must be [2, 3, 3] and trans [2, 3], one transform per chain, not (1, 3, 3) and (2, 3)'),
    'Codec.apply_transform / packed / trans of the wrong shape': (V, 'rot must be [2, 3, 3] and trans [2, 3], one transform per chain, not (2, 3, 3) and (2, 2)'),
    'Codec.apply_transform / packed / row_off of rank 2': (V, 'row_off must be [n + 1]'),
    'Codec.frames / packed / pos rank 2': (V, 'pos must be float32 [n, L, A, 3] or [R, A, 3] with A = 37, 14 or 4, not (37, 3)'),
    'Codec.frames / packed / last axis 2': (V, 'pos must be float32 [n, L, A, 3] or [R, A, 3] with A = 37, 14 or 4, not (16, 37, 2)'),
    'Codec.frames / packed / A = 5': (V, 'pos must be float32 [n, L, A, 3] or [R, A, 3] with A = 37, 14 or 4, not (16, 5, 3)'),
    'Codec.frames / packed / mask one row short': (V, 'mask must be bool / uint8 (16, 37), not uint8 (15, 37)'),
    'Codec.frames / packed / aatype one column short': (V, 'aatype must be uint8 (16,), not (15,)'),
    'Codec.frames / packed / a length': (V, 'the packed form takes no length'),
}


def test_the_table_has_a_row_for_every_case():
    assert sorted(TABLE) == sorted(CASES)


@pytest.mark.parametrize("key", list(CASES))
def test_one_defect_raises_the_pinned_error(key):
    with pytest.raises((E, T, V)) as e:
        CASES[key]()
    assert (type(e.value), str(e.value)) == TABLE[key]


if __name__ == "__main__":
    for key, call in CASES.items():
        try:
            call()
            raise SystemExit(f"{key}: no error")
        except (E, T, V) as e:
            print(f"    {key!r}: ({ {E: 'E', T: 'T', V: 'V'}[type(e)] }, {str(e)!r}),")
