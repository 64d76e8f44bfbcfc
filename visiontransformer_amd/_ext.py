"""Bindings of the family headers: entry points of csrc/libvitseg.so that are declared beside include/vitseg.h.

A feature family has a header of its own (include/vitseg_<family>.h, with its own version) and one entry of EXT_SIGNATURES:
family -> (header file, the words after "built before" in `ext_symbol`'s error, [(name, restype, argtypes)]).  `_lib.SIGNATURES`
and include/vitseg.h do not grow with it.  Functions are bound on first use on the handle `_lib.lib()` loaded;
tests/test_polygons_cpu.py compares the table with the header through the parser of tests/test_binding_cpu.py.
EXT_SIGNATURES is pinned to the polygons family by that test and EXT_FAMILIES to the centre-lines by
tests/test_centerlines_cpu.py; `ext_symbol` consults them in that order and EXT_LATER last.  EXT_LATER is pinned by no test
to one family: it is where the line simplification and every later family go, each with the same kind of entry, so no
further table is needed.
"""
from __future__ import annotations

import ctypes as C

from . import _lib
from ._lib import f32, i32, i64, sz, vp

POLYGONS_VERSION = 100   # include/vitseg_polygons.h VITSEG_POLYGONS_VERSION this binding was written against
CENTERLINES_VERSION = 100   # include/vitseg_centerlines.h VITSEG_CENTERLINES_VERSION
SIMPLIFY_VERSION = 100   # include/vitseg_simplify.h VITSEG_SIMPLIFY_VERSION
OPTIM_VERSION = 100   # include/vitseg_optim.h VITSEG_OPTIM_VERSION
CURVES_VERSION = 100   # include/vitseg_curves.h VITSEG_CURVES_VERSION
DECIDE_VERSION = 100   # include/vitseg_decide.h VITSEG_DECIDE_VERSION
HARDLOSS_VERSION = 100   # include/vitseg_hardloss.h VITSEG_HARDLOSS_VERSION
CLDICE_VERSION = 100   # include/vitseg_cldice.h VITSEG_CLDICE_VERSION
LOVASZ_VERSION = 100   # include/vitseg_lovasz.h VITSEG_LOVASZ_VERSION


class CHardOptions(C.Structure):
    """struct vitseg_hard_options (include/vitseg_hardloss.h)."""
    _fields_ = [("gamma", C.c_float), ("loss_thresh", C.c_float), ("min_kept", C.c_int64), ("keep_q16", C.c_int32),
                ("reserved", C.c_int32), ("scratch", C.c_void_p), ("scratch_bytes", C.c_size_t)]


phard = C.POINTER(CHardOptions)


class CClDiceOptions(C.Structure):
    """struct vitseg_cldice_options (include/vitseg_cldice.h)."""
    _fields_ = [("weight", C.c_float), ("smooth", C.c_float), ("iters", C.c_int32), ("K", C.c_int32),
                ("classes", C.POINTER(C.c_int32)), ("scratch", C.c_void_p), ("scratch_bytes", C.c_size_t),
                ("prob_planes", C.c_void_p), ("class_terms", C.c_void_p)]


pcld = C.POINTER(CClDiceOptions)


class CLovaszOptions(C.Structure):
    """struct vitseg_lovasz_options (include/vitseg_lovasz.h)."""
    _fields_ = [("weight", C.c_float), ("K", C.c_int32), ("classes", C.POINTER(C.c_int32)), ("per_image", C.c_int32),
                ("present_only", C.c_int32), ("scratch", C.c_void_p), ("scratch_bytes", C.c_size_t),
                ("prob_planes", C.c_void_p), ("grad_planes", C.c_void_p), ("class_terms", C.c_void_p)]


plov = C.POINTER(CLovaszOptions)

EXT_SIGNATURES = {
    # region outlines: polygon rings with holes (polygons.py)
    "polygons": ("vitseg_polygons.h", "the region outlines", [
        ("vitseg_polygons_version", i32, []),
        ("vitseg_region_polygons_scratch_bytes", sz, [i32, i32, i32]),
        ("vitseg_region_polygons", i32, [vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, i32, vp, i64, vp, vp, sz, vp]),
    ]),
}
EXT_FAMILIES = {
    # crack centre-lines as a graph: nodes, branches, polylines (centerlines.py)
    "centerlines": ("vitseg_centerlines.h", "the crack centre-lines", [
        ("vitseg_centerlines_version", i32, []),
        ("vitseg_centerlines_scratch_bytes", sz, [i32, i32, i32, i32]),
        ("vitseg_centerlines", i32, [vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, i32, vp, i32, vp, i64, vp, sz, vp]),
    ]),
}
EXT_LATER = {
    # Douglas-Peucker over rings and polylines on the device (simplify.py); a later family adds its entry here
    "simplify": ("vitseg_simplify.h", "the line simplification", [
        ("vitseg_simplify_version", i32, []),
        ("vitseg_simplify_scratch_bytes", sz, [i32, i32, i64]),
        ("vitseg_simplify_lines", i32, [vp, i64, i32, vp, i32, i32, i32, i32, i32, vp, i32, i64, vp, vp, vp, i64, vp, sz, vp]),
    ]),
    # Adam / AdamW over the arena with groups by chunk, clipping, step skip and a weight EMA (optim.py)
    "optim": ("vitseg_optim.h", "the fine-tuning optimiser", [
        ("vitseg_optim_version", i32, []),
        ("vitseg_optim_scratch_bytes", sz, [sz, i32]),
        ("vitseg_optim_check_groups", i32, [vp, i32, vp, sz]),
        ("vitseg_optim_grad_norm", i32, [vp, sz, vp, vp, i32, f32, vp, sz, vp]),
        ("vitseg_optim_prepare", i32, [vp, vp, i32, sz, i32, f32, f32, f32, f32, f32, vp, sz, vp]),
        ("vitseg_optim_step", i32, [vp, vp, vp, vp, vp, sz, vp, vp, f32, f32, f32, f32, f32, vp, sz, vp]),
    ]),
    # precision-recall counts of a probability map over all thresholds, with a pixel tolerance (curves.py)
    "curves": ("vitseg_curves.h", "the precision-recall curves", [
        ("vitseg_curves_version", i32, []),
        ("vitseg_pr_counts_scratch_bytes", sz, [i32, i32, i32]),
        ("vitseg_pr_counts", i32, [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, sz, vp]),
    ]),
    # a class decided by threshold, with hysteresis (decide.py)
    "decide": ("vitseg_decide.h", "the threshold decision", [
        ("vitseg_decide_version", i32, []),
        ("vitseg_decide_scratch_bytes", sz, [i32, i32, i32]),
        ("vitseg_decide", i32, [vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, i32, i32, vp, vp, vp, sz, vp]),
    ]),
    # focal cross-entropy and online hard example mining on the fused loss path (model.ce_loss)
    "hardloss": ("vitseg_hardloss.h", "the hard-pixel losses", [
        ("vitseg_hardloss_version", i32, []),
        ("vitseg_hard_loss_scratch_bytes", sz, [i32, i32]),
        ("vitseg_hard_ce_loss", i32, [vp, vp, i32, vp, vp, vp, i32, i32, i32, i32, _lib.popt, phard, f32, vp, vp, vp]),
        ("vitseg_backward_hard", i32, [_lib.pcfg, i32, vp, vp, vp, i32, i32, f32, _lib.u64, vp, i32, vp, vp, vp, f32, vp, vp, sz,
                                       vp, _lib.popt, phard, vp]),
    ]),
    # the soft-clDice loss: the soft skeleton, the plane loss and the term on the fused loss path (cldice.py, model.ce_cldice_loss)
    "cldice": ("vitseg_cldice.h", "the soft-clDice loss", [
        ("vitseg_cldice_version", i32, []),
        ("vitseg_soft_skeleton_scratch_bytes", sz, [i32, i32, i32]),
        ("vitseg_soft_skeleton", i32, [vp, i32, i32, i32, i32, vp, vp, vp]),
        ("vitseg_soft_cldice_scratch_bytes", sz, [i32, i32, i32, i32]),
        ("vitseg_soft_cldice", i32, [vp, vp, i32, i32, i32, i32, f32, f32, vp, vp, vp, vp]),
        ("vitseg_cldice_scratch_bytes", sz, [i32, i32, i32, i32]),
        ("vitseg_ce_cldice_loss", i32, [vp, vp, i32, vp, vp, vp, i32, i32, i32, i32, _lib.popt, _lib.pdice, pcld, f32, vp]),
        ("vitseg_backward_cldice", i32, [_lib.pcfg, i32, vp, vp, vp, i32, i32, f32, _lib.u64, vp, i32, vp, vp, vp, f32, vp, vp, sz,
                                         vp, _lib.popt, _lib.pdice, pcld, vp]),
    ]),
    # the Lovasz-Softmax loss: the segmented sort on given planes and the term on the fused loss path (lovasz.py,
    # model.ce_lovasz_loss)
    "lovasz": ("vitseg_lovasz.h", "the Lovasz-Softmax loss", [
        ("vitseg_lovasz_version", i32, []),
        ("vitseg_lovasz_planes_scratch_bytes", sz, [i32, i32]),
        ("vitseg_lovasz_planes", i32, [vp, vp, i32, i32, f32, vp, vp, vp, vp, vp]),
        ("vitseg_lovasz_scratch_bytes", sz, [i32, i32, i32]),
        ("vitseg_ce_lovasz_loss", i32, [vp, vp, i32, vp, vp, vp, i32, i32, i32, i32, _lib.popt, _lib.pdice, plov, f32, vp]),
        ("vitseg_backward_lovasz", i32, [_lib.pcfg, i32, vp, vp, vp, i32, i32, f32, _lib.u64, vp, i32, vp, vp, vp, f32, vp, vp, sz,
                                         vp, _lib.popt, _lib.pdice, plov, vp]),
    ]),
}
EXT_VERSIONS = {"polygons": ("vitseg_polygons_version", POLYGONS_VERSION),
                "centerlines": ("vitseg_centerlines_version", CENTERLINES_VERSION),
                "simplify": ("vitseg_simplify_version", SIMPLIFY_VERSION),
                "optim": ("vitseg_optim_version", OPTIM_VERSION),
                "curves": ("vitseg_curves_version", CURVES_VERSION),
                "decide": ("vitseg_decide_version", DECIDE_VERSION),
                "hardloss": ("vitseg_hardloss_version", HARDLOSS_VERSION),
                "cldice": ("vitseg_cldice_version", CLDICE_VERSION),
                "lovasz": ("vitseg_lovasz_version", LOVASZ_VERSION)}


def ext_symbol(family: str, name: str):
    """The entry point `name` of `family` on `_lib.lib()`'s handle, restype and argtypes set from EXT_SIGNATURES / EXT_FAMILIES /
    EXT_LATER on first use;
    a RuntimeError naming the rebuild when the loaded library predates the family (or `name` is not in its table) or was built
    from another version of its header."""
    _, what, rows = next(t for t in (EXT_SIGNATURES, EXT_FAMILIES, EXT_LATER) if family in t)[family]
    row = {n: (restype, argtypes) for n, restype, argtypes in rows}.get(name)
    fn = getattr(_lib.lib(), name, None) if row is not None else None
    if fn is None:
        raise RuntimeError(f"{_lib.LIB_PATH} has no {name} (built before {what}): rebuild it (python -m visiontransformer_amd.build)")
    if getattr(fn, "_ext_bound", False):
        return fn
    fn.restype, fn.argtypes = row[0], list(row[1])
    vname, version = EXT_VERSIONS[family]
    if name != vname and ext_symbol(family, vname)() != version:
        raise RuntimeError(f"{_lib.LIB_PATH} has {what} at version {ext_symbol(family, vname)()}, this binding expects "
                           f"{version}: rebuild it (python -m visiontransformer_amd.build)")
    fn._ext_bound = True
    return fn
