"""CPU (-m "not gpu"): the threshold decision's family header against `_ext.EXT_LATER`, the threshold arithmetic against the
curves' own, the argument checks, the restatement tests/decide_ref.py against an answer written out by hand, the flags of the
evaluation scripts and predict()'s refusals.  No compute entry point runs."""
import argparse
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import decide_ref as DR
from test_binding_cpu import parse_header, signature_errors
from visiontransformer_amd import _ext, _lib, curves, decide, scripts, worker
from visiontransformer_amd.predict import predict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vitseg_decide.h")
NAMES = ["vitseg_decide_version", "vitseg_decide_scratch_bytes", "vitseg_decide"]


# ---- the family header and its table ----

def _table():
    return {name: (restype, list(argtypes)) for name, restype, argtypes in _ext.EXT_LATER["decide"][2]}


def test_family_header_is_the_table_both_ways():
    decls, structs, enums, defines = parse_header(open(HEADER).read())
    assert _ext.EXT_LATER["decide"][:2] == ("vitseg_decide.h", "the threshold decision")
    assert sorted(decls) == sorted(NAMES) == sorted(_table()) and not structs and not enums
    assert signature_errors(decls, _table()) == []
    assert len(decls["vitseg_decide"][1]) == 18 and decls["vitseg_decide"][1][14] == ("int64_t", 1)
    assert defines == {"VITSEG_DECIDE_VERSION": 100}
    assert _ext.DECIDE_VERSION == 100 and _ext.EXT_VERSIONS["decide"] == ("vitseg_decide_version", 100)
    tab = _table()
    tab["vitseg_decide"] = (C.c_int, tab["vitseg_decide"][1][:16] + [C.c_int] + tab["vitseg_decide"][1][17:])
    assert signature_errors(decls, tab) == ["vitseg_decide: argument 16: c_int for size_t"]   # the comparison can fail
    assert not set(NAMES) & set(_lib.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "vitseg.h")).read()
    assert "vitseg_decide" not in hdr.lower() and '#include "vitseg.h"' in open(HEADER).read()


def test_library_exports_the_family_at_its_version():
    l = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(l, name), name
    assert _ext.ext_symbol("decide", "vitseg_decide_version")() == 100
    fn = _ext.ext_symbol("decide", "vitseg_decide")
    assert fn.restype is C.c_int and list(fn.argtypes) == _table()["vitseg_decide"][1]
    size = _ext.ext_symbol("decide", "vitseg_decide_scratch_bytes")
    assert size.restype is C.c_size_t
    assert size(3, 130, 0) == 0 and size(0, 8, 1) == 0 and size(1, 16385, 1) == 0
    regions = _lib.symbol("vitseg_regions_scratch_bytes")
    up = lambda v: (v + 255) // 256 * 256
    for n, S in ((1, 1), (3, 130), (2, 96)):   # the labelling's words, then the level and the flag plane
        assert size(n, S, 1) == up(regions(n, S, S)) + 2 * up(n * S * S)


def test_every_status_code_without_a_device():
    """The argument checks come before any launch: every address is a live host buffer that no call reaches."""
    fn = _ext.ext_symbol("decide", "vitseg_decide")
    size = _ext.ext_symbol("decide", "vitseg_decide_scratch_bytes")
    buf, other = (C.c_uint8 * 4096)(), (C.c_uint8 * 64)()
    p, p2 = C.addressof(buf), C.addressof(other)
    need = size(1, 8, 1)
    assert need > 0

    def call(lowres=p, n=1, Cc=2, g=2, S=8, cls=1, kind=0, high=40000, low=20000, conn=4, base=None, value=1, off=0, mask=p,
             counts=p, scratch=p, nbytes=need):
        return fn(lowres, n, Cc, g, S, cls, kind, high, low, conn, base, value, off, mask, counts, scratch, nbytes, None)
    for kw in (dict(lowres=None), dict(mask=None), dict(base=p), dict(kind=2), dict(kind=-1), dict(kind=1, Cc=1, cls=0),
               dict(cls=-1), dict(cls=2), dict(low=-1), dict(high=65537), dict(low=40001), dict(high=0), dict(conn=6), dict(conn=0),
               dict(value=-1), dict(value=256), dict(off=-1), dict(off=256), dict(value=3, off=3), dict(scratch=None)):
        assert call(**kw) == _lib.EINVAL, kw
        assert b"decide" in _lib.lib().vitseg_last_error()
    for kw in (dict(n=0), dict(n=65536), dict(Cc=0), dict(Cc=256), dict(S=0), dict(S=16385), dict(g=0), dict(g=9)):
        assert call(**kw) == _lib.ESHAPE, kw
        with pytest.raises(ValueError, match="decide: bad shape"):
            _lib.check(_lib.ESHAPE)
    assert call(nbytes=need - 1) == _lib.EWORKSPACE and call(nbytes=0) == _lib.EWORKSPACE
    assert call(base=p2, nbytes=need - 1) == _lib.EWORKSPACE   # a base elsewhere passes the pointer checks
    assert bytes(buf) == bytes(4096) and bytes(other) == bytes(64)   # nothing was written


# ---- thresholds ----

def test_threshold_to_q_inverts_the_curves_thresholds():
    qs = np.arange(65536)
    ts = qs / 65535   # the float division `curves._curve` reports thresholds with
    got = np.array([decide.threshold_to_q(float(t)) for t in ts])
    assert np.array_equal(got, qs)
    assert decide.threshold_to_q(0) == 0 and decide.threshold_to_q(1) == 65535 and decide.threshold_to_q(np.float32(0.5)) == 32768
    assert decide.threshold_to_q(0.5) == 32768 and decide.threshold_to_q(32767 / 65535) == 32767
    assert decide.threshold_to_q(np.nextafter(0.5, 1)) == 32768 and decide.threshold_to_q(np.nextafter(32767 / 65535, 1)) == 32768
    for bad in (-0.001, 1.0001, float("nan"), float("inf"), None, "0.5", True, 2):
        with pytest.raises(ValueError):
            decide.threshold_to_q(bad)


@pytest.mark.parametrize("bins", [1, 7, 256, 1024])
def test_the_ods_threshold_comes_back_as_its_integer(bins):
    rs = np.random.RandomState(bins)
    counts = rs.randint(0, 50, size=(3, bins, 3)).astype(np.int64)
    counts[:, :, 1] = np.minimum(counts[:, :, 1], counts[:, :, 0])
    o = curves.ods(counts)
    assert decide.threshold_to_q(o["threshold"]) == curves.threshold_q(o["k"], bins)
    cur = curves.curve_from_counts(counts)
    for k in range(bins):   # and every other row of the curve
        assert decide.threshold_to_q(cur["threshold"][k]) == curves.threshold_q(k, bins), k


def test_check_options_takes_and_refuses_what_the_header_lists():
    assert decide.check_options() == (32768, 32768, 1)
    assert decide.check_options(2, 0.6, 0.4, 8, "margin") == (decide.threshold_to_q(0.6), decide.threshold_to_q(0.4), 2)
    assert decide.check_options(0, high_q=65536, low_q=0, value=7, off=9) == (65536, 0, 7)
    assert decide.check_options(3, 0.5, 0.5) == (32768, 32768, 3)
    assert decide.check_options(1, high_q=0) == (0, 0, 1) and decide.check_options(1, 1.0, low_q=65535) == (65535, 65535, 1)
    for kw in (dict(cls=-1), dict(cls=255), dict(cls=True), dict(cls=1.0), dict(threshold=1.5), dict(threshold=-0.1),
               dict(threshold=float("nan")), dict(threshold="0.5"), dict(threshold=None), dict(low=0.6), dict(low=-0.1),
               dict(low=float("inf")), dict(connectivity=6), dict(connectivity=None), dict(kind="softmax"), dict(value=256),
               dict(value=-1), dict(value=1.0), dict(off=256), dict(off=-1), dict(off=1), dict(cls=0), dict(value=4, off=4),
               dict(high_q=65537), dict(high_q=-1), dict(high_q=0.5), dict(low_q=65537), dict(high_q=10, low_q=11),
               dict(low=0.2, low_q=100), dict(low_q=40000)):
        with pytest.raises(ValueError):
            decide.check_options(**kw)
    assert decide.check_model_options(2, 1, 0.5, 0.25, 8, "margin") == 1 and decide.check_model_options(17, 16) == 16
    assert decide.check_model_options(1, 0) == 1   # a one-class model's class is the foreground its ground truth labels 1
    for args in ((2, 2), (2, 0), (1, 1), (1, 0, 0.5, None, 4, "margin"), (2, 1, 0.5, 0.6), (2, 1, 2.0), (2, 1, 0.5, None, 5)):
        with pytest.raises(ValueError):
            decide.check_model_options(*args)


def test_threshold_mask_rejects_bad_arguments_before_the_library(monkeypatch):
    def no_call(*a, **k):
        raise AssertionError(f"{a} requested")
    monkeypatch.setattr(_ext, "ext_symbol", no_call)
    low, base = torch.zeros((2, 3, 4, 4)), torch.zeros((2, 8, 8), dtype=torch.uint8)
    for kw in (dict(cls=3), dict(cls=-1), dict(threshold=2), dict(low=0.7), dict(kind="softmax"), dict(connectivity=5),
               dict(size=None), dict(size=0), dict(size=3), dict(size=16385), dict(size=8.0), dict(base=base.float()),
               dict(base=base[0]), dict(base=torch.zeros((2, 8, 9), dtype=torch.uint8)), dict(base=base, size=9),
               dict(base=torch.zeros((3, 8, 8), dtype=torch.uint8)), dict(base=torch.zeros((2, 2, 2), dtype=torch.uint8)),
               dict(lowres=low.double()), dict(lowres=low[:, :, :3]), dict(lowres=low[:, :1], kind="margin", cls=0, value=1),
               dict(lowres=low[0], base=base), dict(value=0), dict(off=1), dict(lowres="z")):
        args = dict(lowres=low, size=8)
        args.update(kw)
        with pytest.raises(ValueError):
            decide.threshold_mask(**args)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        decide.threshold_mask(low, size=8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        decide.threshold_mask(low[0], base=base[0].numpy())


# ---- the restatement against an answer written out by hand ----

# w: weak (q = 30000), S: strong (q = 50000), .: below both (q = 100); low_q = 30000, high_q = 50000
PLANE = ["w.......",    # a diagonal chain from (0, 0) to (3, 3), its far end strong: whole at 8, only its end at 4
         ".w......",
         "..w...ww",    # a weak pair at the frame with no strong pixel: gone at both
         "...S....",
         "........",
         "wwSww..w",    # a row through a strong pixel: whole at both; a lone weak pixel diagonal to nothing strong
         "......S.",    # a strong pixel alone, diagonal to the weak (5, 7): it keeps itself, and (5, 7) at 8
         "S.....w."]    # a strong corner pixel; a weak pixel below the strong (6, 6): kept at both
KEPT4 = ["........",
         "........",
         "........",
         "...S....",
         "........",
         "wwSww...",
         "......S.",
         "S.....w."]
KEPT8 = ["w.......",
         ".w......",
         "..w.....",
         "...S....",
         "........",
         "wwSww..w",
         "......S.",
         "S.....w."]


def _plane(rows):
    return np.array([[{".": 100, "w": 30000, "S": 50000}[c] for c in r] for r in rows], np.int64)[None]


def test_the_restatement_on_a_plane_written_out_by_hand():
    q = _plane(PLANE)
    for conn, rows in ((4, KEPT4), (8, KEPT8)):
        want = np.array([[c != "." for c in r] for r in rows])[None]
        weak, strong, kept = DR.kept_planes(q, 50000, 30000, conn)
        assert np.array_equal(kept, want), conn
        assert int(weak.sum()) == 15 and int(strong.sum()) == 4
        mask, counts = DR.decide_q(q, 50000, 30000, conn, value=3, off=9)
        assert np.array_equal(mask, np.where(want, 3, 9)) and counts.tolist() == [[15, 4, int(want.sum())]]
    assert int(np.array([[c != "." for c in r] for r in KEPT4]).sum()) == 9
    assert int(np.array([[c != "." for c in r] for r in KEPT8]).sum()) == 13
    # the equality: a threshold at a pixel's own score keeps it, one above drops it
    assert DR.kept_planes(q, 50001, 30000, 8)[2].sum() == 0 and DR.kept_planes(q, 50000, 30001, 8)[2].sum() == 4
    # the plain cut is the strong plane; 65536 is reached by nothing; 0 by everything
    assert np.array_equal(DR.kept_planes(q, 30000, 30000)[2], q >= 30000)
    assert DR.kept_planes(q, 65536, 0)[2].sum() == 0 and DR.kept_planes(q, 0, 0)[2].all()
    # the base rule: kept pixels state the value, a base pixel that states it elsewhere becomes off, the rest stays
    base = np.full((1, 8, 8), 2, np.uint8)
    base[0, 0] = 1          # row 0 states the value: (0, 0) is kept at 8, the others become off
    base[0, 5, :3] = 5      # under kept pixels: overwritten
    mask, _ = DR.decide_q(q, 50000, 30000, 8, base=base, value=1, off=7)
    assert mask[0, 0].tolist() == [1, 7, 7, 7, 7, 7, 7, 7] and mask[0, 5].tolist() == [1, 1, 1, 1, 1, 2, 2, 1]
    assert mask[0, 4].tolist() == [2] * 8 and np.array_equal(base[0, 0], np.ones(8))   # (the base itself is not written)


# ---- the flags ----

CSV = "out/ID1/ID1_metrics.csv"


def _options(argv, classes=True):
    ap = argparse.ArgumentParser()
    if classes:
        ap.add_argument("--num-classes", type=int, default=3)
    scripts.add_evaluation_arguments(ap)
    return scripts.evaluation_options(ap, ap.parse_args(argv), CSV)


def test_the_flags_add_their_keys_only_with_threshold_and_are_refused_at_parse_time():
    none = _options([])
    assert not any(k.startswith("threshold") for k in none)   # without the flag nothing new is asked for
    assert _options(["--threshold-class", "2", "--threshold-connectivity", "8"]) == none   # the options alone ask for nothing
    assert _options(["--threshold", "0.31"]) == dict(none, threshold=0.31, threshold_low=None, threshold_class=1,
                                                     threshold_connectivity=4, threshold_over_argmax=False)
    got = _options(["--threshold", "0.6", "--threshold-low", "0.4", "--threshold-class", "2", "--threshold-connectivity", "8",
                    "--threshold-over-argmax", "--score-kind", "margin"])
    assert got == dict(none, threshold=0.6, threshold_low=0.4, threshold_class=2, threshold_connectivity=8,
                       threshold_over_argmax=True, score_kind="margin")
    assert _options(["--threshold", "0.5", "--threshold-class", "0", "--num-classes", "1"])["threshold_class"] == 0
    assert _options(["--threshold", "0.5"], classes=False)["threshold"] == 0.5   # a parser without --num-classes
    for argv in (["--threshold", "0.5", "--tta", "hflip"], ["--threshold-low", "0.2"], ["--threshold-over-argmax"],
                 ["--threshold", "0.4", "--threshold-low", "0.6"], ["--threshold", "1.5"], ["--threshold", "-0.1"],
                 ["--threshold", "nan"], ["--threshold", "x"], ["--threshold", "0.5", "--threshold-low", "-1"],
                 ["--threshold", "0.5", "--threshold-class", "3"], ["--threshold", "0.5", "--threshold-class", "-1"],
                 ["--threshold", "0.5", "--threshold-class", "0"], ["--threshold", "0.5", "--threshold-connectivity", "6"],
                 ["--threshold", "0.5", "--score-kind", "margin", "--num-classes", "1", "--threshold-class", "0"]):
        with pytest.raises(SystemExit):
            _options(argv)

    def boom(*a, **k):
        raise AssertionError("the model was reached")
    model = types.SimpleNamespace(eval=boom, cfg=types.SimpleNamespace(num_classes=2))
    for kw in (dict(threshold=0.5, tta="hflip"), dict(threshold_low=0.2), dict(threshold=0.4, threshold_low=0.6),
               dict(threshold=0.5, threshold_class=2), dict(threshold=0.5, threshold_class=0), dict(threshold=2),
               dict(threshold=0.5, threshold_connectivity=6), dict(threshold=0.5, score_kind="softmax")):
        with pytest.raises(ValueError):
            scripts.evaluate_to_csv(model, [], (1, "m"), CSV, 2, 1, "cpu", **kw)


@pytest.mark.parametrize("rel,trainer,batches", [("model/CE/datasetTestViTmodel.py", "LightningViTModel", "ce_batches"),
                                                ("model/PAED/ViTscriptTest.py", "PAEDTrainer", "paed_binary_batches")])
def test_evaluation_scripts_pass_the_flags_on(rel, trainer, batches, monkeypatch, tmp_path):
    import sys
    from test_polygons_cpu import _load_script
    mod = _load_script(rel)
    seen = []
    monkeypatch.setattr(mod, trainer, lambda *a, **k: types.SimpleNamespace(model=types.SimpleNamespace(cfg=None)))
    monkeypatch.setattr(scripts, "get_latest_checkpoint", lambda *a: None)
    monkeypatch.setattr(scripts, batches, lambda *a, **k: [])
    monkeypatch.setattr(scripts, "evaluate_to_csv", lambda *a, **k: seen.append((a, k)) or [[0.0] * 12])
    monkeypatch.chdir(tmp_path)
    base = [rel, "--ids", "1", "--num-batches", "1", "--num-classes", "2"]
    for extra in ([], ["--threshold", "0.31"], ["--threshold", "0.6", "--threshold-low", "0.4", "--threshold-connectivity", "8"]):
        monkeypatch.setattr(sys, "argv", base + extra)
        mod.main()
    pick = lambda kw: {k: v for k, v in kw.items() if k.startswith("threshold")}
    assert pick(seen[0][1]) == {}
    assert pick(seen[1][1]) == dict(threshold=0.31, threshold_low=None, threshold_class=1, threshold_connectivity=4,
                                    threshold_over_argmax=False)
    assert pick(seen[2][1]) == dict(threshold=0.6, threshold_low=0.4, threshold_class=1, threshold_connectivity=8,
                                    threshold_over_argmax=False)
    for extra in (["--threshold", "0.5", "--tta", "hflip"], ["--threshold", "0.5", "--threshold-class", "2"],
                  ["--threshold-low", "0.3"]):
        monkeypatch.setattr(sys, "argv", base + extra)
        with pytest.raises(SystemExit):
            mod.main()
    assert len(seen) == 3   # refused when the arguments are parsed: no model was built


# ---- predict() and the worker ----

class _Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"the model was reached for {name}")


def test_predict_refuses_sliding_and_tta_before_it_touches_the_model():
    image = np.zeros((8, 8, 3), np.uint8)
    for kw in (dict(sliding=True), dict(tta="hflip"), dict(tta="d4", threshold_low=0.2)):
        with pytest.raises(ValueError, match="threshold with sliding=True or tta="):
            predict(image, _Untouchable(), threshold=0.5, **kw)
    with pytest.raises(ValueError, match="threshold_low needs threshold"):
        predict(image, _Untouchable(), threshold_low=0.2)
    model = types.SimpleNamespace(cfg=types.SimpleNamespace(num_classes=2, image_size=224))   # the options, then nothing else
    for kw in (dict(threshold=1.5), dict(threshold=0.4, threshold_low=0.6), dict(threshold=0.5, threshold_class=2),
               dict(threshold=0.5, threshold_connectivity=6), dict(threshold=0.5, threshold_kind="softmax")):
        with pytest.raises(ValueError):
            predict(image, model, **kw)


def test_the_worker_has_the_flags():
    a = worker.build_parser().parse_args(["--model", "1:2", "--threshold", "0.31", "--threshold-low", "0.2", "--threshold-kind",
                                          "margin", "--threshold-connectivity", "8", "--threshold-over-argmax"])
    assert (a.threshold, a.threshold_low, a.threshold_class, a.threshold_connectivity, a.threshold_kind,
            a.threshold_over_argmax) == (0.31, 0.2, 1, 8, "margin", True)
    a = worker.build_parser().parse_args(["--model", "1:2"])
    assert a.threshold is None and a.threshold_low is None and not a.threshold_over_argmax
