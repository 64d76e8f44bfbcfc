"""CPU (-m "not gpu"): the numpy restatement of vitseg_clean_mask (tests/clean_ref.py) against the committed scipy goldens
and against scipy.ndimage.binary_fill_holes; the argument checks of clean.clean_mask before any library call; the new flags
of the worker and of the evaluation scripts."""
import importlib.util
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

import clean_ref as K
from visiontransformer_amd import _lib, clean, scripts, worker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = np.load(os.path.join(ROOT, "tests", "golden", "clean", "clean.npz"))
CASES = K.clean_cases()


def _kw(variant, bg):
    a, f, h, c = variant
    return dict(min_area=a, fill_holes=bool(f), max_hole_area=h, connectivity=c, background=bg)


def _stats(name, variant):
    return dict(zip(K.STATS, Z[K.key(name, variant) + ".stats"].tolist()))


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_goldens(name):
    m, bg = CASES[name]
    assert np.array_equal(m, Z[f"{name}.mask"]) and int(Z[f"{name}.background"]) == bg   # the generator still makes them
    for v in K.variants(name):
        out, st = K.clean_one(m, **_kw(v, bg))
        assert np.array_equal(out, Z[K.key(name, v) + ".mask"]), v
        assert np.array_equal(st, Z[K.key(name, v) + ".stats"]), v


def test_goldens_hold_the_expected_figures():
    zero = dict.fromkeys(K.STATS, 0)
    # nested: the order of the two steps is the point
    n = "nested_96x120"
    assert _stats(n, (0, 1, 0, 4)) == dict(zero, holes_mixed=1)
    for a in (7, 8):
        assert _stats(n, (a, 1, 0, 4)) == dict(zero, regions_removed=1, pixels_removed=6, holes_filled=1, pixels_filled=6916)
    assert _stats(n, (6, 1, 0, 4)) == dict(zero, holes_mixed=1)                       # the threshold is strict
    assert _stats(n, (8, 1, 6916, 4))["holes_filled"] == 1
    assert _stats(n, (8, 1, 6915, 4)) == dict(zero, regions_removed=1, pixels_removed=6, holes_over_area=1)
    filled = Z[K.key(n, (8, 1, 0, 4)) + ".mask"]
    assert (filled[8:88, 10:110] == 2).all() and filled.sum() == 2 * 80 * 100
    # checkerboard
    c = "checker_64"
    assert _stats(c, (8, 0, 0, 4)) == dict(zero, regions_removed=2048, pixels_removed=2048)
    assert _stats(c, (8, 0, 0, 8)) == zero
    assert _stats(c, (0, 1, 0, 4)) == dict(zero, holes_filled=1922, pixels_filled=1922)
    assert _stats("rings_96", (0, 1, 0, 4)) == dict(zero, holes_filled=1, pixels_filled=52, holes_mixed=3)
    # no enclosed background: fill_holes alone changes nothing; nothing to remove either: no variant changes anything
    for name in K.NO_HOLES + K.UNCHANGED:
        assert np.array_equal(Z[K.key(name, (0, 1, 0, 4)) + ".mask"], Z[f"{name}.mask"]) and _stats(name, (0, 1, 0, 4)) == zero
        for v in K.variants(name):
            assert _stats(name, v)["holes_filled"] == 0
            if name in K.UNCHANGED:
                assert np.array_equal(Z[K.key(name, v) + ".mask"], Z[f"{name}.mask"]) and _stats(name, v) == zero
    # every branch is met on the speckled masks: removed, filled, mixed, over the limit; also with another background
    for name in ("speckle5_97x131", "speckle17_224"):
        assert all(v > 0 for k, v in _stats(name, (8, 1, 20, 4)).items()), name
    s = _stats("speckle5_97x131_bg3", (8, 1, 0, 4))
    assert s["regions_removed"] > 0 and s["holes_filled"] > 0 and s["holes_mixed"] > 0


@pytest.mark.parametrize("name", K.TWO_CLASS)
def test_two_class_fill_is_binary_fill_holes(name):
    ndimage = pytest.importorskip("scipy.ndimage")
    m, bg = CASES[name]
    fg = int(m[m != bg][0])
    for v in [v for v in K.variants(name) if v[1] and not v[2]]:
        step1 = K.clean_one(m, min_area=v[0], connectivity=v[3], background=bg)[0]
        exp = np.where(ndimage.binary_fill_holes(step1 != bg), fg, bg).astype(np.uint8)
        assert np.array_equal(Z[K.key(name, v) + ".mask"], exp), v


@pytest.mark.parametrize("name", ["speckle5_97x131", "speckle17_224", "rings_96", "checker_64"])
def test_restatement_is_idempotent(name):
    m, bg = CASES[name]
    for kw in (dict(min_area=8), dict(min_area=8, connectivity=8), dict(fill_holes=True)):
        once, _ = K.clean_one(m, background=bg, **kw)
        twice, st = K.clean_one(once, background=bg, **kw)
        assert np.array_equal(once, twice) and not st[[0, 1, 2, 3]].any(), kw


def test_clean_ref_shapes():
    m = np.stack([CASES["speckle5_97x131"][0]] * 2)
    out, st = K.clean_ref(m, min_area=8, fill_holes=True)
    one, st1 = K.clean_ref(m[0], min_area=8, fill_holes=True)
    assert out.shape == m.shape and np.array_equal(out[1], one) and st == [st1, st1] and list(st1) == list(K.STATS)


def test_clean_mask_rejects_bad_arguments_before_the_library(monkeypatch):
    def no_call(name):
        raise AssertionError(f"{name} reached")
    monkeypatch.setattr(_lib, "clean_symbol", no_call)
    ok = torch.zeros(2, 4, 4, dtype=torch.uint8)
    bad = [
        (torch.zeros(2, 4, 4, dtype=torch.float32), {}),          # dtype
        (torch.zeros(2, 4, 4, dtype=torch.int32), {}),
        (torch.zeros(4, dtype=torch.uint8), {}),                  # shape
        (torch.zeros(1, 2, 4, 4, dtype=torch.uint8), {}),
        (torch.zeros(2, 0, 4, dtype=torch.uint8), {}),
        (ok, {"connectivity": 6}),                                # connectivity
        (ok, {"background": 256}),                                # background: 0..255, there is no "none"
        (ok, {"background": -1}),
        (ok, {"background": True}),
        (ok, {"min_area": -1}),                                   # the counts
        (ok, {"min_area": 2.5}),
        (ok, {"min_area": True}),
        (ok, {"min_area": 1 << 31}),
        (ok, {"max_hole_area": -3}),
        (ok, {"max_hole_area": "4"}),
        (ok, {"fill_holes": 1}),                                  # a bool
        (ok, {"fill_holes": "yes"}),
        (torch.full((3, 3), 256, dtype=torch.long), {}),          # value range
        (torch.full((3, 3), -1, dtype=torch.long), {}),
        ([[0, 1]], {}),
    ]
    for mask, kw in bad:
        for on in ({}, {"min_area": 8, "fill_holes": True}):      # refused whether or not a step is on
            with pytest.raises(ValueError):
                clean.clean_mask(mask, **{**on, **kw})


def test_clean_mask_with_both_steps_off_returns_its_argument(monkeypatch):
    def no_call(name):
        raise AssertionError(f"{name} reached")
    monkeypatch.setattr(_lib, "clean_symbol", no_call)
    for m in (torch.zeros(2, 4, 4, dtype=torch.uint8), torch.ones(5, 3, dtype=torch.long), np.zeros((3, 4), np.uint8)):
        assert clean.clean_mask(m) is m
        assert clean.clean_mask(m, min_area=1, max_hole_area=9, connectivity=8, background=7) is m   # 0 and 1 change nothing
        out, st = clean.clean_mask(m, return_stats=True)
        assert out is m
        st = [st] if m.ndim == 2 else st
        assert len(st) == (1 if m.ndim == 2 else m.shape[0]) and all(s == dict.fromkeys(K.STATS, 0) for s in st)
    assert clean.STATS == K.STATS


def test_clean_symbols_are_declared_and_exported():
    assert _lib.CLEAN_EXPORTS == ["vitseg_clean_scratch_bytes", "vitseg_clean_mask"]
    hdr = open(os.path.join(ROOT, "include", "vitseg.h")).read()
    for name in _lib.CLEAN_EXPORTS:
        assert name in _lib.EXPORTS and name in _lib._LATE_EXPORTS
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    f = _lib.clean_symbol("vitseg_clean_scratch_bytes")
    r = _lib.region_symbol("vitseg_regions_scratch_bytes")
    assert f(0, 4, 4) == 0 and f(1, 0, 4) == 0 and f(1, 1 << 16, 1 << 15) == 0   # bad shapes: no size
    for shape in ((2, 64, 64), (1, 97, 131), (32, 512, 512)):
        n, H, W = shape
        assert r(*shape) + 4 * n * H * W <= f(*shape) <= r(*shape) + 4 * n * H * W + 512   # the labelling's + one word a pixel


def test_worker_flags_and_slot_validation():
    a = worker.build_parser().parse_args(["--model", "0:2"])
    assert clean.arguments(a) == dict(min_area=0, fill_holes=False, max_hole_area=0)
    a = worker.build_parser().parse_args(["--model", "0:2", "--min-area", "8", "--fill-holes", "--max-hole-area", "64"])
    assert clean.arguments(a) == dict(min_area=8, fill_holes=True, max_hole_area=64)
    for argv in (["--min-area", "-1"], ["--max-hole-area", "x"], ["--min-area", "2.5"], ["--fill-holes", "1"]):
        with pytest.raises(SystemExit):
            worker.build_parser().parse_args(["--model", "0:2"] + argv)
    # a bad value is refused when the slot is built: before a model is loaded, not at the first job
    for kw in (dict(min_area=-1), dict(max_hole_area=-1), dict(fill_holes="yes"), dict(min_area=1.5)):
        with pytest.raises(ValueError):
            worker.gpu_slot(0, 2, device="no-such-device", **kw)


def _load_script(rel):
    """model/<dir>/<script>.py as a module; its `from classes import ...` resolves in its own directory."""
    path = os.path.join(ROOT, *rel.split("/"))
    sys.path.insert(0, os.path.dirname(path))
    kept = sys.modules.pop("classes", None)
    try:
        spec = importlib.util.spec_from_file_location("script_under_test_" + os.path.basename(path)[:-3], path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(os.path.dirname(path))
        sys.modules.pop("classes", None)
        if kept is not None:
            sys.modules["classes"] = kept
    return mod


@pytest.mark.parametrize("rel,trainer,batches", [("model/CE/datasetTestViTmodel.py", "LightningViTModel", "ce_batches"),
                                                ("model/PAED/ViTscriptTest.py", "PAEDTrainer", "paed_binary_batches")])
def test_evaluation_scripts_pass_the_flags_on(rel, trainer, batches, monkeypatch, tmp_path):
    mod = _load_script(rel)
    seen = []
    monkeypatch.setattr(mod, trainer, lambda *a, **k: types.SimpleNamespace(model=types.SimpleNamespace(cfg=None)))
    monkeypatch.setattr(scripts, "get_latest_checkpoint", lambda *a: None)
    monkeypatch.setattr(scripts, batches, lambda *a, **k: [])
    monkeypatch.setattr(scripts, "evaluate_to_csv", lambda *a, **k: seen.append(k) or [[0.0] * 12])
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(sys, "argv", [rel, "--ids", "1", "--num-batches", "1"])
    mod.main()
    monkeypatch.setattr(sys, "argv", [rel, "--ids", "1", "--num-batches", "1", "--min-area", "8", "--fill-holes",
                                      "--max-hole-area", "64"])
    mod.main()
    off, on = [{k: d[k] for k in ("min_area", "fill_holes", "max_hole_area")} for d in seen]
    assert off == dict(min_area=0, fill_holes=False, max_hole_area=0)
    assert on == dict(min_area=8, fill_holes=True, max_hole_area=64)
    monkeypatch.setattr(sys, "argv", [rel, "--min-area", "-8"])
    with pytest.raises(SystemExit):
        mod.main()
    assert len(seen) == 2


def test_single_image_script_passes_the_flags_on(monkeypatch):
    mod = _load_script("model/CE/testViTModel.py")
    seen = []
    monkeypatch.setattr(mod, "load_model", lambda *a, **k: None)
    monkeypatch.setattr(mod, "predict", lambda image, model, **k: seen.append(k) or np.zeros((4, 4), np.uint8))
    monkeypatch.setattr(sys, "argv", ["testViTModel.py", "x.png", "--min-area", "5", "--fill-holes"])
    mod.main()
    assert {k: seen[0][k] for k in ("min_area", "fill_holes", "max_hole_area")} == dict(min_area=5, fill_holes=True,
                                                                                      max_hole_area=0)
    monkeypatch.setattr(sys, "argv", ["testViTModel.py", "x.png", "--max-hole-area", "-1"])
    with pytest.raises(SystemExit):
        mod.main()


def test_evaluate_to_csv_and_predict_refuse_bad_options_first():
    from visiontransformer_amd.predict import predict
    with pytest.raises(ValueError):
        scripts.evaluate_to_csv(None, [], (0, "x", 16, 192, 2, 3), "unused.csv", 2, 1, "cpu", min_area=-1)
    with pytest.raises(ValueError):
        predict(np.zeros((8, 8, 3), np.uint8), None, max_hole_area=-1)
