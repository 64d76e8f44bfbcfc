"""CPU (-m "not gpu"): the confidence entry point's binding and status codes, the host arithmetic on its integers
(scores_from_rows, calibration_from_hist, average_precision), the restatement's own anchor and the flags of the evaluation
scripts.  No compute entry point runs here."""
import ctypes
import math
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

import confidence_ref as CR
from oracle import vitseg_oracle as O
from visiontransformer_amd import _lib, confidence, scripts
from visiontransformer_amd.predict import predict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the binding and the status codes ----

def test_exports_and_header():
    assert _lib.CONFIDENCE_EXPORTS == ["vitseg_confidence"]
    assert set(_lib.CONFIDENCE_EXPORTS) <= set(_lib._LATE_EXPORTS) <= set(_lib.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "vitseg.h")).read()
    assert re.search(r"#define\s+VITSEG_VERSION\s+110\b", hdr) and _lib.VERSION == 110 == _lib.lib().vitseg_version()
    assert re.search(r"\bvitseg_confidence\s*\(", hdr) and _lib.confidence_symbol("vitseg_confidence") is not None
    assert re.search(r"VITSEG_CONF_PROB\s*=\s*0\b", hdr) and re.search(r"VITSEG_CONF_MARGIN\s*=\s*1\b", hdr)
    assert confidence.KINDS == {"prob": _lib.CONF_PROB, "margin": _lib.CONF_MARGIN} == {"prob": 0, "margin": 1} == CR.KINDS


def test_every_status_code_without_a_device():
    """The argument checks come before anything touches a device: every address is a live host buffer no call reaches."""
    fn = _lib.confidence_symbol("vitseg_confidence")
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf)

    def call(*, lowres=p, mask=p, n=1, C=3, g=2, S=8, kind=0, conf=p, conf_q=None, labels=None, scores=None, max_regions=4,
             low_q=100, gt=None, ignore=-1, hist=None, bins=16):
        rc = fn(lowres, mask, n, C, g, S, kind, conf, conf_q, labels, scores, max_regions, low_q, gt, ignore, hist, bins, None)
        assert rc != _lib.OK and _lib.lib().vitseg_last_error()
        return rc

    rows, cal = dict(labels=p, scores=p), dict(gt=p, hist=p)
    for kw in (dict(lowres=None), dict(mask=None), dict(conf=None), dict(conf=None, labels=p), dict(conf=None, gt=p),
               dict(scores=p), dict(hist=p), dict(kind=2), dict(kind=-1), dict(kind=1, C=1),
               dict(max_regions=-1, **rows), dict(low_q=-1, **rows), dict(low_q=65537, **rows),
               dict(bins=0, **cal), dict(bins=257, **cal), dict(ignore=-2, **cal), dict(ignore=256, **cal)):
        assert call(**kw) == _lib.EINVAL, kw
    for kw in (dict(C=0), dict(C=256), dict(n=0), dict(n=65536), dict(S=0), dict(S=16385), dict(g=0), dict(g=9),
               dict(S=16385, g=16385), dict(kind=1, C=256)):
        assert call(**kw) == _lib.ESHAPE, kw
    assert all(b == 0 for b in buf)   # and nothing wrote to the buffers


def test_python_surface_checks_its_arguments_before_the_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(_lib, "confidence_symbol", boom)
    z, m = torch.zeros((1, 3, 2, 2)), torch.zeros((1, 8, 8), dtype=torch.uint8)
    for bad in (dict(kind="max"), dict(lowres=z.double()), dict(lowres=z[0]), dict(mask=m.long()), dict(mask=m[:, :4]),
                dict(lowres=torch.zeros((2, 3, 2, 2))), dict(lowres=torch.zeros((1, 3, 9, 9))), dict(lowres=z[:, :1], kind="margin"),
                dict(lowres=torch.zeros((1, 256, 2, 2)))):
        kw = dict(lowres=z, mask=m, kind="prob")
        kw.update(bad)
        with pytest.raises(ValueError):
            confidence.confidence_map(kw["lowres"], kw["mask"], kind=kw["kind"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        confidence.confidence_map(z, m)
    for low in (-0.1, 1.5, "0.5", True, float("nan")):
        with pytest.raises(ValueError):
            confidence.low_to_q(low)
    assert [confidence.low_to_q(v) for v in (0, 0.5, 1)] == [0, 32768, 65535]


# ---- the restatement's anchor: on the tail's own mask, prob is the sigmoid that won ----

@pytest.mark.parametrize("shape", [(2, 3, 4, 64), (1, 17, 14, 224), (2, 2, 5, 40), (1, 3, 7, 7), (1, 1, 2, 8)])
def test_prob_on_the_argmax_mask_is_the_maximal_sigmoid(shape):
    n, C, g, S = shape
    gen = torch.Generator().manual_seed(S)
    for z in (torch.randn((n, C, g, g), generator=gen), torch.randint(-96, 97, (n, C, g, g), generator=gen).float() * 0.25):
        v = CR.values(z, S)
        sg = O.sigmoid_aten(v)
        own = O.predict_mask(v).to(torch.uint8)
        p, q = CR.score_logits(v, own, "prob")
        assert np.array_equal(p, sg.max(dim=1).values.numpy())
        assert q.min() >= 0 and q.max() <= 65535 and (q[p == 1.0] == 65535).all()
        if C >= 2:
            pm, _ = CR.score_logits(v, own, "margin")
            top2 = sg.topk(2, dim=1).values
            assert np.array_equal(pm, (top2[:, 0] - top2[:, 1]).numpy())   # the winner's lead; 0 on a tie
            wrong = ((own + 1) % C).to(torch.uint8)
            assert (CR.score_logits(v, wrong, "margin")[0] == 0).all()     # a class that did not win leads nobody
    lab = np.array([[[0, 0, -1], [1, 5, 1], [0, -1, 1]]])
    qq = np.array([[[10, 65535, 7], [0, 9, 3], [20, 8, 65535]]])
    rows = CR.score_rows(qq, lab, 3, 10)
    assert rows.tolist() == [[[3, 65565, 65525, 0], [3, 65538, 65535, 2], [0, 0, 0, 0]]]
    h = CR.hist(qq, np.ones((1, 3, 3)), np.array([[[1, 1, 1], [0, 9, 1], [1, 1, 0]]]), 2, 9)
    assert h.tolist() == [[[6, 5, 48], [2, 1, 131070]]]


# ---- host arithmetic on the integers ----

def test_scores_from_rows():
    got = confidence.scores_from_rows(np.array([[4, 4 * 65535, 0, 0], [2, 65535, 65535, 1], [0, 0, 0, 0]], dtype=np.int64))
    assert got[0] == {"pixels": 4, "score": 1.0, "score_min": 1.0, "low_fraction": 0.0}
    assert got[1] == {"pixels": 2, "score": 0.5, "score_min": 0.0, "low_fraction": 0.5}
    assert got[2]["pixels"] == 0 and all(math.isnan(got[2][k]) for k in ("score", "score_min", "low_fraction"))
    with pytest.raises(ValueError):
        confidence.scores_from_rows(np.zeros((2, 3), np.int64))
    recs = np.array([[2, 0, 0, 1, 1, 4, 17]], dtype=np.int32)
    assert confidence.region_dicts(recs, [[4, 2 * 65535, 65535, 2]]) == [
        {"class": 2, "first": 17, "area": 4, "score": 0.5, "score_min": 0.0, "low_fraction": 0.5}]


def test_calibration_from_hist():
    # bin 0: 10 pixels, 2 right, mean confidence 0.25; bin 1 empty; bin 3: 30 pixels, 27 right, mean confidence 1
    h = np.array([[10, 2, 163838], [0, 0, 0], [0, 0, 0], [30, 27, 30 * 65535]], dtype=np.int64)
    cal = confidence.calibration_from_hist(h)
    assert cal["n"] == [10, 0, 0, 30] and cal["total"] == 40
    assert cal["accuracy"][0] == 0.2 and cal["accuracy"][3] == 0.9 and math.isnan(cal["accuracy"][1])
    assert cal["confidence"][0] == 163838 / 655350 and cal["confidence"][3] == 1.0 and math.isnan(cal["confidence"][2])
    assert cal["ece"] == pytest.approx(10 / 40 * abs(0.2 - 163838 / 655350) + 30 / 40 * 0.1, rel=1e-12)
    # pooling before the ratios: two images whose own ECEs are 0.5 and 0.5 pool to a perfectly calibrated bin
    a = np.array([[4, 4, 2 * 65535]], dtype=np.int64)    # accuracy 1, confidence 0.5
    b = np.array([[4, 0, 2 * 65535]], dtype=np.int64)    # accuracy 0, confidence 0.5
    assert confidence.calibration_from_hist(a)["ece"] == confidence.calibration_from_hist(b)["ece"] == 0.5
    assert confidence.calibration_from_hist(np.stack([a, b]))["ece"] == 0.0
    assert confidence.calibration_from_hist(a + b)["ece"] == 0.0
    empty = confidence.calibration_from_hist(np.zeros((4, 3), np.int64))
    assert empty["total"] == 0 and math.isnan(empty["ece"])
    for bad in (np.zeros((4, 2), np.int64), np.zeros((4, 3)), np.zeros(3, np.int64)):
        with pytest.raises(ValueError):
            confidence.calibration_from_hist(bad)
    rows = confidence.calibration_csv_rows((7, "m"), h, 4)
    assert len(rows) == 5 and all(len(r) == len(confidence.CALIBRATION_CSV_COLUMNS) for r in rows)
    assert rows[0][:6] == [7, "m", 0, 0.0, 0.25, 10] and rows[-1][2] == "all" and rows[-1][5] == 40 and rows[-1][8] == cal["ece"]


def test_average_precision():
    ap = confidence.average_precision
    assert ap([0.9, 0.8, 0.7, 0.6, 0.5], [1, 0, 1, 1, 0], 4) == 0.625          # the worked example
    assert ap([0.5, 0.9, 0.6, 0.8, 0.7], [0, 1, 1, 0, 1], 4) == 0.625          # the order given does not matter
    # a tie group enters as one: {0.9: tp} then {0.5: tp, fp, fp} -> P = 1 at R = 1/2, P = 2/4 at R = 1
    assert ap([0.9, 0.5, 0.5, 0.5], [1, 0, 1, 0], 2) == 0.5 * 1.0 + 0.5 * 0.5
    assert ap([0.9, 0.5, 0.5, 0.5], [1, 1, 0, 0], 2) == ap([0.9, 0.5, 0.5, 0.5], [1, 0, 0, 1], 2) == 0.75
    assert ap([1.0, 1.0], [1, 1], 2) == 1.0 and ap([0.3], [0], 5) == 0.0 and ap([], [], 3) == 0.0
    assert math.isnan(ap([0.9], [0], 0)) and math.isnan(ap([], [], 0))
    for bad in (dict(scores=[0.5], matched=[1, 0], n_gt=1), dict(scores=[0.5], matched=[1], n_gt=-1),
                dict(scores=[float("nan")], matched=[1], n_gt=1), dict(scores=[0.5, 0.4], matched=[1, 1], n_gt=1),
                dict(scores=[0.5], matched=[1], n_gt=1.5)):
        with pytest.raises(ValueError):
            ap(**bad)


# ---- predict() and the evaluation scripts ----

def test_predict_refuses_scores_of_blended_views_before_anything_runs():
    def boom(*a, **k):
        raise AssertionError("the model was reached")
    model = types.SimpleNamespace(cfg=types.SimpleNamespace(image_size=224), arena=None, predict_mask=boom,
                                  predict_mask_windowed=boom, predict_mask_tta=boom, _lowres_and_mask=boom)
    img = np.zeros((300, 300, 3), np.uint8)
    for kw in (dict(sliding=True, return_scores=True), dict(sliding=True, return_confidence=True),
               dict(tta="hflip", return_scores=True), dict(tta="d4", return_confidence=True),
               dict(return_scores=True, score_kind="max"), dict(return_confidence=True, low=2.0)):
        with pytest.raises(ValueError):
            predict(img, model, **kw)


def _load_script(rel):
    """model/<dir>/<script>.py as a module; its `from classes import ...` resolves in its own directory."""
    import importlib.util
    path = os.path.join(ROOT, *rel.split("/"))
    sys.path.insert(0, os.path.dirname(path))
    kept = sys.modules.pop("classes", None)
    try:
        spec = importlib.util.spec_from_file_location("confidence_script_" + os.path.basename(path)[:-3], path)
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
def test_evaluation_scripts_pass_the_flags_on(rel, trainer, batches, monkeypatch, tmp_path, capsys):
    mod = _load_script(rel)
    seen = []
    monkeypatch.setattr(mod, trainer, lambda *a, **k: types.SimpleNamespace(model=types.SimpleNamespace(cfg=None)))
    monkeypatch.setattr(scripts, "get_latest_checkpoint", lambda *a: None)
    monkeypatch.setattr(scripts, batches, lambda *a, **k: [])
    monkeypatch.setattr(scripts, "evaluate_to_csv", lambda *a, **k: seen.append(k) or [[0.0] * 12])
    monkeypatch.chdir(tmp_path)
    base = [rel, "--ids", "1", "--num-batches", "1"]
    for extra in ([], ["--region-scores"], ["--calibration"],
                  ["--region-scores", "--score-kind", "margin", "--score-low", "0.7", "--calibration", "32", "--region-metrics"]):
        monkeypatch.setattr(sys, "argv", base + extra)
        mod.main()
    got = [(d["region_scores"], d["score_kind"], d["score_low"], d["calibration_bins"], d["region_classes"]) for d in seen]
    assert got == [(False, "prob", 0.5, None, None), (True, "prob", 0.5, None, None), (False, "prob", 0.5, 16, None),
                   (True, "margin", 0.7, 32, True)]   # without the flags nothing new is asked for
    for extra in (["--region-scores", "--tta", "hflip"], ["--calibration", "--tta", "d4"], ["--calibration", "0"],
                  ["--calibration", "257"], ["--region-scores", "--score-low", "1.5"], ["--score-kind", "max"]):
        monkeypatch.setattr(sys, "argv", base + extra)
        with pytest.raises(SystemExit) as e:
            mod.main()
        assert e.value.code == 2   # refused when the arguments are parsed
    assert len(seen) == 4
    assert "--tta" in capsys.readouterr().err


def test_evaluate_to_csv_refuses_scores_with_tta_before_the_model_runs():
    def boom(*a, **k):
        raise AssertionError("the model was reached")
    model = types.SimpleNamespace(eval=boom, predict_mask=boom)
    for kw in (dict(region_scores=True, tta="hflip"), dict(calibration_bins=16, tta="d4"), dict(calibration_bins=0),
               dict(calibration_bins=257), dict(region_scores=True, score_kind="max"), dict(region_scores=True, score_low=2)):
        with pytest.raises(ValueError):
            scripts.evaluate_to_csv(model, [], (1, "m"), "m_metrics.csv", 3, 1, "cpu", **kw)
