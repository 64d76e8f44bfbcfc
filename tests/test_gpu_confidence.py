"""GPU (-m gpu): confidence on the device (vitseg_confidence, confidence.confidence_map / region_scores / calibration_hist,
predict_confidence, predict_regions(scores=True)) against the CPU restatement tests/confidence_ref.py.  The device results are
integers or single-rounded fp32 values: every comparison is bit for bit, there is no tolerance.  Outputs live in guard-banded
buffers."""
import numpy as np
import pytest
import torch

import confidence_ref as CR
from guard import check, guarded, snapshot, unchanged
from oracle import vitseg_oracle as O
from visiontransformer_amd import _lib, clean, confidence, regions

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_REF = {}

# (n, C, g, S): 40 is no multiple of the chunk's rows; 7: g == S and odd (scalar path, identity taps); (1, 3, 256, 256): the
# source rows of a chunk do not fit the LDS (global-memory route)
SHAPES = [(2, 3, 4, 64), (1, 17, 14, 224), (2, 2, 5, 40), (1, 3, 7, 7), (1, 1, 2, 8), (1, 3, 256, 256)]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _inputs(shape, src):
    """(lowres, v = the oracle's full-size logits, the oracle's argmax mask, a scrambled mask with values >= C), once per key"""
    key = (shape, src)
    if key not in _REF:
        n, C, g, S = shape
        gen = torch.Generator().manual_seed(1000 * S + 10 * C + (src == "quantised"))
        if src == "randn":
            z = torch.randn((n, C, g, g), generator=gen)
        else:   # multiples of 0.25 up to +-24: saturated sigmoids (exactly 1.0f) and ties between classes
            z = torch.randint(-96, 97, (n, C, g, g), generator=gen).float() * 0.25
        v = CR.values(z, S)
        own = O.predict_mask(v).to(torch.uint8)
        scr = torch.randint(0, C + 2, (n, S, S), generator=gen).to(torch.uint8)
        _REF[key] = (z, v, own, scr)
    return _REF[key]


def _call(z, mask, kind, want_conf=False, want_q=False, labels=None, max_regions=0, low_q=0, gt=None, ignore=-1, bins=0):
    """One vitseg_confidence call through the C ABI on guarded buffers: dict of numpy results"""
    n, C, g, _ = z.shape
    S = mask.shape[-1]
    zd = guarded(z.shape, torch.float32, z.to(DEV), name="lowres")
    md = guarded(mask.shape, torch.uint8, mask.to(DEV), name="mask")
    ld = None if labels is None else guarded(labels.shape, torch.int32, labels.to(DEV), name="labels")
    gd = None if gt is None else guarded(gt.shape, torch.uint8, gt.to(DEV), name="gt")
    conf = guarded((n, S, S), torch.float32, name="conf") if want_conf else None
    cq = guarded((n, S, S), torch.uint16, name="conf_q") if want_q else None
    rows = guarded((n, max_regions, 4), torch.int64, name="scores") if labels is not None else None
    hist = guarded((n, bins, 3), torch.int64, name="hist") if gt is not None else None
    snap = snapshot(zd, md, ld, gd)
    p = lambda t: None if t is None else t.data_ptr()
    _lib.check(_lib.confidence_symbol("vitseg_confidence")(
        p(zd), p(md), n, C, g, S, CR.KINDS[kind], p(conf), p(cq), p(ld), p(rows), max_regions, low_q, p(gd), ignore, p(hist),
        bins, _stream()))
    torch.cuda.synchronize()
    check(zd, md, ld, gd, conf, cq, rows, hist)
    unchanged(snap)
    out = dict(conf=conf, q=cq, rows=rows, hist=hist)
    return {k: None if t is None else t.cpu().numpy() for k, t in out.items()}


def _labels(mask, max_regions=1024, background=0, connectivity=4):
    """vitseg_regions on the mask: (counts, records [n, max_regions, 7], labels int32 [n, S, S]) on the host"""
    counts, recs, labels = regions._launch(mask.to(DEV).contiguous(), background, connectivity, max_regions, True)
    torch.cuda.synchronize()
    return counts.cpu().numpy(), recs[:, :, :7].cpu().numpy(), labels.cpu()


@pytest.mark.parametrize("src", ["randn", "quantised"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_maps_equal_the_restatement(shape, src):
    z, v, own, scr = _inputs(shape, src)
    C = shape[1]
    if src == "quantised" and shape[3] >= 64 and C >= 2:
        s = O.sigmoid_aten(v)
        assert (s.max(dim=1).values == 1.0).float().mean() > 0.01                       # saturated to exactly 1.0f
        assert int(((s == s.max(dim=1, keepdim=True).values).sum(dim=1) > 1).sum()) > 0   # ties between classes
    for kind in (("prob", "margin") if C >= 2 else ("prob",)):
        for mask in (own, scr):
            p, q = CR.score_logits(v, mask, kind)
            if mask is scr:
                assert (p[(scr >= C).numpy()] == 0).all() and int((scr >= C).sum()) > 0
            both = _call(z, mask, kind, want_conf=True, want_q=True)
            assert np.array_equal(both["conf"].view(np.uint32), p.view(np.uint32)), (kind, "conf")
            assert np.array_equal(both["q"].astype(np.int64), q), (kind, "conf_q")
            assert np.array_equal(_call(z, mask, kind, want_conf=True)["conf"].view(np.uint32), p.view(np.uint32))
            assert np.array_equal(_call(z, mask, kind, want_q=True)["q"].astype(np.int64), q)
        if kind == "prob":   # on the tail's own mask: the sigmoid that won
            assert np.array_equal(CR.score_logits(v, own, "prob")[0], O.sigmoid_aten(v).max(dim=1).values.numpy())


def test_the_global_route_gives_the_staged_bits():
    shape = (2, 3, 4, 64)
    z, v, own, _ = _inputs(shape, "quantised")
    for kind in ("prob", "margin"):
        p, q = CR.score_logits(v, own, kind)
        with _lib.option("upsample_global", 1):
            got = _call(z, own, kind, want_conf=True, want_q=True)
        assert np.array_equal(got["conf"].view(np.uint32), p.view(np.uint32)) and np.array_equal(got["q"].astype(np.int64), q)


@pytest.mark.parametrize("shape", [(2, 3, 4, 64), (1, 17, 14, 224), (2, 2, 5, 40), (1, 3, 7, 7)], ids=lambda s: "x".join(map(str, s)))
def test_region_rows_equal_the_restatement(shape):
    z, v, own, scr = _inputs(shape, "quantised")
    C = shape[1]
    shifted = torch.where(own == 0, own, own + 1)   # the same shapes under classes that did not win, and the value C
    for mask, kind in ((own, "prob"), (shifted, "margin")):
        counts, recs, labels = _labels(mask)
        assert (labels == -1).any() and int(counts.max()) <= 1024 and int(counts.min()) >= 1
        _, q = CR.score_logits(v, mask, kind)
        for low_q in (0, 32768, 65536):
            exp = CR.score_rows(q, labels.numpy(), 1024, low_q)
            got = _call(z, mask, kind, labels=labels, max_regions=1024, low_q=low_q)["rows"]
            assert np.array_equal(got, exp), (kind, low_q)
            for i, c in enumerate(counts):
                assert np.array_equal(got[i, :c, 0], recs[i, :c, 5])   # pixels == the records' area
                assert not got[i, c:].any()                            # rows past the count stay zero
            if low_q == 0:
                assert not got[..., 3].any()
            if low_q == 65536:
                assert np.array_equal(got[..., 3], got[..., 0])
        # fewer rows than regions: truncated, nothing past them (the guards), the maps alongside
        few = max(1, int(counts.min()) // 2)
        got = _call(z, mask, kind, want_q=True, labels=labels, max_regions=few, low_q=32768)
        assert np.array_equal(got["rows"], CR.score_rows(q, labels.numpy(), 1024, 32768)[:, :few])
        assert np.array_equal(got["q"].astype(np.int64), q)


@pytest.mark.parametrize("S,g", [(224, 14), (288, 18)])
def test_one_saturated_region_needs_64_bit_sums(S, g):
    """one region over the whole frame, every pixel at p = 1: sum_q = S S 65535 is 3.29e9 at 224 (past 2^31) and 5.4e9 at 288
    (past 2^32) -- and the frame-filling region goes through the workgroup's LDS row"""
    z = torch.full((1, 2, g, g), -30.0)
    z[:, 1] = 30.0
    mask = torch.ones((1, S, S), dtype=torch.uint8)
    counts, recs, labels = _labels(mask)
    assert counts.tolist() == [1] and int(recs[0, 0, 5]) == S * S
    got = _call(z, mask, "prob", labels=labels, max_regions=4, low_q=65535)["rows"]
    assert got[0, 0].tolist() == [S * S, S * S * 65535, 0, 0] and not got[0, 1:].any()
    assert S * S * 65535 > (1 << 31) and (S < 288 or S * S * 65535 > (1 << 32))
    got = _call(z, mask, "margin", labels=labels, max_regions=4, low_q=65535)["rows"]
    assert got[0, 0].tolist() == [S * S, S * S * 65535, 0, 0]
    z0 = torch.zeros((1, 2, g, g))   # p = 0.5 -> q = 32768 (32767.5 to even); margin 0
    got = _call(z0, mask, "prob", labels=labels, max_regions=4, low_q=32769)["rows"]
    assert got[0, 0].tolist() == [S * S, S * S * 32768, 65535 - 32768, S * S]
    got = _call(z0, mask, "margin", labels=labels, max_regions=4, low_q=1)["rows"]
    assert got[0, 0].tolist() == [S * S, 0, 65535, S * S]


def test_same_bits_twice_and_alone_as_in_the_batch():
    shape = (2, 3, 4, 64)
    z, v, own, _ = _inputs(shape, "randn")
    gt = torch.randint(0, 3, own.shape, generator=torch.Generator().manual_seed(5)).to(torch.uint8)
    _, _, labels = _labels(own)
    kw = dict(want_conf=True, want_q=True, max_regions=256, low_q=40000, ignore=2, bins=16)
    a = _call(z, own, "margin", labels=labels, gt=gt, **kw)
    b = _call(z, own, "margin", labels=labels, gt=gt, **kw)
    assert all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)
    for i in range(2):
        one = _call(z[i:i + 1], own[i:i + 1], "margin", labels=labels[i:i + 1], gt=gt[i:i + 1], **kw)
        assert all(np.array_equal(one[k].view(np.uint8), a[k][i:i + 1].view(np.uint8)) for k in a), i


@pytest.mark.parametrize("bins", [1, 16, 256])
def test_histogram_equals_the_restatement(bins):
    for shape, kind in (((2, 3, 4, 64), "prob"), ((2, 2, 5, 40), "margin"), ((1, 3, 7, 7), "prob")):
        z, v, own, scr = _inputs(shape, "quantised")
        C = shape[1]
        gen = torch.Generator().manual_seed(bins)
        gt = torch.where(torch.rand(own.shape, generator=gen) < 0.7, own, torch.randint(0, C + 1, own.shape, generator=gen).to(torch.uint8))
        for mask in (own, scr):
            _, q = CR.score_logits(v, mask, kind)
            for ignore in (-1, C, 0):
                exp = CR.hist(q, mask.numpy(), gt.numpy(), bins, ignore)
                got = _call(z, mask, kind, gt=gt, ignore=ignore, bins=bins)["hist"]
                assert np.array_equal(got, exp), (shape, kind, ignore)
                assert int(exp[..., 0].sum()) == int((gt != ignore).sum())


def test_python_surface_equals_the_c_abi():
    shape = (2, 3, 4, 64)
    z, v, own, _ = _inputs(shape, "quantised")
    zd, md = z.to(DEV), own.to(DEV)
    p, q = CR.score_logits(v, own, "margin")
    assert np.array_equal(confidence.confidence_map(zd, md, "margin").cpu().numpy(), p)
    assert np.array_equal(confidence.confidence_map(zd[0], md[0], "margin", quantised=True).cpu().numpy().astype(np.int64), q[0])
    recs, rows = confidence.region_scores(zd, md, "margin", low=0.5)
    counts, want_recs, labels = _labels(own)
    exp = CR.score_rows(q, labels.numpy(), 1024, 32768)
    for i in range(2):
        assert np.array_equal(recs[i], want_recs[i, :counts[i]]) and np.array_equal(rows[i], exp[i, :counts[i]])
    gt = own.clone()
    gt[:, ::3] = 1
    h = confidence.calibration_hist(zd, md, gt, bins=16, ignore_label=2, kind="margin")
    assert np.array_equal(h, CR.hist(q, own.numpy(), gt.numpy(), 16, 2))
    cal = confidence.calibration_from_hist(h)
    assert cal["total"] == int((gt != 2).sum()) and 0.0 <= cal["ece"] <= 1.0


def test_region_scores_resizes_past_the_default(monkeypatch):
    z, v, own, _ = _inputs((2, 3, 4, 64), "quantised")
    full = confidence.region_scores(z.to(DEV), own.to(DEV))
    monkeypatch.setattr(regions, "DEFAULT_MAX_REGIONS", 2)
    small = confidence.region_scores(z.to(DEV), own.to(DEV))
    assert max(len(r) for r in full[0]) > 2
    assert all(np.array_equal(a, b) for pair in zip(full, small) for a, b in zip(*pair))


def test_model_level():
    from visiontransformer_amd import synth
    from visiontransformer_amd.model import ViTSegmentationModel
    model = ViTSegmentationModel(3, 16, 192, 1, 3, image_size=224, device=DEV).eval()
    x = torch.from_numpy(synth.make_images(model.cfg, 2, seed=1)).to(DEV)
    want_mask, logits = model.predict_mask(x, return_logits=True)
    for kind in ("prob", "margin"):
        mask, conf = model.predict_confidence(x, kind=kind)
        assert torch.equal(mask, want_mask)
        p, q = CR.score_logits(logits.cpu(), want_mask.cpu(), kind)
        assert np.array_equal(conf.cpu().numpy().view(np.uint32), p.view(np.uint32)), kind
        _, cq = model.predict_confidence(x, kind=kind, quantised=True)
        assert cq.dtype == torch.uint16 and np.array_equal(cq.cpu().numpy().astype(np.int64), q)
    recs, rows, mask = model.predict_regions(x, scores=True, min_area=8, fill_holes=True, return_mask=True)
    cleaned = clean.clean_mask(want_mask, min_area=8, fill_holes=True)
    assert torch.equal(mask, cleaned)
    want = regions.region_boxes(cleaned)
    _, q = CR.score_logits(logits.cpu(), cleaned.cpu(), "prob")
    _, _, labels = _labels(cleaned.cpu())
    exp = CR.score_rows(q, labels.numpy(), 1024, 32768)
    for i in range(2):
        assert np.array_equal(recs[i], want[i]) and len(recs[i]) > 0
        assert np.array_equal(rows[i], exp[i, :len(want[i])]) and np.array_equal(rows[i][:, 0], recs[i][:, 5])
    props, rows2 = model.predict_regions(x, scores=True, props=True, min_area=8, fill_holes=True)
    assert all(np.array_equal(a, b) for a, b in zip(rows, rows2)) and all(p.shape[1] == 20 for p in props)
    assert all(np.array_equal(p[:, 2], r[:, 0]) for p, r in zip(props, rows2))
    plain = model.predict_regions(x)   # the defaults: what it returned before
    assert all(np.array_equal(a, b) for a, b in zip(plain, regions.region_boxes(want_mask)))


def test_evaluate_to_csv_writes_the_score_files_and_leaves_the_first(tmp_path):
    import csv
    import os
    from visiontransformer_amd import metrics, scripts
    from visiontransformer_amd.model import ViTSegmentationModel
    model = ViTSegmentationModel(3, 16, 192, 1, 3, image_size=224, device=DEV).eval()
    batches = scripts.ce_batches(model.cfg, 4, 2, seed=3)
    info = (7, "ID7P16H192A3", 16, 192, 1, 3)
    plain, both = str(tmp_path / "a" / "m_metrics.csv"), str(tmp_path / "b" / "m_metrics.csv")
    scripts.evaluate_to_csv(model, batches, info, plain, 3, 2, DEV, min_area=4)
    scripts.evaluate_to_csv(model, batches, info, both, 3, 2, DEV, region_scores=True, score_kind="margin", score_low=0.6,
                            calibration_bins=8, region_classes=True, min_area=4)
    assert os.listdir(tmp_path / "a") == ["m_metrics.csv"]       # without the arguments: the file of before
    assert sorted(os.listdir(tmp_path / "b")) == ["m_calibration.csv", "m_metrics.csv", "m_region_metrics.csv",
                                                  "m_region_scores.csv"]
    strip = lambda p: [r[:11] for r in csv.reader(open(p, newline=""))]   # (column 11 is the time per image)
    assert strip(plain) == strip(both)
    rows = list(csv.reader(open(tmp_path / "b" / "m_region_scores.csv", newline="")))
    assert rows[0] == confidence.SCORES_CSV_COLUMNS
    ev = metrics.Evaluator(3, DEV)
    want, ranked, stats, pooled = [], {1: [], 2: []}, [], 0
    for bn in range(2):
        x = batches[bn][0].to(DEV)
        gt = batches[bn][1].reshape(2, batches[bn][1].shape[-2], batches[bn][1].shape[-1])
        with torch.no_grad():
            raw, logits = model.predict_mask(x, return_logits=True)
            mask = clean.clean_mask(raw, min_area=4)
        recs, srows = confidence.region_scores(logits, mask, kind="margin", low=0.6)   # the full-size logits, g == S
        found = ev.region_metrics(mask, gt, classes=[1, 2], return_matches=True)
        for idx in range(2):
            flags = {(int(r[0]), int(r[6])): int(r[7]) >= 0 for r in found[idx]["matches"]["pred"]}
            stats.append(found[idx]["stats"])
            for r, d in enumerate(confidence.region_dicts(recs[idx], srows[idx])):
                f = flags[(d["class"], d["first"])]
                ranked[d["class"]].append((d["score"], f))
                want.append([7, "ID7P16H192A3", bn, idx, r, d["class"], d["first"], d["area"], d["score"], d["score_min"],
                             d["low_fraction"], int(f), "", ""])
        pooled = pooled + confidence.calibration_hist(logits, mask, ev.resized_gt(gt, mask), bins=8, kind="margin").sum(axis=0)
    assert len(want) > 4 and len(rows) == 1 + len(want) + 2
    for r, w in zip(rows[1:], want):
        assert r == [str(v) for v in w]
    n_gt = metrics.pool_region_stats(stats)[:, 0]
    for r, c, k in zip(rows[-2:], (1, 2), n_gt):
        ap = confidence.average_precision([s for s, _ in ranked[c]], [f for _, f in ranked[c]], int(k))
        assert r[2] == "pooled" and int(r[5]) == c and int(r[13]) == int(k)
        assert float(r[12]) == pytest.approx(ap, rel=1e-12, nan_ok=True)
    cal = list(csv.reader(open(tmp_path / "b" / "m_calibration.csv", newline="")))
    assert cal[0] == confidence.CALIBRATION_CSV_COLUMNS and len(cal) == 1 + 8 + 1
    assert [[str(v) for v in r] for r in confidence.calibration_csv_rows(info, pooled, 8)] == cal[1:]
    assert int(cal[-1][5]) == 4 * 224 * 224


def test_predict_returns_scores_and_the_map():
    from visiontransformer_amd import synth
    from visiontransformer_amd.model import ViTSegmentationModel
    from visiontransformer_amd.predict import predict, preprocess
    model = ViTSegmentationModel(3, 16, 192, 1, 3, image_size=224, device=DEV).eval()
    img = (synth.make_images(model.cfg, 1, seed=4)[0].transpose(1, 2, 0) * 255).astype(np.uint8)
    plain = predict(img, model)
    mask, boxes, scores, conf = predict(img, model, return_boxes=True, return_scores=True, return_confidence=True, low=0.7)
    assert np.array_equal(mask, plain) and conf.shape == (224, 224) and conf.dtype == np.float32
    want_mask, want_conf = model.predict_confidence(preprocess(img, 224, DEV))
    assert np.array_equal(mask, want_mask[0].cpu().numpy()) and np.array_equal(conf, want_conf[0].cpu().numpy())
    recs = regions.region_boxes(want_mask[0])
    assert [(d["class"], d["first"], d["area"]) for d in scores] == [(int(r[0]), int(r[6]), int(r[5])) for r in recs]
    assert all(0.0 <= d["score_min"] <= d["score"] <= 1.0 and 0.0 <= d["low_fraction"] <= 1.0 for d in scores)
    m2, logits, s2, c2 = predict(img, model, return_logits=True, return_scores=True, return_confidence=True, low=0.7)
    assert np.array_equal(m2, mask) and np.array_equal(c2, conf) and s2 == scores   # scored from the logits: the same bits
