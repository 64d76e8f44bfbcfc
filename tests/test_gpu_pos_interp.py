"""GPU: interpolated position embeddings (HF `interpolate_pos_encoding=True`) -- the two kernels against torch, the forward
and the training step against goldens of the real reference class run at other input sizes
(tests/golden/posinterp, tools/make_golden_posinterp.py), identity at the native size, batch invariance at the headline
geometry, the gradient bucket of the position table, and serving a 224 checkpoint at 512."""
import ctypes
import dataclasses
import io
import os
import time

import numpy as np
import pytest
import torch

from guard import check, guarded, snapshot, unchanged
from oracle import vitseg_oracle as O
from test_pos_interp_cpu import torch_pos_interp
from util import GOLDEN, Golden
from visiontransformer_amd import _lib, synth
from visiontransformer_amd.config import ViTSegConfig
from visiontransformer_amd.lightning import LightningViTModel
from visiontransformer_amd.model import ViTSegmentationModel
from visiontransformer_amd.params import arena_views

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL_LOGITS = 1e-3                           # test_gpu_forward's fp32 gate
TOL_LOGITS_16 = {"bf16": 3e-2, "fp16": 1e-3}
MISMATCH_16 = {"bf16": 0.015, "fp16": 0.001}
CASES = sorted(f[:-4] for f in os.listdir(os.path.join(GOLDEN, "posinterp")) if f.endswith(".npz"))
FWD_CASES = [c for c in CASES if not c.endswith("_train")]


class PGolden(Golden):
    """A posinterp fixture: cfg = the checkpoint's geometry (224), S_in = the input's side."""

    def __init__(self, name):
        super().__init__("posinterp/" + name)
        self.S_in = int(self.z["meta.image_in"][0])
        self.cfg_in = dataclasses.replace(self.cfg, image_size=self.S_in)

    def images(self):
        return torch.from_numpy(synth.make_images(self.cfg_in, self.batch, seed=0))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def build(g, precision="fp32"):
    c = g.cfg
    m = ViTSegmentationModel(c.num_classes, c.patch_size, c.hidden_size, c.num_hidden_layers, c.num_attention_heads,
                             image_size=c.image_size, intermediate_size=c.intermediate_size, precision=precision,
                             device=DEV).eval()
    m.load_state_dict(g.state_dict())
    return m


# ---- 1. + 2. the kernels on their own ----------------------------------------------------------------------------
GRIDS = [(14, 32), (14, 24), (14, 7), (28, 64), (14, 14)]


@pytest.mark.parametrize("D", [192, 768])
@pytest.mark.parametrize("g0,g1", GRIDS)
def test_resampling_kernel_matches_torch(g0, g1, D):
    gen = torch.Generator().manual_seed(g0 * 1000 + g1 + D)
    table = torch.randn(1 + g0 * g0, D, generator=gen) * 0.02
    src = guarded((1 + g0 * g0, D), fill=table.to(DEV), name="pos_in")
    dst = guarded((1 + g1 * g1, D), name="pos_out")
    snap = snapshot(src)
    _lib.check(_lib.at_symbol("vitseg_pos_interp")(src.data_ptr(), dst.data_ptr(), g0, g1, D, _stream()))
    torch.cuda.synchronize()
    check(src, dst)
    unchanged(snap)
    got = dst.cpu()
    if g0 == g1:
        assert torch.equal(got, table)   # weights (0, 1, 0, 0): the arena rows themselves
        return
    ref = torch_pos_interp(table, g0, g1)
    rel = (got - ref).abs().max().item() / table.abs().max().item()
    print(f"pos_interp {g0}->{g1} D={D}: max |kernel - torch| = {rel:.2e} x max|table|")
    assert rel <= 1e-6, rel


@pytest.mark.parametrize("D", [192, 768])
@pytest.mark.parametrize("g0,g1", GRIDS)
def test_adjoint_kernel_matches_fp64_autograd_and_is_reproducible(g0, g1, D):
    gen = torch.Generator().manual_seed(7 * g1 + D)
    dout = torch.randn(1 + g1 * g1, D, generator=gen)
    leaf = torch.zeros(1 + g0 * g0, D, dtype=torch.float64, requires_grad=True)
    (torch_pos_interp(leaf, g0, g1) * dout.double()).sum().backward()
    ref = leaf.grad
    din = guarded((1 + g1 * g1, D), fill=dout.to(DEV), name="dpos_out")
    snap = snapshot(din)
    outs = []
    for run in range(2):
        dst = guarded((1 + g0 * g0, D), name=f"dpos_in{run}")
        scratch = guarded((g1 * g0 * D,), name=f"scratch{run}")
        _lib.check(_lib.at_symbol("vitseg_pos_interp_bwd")(din.data_ptr(), dst.data_ptr(), scratch.data_ptr(), g0, g1, D,
                                                            _stream()))
        torch.cuda.synchronize()
        check(din, dst, scratch)
        outs.append(dst.cpu())
    unchanged(snap)
    assert torch.equal(outs[0], outs[1])
    rel = (outs[0].double() - ref).abs().max().item() / ref.abs().max().item()
    print(f"pos_interp_bwd {g0}->{g1} D={D}: max |kernel - fp64 autograd| = {rel:.2e} x max|grad|")
    assert rel <= 1e-5, rel


# ---- 3. the forward against the reference at other input sizes ---------------------------------------------------
def _fp32_gate(g, m, label):
    x = g.images().to(DEV)
    S, gi = g.S_in, g.S_in // g.cfg.patch_size
    with torch.no_grad():
        mask, logits = m.predict_mask(x, return_logits=True, interpolate_pos_encoding=True)
    torch.cuda.synchronize()
    assert tuple(logits.shape) == (g.batch, g.cfg.num_classes, S, S)
    err, _ = g.max_abs_err("logits", logits)
    assert err <= TOL_LOGITS, (label, err)
    assert g.checksum_rel_err("logits", logits) < 1e-4
    low = m.debug_buffer(g.batch, _lib.BUF_LOWRES, S).view(g.batch, g.cfg.num_classes, gi, gi).cpu()
    low_err = float(np.abs(low.numpy() - g.z["lowres_logits.full"]).max())
    assert low_err <= TOL_LOGITS, (label, low_err)
    # gate 1: the mask is the ATen post-processing of the kernel's own low-res logits, on every pixel
    own = O.upsample_bilinear(low, (S, S))
    assert torch.equal(logits.cpu(), own)
    got = mask.cpu().numpy()
    assert np.array_equal(got, O.predict_mask(own).numpy())
    # gate 2: the reference mask on every pixel the measured error cannot flip
    ref = g.mask()
    ref_logits = O.upsample_bilinear(torch.from_numpy(g.z["lowres_logits.full"]), (S, S))
    stable = O.mask_stable(ref_logits, 2.0 * low_err + 1e-7).numpy()
    bad = (got != ref) & stable
    assert bad.sum() == 0, (label, int(bad.sum()))
    assert (~stable).mean() < 2e-3 and (got != ref).mean() < 2e-3
    with torch.no_grad():
        assert torch.equal(m(x, interpolate_pos_encoding=True), logits)
    print(f"{label}: max |logits - reference| {err:.2e}, low-res {low_err:.2e}")


@pytest.mark.parametrize("route", ["small", "large"])
@pytest.mark.parametrize("name", FWD_CASES)
def test_forward_matches_reference_at_other_sizes(name, route):
    g = PGolden(name)
    m = build(g)
    with _lib.option("no_small", int(route == "large")):
        _fp32_gate(g, m, f"{name} {route}")


@pytest.mark.parametrize("name", FWD_CASES)
def test_forward_f32x3_meets_the_fp32_gate(name):
    g = PGolden(name)
    _fp32_gate(g, build(g, "fp32x3"), f"{name} fp32x3")


@pytest.mark.parametrize("route", ["small", "large"])
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("name", FWD_CASES)
def test_forward_16bit_close_to_reference(name, precision, route):
    g = PGolden(name)
    m = build(g, precision)
    x = g.images().to(DEV)
    with torch.no_grad(), _lib.option("no_small", int(route == "large")):
        mask, logits = m.predict_mask(x, return_logits=True, interpolate_pos_encoding=True)
    torch.cuda.synchronize()
    err, _ = g.max_abs_err("logits", logits)
    assert err <= TOL_LOGITS_16[precision], err
    mism = (mask.cpu().numpy() != g.mask()).mean()
    print(f"{name} {precision} {route}: logits err {err:.2e}, mask mismatch {mism:.4%}")
    assert mism < MISMATCH_16[precision], mism


# ---- 4. identity at the native size --------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_flag_at_the_native_size_is_the_plain_forward(precision):
    g = Golden("tiny16_224_c2")
    m = build(g, precision)
    x = g.images().to(DEV)
    with torch.no_grad():
        plain = m(x)
        flagged = m(x, interpolate_pos_encoding=True)
        mask_f = m.predict_mask(x, interpolate_pos_encoding=True)
        mask_p = m.predict_mask(x)
    assert torch.equal(plain, flagged)
    assert torch.equal(mask_p, mask_f)


# ---- 5. batch invariance at 224 -> 512 ------------------------------------------------------------------------------
def test_batch_invariance_224_checkpoint_at_512():
    """ViT-B/16 with a 224 position table on 512 x 512 inputs, fp32: images 5..20 of a batch of 32 against the same 16
    images as a batch of their own (16 400 token rows: the large route like the batch of 32), bit for bit."""
    cfg = ViTSegConfig(2, 16, 768, 12, 12, image_size=224)
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, seed=5).items()}
    x = torch.from_numpy(synth.make_images(dataclasses.replace(cfg, image_size=512), 32, seed=9)).to(DEV)
    m = ViTSegmentationModel(2, 16, 768, 12, 12, image_size=224, device=DEV).eval()
    m.load_state_dict(sd)
    assert m.forward_route(32, 512) == "large" and m.forward_route(16, 512) == "large"
    with torch.no_grad():
        _, lg = m.predict_mask(x[:4].contiguous(), return_logits=True, interpolate_pos_encoding=True)
        sd["seg_head.2.bias"] = sd["seg_head.2.bias"].clone()
        sd["seg_head.2.bias"][1] += float((lg[:, 0] - lg[:, 1]).median())
        m.load_state_dict(sd)
        mask_all, logits_all = m.predict_mask(x, return_logits=True, interpolate_pos_encoding=True)
        mask_16, logits_16 = m.predict_mask(x[5:21].contiguous(), return_logits=True, interpolate_pos_encoding=True)
    assert torch.isfinite(logits_all).all()
    assert 0.05 < float(mask_all.float().mean()) < 0.95
    assert torch.equal(logits_all[5:21], logits_16)
    assert torch.equal(mask_all[5:21], mask_16)


# ---- 6. the training step -------------------------------------------------------------------------------------------
def _lightning(g, precision="fp32"):
    c = g.cfg
    lm = LightningViTModel(c.num_classes, c.patch_size, c.hidden_size, c.num_hidden_layers, c.num_attention_heads,
                           image_size=c.image_size, dropout=0.0, precision=precision, device=DEV,
                           interpolate_pos_encoding=True)
    lm.load_state_dict({"model." + k: v for k, v in g.state_dict().items()})
    return lm


@pytest.mark.parametrize("route", ["small", "large"])
def test_training_step_matches_reference_at_another_size(route):
    g = PGolden("base16w_l2_224to320_c2_train")
    lm = _lightning(g).train()
    opt = lm.configure_optimizers()
    with _lib.option("no_small", int(route == "large")):
        loss = lm.training_step((g.images().to(DEV), g.targets().to(DEV)), 0)
        assert abs(float(loss) - float(g.z["train.loss"][0])) < 2e-6, float(loss)
        loss.backward()
    grads = arena_views(g.cfg, lm.model.arena.grad)
    keys = [k[5:-4] for k in g.z.files if k.startswith("grad.") and k.endswith(".idx")]
    assert "backbone.embeddings.position_embeddings" in keys
    assert tuple(grads["backbone.embeddings.position_embeddings"].shape) == (1, 197, 768)
    for key in keys:
        err, scale = g.max_abs_err("grad." + key, grads[key])
        assert err <= 5e-4 * scale + 1e-9, (key, err, scale)
    before = {k: v.clone() for k, v in lm.model.named_views().items()}
    opt.step()
    after = lm.model.named_views()
    for key in [k[6:-4] for k in g.z.files if k.startswith("adam1.") and k.endswith(".idx")]:
        err, _ = g.max_abs_err("adam1." + key, after[key] - before[key])
        assert err <= 2.1e-5, (key, err)


def test_bf16_training_step_at_another_size_is_finite_and_reproducible():
    g = PGolden("base16w_l2_224to320_c2_train")
    x, y = g.images().to(DEV), g.targets().to(DEV)
    out = []
    for _ in range(2):
        lm = _lightning(g, "bf16").train()
        loss = lm.training_step((x, y), 0)
        loss.backward()
        out.append((float(loss), lm.model.arena.grad.clone()))
    assert np.isfinite(out[0][0]) and torch.isfinite(out[0][1]).all()
    assert abs(out[0][0] - float(g.z["train.loss"][0])) < 1e-2
    assert out[0][0] == out[1][0] and torch.equal(out[0][1], out[1][1])
    pos = arena_views(g.cfg, out[0][1])["backbone.embeddings.position_embeddings"]
    assert float(pos.abs().max()) > 0


# ---- 7. the position table's gradient bucket --------------------------------------------------------------------------
def test_position_gradient_is_final_when_its_bucket_event_fires():
    """vitseg_backward_at records the bucket events; the VITSEG_T_POS range copied on a side stream right after its
    bucket's event equals its value after the whole backward (the adjoint runs before the event)."""
    g = PGolden("base16w_l2_224to320_c2_train")
    m = build(g).train()
    m.dropout = 0.0
    cfg, B, S = g.cfg, g.batch, g.S_in
    x = g.images().to(DEV).contiguous()
    y = torch.from_numpy(g.z["train.target_resized"]).to(DEV).contiguous()
    pos_off, pos_n = _lib.param_offset(cfg, _lib.T_POS)
    ranges = _lib.grad_buckets(cfg)
    bucket = [i for i, (o, n) in enumerate(ranges) if o <= pos_off < o + n][0]
    events = [torch.cuda.Event() for _ in ranges]
    for e in events:
        e.record()
    handles = (ctypes.c_void_p * len(events))(*[e.cuda_event for e in events])
    ws = torch.empty(_lib.train_workspace(cfg, B, _lib.F32, S), dtype=torch.uint8, device=DEV)
    grads = torch.empty_like(m.arena.data)
    loss = torch.zeros((), device=DEV)
    side = torch.cuda.Stream()
    early = torch.empty(pos_n, device=DEV)
    c = ctypes.byref(_lib.CConfig.from_config(cfg))
    _lib.check(_lib.at_symbol("vitseg_forward_train_at")(c, S, m.arena.data_ptr(), None, x.data_ptr(), B, _lib.F32, 0.0, 0,
                                                         None, ws.data_ptr(), ws.numel(), _stream()))
    _lib.check(_lib.at_symbol("vitseg_backward_at")(c, S, m.arena.data_ptr(), None, x.data_ptr(), B, _lib.F32, 0.0, 0,
                                                    y.data_ptr(), 1, None, grads.data_ptr(), loss.data_ptr(), 1.0, handles,
                                                    ws.data_ptr(), ws.numel(), _stream()))
    with torch.cuda.stream(side):
        side.wait_event(events[bucket])
        early.copy_(grads[pos_off:pos_off + pos_n])
    torch.cuda.synchronize()
    assert torch.equal(early, grads[pos_off:pos_off + pos_n])
    assert float(early.abs().max()) > 0


# ---- 8. serving a 224 checkpoint at 512 -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base_checkpoint(tmp_path_factory):
    cfg = ViTSegConfig(2, 16, 768, 12, 12, image_size=224)
    sd = {"model." + k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, seed=3).items()}
    path = tmp_path_factory.mktemp("ckpt") / "vitb16_224.ckpt"
    torch.save({"state_dict": sd}, path)
    return str(path)


def _image(seed=0):
    return np.random.default_rng(seed).integers(0, 256, (300, 420, 3), dtype=np.uint8)


def test_predict_serves_a_224_checkpoint_at_512(base_checkpoint):
    from visiontransformer_amd.predict import load_model, predict, preprocess
    model = load_model(0, 2, base_checkpoint, image_size=224, serve_size=512, device=DEV)
    assert model.model.cfg.image_size == 224
    img = _image()
    mask = predict(img, model)
    assert mask.shape == (512, 512)
    x512 = preprocess(img, 512, DEV)
    ref = model.model.predict_mask(x512, interpolate_pos_encoding=True)[0].cpu().numpy()
    assert np.array_equal(mask, ref)
    # the same model without serve_size serves at its own 224
    assert predict(img, model, serve_size=224).shape == (224, 224)


def test_worker_round_trip_with_the_serve_size_field(base_checkpoint):
    from PIL import Image
    from visiontransformer_amd.worker import Job, Worker, gpu_slot, parse_model_spec, png_bytes
    spec = parse_model_spec(f"7:2:{base_checkpoint}:0:224:512")
    slot = gpu_slot(spec["config_id"], spec["num_classes"], spec["checkpoint"], image_size=spec["image_size"],
                    serve_size=spec["serve_size"], device=DEV)
    w = Worker({7: slot}, "http://127.0.0.1:9", "t")
    got = []
    w._complete = lambda job, png: got.append((job.job_id, png))
    w.start()
    try:
        w.submit(Job("j1", 7, png_bytes(_image(1))))
        t0 = time.time()
        while not got and time.time() - t0 < 120 and w.stats["failed"] == 0:
            time.sleep(0.05)
    finally:
        w.stop()
    assert w.stats["failed"] == 0 and got, w.stats
    assert Image.open(io.BytesIO(got[0][1])).size == (512, 512)
