"""GPU (-m gpu): backward kernels and the training step, through the C ABI, against the oracle
(autograd on the CPU restatement) and the golden gradients of the real reference class."""
import numpy as np
import pytest
import torch

from guard import check, guarded, snapshot, unchanged
from oracle import bf16_model as BM
from oracle import vitseg_oracle as O
from util import BF16_GRAD_COS, BF16_GRAD_REL, CASES, Golden, grad_check as _grad_check
from visiontransformer_amd import _lib, synth
from visiontransformer_amd.config import ViTSegConfig
from visiontransformer_amd.lightning import LightningViTModel
from visiontransformer_amd.model import ViTSegmentationModel

pytestmark = pytest.mark.gpu

# bf16 gradient gates: BF16_GRAD_REL / BF16_GRAD_COS (tests/util.py) for shallow models (<= 2 layers).  At depth no constant
# is used: the distance of the HIP gradients from the exact ones is compared, tensor by tensor, with the distance of the
# ROUNDING MODEL of the same step (oracle/bf16_model.py: fp64 arithmetic, rounded to bf16 where the HIP path stores or
# multiplies a bf16) from the exact ones -- see _check_against_rounding_model.
MODEL_RATIO, MODEL_SLACK = 1.3, 0.02                  # HIP error <= MODEL_RATIO * model error + MODEL_SLACK, per tensor
DEV = "cuda:0"


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


def _dev(t, dtype=None, name=None):
    """guard-banded device copy of a CPU tensor (tests/guard.py)"""
    return guarded(tuple(t.shape), dtype or t.dtype, t, device=DEV, name=name)


def _out(shape, dtype=torch.float32, fill="nan", name=None):
    return guarded(shape, dtype, fill, device=DEV, name=name)


def _after(snap, *outs):
    """after a call: every guard (inputs and outputs) intact, every input bitwise unchanged"""
    torch.cuda.synchronize()
    check(*[t for t, _ in snap], *outs)
    unchanged(snap)


@pytest.mark.parametrize("M,N,K,ta,tb,epi", [
    (257, 192, 96, 0, 1, 0), (1025, 768, 2304, 0, 1, 0), (300, 3072, 768, 0, 1, 5),
    (192, 576, 1025, 1, 1, 0), (768, 3072, 2050, 1, 1, 0), (256, 6912, 300, 1, 1, 0), (64, 100, 37, 1, 1, 0),
    (1, 132, 36, 0, 1, 0), (132, 4, 100, 1, 1, 0), (124, 252, 1, 1, 1, 0)])   # M = 1, N = 4, K = 1 against 128-wide tiles
    # (leading dimensions are multiples of 4)
def test_gemm_operand_forms(M, N, K, ta, tb, epi):
    A = _rand(K, M, seed=1) if ta else _rand(M, K, seed=1)
    W = _rand(K, N, seed=2, scale=0.05) if tb else _rand(N, K, seed=2, scale=0.05)
    R = _rand(M, N, seed=3)
    a64 = A.double().T if ta else A.double()
    w64 = W.double() if tb else W.double().T
    ref = a64 @ w64
    if epi == 5:
        u = R.double()
        ref = ref * (0.5 * (1 + torch.erf(u / 2 ** 0.5)) + u * torch.exp(-0.5 * u * u) / (2 * np.pi) ** 0.5)
    Ad, Wd, Rd = _dev(A, name="A"), _dev(W, name="W"), _dev(R, name="R")
    C = _out((M, N), name="C")
    snap = snapshot(Ad, Wd, Rd)
    _lib.check(_lib.lib().vitseg_op_gemm_f32(Ad.data_ptr(), Wd.data_ptr(), Rd.data_ptr(), C.data_ptr(), M, N, K, ta, tb,
                                             epi, _stream()))
    _after(snap, C)
    bound = 4e-7 * (a64.abs() @ w64.abs()).max().item() + 1e-6
    assert (C.cpu().double() - ref).abs().max().item() < bound


@pytest.mark.parametrize("rows,D", [(7, 192), (1025, 768), (130, 1024), (64, 512), (788, 768), (20000, 192),
                                    (1, 192),   # one row
                                    (16383, 192), (16385, 192)])   # either side of 64 x CUs rows (lnb_blocks: 8 / 64 rows per block)
def test_layernorm_backward(rows, D):
    x = (_rand(rows, D, seed=1, scale=2.0) + 0.3).double().requires_grad_(True)
    w = (_rand(D, seed=2) + 1.0).double().requires_grad_(True)
    b = _rand(D, seed=3).double().requires_grad_(True)
    g, dres = _rand(rows, D, seed=4), _rand(rows, D, seed=5)
    y = O.layer_norm(x, w, b, 1e-12)
    y.backward(g.double())
    xd, wd, gd, rd = _dev(x.detach().float(), name="x"), _dev(w.detach().float(), name="w"), _dev(g, name="g"), \
        _dev(dres, name="dres")
    out, dw, db = _out((rows, D), name="dx"), _out((D,), name="dw"), _out((D,), name="db")
    scratch = _out((_lib.lib().vitseg_op_layernorm_bwd_scratch_floats(rows, D),), name="layernorm_bwd scratch")
    snap = snapshot(xd, wd, gd, rd)
    _lib.check(_lib.lib().vitseg_op_layernorm_bwd_f32(xd.data_ptr(), wd.data_ptr(), gd.data_ptr(), rd.data_ptr(),
                                                      out.data_ptr(), dw.data_ptr(), db.data_ptr(), scratch.data_ptr(),
                                                      rows, D, 1e-12, _stream()))
    _after(snap, out, dw, db, scratch)
    assert (out.cpu().double() - (dres.double() + x.grad)).abs().max().item() < 2e-5
    assert (dw.cpu().double() - w.grad).abs().max().item() < 1e-5 * max(1.0, w.grad.abs().max().item())
    assert (db.cpu().double() - b.grad).abs().max().item() < 1e-5 * max(1.0, b.grad.abs().max().item())


@pytest.mark.parametrize("B,Np,A", [(2, 196, 3), (1, 1024, 2), (1, 64, 1), (2, 100, 2),
                                    # ragged against the query / key blocks: below one block, one either side of 128
                                    (1, 4, 1), (2, 31, 2), (3, 127, 1), (1, 129, 3), (2, 200, 2)])
def test_attention_backward(B, Np, A):
    D, Mt = 64 * A, B * Np + B
    qkv = _rand(Mt, 3 * D, seed=Np + A, scale=1.2)
    dctx = _rand(Mt, D, seed=9)
    x = qkv.double().requires_grad_(True)
    outs = []
    for b in range(B):
        r = torch.cat([torch.tensor([B * Np + b]), torch.arange(b * Np, (b + 1) * Np)])
        q, k, v = [x[r][:, i * D:(i + 1) * D].reshape(Np + 1, A, 64).transpose(0, 1) for i in range(3)]
        s = torch.softmax(q @ k.transpose(-1, -2) * 0.125, dim=-1)
        outs.append(((s @ v).transpose(0, 1).reshape(Np + 1, D) * dctx.double()[r]).sum())
    torch.stack(outs).sum().backward()
    qd, dd = _dev(qkv, name="qkv"), _dev(dctx, name="dctx")
    ctx = _out((Mt, D), name="ctx")
    lse = _out((B * A * (Np + 1),), name="lse")
    scr = _out((B * A * (Np + 1),), name="attention_bwd scratch")   # delta [B, A, Np + 1]: what the fp32 kernels use
    dqkv = _out((Mt, 3 * D), name="dqkv")
    snap = snapshot(qd, dd)
    _lib.check(_lib.lib().vitseg_op_attention_bwd_f32(qd.data_ptr(), dd.data_ptr(), ctx.data_ptr(), lse.data_ptr(),
                                                      scr.data_ptr(), dqkv.data_ptr(), B, Np, A, _stream()))
    _after(snap, ctx, lse, scr, dqkv)
    err = (dqkv.cpu().double() - x.grad).abs().max().item()
    assert err < 5e-5 * max(1.0, x.grad.abs().max().item()), err


def _build(g: Golden, precision="fp32"):
    c = g.cfg
    lm = LightningViTModel(c.num_classes, c.patch_size, c.hidden_size, c.num_hidden_layers, c.num_attention_heads,
                           image_size=c.image_size, dropout=0.0, precision=precision, device=DEV)  # parity runs with dropout off
    lm.load_state_dict({"model." + k: v for k, v in g.state_dict().items()})
    return lm


@pytest.mark.parametrize("route", ["small", "large"])
@pytest.mark.parametrize("name", [c for c in CASES if Golden(c).has("grad.seg_head.2.weight")])
def test_training_step_matches_reference_gradients(name, route):
    """LightningViTModel.training_step + backward + one Adam(lr=1e-5) step vs the real reference class -- through the
    small-batch route of the fp32 step (csrc/small.hpp: every fixture is that small) and, with the `no_small` switch held over
    forward and backward, through the large-batch kernels (what an fp32 step of 16 384 token rows or more runs)."""
    g = Golden(name)
    lm = _build(g).train()
    opt = lm.configure_optimizers()
    with _lib.option("no_small", int(route == "large")):
        loss = lm.training_step((g.images().to(DEV), g.targets().to(DEV)), 0)
        assert abs(float(loss) - float(g.z["train.loss"][0])) < 2e-6
        loss.backward()
    views = {k: v for k, v in zip(lm.model.named_views().keys(),
                                  __import__("visiontransformer_amd.params", fromlist=["x"]).arena_views(
                                      g.cfg, lm.model.arena.grad).values())}
    for key in [k[5:-4] for k in g.z.files if k.startswith("grad.") and k.endswith(".idx")]:
        err, scale = g.max_abs_err("grad." + key, views[key])
        assert err <= 5e-4 * scale + 1e-9, (key, err, scale)
    before = {k: v.clone() for k, v in lm.model.named_views().items()}
    opt.step()
    after = lm.model.named_views()
    for key in [k[6:-4] for k in g.z.files if k.startswith("adam1.") and k.endswith(".idx")]:
        err, _ = g.max_abs_err("adam1." + key, after[key] - before[key])
        assert err <= 2.1e-5, (key, err)  # a sign flip of a ~0 gradient moves the first Adam update by 2*lr


def test_logits_autograd_matches_oracle():
    """Arbitrary loss on the logits (the PAED losses' route): d loss / d arena through vitseg_backward."""
    cfg = ViTSegConfig(3, 16, 192, 2, 3, image_size=96)
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, seed=31).items()}
    x = torch.from_numpy(synth.make_images(cfg, 2, seed=4))
    wgt = _rand(2, 3, 96, 96, seed=6)
    leaf = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    (O.forward(x.double(), leaf, cfg) * wgt.double()).sum().backward()
    m = ViTSegmentationModel(3, 16, 192, 2, 3, image_size=96, dropout=0.0, device=DEV).train()
    m.load_state_dict(sd)
    (m(x.to(DEV)) * wgt.to(DEV)).sum().backward()
    from visiontransformer_amd.params import arena_views
    gv = arena_views(cfg, m.arena.grad)
    for k, ref in leaf.items():
        err = (gv[k].cpu().double() - ref.grad).abs().max().item()
        assert err <= 2e-4 * max(ref.grad.abs().max().item(), 1e-3), (k, err, ref.grad.abs().max().item())


def test_batch_shard_gradient_equivalence():
    """Data-parallel contract (section 8e): the mean of per-shard gradients (each shard's loss is the mean over
    ITS pixels, equal shard sizes) equals the gradient of the global-batch loss."""
    g = Golden("base16w_l2_224_c2_train")
    lm = _build(g).train()
    x, y = g.images().to(DEV), lm._resize_target(g.targets().to(DEV), (224, 224))
    m = lm.model

    def grads(xs, ys):
        m.arena.grad = None
        m.ce_loss(xs, ys).backward()
        return m.arena.grad.clone()

    full = grads(x, y)
    halves = (grads(x[:1], y[:1]) + grads(x[1:], y[1:])) / 2
    assert (full - halves).abs().max().item() <= 1e-6 * max(1.0, full.abs().max().item())


def test_gradient_buffer_is_handed_over_not_cloned():
    """The buffer vitseg_backward writes becomes `arena.grad` itself (no arena-sized clone per step): with
    zero_grad(set_to_none=True) between steps the same storage serves every step; while a gradient is pending the next
    backward gets a temporary and is ADDED (accumulation), and the logits path behaves the same."""
    g = Golden("base16w_l2_224_c2_train")
    lm = _build(g).train()
    m = lm.model
    m.dropout = 0.0
    x, y = g.images().to(DEV), lm._resize_target(g.targets().to(DEV), (224, 224))
    m.arena.grad = None
    m.ce_loss(x, y).backward()
    p0, g0 = m.arena.grad.data_ptr(), m.arena.grad.clone()
    assert p0 == m._grad_buf.data_ptr()
    m.arena.grad = None                       # zero_grad(set_to_none=True)
    m.ce_loss(x, y).backward()
    assert m.arena.grad.data_ptr() == p0 and torch.equal(m.arena.grad, g0)
    m.ce_loss(x, y).backward()                # gradient pending: accumulate, the installed buffer is not overwritten
    assert m.arena.grad.data_ptr() == p0 and torch.equal(m.arena.grad, g0 + g0)
    m.arena.grad = None
    logits = m(x)                             # autograd path through the logits
    torch.nn.functional.cross_entropy(logits, y.long()).backward()
    assert m.arena.grad.data_ptr() == p0
    assert (m.arena.grad - g0).abs().max().item() <= 2e-6 * max(1.0, g0.abs().max().item())


@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp32_large"])
def test_overlapped_bucket_allreduce_inside_backward(precision):
    """Section 8(e): vitseg_backward records one event per gradient bucket; the host queues one RCCL all-reduce
    per bucket behind its event on a side stream.  Run on a one-rank RCCL group (sum over one rank = identity):
    gradients and loss must equal the plain backward bit for bit, and the bucket events must fire in order.
    fp32_large: `no_small` held over forward and backward -- the fixture is small enough for the small-batch route, so
    without the switch the large fp32 route's event placement would go untested."""
    import os
    import torch.distributed as dist
    from visiontransformer_amd.dist import sync_grads
    large, precision = precision == "fp32_large", precision.split("_")[0]
    g = Golden("base16w_l2_224_c2_train")
    lm = _build(g, precision=precision).train()
    with _lib.option("no_small", int(large)):
        m = lm.model
        m.dropout = 0.0
        x, y = g.images().to(DEV), lm._resize_target(g.targets().to(DEV), (224, 224))

        def run():
            m.arena.grad = None
            loss = m.ce_loss(x, y)
            loss.backward()
            return loss.detach().clone(), m.arena.grad.clone()

        m.grad_sync = "after"
        l0, g0 = run()
        assert not m._grads_reduced
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29533", RANK="0", WORLD_SIZE="1")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV))
        try:
            m.grad_sync = "force"
            m.grad_bucket_mb = 8.0
            l1, g1 = run()
            assert m._grads_reduced
            reducer, events, _, _ = m._buckets
            assert len(reducer.groups) > 1
            torch.cuda.synchronize()
            assert all(e.query() for e in events)
            sync_grads(m)                      # consumes the flag, must not reduce again
            assert not m._grads_reduced
            assert torch.equal(l0, l1) and torch.equal(g0, g1)
        finally:
            dist.destroy_process_group()
            m.grad_sync = "overlap"


def test_trainer_writes_lightning_style_checkpoints(tmp_path):
    from visiontransformer_amd import trainer
    cfg = ViTSegConfig(2, 16, 192, 2, 3, image_size=96)
    lm = LightningViTModel(2, 16, 192, 2, 3, image_size=96, device=DEV)
    xs = torch.from_numpy(synth.make_images(cfg, 8, seed=0))
    ys = torch.from_numpy(synth.make_targets(cfg, 8, seed=0))
    batches = [(xs[i:i + 2], ys[i:i + 2]) for i in range(0, 8, 2)]
    w0 = lm.model.arena.detach().clone()
    rows = trainer.fit(lm, batches, batches, max_epochs=2, accumulate_grad_batches=4, patience=3,
                       ckpt_dir=str(tmp_path / "ck"), log_dir=str(tmp_path / "log"), device=DEV)
    assert not torch.equal(w0, lm.model.arena.detach())           # one optimizer step per epoch happened
    assert all(np.isfinite(r["valid_loss"]) for r in rows if "valid_loss" in r)
    ck = torch.load(tmp_path / "ck" / "epoch=1-step=2.ckpt")
    assert all(k.startswith("model.") for k in ck["state_dict"])
    lm2 = LightningViTModel(2, 16, 192, 2, 3, image_size=96, device=DEV)
    lm2.load_state_dict(ck["state_dict"])
    assert torch.equal(lm2.model.arena.detach(), lm.model.arena.detach())
    assert (tmp_path / "log" / "metrics.csv").read_text().startswith("epoch,step,train_loss_step")


def test_fused_adam_matches_torch_adam():
    """vitseg_adam_step against torch.optim.Adam(lr=1e-5) (classes.py:296-297) over several steps."""
    from visiontransformer_amd.optim import FusedAdam
    n = 4096 * 5
    p0 = _rand(n, seed=1, scale=0.02)
    a = torch.nn.Parameter(p0.clone().to(DEV))
    b = torch.nn.Parameter(p0.clone().to(DEV))
    oa, ob = FusedAdam([a], lr=1e-5), torch.optim.Adam([b], lr=1e-5)
    for step in range(4):
        g = _rand(n, seed=10 + step, scale=10.0 ** (-step)).to(DEV)
        a.grad, b.grad = g.clone(), g.clone()
        oa.step()
        ob.step()
        assert (a.detach() - b.detach()).abs().max().item() < 2e-9, step
    assert (a.detach().cpu() - p0).abs().max().item() > 1e-5  # it did move


def test_fused_adamw_matches_torch_adamw():
    """vitseg_adamw_step against torch.optim.AdamW(lr=1e-4) -- PAEDTrainer.configure_optimizers, model/PAED/classes.py:536-548
    (decoupled weight decay, torch's default 1e-2) -- over several steps, and PAEDTrainer really builds the fused one."""
    from visiontransformer_amd import paed
    from visiontransformer_amd.optim import FusedAdamW
    n = 4096 * 5
    p0 = _rand(n, seed=2, scale=0.1)   # |p| < 0.5: one ulp is 3e-8
    a = torch.nn.Parameter(p0.clone().to(DEV))
    b = torch.nn.Parameter(p0.clone().to(DEV))
    oa, ob = FusedAdamW([a], lr=1e-4), torch.optim.AdamW([b], lr=1e-4)
    assert oa.param_groups[0]["weight_decay"] == ob.param_groups[0]["weight_decay"] == 1e-2
    for step in range(4):
        g = _rand(n, seed=20 + step, scale=10.0 ** (-step)).to(DEV)
        a.grad, b.grad = g.clone(), g.clone()
        oa.step()
        ob.step()
        assert (a.detach() - b.detach()).abs().max().item() < 1e-7, step   # 1-2 ulp: torch divides by sqrt(bc2), the kernel multiplies by its reciprocal
    moved = (a.detach().cpu() - p0)
    assert moved.abs().max().item() > 1e-4
    # the decay itself: a zero gradient leaves p * (1 - lr wd)^k
    c = torch.nn.Parameter(p0.clone().to(DEV))
    oc = FusedAdamW([c], lr=1e-2, weight_decay=0.5)
    c.grad = torch.zeros_like(c)
    oc.step()
    assert torch.allclose(c.detach().cpu(), p0 * (1 - 1e-2 * 0.5), rtol=3e-7, atol=0)   # 2 ulp: the factor is formed in fp32
    t = paed.PAEDTrainer(1, 16, 192, 1, 3, image_size=96, device=DEV)
    cfgd = t.configure_optimizers()
    assert isinstance(cfgd["optimizer"], FusedAdamW) and cfgd["optimizer"].param_groups[0]["lr"] == 1e-4
    assert isinstance(cfgd["lr_scheduler"]["scheduler"], torch.optim.lr_scheduler.ReduceLROnPlateau)


def test_iou_score_from_class_counts_matches_the_reference_formula():
    """paed.iou_score on the device (one vitseg_eval_counts launch) against the reference's per-class loop
    (model/PAED/classes.py:430-447) on the CPU."""
    from visiontransformer_amd import paed
    g = torch.Generator().manual_seed(5)
    pred = torch.randint(0, 17, (3, 224, 224), generator=g)
    tgt = torch.randint(0, 17, (3, 224, 224), generator=g)
    tgt[0] = pred[0]                     # a perfect image
    pred[1][pred[1] == 4] = 5            # a class that is never predicted in image 1
    ref = paed.iou_score(pred, tgt, 17)                       # CPU tensors: the reference loop
    got = paed.iou_score(pred.to(DEV), tgt.to(DEV), 17)       # device: class counts
    assert got.is_cuda and abs(float(got) - float(ref)) < 1e-6, (float(got), float(ref))


def test_paed_trainer_step_gradients_match_oracle():
    """PAEDTrainer (binary BCE + Dice + |soft-PAED|, model/PAED/classes.py:664-701): the loss tail runs as tensor
    ops on the logits, its gradient reaches the arena through vitseg_backward(grad_logits)."""
    from visiontransformer_amd import paed
    from visiontransformer_amd.params import arena_views
    cfg = ViTSegConfig(1, 16, 192, 2, 3, image_size=96)
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, seed=41).items()}
    x = torch.from_numpy(synth.make_images(cfg, 2, seed=7))
    g = torch.Generator().manual_seed(3)
    masks = (torch.rand(2, 128, 128, generator=g) > 0.5).long()
    sdf_e, sdf_i = torch.rand(2, 64, 64, generator=g) * 4, torch.rand(2, 64, 64, generator=g) * 2
    # oracle: CPU restatement forward + the same loss tail, autograd in fp64
    leaf = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    from oracle import paed_oracle as PO   # pinned to the reference's own functions by tests/test_paed_cpu.py
    m = O.resize_target(masks, (96, 96)).unsqueeze(1).double()
    ref = PO.binary_total(O.forward(x.double(), leaf, cfg), m, sdf_e.unsqueeze(1).double(), sdf_i.unsqueeze(1).double())
    ref.backward()
    t = paed.PAEDTrainer(1, 16, 192, 2, 3, image_size=96, dropout=0.0, device=DEV).train()
    t.load_state_dict({"model." + k: v for k, v in sd.items()})
    loss = t.training_step((x.to(DEV), masks.to(DEV), sdf_e.to(DEV), sdf_i.to(DEV)), 0)
    loss.backward()
    assert abs(float(loss.detach()) - float(ref)) < 1e-5
    gv = arena_views(cfg, t.model.arena.grad)
    for k, r in leaf.items():
        err = (gv[k].cpu().double() - r.grad).abs().max().item()
        assert err <= 3e-4 * max(r.grad.abs().max().item(), 1e-3), (k, err)
    # the 17-class module runs too (loss value vs the oracle forward)
    lm = paed.LightningViTModel(2, 16, 192, 1, 3, image_size=96, device=DEV).train()
    y17 = torch.randint(0, 17, (2, 128, 128), generator=g)
    l17 = lm.training_step((x.to(DEV), y17.to(DEV)), 0)
    l17.backward()
    assert torch.isfinite(l17) and lm.model.arena.grad.abs().sum() > 0 and lm.model.cfg.num_classes == 17


@pytest.mark.parametrize("name", [c for c in CASES if Golden(c).has("grad.seg_head.2.weight")])
def test_bf16_training_step_close_to_reference(name):
    """Mixed-precision training step (bf16 MFMA operands, fp32 master weights and gradients) against the fp32
    reference gradients: bf16 operand rounding (2^-9) through 12 layers -> per-tensor relative L2 error of a few
    per cent, direction (cosine) essentially unchanged.  No hard gate from the reference; the budget is written here."""
    g = Golden(name)
    c = g.cfg
    lm = LightningViTModel(c.num_classes, c.patch_size, c.hidden_size, c.num_hidden_layers, c.num_attention_heads,
                           image_size=c.image_size, precision="bf16", dropout=0.0, device=DEV).train()
    lm.load_state_dict({"model." + k: v for k, v in g.state_dict().items()})
    loss = lm.training_step((g.images().to(DEV), g.targets().to(DEV)), 0)
    assert abs(float(loss.detach()) - float(g.z["train.loss"][0])) < 5e-3
    loss.backward()
    from visiontransformer_amd.params import arena_views
    gv = arena_views(c, lm.model.arena.grad)
    if c.num_hidden_layers > 2:
        # at depth: exact fp64 gradients and the rounding model of the same step on the CPU, HIP held to the model's distance
        sd = g.state_dict()
        y = O.resize_target(g.targets(), (c.image_size, c.image_size))
        leaf = {k: v.double().requires_grad_(True) for k, v in sd.items()}
        O.ce_loss(O.forward(g.images().double(), leaf, c), y).backward()
        _, g_model = BM.training_step(g.images(), y, sd, c)
        _check_against_rounding_model(name, gv, {k: v.grad for k, v in leaf.items()}, g_model)
        return
    # fp32 path on the same inputs = dense reference for cosine / relative-L2 (goldens only hold samples)
    lm32 = _build(g).train()
    l32 = lm32.training_step((g.images().to(DEV), g.targets().to(DEV)), 0)
    l32.backward()
    g32 = arena_views(c, lm32.model.arena.grad)
    worst, worst_cos = 0.0, 1.0
    for k in gv:
        a, b = gv[k].double().flatten(), g32[k].double().flatten()
        if b.norm() < 1e-6:  # e.g. k_proj.bias: its gradient is identically zero (softmax is shift-invariant)
            assert a.norm() < 1e-4, (k, float(a.norm()))
            continue
        rel = float((a - b).norm() / b.norm())
        cos = float((a @ b) / (a.norm() * b.norm()))
        worst, worst_cos = max(worst, rel), min(worst_cos, cos)
        assert cos > BF16_GRAD_COS and rel < BF16_GRAD_REL, (k, rel, cos)
    print(f"{name}: bf16 vs fp32 gradients, worst per-tensor relative L2 error {worst:.3e}, worst cosine {worst_cos:.5f}")


def _dropout_case(image_size=96):
    cfg = ViTSegConfig(3, 16, 192, 2, 3, image_size=image_size)
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, seed=61).items()}
    x = torch.from_numpy(synth.make_images(cfg, 2, seed=8))
    y = torch.from_numpy(synth.make_targets(cfg, 2, seed=8, size=image_size))
    return cfg, sd, x, y


@pytest.mark.parametrize("image_size", [96, 208, 224])   # Np = 36 (below one key block), 169 and 196 (ragged, above one)
@pytest.mark.parametrize("route", ["small", "large"])
def test_dropout_training_step_matches_oracle_with_identical_masks(route, image_size):
    """Train-mode dropout (p = 0.1 at the four HF sites).  torch's RNG stream cannot be matched, but the build's
    masks are a pure function of (seed, layer, site, element): tests/dropout_ref.py regenerates them in numpy and
    injects them into the oracle, so forward AND backward can be compared exactly like the p = 0 case.  Both routes of the
    fp32 step (small-batch kernels / `no_small`: large-batch kernels) draw the same masks.  At the larger sizes `no_small` is the
    only way the fp32 large-batch attention pair with dropout meets injected masks at a ragged length above one key block."""
    from dropout_ref import Masks
    from visiontransformer_amd.params import arena_views
    cfg, sd, x, y = _dropout_case(image_size)
    m = ViTSegmentationModel(3, 16, 192, 2, 3, image_size=image_size, dropout=0.1, device=DEV).train()
    m.load_state_dict(sd)
    seed64 = (m.dropout_seed * 0x9E3779B97F4A7C15 + 1 * 0x100000001B3 + 0) & (2 ** 64 - 1)  # first training forward
    with _lib.option("no_small", int(route == "large")):
        loss = m.ce_loss(x.to(DEV), y.to(DEV))
        loss.backward()
    masks = Masks(0.1, seed64, 2, cfg.num_patches, 3)
    assert abs(float((masks.rows(0, 0, (2, cfg.num_patches + 1, 192)) > 0).float().mean()) - 0.9) < 0.01
    leaf = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    ref = O.ce_loss(O.forward(x.double(), leaf, cfg, drop=masks), y)
    ref.backward()
    assert abs(float(loss.detach()) - float(ref)) < 2e-6
    gv = arena_views(cfg, m.arena.grad)
    for k, r in leaf.items():
        err = (gv[k].cpu().double() - r.grad).abs().max().item()
        assert err <= 3e-4 * max(r.grad.abs().max().item(), 1e-4), (k, err, r.grad.abs().max().item())
    # a second step draws different masks; eval() / no_grad switch dropout off
    l2 = float(m.ce_loss(x.to(DEV), y.to(DEV)).detach())
    assert abs(l2 - float(loss.detach())) > 1e-7
    m.eval()
    with torch.no_grad():
        l_eval = float(m.ce_loss(x.to(DEV), y.to(DEV)))
    assert abs(l_eval - float(O.ce_loss(O.forward(x, sd, cfg), y))) < 2e-6


def test_dropout_bf16_consistent_with_fp32_same_masks():
    from visiontransformer_amd.params import arena_views
    cfg, sd, x, y = _dropout_case()
    grads = {}
    for prec in ("fp32", "bf16"):
        m = ViTSegmentationModel(3, 16, 192, 2, 3, image_size=96, dropout=0.1, precision=prec, device=DEV).train()
        m.load_state_dict(sd)
        m.ce_loss(x.to(DEV), y.to(DEV)).backward()  # same seed/step in both -> same masks
        grads[prec] = arena_views(cfg, m.arena.grad.clone())
    worst, worst_cos = 0.0, 1.0
    for k in grads["fp32"]:
        a, b = grads["bf16"][k].double().flatten(), grads["fp32"][k].double().flatten()
        if b.norm() < 1e-6:
            continue
        rel, cos = float((a - b).norm() / b.norm()), float((a @ b) / (a.norm() * b.norm()))
        worst, worst_cos = max(worst, rel), min(worst_cos, cos)
        assert rel < BF16_GRAD_REL and cos > BF16_GRAD_COS, (k, rel, cos)
    print(f"dropout, bf16 vs fp32 with the same masks: worst relative L2 {worst:.3e}, worst cosine {worst_cos:.5f}")


@pytest.mark.parametrize("precision,tol", [("fp32", 2e-4), ("bf16", 1.2e-1)])   # bf16: the tiny CLS gradient is the noisiest
def test_training_step_patch4_against_oracle_autograd(precision, tol):
    """Patch size 4 (48-wide im2col, 64 tokens at 32x32) through forward + CE + backward against autograd on the
    oracle: per-tensor relative L2 error of the gradients."""
    from visiontransformer_amd.params import arena_views
    cfg = ViTSegConfig(3, 4, 128, 1, 2, image_size=32)
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, seed=44).items()}
    x = torch.from_numpy(synth.make_images(cfg, 2, seed=4))
    y = torch.from_numpy(synth.make_targets(cfg, 2, seed=4, size=32))
    leaf = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    ref = O.ce_loss(O.forward(x.double(), leaf, cfg), y)
    ref.backward()
    m = ViTSegmentationModel(3, 4, 128, 1, 2, image_size=32, precision=precision, dropout=0.0, device=DEV).train()
    m.load_state_dict(sd)
    loss = m.ce_loss(x.to(DEV), y.to(DEV))
    loss.backward()
    assert abs(float(loss.detach()) - float(ref)) < (1e-5 if precision == "fp32" else 5e-3)
    gv = arena_views(cfg, m.arena.grad)
    for k, r in leaf.items():
        if r.grad is None or r.grad.norm().item() < 1e-6 or "pooler" in k:
            continue
        rel = (gv[k].cpu().double() - r.grad).norm().item() / r.grad.norm().item()
        assert rel < tol, (k, rel)


# ---------------------------------------------------------------- BASELINE configs[2] at its own image size
def _vitb_512_case(B, L=1, seed=71):
    cfg = ViTSegConfig(2, 16, 768, L, 12, image_size=512)
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, seed=seed).items()}
    x = torch.from_numpy(synth.make_images(cfg, B, seed=9))
    y = torch.from_numpy(synth.make_targets(cfg, B, seed=9, size=512))
    return cfg, sd, x, y


def _check_against_rounding_model(tag, hip, exact, model):
    """bf16 HIP gradients `hip` (name -> tensor), exact fp64 gradients `exact`, gradients of the rounding model `model`
    (oracle/bf16_model.py).  The model has no kernels, hence no kernel defects; its distance from the exact gradient is what
    bf16 storage costs at this depth (rounding noise compounds through the layers, and the q/k gradients of near-uniform
    attention are differences of nearly equal sums: test_attention_backward_bf16_is_its_rounding_model).  The HIP path
    must sit at the same distance, per tensor: a kernel that loses part of a gradient adds its loss on top."""
    rows, bad = [], []
    num_h = num_e = den = 0.0
    for k, r in exact.items():
        if r is None or "pooler" in k:
            continue
        r = r.double().flatten()
        h, e = hip[k].detach().cpu().double().flatten(), model[k].double().flatten()
        if r.norm() < 1e-7:
            if h.norm() >= 1e-4:
                bad.append((k, "zero-gradient tensor", float(h.norm())))
            continue
        rel_h, rel_e = float((h - r).norm() / r.norm()), float((e - r).norm() / r.norm())
        cos_h, cos_e = float((h @ r) / (h.norm() * r.norm())), float((e @ r) / (e.norm() * r.norm()))
        num_h, num_e, den = num_h + float((h - r).pow(2).sum()), num_e + float((e - r).pow(2).sum()), den + float(r.pow(2).sum())
        rows.append((rel_h / max(rel_e, 1e-12), k, rel_h, rel_e, cos_h, cos_e))
        if not (rel_h <= MODEL_RATIO * rel_e + MODEL_SLACK and cos_h >= cos_e - MODEL_SLACK):
            bad.append((k, rel_h, rel_e, cos_h, cos_e))
    whole_h, whole_e = (num_h / den) ** 0.5, (num_e / den) ** 0.5
    rows.sort(reverse=True)
    worst = max(rows, key=lambda t: t[2])
    print(f"{tag}: bf16 gradients vs fp64, HIP | rounding model: whole gradient {whole_h:.3e} | {whole_e:.3e}; "
          f"worst tensor {worst[1]} {worst[2]:.3e} | {worst[3]:.3e} (cosine {worst[4]:.4f} | {worst[5]:.4f}); "
          f"largest HIP/model ratios: " + ", ".join(f"{k} {a:.3f}/{b:.3f}" for _, k, a, b, _, _ in rows[:4]))
    assert not bad, bad[:8]
    assert whole_h <= MODEL_RATIO * whole_e + 0.005, (whole_h, whole_e)
    return whole_h, whole_e


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_training_step_vitb_width_512(precision):
    """ViT-B width (D 768, 12 heads, I 3072), 512x512, batch 8 (M = 8200 token rows), one layer: the shapes at which
    the bf16 path takes the 256x256 / 256x128 tiles and the CLS rows of the QKV / dgrad GEMMs go through the split-K
    side launch (forward.hip walk_large / vitseg_train.hip backward_bf16), against autograd on the oracle
    (model/CE/classes.py:276-285 restated by O.training_step)."""
    B = 8
    cfg, sd, x, y = _vitb_512_case(B)
    torch.set_num_threads(16)
    leaf = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    stages = {}
    ref = O.ce_loss(O.forward(x.double(), leaf, cfg, stages=stages), y)
    ref.backward()
    m = ViTSegmentationModel(2, 16, 768, 1, 12, image_size=512, precision=precision, dropout=0.0, device=DEV).train()
    m.load_state_dict(sd)
    loss = m.ce_loss(x.to(DEV), y.to(DEV))
    loss.backward()
    assert abs(float(loss.detach()) - float(ref)) < (2e-6 if precision == "fp32" else 5e-3)
    worst, _ = _grad_check(cfg, m.arena.grad, leaf, precision, stages)
    print(f"512x512 ViT-B-width training step, {precision}: worst per-tensor relative L2 gradient error {worst:.3e}")


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_training_step_vitb_width_512_dropout_masks_injected(precision):
    """The same step at batch 4 (M = 4100: the >= 4096-row tiles) in train mode with the reference's dropout 0.1 at the
    four HF sites; the build's counter-based masks are regenerated in numpy and injected into the oracle."""
    from dropout_ref import Masks
    B = 4
    cfg, sd, x, y = _vitb_512_case(B, seed=72)
    torch.set_num_threads(16)
    m = ViTSegmentationModel(2, 16, 768, 1, 12, image_size=512, precision=precision, dropout=0.1, device=DEV).train()
    m.load_state_dict(sd)
    seed64 = (m.dropout_seed * 0x9E3779B97F4A7C15 + 1 * 0x100000001B3 + 0) & (2 ** 64 - 1)  # first training forward
    loss = m.ce_loss(x.to(DEV), y.to(DEV))
    loss.backward()
    masks = Masks(0.1, seed64, B, cfg.num_patches, 12)
    leaf = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    stages = {}
    ref = O.ce_loss(O.forward(x.double(), leaf, cfg, stages=stages, drop=masks), y)
    ref.backward()
    assert abs(float(loss.detach()) - float(ref)) < (2e-6 if precision == "fp32" else 5e-3)
    _grad_check(cfg, m.arena.grad, leaf, precision, stages)


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_training_step_vitb16_full_depth_512(p):
    """BASELINE configs[2] at full depth: ViT-B/16 (D 768, L 12, 12 heads, I 3072) on 512x512 inputs, batch 2, one training
    step (forward + CE + backward; model/CE/classes.py:276-285 over transformers' modeling_vit.py:164-286) in bf16 mixed
    precision AND in fp32 against fp64 autograd on the oracle -- every parameter tensor, dense -- with dropout off and with
    the reference's dropout 0.1 (the build's counter-based masks regenerated in numpy and injected into the oracle)."""
    from dropout_ref import Masks
    B = 2
    cfg, sd, x, y = _vitb_512_case(B, L=12, seed=73)
    torch.set_num_threads(16)
    models = {}
    for prec in ("fp32", "bf16"):
        m = ViTSegmentationModel(2, 16, 768, 12, 12, image_size=512, precision=prec, dropout=p, device=DEV).train()
        m.load_state_dict(sd)
        seed64 = (m.dropout_seed * 0x9E3779B97F4A7C15 + 1 * 0x100000001B3 + 0) & (2 ** 64 - 1)  # first training forward
        loss = m.ce_loss(x.to(DEV), y.to(DEV))
        loss.backward()
        models[prec] = (m, float(loss.detach()), seed64)
    assert models["fp32"][2] == models["bf16"][2]          # same seed and step: the same masks in both precisions
    masks = Masks(p, models["fp32"][2], B, cfg.num_patches, 12) if p else None
    leaf = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    stages = {}
    ref = O.ce_loss(O.forward(x.double(), leaf, cfg, stages=stages, drop=masks), y)
    ref.backward()
    print(f"full-depth ViT-B/16 512x512 step, dropout {p}: loss oracle {float(ref):.6f}, fp32 {models['fp32'][1]:.6f}, "
          f"bf16 {models['bf16'][1]:.6f}")
    assert abs(models["fp32"][1] - float(ref)) < 5e-6
    assert abs(models["bf16"][1] - float(ref)) < 5e-3
    _, whole = _grad_check(cfg, models["fp32"][0].arena.grad, leaf, "fp32", stages)
    assert whole < 1e-4, whole                 # the gradient as ONE vector (what the optimizer sees)
    # bf16: against the rounding model of the same step (same masks), tensor by tensor
    from visiontransformer_amd.params import arena_views
    loss_m, g_model = BM.training_step(x, y, sd, cfg, drop=masks)
    assert abs(models["bf16"][1] - float(loss_m)) < 1e-3
    _check_against_rounding_model(f"full-depth ViT-B/16 512x512, dropout {p}", arena_views(cfg, models["bf16"][0].arena.grad),
                                  {k: v.grad for k, v in leaf.items()}, g_model)


def test_training_step_reproducible_at_the_training_size():
    """BASELINE configs[2] size (ViT-B/16, 512 x 512, batch 64, bf16 mixed precision, dropout 0.1).  With dropout 0 the step is
    compared with its decomposition into B = 2 steps in test_gpu_production_size.py; the dropout masks depend on an image's
    index in the batch, so here a size-independent property -- the step has no atomics and every reduction a fixed order, so the
    same step (same parameters, batch, dropout seed and step counter) gives the same loss and the same gradient of all
    88.8 M parameters BIT FOR BIT; and a different dropout step changes them (the masks are really applied)."""
    B = 64
    cfg, sd, x, y = _vitb_512_case(B, L=12, seed=73)
    xd, yd = x.to(DEV), y.to(DEV)
    grads, losses = [], []
    for step0 in (0, 0, 1):
        m = ViTSegmentationModel(2, 16, 768, 12, 12, image_size=512, precision="bf16", dropout=0.1, device=DEV).train()
        m.load_state_dict(sd)
        m._dropout_step = step0
        loss = m.ce_loss(xd, yd)
        loss.backward()
        grads.append(m.arena.grad.detach().clone())
        losses.append(float(loss.detach()))
        del m
        torch.cuda.empty_cache()
    assert all(torch.isfinite(g).all() for g in grads)
    assert losses[0] == losses[1] and torch.equal(grads[0], grads[1])
    assert losses[2] != losses[0] and not torch.equal(grads[2], grads[0])
    rel = float((grads[2] - grads[0]).norm() / grads[0].norm())
    assert 1e-3 < rel < 1.0, rel   # other masks: a different but comparable gradient


@pytest.mark.parametrize("B,Np,A,p", [(2, 256, 2, 0.0), (1, 1024, 2, 0.0), (2, 196, 3, 0.0), (1, 64, 1, 0.0), (2, 100, 2, 0.0),
                                      (1, 1024, 1, 0.1), (2, 196, 2, 0.1), (2, 256, 3, 0.1),
                                      (1, 1024, 1, -0.1), (2, 256, 3, -0.1),
                                      # ragged against the query / key blocks: below one block, one either side of 128 and 256
                                      (1, 4, 1, 0.0), (2, 31, 2, 0.0), (3, 127, 1, 0.0), (1, 129, 3, 0.0), (2, 255, 2, 0.1),
                                      (1, 257, 1, 0.0), (1, 128, 2, -0.1)])
def test_attention_backward_bf16(B, Np, A, p):
    """bf16 attention core, forward (ctx, log-sum-exp) + backward (dq | dk | dv), with and without the attention-probability
    dropout (the kernels' counter-based mask regenerated in numpy and injected into the reference), against fp64 autograd
    on the same bf16-rounded inputs.  Whole-tile (Np % 128 == 0) and ragged shapes; the CLS token takes the vector paths.
    p < 0: |p| with the keep bits precomputed as mask words (attention_dropmask.hip, the training step's path) -- the same
    reference masks, so this also pins the word layout against tests/dropout_ref.py."""
    from dropout_ref import Masks
    words = p < 0
    p = abs(p)
    D, Mt, N = 64 * A, B * Np + B, Np + 1
    qkv = _rand(Mt, 3 * D, seed=Np + A, scale=1.2).to(torch.bfloat16)
    dctx = _rand(Mt, D, seed=9).to(torch.bfloat16)
    seed, stream_id = 0xBEEF1234, 3 * 8 + 1
    x = qkv.double().requires_grad_(True)
    mask = None
    if p:
        mk = Masks(p, seed, B, Np, A)
        mask = mk.attn(3, (B, A, N, N)).double()      # reference token order (CLS first), layer 3 -> stream 3 * 8 + 1
    ctx_ref = torch.empty(Mt, D, dtype=torch.float64)
    lse_ref = torch.empty(B, A, N, dtype=torch.float64)
    outs = []
    for b in range(B):
        r = torch.cat([torch.tensor([B * Np + b]), torch.arange(b * Np, (b + 1) * Np)])
        q, k, v = [x[r][:, i * D:(i + 1) * D].reshape(N, A, 64).transpose(0, 1) for i in range(3)]
        sc = q @ k.transpose(-1, -2) * 0.125
        s = torch.softmax(sc, dim=-1)
        if mask is not None:
            s = s * mask[b]
        o = (s @ v).transpose(0, 1).reshape(N, D)
        ctx_ref[r] = o.detach()
        l2 = torch.logsumexp(sc.detach(), dim=-1) * 1.4426950408889634           # [A, N] reference order, log2 domain
        lse_ref[b] = torch.cat([l2[:, 1:], l2[:, :1]], dim=1)                    # kernel order: CLS last
        outs.append((o * dctx.double()[r]).sum())
    torch.stack(outs).sum().backward()
    qd, dd = _dev(qkv, name="qkv"), _dev(dctx, name="dctx")
    ctx = _out((Mt, D), torch.bfloat16, name="ctx")
    lse = _out((B * A * N,), name="lse")
    scr = _out((_lib.lib().vitseg_attention_bwd_scratch_floats(B, Np, A),), name="attention_bwd scratch")
    dqkv = _out((Mt, 3 * D), torch.bfloat16, name="dqkv")
    mw = _out((_lib.lib().vitseg_attention_dropmask_bytes(B, Np, A),), torch.uint8, name="dropmask words") if words else None
    dbias = _out((3 * D,), name="dbias_qkv")
    snap = snapshot(qd, dd)
    _lib.check(_lib.lib().vitseg_op_attention_bwd_bf16(qd.data_ptr(), dd.data_ptr(), ctx.data_ptr(), lse.data_ptr(),
                                                       scr.data_ptr(), dqkv.data_ptr(), B, Np, A, p, seed, stream_id,
                                                       mw.data_ptr() if words else None, dbias.data_ptr(), _stream()))
    _after(snap, ctx, lse, scr, dqkv, mw, dbias)
    got, ref = dqkv.float().cpu().double(), x.grad
    assert torch.isfinite(got).all()
    # the fused QKV bias gradient = the column sums of dqkv (the kernels sum their fp32 accumulators, the stored values are
    # those rounded to bf16: the two differ by the rounding noise of Mt values per column), and the same bits without it
    csum = got.sum(dim=0)
    db = dbias.cpu().double()
    assert torch.isfinite(db).all()
    assert float((db - csum).norm() / got.abs().sum(dim=0).norm()) < 1e-3, float((db - csum).norm() / got.abs().sum(dim=0).norm())
    assert float((db - ref.sum(dim=0)).norm() / ref.abs().sum(dim=0).norm()) < 5e-3
    dqkv2 = _out((Mt, 3 * D), torch.bfloat16, name="dqkv (second call)")
    _lib.check(_lib.lib().vitseg_op_attention_bwd_bf16(qd.data_ptr(), dd.data_ptr(), ctx.data_ptr(), lse.data_ptr(),
                                                       scr.data_ptr(), dqkv2.data_ptr(), B, Np, A, p, seed, stream_id,
                                                       mw.data_ptr() if words else None, None, _stream()))
    _after(snap, ctx, lse, scr, dqkv2, mw)
    assert torch.equal(dqkv.view(torch.int16), dqkv2.view(torch.int16))
    assert (ctx.float().cpu().double() - ctx_ref).abs().max().item() < 4e-2
    # the log-sum-exp the backward rebuilds P from: fp32 out of exact products of bf16 values and fp32 sums, held to the fp32
    # gate of test_attention_small_forward_and_backward_for_training (tests/test_gpu_attention_keys.py LSE_GATE)
    lse_err = (lse.cpu().double().view(B, A, N) - lse_ref).abs().max().item()
    assert lse_err < 2e-5, lse_err
    # P, dS and the outputs are rounded to bf16 (2^-9): a few 1e-3 relative to the gradient scale, per slot
    for i, name in enumerate(("dq", "dk", "dv")):
        a, r_ = got[:, i * D:(i + 1) * D], ref[:, i * D:(i + 1) * D]
        assert (a - r_).abs().max().item() < 2e-2 * r_.abs().max().item(), name
        assert float((a - r_).norm() / r_.norm()) < 1e-2, name
    # the CLS rows take the vector kernels: check them on their own
    cls = slice(B * Np, Mt)
    assert (got[cls] - ref[cls]).abs().max().item() < 2e-2 * ref[cls].abs().max().item()


@pytest.mark.parametrize("Np,A,spread,p", [(1024, 2, 1.0, 0.0), (1024, 2, 0.3, 0.0), (1024, 1, 0.1, 0.0), (256, 3, 0.3, 0.0),
                                           (1024, 1, 0.3, -0.1), (196, 2, 0.3, 0.1)])
def test_attention_backward_bf16_is_its_rounding_model(Np, A, spread, p):
    """Where the bf16 q/k gradients' large relative error at depth comes from, shown on the kernels themselves.  At random
    init the tokens of an image are nearly alike by the middle of the encoder (attention is near-uniform), i.e. every key
    is a common vector plus a small own part (`spread`).  Then dq_i = c sum_j dS_ij k_j is the small remainder of a sum whose
    bulk, (sum_j dS_ij) k_mean, vanishes only in exact arithmetic: rounding dS to bf16 and taking delta from the bf16
    context leave sum_j dS_ij != 0 and the error rides on the LARGE common part of the keys.  The test runs the three HIP
    backward kernels and (a) exact fp64 autograd, (b) the rounding model (oracle/bf16_model.py attention_backward: the same
    formulas with bf16(dS), bf16(P~) and delta from the kernel's own bf16 context), all on identical bf16 inputs:
    the kernels must equal the MODEL to ~1e-2 per slot even where both are tens of per cent from exact arithmetic.
    p < 0: dropout |p| through precomputed mask words."""
    from dropout_ref import Masks
    words, p = p < 0, abs(p)
    B, hd = 1, 64
    D, Mt, N = hd * A, B * Np + B, Np + 1
    gen = torch.Generator().manual_seed(Np + A)
    base = torch.randn(1, 3 * D, generator=gen) * 0.55
    qkv = (base + spread * 0.55 * torch.randn(Mt, 3 * D, generator=gen)).to(torch.bfloat16)
    dctx = (torch.randn(1, D, generator=gen) + torch.randn(Mt, D, generator=gen)).to(torch.bfloat16)
    seed, stream_id = 0xBEEF1234, 3 * 8 + 1
    qd, dd = _dev(qkv, name="qkv"), _dev(dctx, name="dctx")
    ctx = _out((Mt, D), torch.bfloat16, name="ctx")
    lse = _out((B * A * N,), name="lse")
    scr = _out((_lib.lib().vitseg_attention_bwd_scratch_floats(B, Np, A),), name="attention_bwd scratch")
    dqkv = _out((Mt, 3 * D), torch.bfloat16, name="dqkv")
    mw = _out((_lib.lib().vitseg_attention_dropmask_bytes(B, Np, A),), torch.uint8, name="dropmask words") if words else None
    snap = snapshot(qd, dd)
    _lib.check(_lib.lib().vitseg_op_attention_bwd_bf16(qd.data_ptr(), dd.data_ptr(), ctx.data_ptr(), lse.data_ptr(),
                                                       scr.data_ptr(), dqkv.data_ptr(), B, Np, A, p, seed, stream_id,
                                                       mw.data_ptr() if words else None, None, _stream()))
    _after(snap, ctx, lse, scr, dqkv, mw)
    got = dqkv.float().cpu().double()
    assert torch.isfinite(got).all()
    # reference token order (CLS first) <- patches-first rows; [1, A, N, hd] views
    r = torch.cat([torch.tensor([B * Np]), torch.arange(0, Np)])

    def heads(t):
        return t[r].reshape(N, A, hd).transpose(0, 1)[None]

    x = qkv.double()
    q, k, v = [heads(x[:, i * D:(i + 1) * D]).clone().requires_grad_(True) for i in range(3)]
    do = heads(dctx.double())
    mask = Masks(p, seed, B, Np, A).attn(3, (B, A, N, N)).double() if p else None
    prob = torch.softmax(q @ k.transpose(-1, -2) * hd ** -0.5, dim=-1)
    ((prob if mask is None else prob * mask) @ v * do).sum().backward()
    exact = [t.grad for t in (q, k, v)]
    # the model's backward on the kernel's OWN context and log-sum-exp (log2 units, CLS last -> natural log, CLS first)
    o_k = heads(ctx.float().cpu().double())
    lse_k = lse.cpu().double().reshape(B, A, N)
    lse_k = (torch.cat([lse_k[..., Np:], lse_k[..., :Np]], dim=-1) * float(np.log(2.0)))[..., None]
    with torch.no_grad():
        model = BM.attention_backward(q.detach(), k.detach(), v.detach(), do, o_k, lse_k, mask)
    line = []
    for i, name in enumerate(("dq", "dk", "dv")):
        gk = heads(got[:, i * D:(i + 1) * D])
        vs_model = float((gk - BM.rb(model[i])).norm() / model[i].norm())
        vs_exact = float((gk - exact[i]).norm() / exact[i].norm())
        model_vs_exact = float((model[i] - exact[i]).norm() / exact[i].norm())
        line.append(f"{name}: kernel-model {vs_model:.2e}, kernel-exact {vs_exact:.2e}, model-exact {model_vs_exact:.2e}")
        # the output rounding alone is 2^-9 (rel. L2 ~2e-3); the rest is fp32 vs fp64 inside: a few roundings of dS flip
        assert vs_model < 1e-2 + 0.05 * model_vs_exact, (name, vs_model, vs_exact, model_vs_exact)
    print(f"Np {Np}, heads {A}, own part {spread}, dropout {p}{' (words)' if words else ''}: " + "; ".join(line))


def test_resume_restores_optimizer_state(tmp_path):
    """trainer.fit(ckpt_path=...) in the reference (model/CE/trainCurrentViTmodel.py:67-73) restores Adam's moments and
    step count; so does the checkpoint written here: epoch 0 -> checkpoint -> resume for epoch 1 must land on exactly
    the parameters of an uninterrupted two-epoch run (a restart from zero moments would not)."""
    from visiontransformer_amd import trainer
    cfg = ViTSegConfig(2, 16, 192, 2, 3, image_size=96)
    xs = torch.from_numpy(synth.make_images(cfg, 8, seed=0))
    ys = torch.from_numpy(synth.make_targets(cfg, 8, seed=0))
    batches = [(xs[i:i + 2], ys[i:i + 2]) for i in range(0, 8, 2)]

    def make():
        lm = LightningViTModel(2, 16, 192, 2, 3, image_size=96, dropout=0.0, device=DEV)
        lm.model.reset_parameters(seed=5)
        return lm

    a = make()
    trainer.fit(a, batches, None, max_epochs=2, accumulate_grad_batches=2, device=DEV)
    b = make()
    trainer.fit(b, batches, None, max_epochs=1, accumulate_grad_batches=2, ckpt_dir=str(tmp_path / "ck"), device=DEV)
    ck = tmp_path / "ck" / "epoch=0-step=2.ckpt"
    saved = torch.load(ck)
    assert saved["optimizer_states"][0]["state"][0]["step"] == 2 and "exp_avg_sq" in saved["optimizer_states"][0]["state"][0]
    c = make()
    trainer.fit(c, batches, None, max_epochs=2, accumulate_grad_batches=2, resume_from=str(ck), device=DEV)
    assert torch.equal(c.model.arena.detach(), a.model.arena.detach())
    d = make()                                   # control: weights only, moments from zero -> a different epoch-1 update
    d.load_state_dict(saved["state_dict"])
    trainer.fit(d, batches, None, max_epochs=1, accumulate_grad_batches=2, device=DEV)
    assert not torch.equal(d.model.arena.detach(), a.model.arena.detach())
