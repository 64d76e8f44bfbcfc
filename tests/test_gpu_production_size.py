"""GPU (-m gpu): the production sizes against references that are cheap to compute there.

The fp64 oracle, the decomposition of a batch into independent B = 2 training steps and torch.optim run at the batch sizes the
project exists for -- the headline inference batch (ViT-B/16, 32 x 512^2), the benchmarked training steps (fp32 B = 16 on
the large-batch route, bf16 B = 64) and the Adam kernel over whole grid strides of the real arena -- where only
size-independent properties (batch invariance, bit-for-bit reproducibility) were checked before: a kernel that is wrong the
same way on every run, or only past a trip count, a split count or a stride that small batches never reach, fails here."""
import pytest
import torch

from guard import check, guarded, snapshot, unchanged
from oracle import vitseg_oracle as O
from test_gpu_backward import _vitb_512_case
from util import BF16_GRAD_COS, BF16_GRAD_REL
from visiontransformer_amd import _lib, synth
from visiontransformer_amd.config import ViTSegConfig
from visiontransformer_amd.model import ViTSegmentationModel
from visiontransformer_amd.params import arena_views

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---------------------------------------------------------------- 1. the headline forward against the fp64 oracle
HEADLINE_IMAGES = [0, 15, 31]   # the first, a middle and the last image: 31's CLS row is the last token row of the batch


@pytest.fixture(scope="module")
def headline():
    """The batch of test_batch_invariance_at_the_headline_size (BASELINE configs[1]: ViT-B/16, 512 x 512, batch 32, weights
    seed 5, images seed 9) with the bias of class 1 shifted by the median fp32 logit difference of images 0-3, so that the
    decision boundary runs through the images; the fp64 oracle of the sampled images (one image is ~0.2 TFLOP: seconds on
    16 threads, not minutes)."""
    cfg = ViTSegConfig(2, 16, 768, 12, 12, image_size=512)
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, seed=5).items()}
    x = torch.from_numpy(synth.make_images(cfg, 32, seed=9))
    m = ViTSegmentationModel(2, 16, 768, 12, 12, image_size=512, device=DEV).eval()
    m.load_state_dict(sd)
    with torch.no_grad():
        _, lg = m.predict_mask(x[:4].to(DEV), return_logits=True)
    sd["seg_head.2.bias"] = sd["seg_head.2.bias"].clone()
    sd["seg_head.2.bias"][1] += float((lg[:, 0] - lg[:, 1]).median())
    del m, lg
    torch.cuda.empty_cache()
    torch.set_num_threads(16)
    with torch.no_grad():
        ref = O.forward(x[HEADLINE_IMAGES].double(), {k: v.double() for k, v in sd.items()}, cfg)
    return cfg, sd, x, ref


def _compare_forward(tag, logits, mask, ref, tol):
    """max |logits - oracle| < tol, and the mask equal to the oracle's on every pixel the measured error cannot flip."""
    err = (logits.cpu().double() - ref).abs().max().item()
    ref_mask = O.predict_mask(ref.float())
    stable = O.mask_stable(ref.float(), 2.0 * err + 1e-7)
    differ = mask.cpu().long() != ref_mask
    unstable = float((~stable).float().mean())
    print(f"{tag}: logits max-abs err {err:.3e} (gate {tol:.0e}), {int((differ & stable).sum())} mask mismatches at "
          f"stable pixels, {int(differ.sum())} among the {unstable:.4%} others")
    assert err < tol, (tag, err)
    assert int((differ & stable).sum()) == 0, tag
    return err, unstable


@pytest.mark.parametrize("precision,tol", [("fp32", 2e-5), ("fp16", 2e-3), ("bf16", 3e-2)])
def test_headline_forward_against_fp64_oracle(headline, precision, tol):
    """Images 0, 15 and 31 of the headline batch of 32 (fp32: 32 800 token rows, the large-batch route) against the fp64
    oracle, at the logit gates of test_reference_configuration_grid (fp32 2e-5, fp16 2e-3, bf16 3e-2); masks identical on
    every pixel `O.mask_stable` marks stable.  fp32 also keeps the stable share of test_forward_matches_golden (> 99.8 %).
    Measured on the MI355X: logits 1.7e-6 fp32, 5.8e-4 fp16, 4.9e-3 bf16; 0 mismatches at stable pixels (0.011 % of the
    pixels unstable in fp32, 3.0 % fp16, 25 % bf16: the class logits are ~0.02 apart with the shifted bias)."""
    cfg, sd, x, ref = headline
    m = ViTSegmentationModel(2, 16, 768, 12, 12, image_size=512, precision=precision, device=DEV).eval()
    m.load_state_dict(sd)
    with torch.no_grad():
        mask, logits = m.predict_mask(x.to(DEV), return_logits=True)
        mask, logits = mask[HEADLINE_IMAGES], logits[HEADLINE_IMAGES]
    frac1 = float(mask.float().mean())
    assert 0.05 < frac1 < 0.95, frac1
    _, unstable = _compare_forward(f"headline ViT-B/16 32 x 512^2 {precision}, images {HEADLINE_IMAGES}", logits, mask, ref, tol)
    if precision == "fp32":
        assert unstable < 2e-3, unstable


def test_seventeen_classes_headline_against_fp64_oracle():
    """The 17-class headline case of test_seventeen_classes_at_the_headline_size (2 layers, head gain 8, batch 32 at
    512 x 512, fp32 on the large-batch route): images 0 and 31 against the fp64 oracle.  Gate 2e-5 x the head gain (the logits
    are 8 x larger; test_forward_matches_golden scales its gate the same way).  Measured on the MI355X: 1.2e-5, 0 mask
    mismatches, 0.0004 % of the pixels unstable."""
    cfg = ViTSegConfig(17, 16, 768, 2, 12, image_size=512)
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, seed=6, head_gain=8.0).items()}
    x = torch.from_numpy(synth.make_images(cfg, 32, seed=4))
    m = ViTSegmentationModel(17, 16, 768, 2, 12, image_size=512, device=DEV).eval()
    m.load_state_dict(sd)
    with torch.no_grad():
        mask, logits = m.predict_mask(x.to(DEV), return_logits=True)
        mask, logits = mask[[0, 31]], logits[[0, 31]]
    torch.set_num_threads(16)
    with torch.no_grad():
        ref = O.forward(x[[0, 31]].double(), {k: v.double() for k, v in sd.items()}, cfg)
    assert len(torch.unique(mask[1])) >= 5
    _, unstable = _compare_forward("17 classes 32 x 512^2 fp32, images [0, 31]", logits, mask, ref, 2e-5 * 8.0)
    assert unstable < 2e-3, unstable


# ---------------------------------------------------------------- 2. the training step against its decomposition
# With dropout 0 an image's forward does not depend on the batch and the CE loss is a mean over pixels, so the loss and the
# gradient of a batch of B are the mean of those of its B / 2 sub-batches of 2 images.  synth's images and targets are
# prefix-stable (image i depends on (seed, i) only): piece 0 is exactly the case test_training_step_vitb16_full_depth_512
# pins to fp64 autograd.  Dropout at these sizes stays covered by test_training_step_reproducible_at_the_training_size and
# the small-size mask tests only: the keep bits depend on an image's index in the batch, so no decomposition exists for them.
PIECE = 2


def _model(precision):
    return ViTSegmentationModel(2, 16, 768, 12, 12, image_size=512, precision=precision, dropout=0.0, device=DEV).train()


def _full_step(sd, x, y, precision):
    """loss and float64 gradient of ONE training step over the whole batch; the model is freed afterwards"""
    m = _model(precision)
    m.load_state_dict(sd)
    loss = m.ce_loss(x.to(DEV), y.to(DEV))
    loss.backward()
    out = float(loss.detach()), m.arena.grad.detach().double()
    del m, loss
    torch.cuda.empty_cache()
    return out


def _pieces(sd, x, y, precision, n):
    """the first n B = 2 steps: running float64 sums of their losses and gradients after 8 and after n pieces, each with the
    gradient of its last piece (for the negative controls)"""
    m = _model(precision)
    m.load_state_dict(sd)
    gsum = torch.zeros(m.arena.numel(), dtype=torch.float64, device=DEV)
    lsum, sums = 0.0, {}
    for k in range(n):
        m.arena.grad = None
        sl = slice(k * PIECE, (k + 1) * PIECE)
        loss = m.ce_loss(x[sl].to(DEV), y[sl].to(DEV))
        loss.backward()
        g = m.arena.grad.detach().double()
        gsum += g
        lsum += float(loss.detach())
        if k + 1 in (8, n):
            sums[k + 1] = (lsum, gsum.clone(), g)
    del m
    torch.cuda.empty_cache()
    return sums


@pytest.fixture(scope="module")
def training_case():
    """ViT-B/16 at 512 x 512, 12 layers, batch 64 (_vitb_512_case(64, L=12, seed=73)); the B = 2 decompositions in fp32 (the
    small-batch route) and bf16: sums over the first 8 pieces (the batch of 16) and over all 32 (the batch of 64)."""
    cfg, sd, x, y = _vitb_512_case(64, L=12, seed=73)
    return dict(cfg=cfg, sd=sd, x=x, y=y, f32=_pieces(sd, x, y, "fp32", 32), b16=_pieces(sd, x, y, "bf16", 32))


def _distances(cfg, got, ref):
    """relative L2 distance of `got` from `ref` (float64 arenas): per parameter tensor and over all of them as one vector.
    Left out: the pooler (not part of the model's loss) and the key biases, whose exact gradient is zero (softmax is
    shift-invariant): both sides hold only rounding noise there, which the bf16 steps make large relative to nothing."""
    gv, rv = arena_views(cfg, got), arena_views(cfg, ref)
    per, num, den = {}, 0.0, 0.0
    for k, r in rv.items():
        if "pooler" in k or k.endswith("k_proj.bias"):
            continue
        d2, r2 = float((gv[k] - r).pow(2).sum()), float(r.pow(2).sum())
        per[k] = (d2 / r2) ** 0.5
        num, den = num + d2, den + r2
    return (num / den) ** 0.5, per


def _violations(whole, per, whole_gate, tensor_gate):
    """gates that a distance breaks; tensor_gate: name -> gate"""
    bad = [("whole gradient", whole, whole_gate)] if not whole < whole_gate else []
    bad += [(k, d, tensor_gate(k)) for k, d in per.items() if not d < tensor_gate(k)]
    return bad


def _worst(per, n=1):
    return ", ".join(f"{k} {per[k]:.3e}" for k in sorted(per, key=per.get, reverse=True)[:n])


def _decomposition_check(tag, cfg, loss, grad, lsum, gsum, n, last, loss_gate, whole_gate, tensor_gate):
    """the step's loss and gradient against the mean of its n pieces (loss sum `lsum`, float64 gradient sum `gsum`), and the
    negative control: the same gates applied to the reference without its last piece `last`, rescaled (1 / n of the rows
    missing, computed on the host side only) must break at least one of them"""
    lref = lsum / n
    whole, per = _distances(cfg, grad, gsum / n)
    c_whole, c_per = _distances(cfg, grad, (gsum - last) / (n - 1))
    bad = _violations(whole, per, whole_gate, tensor_gate)
    c_bad = _violations(c_whole, c_per, whole_gate, tensor_gate)
    print(f"{tag}: loss {loss:.7f} vs the mean of {n} pieces {lref:.7f} (|d| {abs(loss - lref):.2e}, gate {loss_gate:.0e}); "
          f"gradient relative L2 whole {whole:.3e} (gate {whole_gate:.0e}), worst tensors {_worst(per, 3)}; "
          f"negative control (one piece dropped): whole {c_whole:.3e}, worst tensors {_worst(c_per, 3)}, "
          f"{len(c_bad)} gates broken: {[b[0] for b in c_bad[:4]]}")
    assert abs(loss - lref) < loss_gate, (loss, lref)
    assert not bad, bad[:8]
    assert c_bad, "the gates cannot see a missing B = 2 share of the batch"


def test_training_step_fp32_b16_against_its_decomposition(training_case):
    """fp32 training step at B = 16 (16 400 token rows: the large-batch route, split-K weight gradients with up to 28 slabs)
    against the float64 mean of its 8 B = 2 steps (small-batch route, each pinned to fp64 autograd at B = 2).  Gates: the
    loss at 5e-6 and the gradient as one vector at 1e-4 (test_training_step_vitb16_full_depth_512), every tensor at
    grad_check's fp32 2e-4.  Measured on the MI355X: loss 2.2e-8, whole 2.8e-7, worst tensor 1.4e-6 (layer 8 k_proj.weight;
    no seg-head ReLU flip shows: both routes compute the head in fp32 within ~1e-7 of each other, so position_embeddings is
    gated like every tensor); negative control: whole 3.3e-3, worst tensor 5.6e-2, 191 gates broken."""
    c = training_case
    cfg, sd, x, y = c["cfg"], c["sd"], c["x"], c["y"]
    lsum, gsum, last = c["f32"][8]
    loss, grad = _full_step(sd, x[:16], y[:16], "fp32")
    _decomposition_check("fp32 B = 16", cfg, loss, grad, lsum, gsum, 8, last, 5e-6, 1e-4, lambda k: 2e-4)


BF16_WHOLE, BF16_NOISE_RATIO = 5e-4, 1.0


def test_training_step_bf16_b64_against_its_decomposition(training_case):
    """bf16 training step at B = 64 (65 600 token rows, the benchmarked step) against the float64 mean of its 32 bf16 B = 2
    steps.  The tile shapes (and so the fp32 summation trees in front of each bf16 rounding) differ by row count, so the two
    agree only up to bf16 rounding noise, which differs a lot between tensors (the q/k gradients of the middle layers carry
    ~5e-2 of it, the head biases ~2e-3).  Each tensor's noise is measured in the test itself: the distance of the bf16
    decomposition from the fp32 one (32 fp32 B = 2 steps).  Gates: the loss at 5e-3 (the bf16 loss gate of the full-depth
    test); the gradient as one vector at 5e-4; every tensor within 1.0 x its own noise.  Measured on the MI355X: loss 4.6e-7,
    whole 2.2e-4, worst tensor / noise 0.44 (position_embeddings); negative control: whole 8.6e-4, tensor / noise up to 1.8
    (layer 0 q_proj).  Also against the fp32 decomposition at grad_check's bf16 gates (relative L2 0.10, cosine 0.997):
    measured whole 6.0e-3, worst tensor 4.7e-2, worst cosine 0.9989 (layer 8 q_proj.weight)."""
    c = training_case
    cfg = c["cfg"]
    lsum, gsum, last = c["b16"][32]
    f_lsum, f_gsum, _ = c["f32"][32]
    _, noise = _distances(cfg, gsum / 32, f_gsum / 32)
    loss, grad = _full_step(c["sd"], c["x"], c["y"], "bf16")
    print(f"bf16 rounding noise of the B = 2 decomposition (vs fp32): largest {_worst(noise, 2)}, smallest "
          f"{', '.join(f'{k} {noise[k]:.2e}' for k in sorted(noise, key=noise.get)[:2])}")
    _decomposition_check("bf16 B = 64", cfg, loss, grad, lsum, gsum, 32, last, 5e-3, BF16_WHOLE,
                         lambda k: BF16_NOISE_RATIO * noise[k])
    whole, per32 = _distances(cfg, grad, f_gsum / 32)
    rv, gv = arena_views(cfg, f_gsum / 32), arena_views(cfg, grad)
    cos = {k: float((gv[k].flatten() @ rv[k].flatten()) / (gv[k].norm() * rv[k].norm())) for k in per32}
    print(f"bf16 B = 64 vs the fp32 decomposition: whole {whole:.3e}, worst tensor {_worst(per32)}, worst cosine "
          f"{min(cos.values()):.5f} ({min(cos, key=cos.get)}); loss {loss:.6f} vs {f_lsum / 32:.6f}")
    bad = [(k, per32[k], cos[k]) for k in per32 if not (per32[k] < BF16_GRAD_REL and cos[k] > BF16_GRAD_COS)]
    assert not bad, bad[:8]


# ---------------------------------------------------------------- 4. Adam / AdamW over whole grid strides
S4 = 4096 * 256   # float4 units one trip of adam_kernel's grid covers (grid_for: at most 4096 blocks of 256 threads)
ARENA = "vitb16_512"
ADAM_N4 = [1, 255, S4 - 1, S4, S4 + 1, 2 * S4 - 1, 2 * S4, 2 * S4 + 1, 3 * S4 + 7, ARENA]


@pytest.mark.parametrize("kind", ["adam", "adamw"])
@pytest.mark.parametrize("n4", ADAM_N4, ids=str)
def test_adam_kernel_over_whole_strides_against_torch(n4, kind):
    """vitseg_adam_step / vitseg_adamw_step through the C ABI against torch.optim.Adam(lr=1e-5) / AdamW(lr=1e-4, weight_decay
    1e-2) (foreach=False) fed g * grad_scale, 5 steps, grad_scale 1 and 1/8, at sizes on either side of one, two and three
    strides of the kernel's grid (each thread does two 16-byte pieces per trip: below one stride the second piece, its clamped
    load and every trip after the first never run) and at the real arena (ViT-B/16 at 512: 88.2 M floats, ~11 trips).  Half
    the gradients are tiny (|g * s| 1e-9 .. 1e-7, sqrt(v) comparable to eps): only there does a misplaced grad_scale move the
    update (elsewhere m / sqrt(v) does not depend on the scale).  p, m, v and g are guard-banded; g must be left unchanged.
    Gates on p: those of test_fused_adam(w)_matches_torch_adam(w), 2e-9 / 1e-7 absolute, with |p| kept below 0.0075 / 0.24 so
    that one ulp of p is at most 4.7e-10 / 1.5e-8 (the kernel multiplies by 1 / sqrt(bc2) where torch divides, so a last
    bit of p flips now and then; over 5 steps and 88 M elements two flips land on one element).  Measured on the MI355X:
    at most 9.3e-10 (Adam) / 3.0e-8 (AdamW), 2.1 / 3.4 x inside.  Gates on the moments, relative L2 over the buffer: m 1e-6,
    v 5e-5.  torch forms 1 - beta from the Python double (fp32 0.1 / 0.001), the kernel subtracts the fp32 beta (0.10000002 /
    0.00099998713) and matches its own bias corrections to it; measured m 2.2e-7, v 1.3e-5 at every size.  A planted defect
    that skips the second piece fails every size above one stride (p off by 3e-5 .. 5e-4)."""
    n = _lib.param_count(ViTSegConfig(2, 16, 768, 12, 12, image_size=512)) if n4 == ARENA else 4 * n4
    adamw = kind == "adamw"
    lr, wd, tol, pscale, pmax = (1e-4, 1e-2, 1e-7, 0.1, 0.24) if adamw else (1e-5, 0.0, 2e-9, 0.0025, 0.0075)
    L = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device=DEV).manual_seed(n % 1000003 + 7 * adamw)
    worst = {}
    for gs in (1.0, 0.125):
        p0 = (torch.randn(n, generator=gen, device=DEV) * pscale).clamp_(-pmax, pmax)
        p = guarded((n,), torch.float32, p0, name="params")
        m = guarded((n,), torch.float32, "zero", name="exp_avg")
        v = guarded((n,), torch.float32, "zero", name="exp_avg_sq")
        g = guarded((n,), torch.float32, "zero", name="grads")
        ref = torch.nn.Parameter(p0.clone())
        opt = (torch.optim.AdamW([ref], lr=lr, weight_decay=wd, foreach=False) if adamw else
               torch.optim.Adam([ref], lr=lr, foreach=False))
        err = 0.0
        for step in range(1, 6):
            tiny = torch.rand(n, generator=gen, device=DEV) < 0.5
            mag = torch.where(tiny, 10.0 ** (-9.0 + 2.0 * torch.rand(n, generator=gen, device=DEV)),
                              torch.randn(n, generator=gen, device=DEV).abs() * 10.0 ** (1 - step))
            sign = torch.where(torch.rand(n, generator=gen, device=DEV) < 0.5, -1.0, 1.0)
            g.copy_(sign * mag / gs)                                  # g * gs is the designed gradient (gs a power of 2)
            snap = snapshot(g)
            if adamw:
                _lib.check(L.vitseg_adamw_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, lr, 0.9, 0.999,
                                               1e-8, wd, step, gs, stream))
            else:
                _lib.check(L.vitseg_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, lr, 0.9, 0.999,
                                              1e-8, step, gs, stream))
            ref.grad = g * gs
            opt.step()
            torch.cuda.synchronize()
            unchanged(snap)
            err = max(err, (p - ref.detach()).abs().max().item())
        st = opt.state[ref]
        em = float((m - st["exp_avg"]).norm() / st["exp_avg"].norm())
        ev = float((v - st["exp_avg_sq"]).norm() / st["exp_avg_sq"].norm())
        worst[gs] = (err, em, ev, int((p != ref.detach()).sum()))
        check(p, m, v, g)
        del p, m, v, g, ref, opt, st
    print(f"{kind} n = {n} ({n4} float4): " + "; ".join(
        f"grad_scale {gs}: max |p - torch| {e:.2e} (gate {tol:.0e}, {nd} elements differ), m rel L2 {em:.1e}, v rel L2 {ev:.1e}"
        for gs, (e, em, ev, nd) in worst.items()))
    for gs, (e, em, ev, _) in worst.items():
        assert e < tol, (gs, e)
        assert em < 1e-6 and ev < 5e-5, (gs, em, ev)
    torch.cuda.empty_cache()
