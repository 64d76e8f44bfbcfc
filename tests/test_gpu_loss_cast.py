"""GPU (-m gpu): the fused cross-entropy kernel (vitseg_ce_loss) against an fp64 reference, and the parameter-arena casts
(vitseg_cast_params_bf16 / _f16 / _split) bit for bit against torch's CPU conversions.  Every buffer is guard-banded."""
import pytest
import torch
import torch.nn.functional as F

from guard import check, guarded, snapshot, unchanged
from visiontransformer_amd import _lib, synth
from visiontransformer_amd.model import ViTSegmentationModel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -23   # fp32 unit roundoff (half an ulp of 1)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ce_ref(z, target, S):
    """fp64 loss and d loss / d logits of F.cross_entropy on the bilinearly upsampled logits."""
    z64 = z.double().requires_grad_(True)
    up = F.interpolate(z64, (S, S), mode="bilinear", align_corners=False)
    up.retain_grad()
    loss = F.cross_entropy(up, target.long())
    loss.backward()
    lse = torch.logsumexp(up.detach(), dim=1)
    return loss.detach(), up.grad, lse, up.detach()


def _ce_run(z, target, C, g, S, want_grad=True):
    """One vitseg_ce_loss call with guarded inputs, gradient, loss and scratch (exactly vitseg_ce_scratch_bytes)."""
    B = z.shape[0]
    L = _lib.lib()
    zd = guarded(z.shape, torch.float32, z, name="lowres")
    td = guarded(target.shape, target.dtype, target, name="target")
    gd = guarded((B, C, S, S), torch.float32, "nan", name="grad_logits") if want_grad else None
    scratch = guarded(L.vitseg_ce_scratch_bytes(B, S), torch.uint8, "nan", name="ce scratch")
    loss = guarded((1,), torch.float32, "nan", name="loss")
    snap = snapshot(zd, td)
    _lib.check(L.vitseg_ce_loss(zd.data_ptr(), td.data_ptr(), int(target.dtype == torch.uint8),
                                gd.data_ptr() if gd is not None else None, scratch.data_ptr(), loss.data_ptr(), B, C, g,
                                S, _stream()))
    torch.cuda.synchronize()
    check(zd, td, gd, scratch, loss)
    unchanged(snap)
    return loss.cpu()[0], (gd.cpu() if gd is not None else None)


def _ce_bounds(up, lse, C, npx):
    """Per-pixel error of the fp32 loss: the re-generated logit (an fmaf chain of 4 products, <= 4 u |z|), the online
    log-sum-exp (m + log(sum), a rounding of |lse| plus a few ulps per exp and the log: <= 4 u |lse| + 4 (C + 2) u) and
    the picked logit.  The mean of per-pixel errors is bounded by their maximum.  The gradient (softmax - onehot) / npx
    carries the exponent error relatively (p <= 1) plus the roundings of the difference and the scale."""
    zmax = up.abs().max().item()
    e_pix = 4 * U * lse.abs().max().item() + 8 * U * zmax + 4 * (C + 2) * U
    return e_pix, (e_pix + 8 * U) / npx


@pytest.mark.parametrize("B,C,g,S,kind", [
    (2, 2, 14, 224, "randn"), (1, 17, 14, 224, "randn"), (2, 32, 32, 512, "randn"), (1, 1, 16, 64, "randn"),
    (2, 5, 7, 28, "randn"), (2, 5, 7, 28, "big"), (2, 17, 14, 224, "big"), (2, 4, 7, 28, "ties"),
    # the training sizes: B * S * S / 256 = 65 536 and 32 768 partial sums, where ce_finish_kernel's four-chain loop runs
    # (it needs more than 4 096; the largest case above makes 2 048)
    (64, 2, 32, 512, "randn"), (32, 17, 32, 512, "randn")])
def test_ce_loss_against_fp64(B, C, g, S, kind):
    gen = torch.Generator().manual_seed(B * 1000 + C * 10 + g)
    z = torch.randn(B, C, g, g, generator=gen).float() * 3.0
    if kind == "big":   # logits at +-60: exp of the raw values would overflow without the running max
        z = (torch.rand(B, C, g, g, generator=gen) * 120.0 - 60.0).float()
    elif kind == "ties":   # exact ties between classes: the first two equal everywhere, all four equal in image 0
        z[:, 1] = z[:, 0]
        z[0] = z[0, :1].expand(C, g, g)
    t64 = torch.randint(0, C, (B, S, S), generator=gen)
    loss_ref, grad_ref, lse, up = _ce_ref(z, t64, S)
    npx = B * S * S
    e_pix, g_bound = _ce_bounds(up, lse, C, npx)

    loss8, grad8 = _ce_run(z, t64.to(torch.uint8), C, g, S)
    loss64, grad64 = _ce_run(z, t64, C, g, S)
    loss_again, grad_again = _ce_run(z, t64, C, g, S)
    # uint8 and int64 targets, and a second call: bitwise the same
    assert torch.equal(loss8.view(torch.int32), loss64.view(torch.int32))
    assert torch.equal(grad8.view(torch.int32), grad64.view(torch.int32))
    assert torch.equal(loss_again.view(torch.int32), loss64.view(torch.int32))
    assert torch.equal(grad_again.view(torch.int32), grad64.view(torch.int32))

    assert torch.isfinite(grad64).all()
    # the loss without the gradient output is the same value
    loss_nog, _ = _ce_run(z, t64, C, g, S, want_grad=False)
    assert torch.equal(loss_nog.view(torch.int32), loss64.view(torch.int32))
    if C == 1:   # one class: log-sum-exp of one value minus itself, softmax 1 - onehot 1
        assert float(loss64) == 0.0 and (grad64 == 0).all()
        return
    err = abs(float(loss64) - float(loss_ref))
    bound = e_pix + 2 * U * abs(float(loss_ref))   # (+ the fp32 rounding of the fp64 mean)
    assert err < bound, (err, bound)
    gerr = (grad64.double() - grad_ref).abs().max().item()
    print(f"ce loss err {err:.2e} (bound {bound:.2e}), grad err {gerr:.2e} (bound {g_bound:.2e})")
    assert gerr < g_bound, (gerr, g_bound)


@pytest.mark.parametrize("dtype,bad", [(torch.uint8, 255), (torch.int64, -100), (torch.int64, 5), (torch.uint8, 5)])
def test_ce_loss_invalid_label_is_nan(dtype, bad):
    """A label outside [0, C) is not scored as a plausible number: the loss is NaN, and so is the gradient at that pixel
    (every class), while every other pixel's gradient is the valid one."""
    B, C, g, S = 2, 5, 7, 28
    gen = torch.Generator().manual_seed(17)
    z = torch.randn(B, C, g, g, generator=gen).float()
    t = torch.randint(0, C, (B, S, S), generator=gen)
    _, grad_ok = _ce_run(z, t.to(dtype), C, g, S)
    t[1, 5, 9] = bad
    loss, grad = _ce_run(z, t.to(dtype), C, g, S)
    assert torch.isnan(loss)
    assert torch.isnan(grad[1, :, 5, 9]).all()
    keep = torch.ones(B, S, S, dtype=torch.bool)
    keep[1, 5, 9] = False
    assert torch.equal(grad.permute(1, 0, 2, 3)[:, keep], grad_ok.permute(1, 0, 2, 3)[:, keep])


def test_backward_fused_loss_with_invalid_label_is_nan():
    """The same contract through vitseg_backward's fused loss: the loss is NaN, and the NaN gradient of that pixel reaches the
    parameter gradients (the seg head's last bias sums d loss / d logits over every pixel); with a valid label there, all
    finite."""
    C, P, D, S = 3, 16, 64, 64
    m = ViTSegmentationModel(C, P, D, 1, 1, image_size=S, intermediate_size=128, device=DEV)
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(m.cfg, seed=4).items()}
    m.load_state_dict(sd)
    m.train()
    x = torch.from_numpy(synth.make_images(m.cfg, 1, seed=4)).to(DEV)
    off, n = _lib.param_offset(m.cfg, _lib.T_HEAD2_B)
    t = torch.zeros(1, S, S, dtype=torch.uint8, device=DEV)
    m._forward_train(x, False)
    grads, loss = m._backward(x, target=t)
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and torch.isfinite(grads).all()
    m._release_grad_buffer(grads)
    t[0, 3, 3] = 255
    m._forward_train(x, False)
    grads, loss = m._backward(x, target=t)
    torch.cuda.synchronize()
    assert torch.isnan(loss)
    assert torch.isnan(grads[off:off + n]).all()
    m._release_grad_buffer(grads)


# ------------------------------------------------------------------ arena casts
GRID_STRIDE = 2048 * 256 * 4   # floats one pass of the cast kernels' grid covers (2048 blocks x 256 threads x 4)
N_CAST = GRID_STRIDE + 4       # the grid-stride loop runs twice; the second pass covers one 4-value group


def _cast_inputs():
    gen = torch.Generator().manual_seed(5)
    scales = torch.tensor([1e-30, 1e-8, 1e-3, 1.0, 3e2, 6e4, 1e6], dtype=torch.float32)
    x = torch.randn(N_CAST, generator=gen).float() * scales[torch.randint(0, len(scales), (N_CAST,), generator=gen)]
    bits = []
    # bf16 ties (low 16 bits exactly 0x8000) with an even and an odd kept bit, and one ulp either side of a tie
    for hi in (0x3F80, 0x3F81, 0xBF80, 0xBF81, 0x4000, 0x7F7F):
        bits += [(hi << 16) | 0x8000, (hi << 16) | 0x7FFF, (hi << 16) | 0x8001]
    # fp16 ties: 1 + 2^-11 (even kept bit: down), 1 + 3 * 2^-11 (odd: up), and their negatives
    bits += [0x3F801000, 0x3F803000, 0xBF801000, 0xBF803000, 0x3F801001, 0x3F802FFF]
    # +-0, fp32 subnormals, the smallest normal, +-inf, NaNs
    bits += [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00400000, 0x007FFFFF, 0x00800000, 0x80800000,
             0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001]
    special = torch.tensor(bits, dtype=torch.int64).to(torch.int32).view(torch.float32)
    vals = torch.tensor([
        65504.0, -65504.0, 65519.0, 65520.0, -65520.0, 7e4, -1e6, 3.4e38,      # fp16 max, its rounding edge, beyond
        6.1e-5, 2 ** -14, 2 ** -15, 2 ** -24, 2 ** -25, 1.5 * 2 ** -25, 2 ** -26, 3e-6, -3e-6, 1e-7, -5.96e-8,  # fp16 subnormals
        1e-40, -1e-42,                                                          # fp32 subnormals again, by value
    ], dtype=torch.float32)
    special = torch.cat([special, vals])
    x[:len(special)] = special
    x[-len(special):] = special            # and in the second pass of the grid-stride loop
    x[GRID_STRIDE - 8:GRID_STRIDE] = special[:8]
    return x


def _same_bits(got, ref, name):
    """bitwise equal as 16-bit patterns; NaN positions compared by NaN-ness only."""
    gn, rn = torch.isnan(got.float()), torch.isnan(ref.float())
    assert torch.equal(gn, rn), f"{name}: NaN-ness differs at {int((gn != rn).sum())} elements"
    gb, rb = got.view(torch.int16)[~gn], ref.view(torch.int16)[~rn]
    bad = (gb != rb).nonzero().flatten()
    if bad.numel():
        xs = _cast_inputs()[~rn][bad[:8]]
        raise AssertionError(f"{name}: {bad.numel()} elements differ; first inputs {xs.tolist()} "
                             f"got {gb[bad[:8]].tolist()} expected {rb[bad[:8]].tolist()}")


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_cast_params_16bit_bit_exact(kind):
    """vitseg_cast_params_bf16 / _f16 are torch's round-to-nearest-even conversions, bit for bit: ties to even, fp32
    subnormals kept, fp16 subnormal results, overflow to +-inf at 65520, NaN stays NaN."""
    L = _lib.lib()
    dt = torch.bfloat16 if kind == "bf16" else torch.float16
    cast = L.vitseg_cast_params_bf16 if kind == "bf16" else L.vitseg_cast_params_f16
    x = _cast_inputs()
    xd = guarded(x.shape, torch.float32, x, name="params")
    dst = guarded(x.shape, dt, "nan", name=f"params_{kind}")
    snap = snapshot(xd)
    _lib.check(cast(xd.data_ptr(), dst.data_ptr(), N_CAST, _stream()))
    torch.cuda.synchronize()
    check(xd, dst)
    unchanged(snap)
    _same_bits(dst.cpu(), x.to(dt), kind)
    # n % 4 != 0 is refused and writes nothing
    before = dst.clone()
    assert cast(xd.data_ptr(), dst.data_ptr(), N_CAST - 2, _stream()) == _lib.EINVAL
    torch.cuda.synchronize()
    assert torch.equal(dst.view(torch.int16), before.view(torch.int16))
    check(dst)


def test_cast_params_split_bit_exact():
    """vitseg_cast_params_split: per 4 values, 4 hi halves | 4 scaled lo halves with hi = x.half() and
    lo = ((x - hi) * 2048).half(), bit for bit; hi + lo 2^-11 gives x to the ~2^-21 relative precision the fp32x3 GEMM
    (test_linear_f32x3_is_fp32_grade) assumes."""
    L = _lib.lib()
    x = _cast_inputs()
    xd = guarded(x.shape, torch.float32, x, name="params")
    dst = guarded(x.shape, torch.float32, "nan", name="params_split")
    snap = snapshot(xd)
    _lib.check(L.vitseg_cast_params_split(xd.data_ptr(), dst.data_ptr(), N_CAST, _stream()))
    torch.cuda.synchronize()
    check(xd, dst)
    unchanged(snap)
    halves = dst.cpu().view(torch.float16).reshape(-1, 8)
    hi, lo = halves[:, :4].reshape(-1), halves[:, 4:].reshape(-1)
    hi_ref = x.to(torch.float16)
    lo_ref = ((x - hi_ref.float()) * 2048.0).to(torch.float16)
    _same_bits(hi, hi_ref, "split hi")
    _same_bits(lo, lo_ref, "split lo")
    inr = torch.isfinite(x) & (x.abs() <= 65504.0)
    rec = hi[inr].double() + lo[inr].double() * 2.0 ** -11
    err = (rec - x[inr].double()).abs()
    assert (err <= 2.0 ** -21 * x[inr].double().abs() + 2.0 ** -35).all(), err.max().item()
    assert L.vitseg_cast_params_split(xd.data_ptr(), dst.data_ptr(), N_CAST - 1, _stream()) == _lib.EINVAL
    torch.cuda.synchronize()
    check(dst)
