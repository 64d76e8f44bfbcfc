"""GPU (-m gpu): the whole model against the fp64 oracle at the corners of the accepted config domain.

`check_config` (csrc/plan.hpp) accepts any patch size that is a multiple of 4, S = P (a 1 x 1 token grid), any I that is a
multiple of 4 (also I <= D), up to 255 classes and D up to 2048.  The forward and training drivers pick kernels by shape
predicates; each row of CASES exists for a branch no golden or grid test reaches, with the arithmetic that puts it there.
Every case runs the forward in fp32 on both routes, fp32x3, bf16 and fp16 (16-bit on both routes where the small one
applies), and the training step in fp32 on both routes and in bf16, against `oracle.vitseg_oracle` in fp64 with the gates
of test_reference_configuration_grid / test_training_step_vitb_width_512.  A config the build cannot run must be refused up
front with ValueError (ESHAPE): 16-bit precisions need I % 64 == 0, training C <= 32 and D <= 1024 (include/vitseg.h).

The second half holds the dispatcher switches (`vitseg_set_option`, `VITSEG_*` in the environment) to the function of the
default path, at shapes where each switch changes the kernel that runs."""
import ctypes as C

import pytest
import torch

from guard import check, guarded, snapshot, unchanged
from oracle import vitseg_oracle as O
from util import grad_check
from visiontransformer_amd import _lib, synth
from visiontransformer_amd.config import ViTSegConfig
from visiontransformer_amd.model import ViTSegmentationModel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PREC = {"fp32": _lib.F32, "bf16": _lib.BF16, "fp16": _lib.F16, "fp32x3": _lib.F32X3}
TOL = {"fp32": 2e-5, "fp32x3": 2e-5, "fp16": 2e-3, "bf16": 3e-2}   # logits max-abs, as test_reference_configuration_grid
LOSS_TOL = {"fp32": 2e-6, "bf16": 5e-3}                             # as test_training_step_vitb_width_512

# (C, P, D, L, A, S, I, B); small: the default route of fp32 / of the 16-bit precisions (None: 16-bit rejected); train:
# whether training is in the domain.  Np = (S / P)^2, Mt = B (Np + 1), Kp = 3 P^2.
CASES = {
    # g = 1: Np = 1, N = 2 tokens; the 3x3 head conv sees 8 padding taps of 9; upsample from a 1 x 1 map; CE at g = 1.
    # S = 16: 4 quads per output row, so no staged block reaches 48 threads -> upsample_kernel<false> (so do S = 4, 24)
    "g1_p16": dict(c=(3, 16, 128, 1, 2, 16, 256, 2), small=("small", "small"), train=True),
    # the smallest image: S = P = 4, Kp = 48 (one float4 per patch row, not a DMA patch), g = 1
    "g1_p4": dict(c=(2, 4, 64, 1, 1, 4, 128, 3), small=("small", "small"), train=True),
    # g = 3: every one of the 9 tokens touches the conv border; two layers
    "g3_p8": dict(c=(2, 8, 64, 2, 1, 24, 128, 2), small=("small", "small"), train=True),
    # P = 12: not in {8, 16, 32}, so the generic A_PATCH gather and im2col; 3 float4 per patch row, Kp = 432 = 27 * 16
    "p12": dict(c=(3, 12, 128, 1, 2, 96, 256, 2), small=("small", "small"), train=True),
    # P = 20: 5 float4 per row, Kp = 1200 (a 16-wide K tail after 37 * 32), S = 100 with S % 8 = 4
    "p20": dict(c=(2, 20, 128, 1, 2, 100, 256, 1), small=("small", "small"), train=True),
    # P = 24: Kp = 1728 = 54 * 32 passes the Kp % 32 test but 24 is not a DMA patch; 6 float4 per row
    "p24": dict(c=(2, 24, 192, 1, 3, 96, 384, 2), small=("small", "small"), train=True),
    # P = 28: 7 float4 per row, Kp = 2352 = 73 * 32 + 16
    "p28": dict(c=(2, 28, 64, 1, 1, 224, 256, 1), small=("small", "small"), train=True),
    # I = 100: I % 32 = 4 rules the small route out at any batch (large route because of I, not no_small); fc1 N = 100 and
    # fc2 K = 100 are ragged against every tile; 16-bit: I % 64 != 0, rejected
    "i100": dict(c=(2, 16, 128, 1, 2, 64, 100, 2), small=("large", None), train=True),
    # I = 224 = 7 * 32: the fp32 small route takes it; 224 % 64 = 32, so the 16-bit precisions are rejected up front
    "i224": dict(c=(2, 16, 128, 1, 2, 64, 224, 2), small=("small", None), train=True),
    # I <= D: the small route needs I > D, so the large one at batch 2
    "i_eq_d": dict(c=(2, 16, 256, 1, 4, 64, 256, 2), small=("large", "large"), train=True),
    "i_lt_d": dict(c=(2, 16, 256, 1, 4, 64, 64, 2), small=("large", "large"), train=True),
    # one class: the mask is 0 everywhere, the CE loss and its gradient are 0
    "c1": dict(c=(1, 16, 64, 1, 1, 64, 256, 2), small=("small", "small"), train=True),
    # 150 classes at S = 512: one band of 4 output rows stages 3 source rows of 32 per class, 150 * 3 * 32 * 4 B = 56 KiB
    # > 48 KiB -> upsample_kernel<false> (forward only: training holds C <= 32); 16-bit: 1025 tokens are not a key-split
    # attention length -> large
    "c150_s512": dict(c=(150, 16, 64, 1, 1, 512, 256, 1), small=("small", "large"), train=False),
    # the most classes (forward only); S = 224 stages 255 * 3 * 14 * 4 B = 42 KiB of source rows, the
    # staged upsample near its 48 KiB limit
    "c255": dict(c=(255, 16, 64, 1, 1, 224, 256, 2), small=("small", "small"), train=False),
    # the widest: D = 2048 = 32 heads (LayerNorm / resln at their limit); training: the LayerNorm backward holds D <= 1024
    "d2048": dict(c=(2, 16, 2048, 1, 32, 32, 2304, 1), small=("small", "small"), train=False),
    # A = 5: 3D = 960 and D = 320 are not multiples of 256, so at Mt = 17 * 197 = 3349 >= 2048 neither gemm_p8 nor
    # gemm_h16p applies and every 16-bit linear runs on the round-1 kernels (16-bit: 3349 rows > 3200 -> large route)
    "a5": dict(c=(2, 16, 320, 1, 5, 224, 1280, 17), small=("small", "large"), train=True),
    # A = 7: Mp = 2 * 256 = 512 rows, a whole number of 256-row tiles, so on the large route the two CLS rows take the
    # thin-row split-K launch with K = D = 448 = 3.5 * 128; bf16 training: Np = 256 has keep-bit words.  16-bit: o_proj's
    # K = 448 splits into 2 chunks of 224 values, not whole 64-value steps -> the large route (small_applies)
    "a7_thin": dict(c=(2, 16, 448, 1, 7, 256, 1792, 2), small=("small", "large"), train=True),
}


def _cfg(name):
    c = CASES[name]["c"]
    return ViTSegConfig(*c[:5], image_size=c[5], intermediate_size=c[6]), c[7]


def _forward_runs():
    out = []
    for name, e in CASES.items():
        s32, s16 = e["small"]
        for precision in ("fp32", "bf16", "fp16"):
            default = s32 if precision == "fp32" else s16
            if default is None:
                out.append((name, precision, "rejected"))
                continue
            out.append((name, precision, "large"))
            if default == "small":
                out.append((name, precision, "small"))
        out.append((name, "fp32x3", "large"))
    return out


def _train_runs():
    out = []
    for name, e in CASES.items():
        s32, s16 = e["small"]
        if not e["train"]:
            out += [(name, "fp32", "rejected"), (name, "bf16", "rejected")]
            continue
        out.append((name, "fp32", "large"))
        if s32 == "small":
            out.append((name, "fp32", "small"))
        out.append((name, "bf16", "rejected" if s16 is None else "single"))
    return out


def _model(cfg, precision, sd, dropout=0.0):
    m = ViTSegmentationModel(cfg.num_classes, cfg.patch_size, cfg.hidden_size, cfg.num_hidden_layers,
                             cfg.num_attention_heads, image_size=cfg.image_size, intermediate_size=cfg.intermediate_size,
                             precision=precision, dropout=dropout, device=DEV)
    m.load_state_dict(sd)
    return m


class _Ref:
    """Inputs and fp64 oracle results of one case, computed once per module (autograd only where training runs)."""

    def __init__(self, name):
        cfg, B = _cfg(name)
        seed = sum(CASES[name]["c"])
        self.cfg, self.B = cfg, B
        self.sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, seed=seed).items()}
        self.x = torch.from_numpy(synth.make_images(cfg, B, seed=seed))
        # (synth's targets are 8 x 8 cells: made at 256 and nearest-resized to S, as the reference's training step does)
        self.y = O.resize_target(torch.from_numpy(synth.make_targets(cfg, B, seed=seed)), (cfg.image_size, cfg.image_size))
        self.stages = {}
        x64 = self.x.double()
        if CASES[name]["train"]:
            self.leaf = {k: v.double().requires_grad_(True) for k, v in self.sd.items()}
            logits = O.forward(x64, self.leaf, cfg, stages=self.stages)
            self.loss = O.ce_loss(logits, self.y)
            self.loss.backward()
            self.logits = logits.detach()
        else:
            with torch.no_grad():
                self.logits = O.forward(x64, {k: v.double() for k, v in self.sd.items()}, cfg)
        self.mask = O.predict_mask(self.logits)
        srt = self.logits.sort(dim=1, descending=True).values
        self.margin = srt[:, 0] - srt[:, 1] if cfg.num_classes > 1 else None


@pytest.fixture(scope="module")
def ref():
    cache = {}

    def get(name):
        if name not in cache:
            torch.set_num_threads(16)
            cache[name] = _Ref(name)
        return cache[name]
    return get


@pytest.mark.parametrize("name,precision,route", _forward_runs(), ids=lambda v: str(v))
def test_forward_matches_fp64_oracle(ref, name, precision, route):
    cfg, B = _cfg(name)
    p = PREC[precision]
    if route == "rejected":
        with pytest.raises(ValueError, match="intermediate_size"):
            _lib.query_workspace(cfg, B, p)
        m = _model(cfg, precision, {k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, seed=1).items()}).eval()
        with pytest.raises(ValueError, match="intermediate_size"), torch.no_grad():
            m.predict_mask(torch.zeros(B, 3, cfg.image_size, cfg.image_size, device=DEV), return_logits=True)
        return
    r = ref(name)
    m = _model(cfg, precision, r.sd).eval()
    with _lib.option("no_small", int(route == "large")):
        assert _lib.forward_route(cfg, B, p) == route
        with torch.no_grad():
            mask, logits = m.predict_mask(r.x.to(DEV), return_logits=True)
    torch.cuda.synchronize()
    tol = TOL[precision]
    err = (logits.cpu().double() - r.logits).abs().max().item()
    print(f"{name} {precision} {route}: logits max-abs error {err:.3e} (gate {tol:.0e})")
    assert err < tol, (name, precision, route, err)
    mask = mask.cpu().long()
    if r.margin is None:
        assert int(mask.max()) == 0
    else:
        solid = r.margin > 4 * tol
        assert bool((mask == r.mask)[solid].all()), (name, precision, route, int((mask != r.mask)[solid].sum()))


@pytest.mark.parametrize("name,precision,route", _train_runs(), ids=lambda v: str(v))
def test_training_step_matches_fp64_autograd(ref, name, precision, route):
    cfg, B = _cfg(name)
    p = PREC[precision]
    if route == "rejected":
        with pytest.raises(ValueError):
            _lib.train_workspace(cfg, B, p)
        m = _model(cfg, precision, {k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, seed=1).items()}).train()
        S = cfg.image_size
        with pytest.raises(ValueError):
            m.ce_loss(torch.zeros(B, 3, S, S, device=DEV), torch.zeros(B, S, S, dtype=torch.int64, device=DEV)).backward()
        return
    r = ref(name)
    m = _model(cfg, precision, r.sd).train()
    with _lib.option("no_small", int(route == "large")):
        if precision == "fp32":
            assert _lib.forward_route(cfg, B, _lib.F32) == route
        loss = m.ce_loss(r.x.to(DEV), r.y.to(DEV))
        loss.backward()
    torch.cuda.synchronize()
    lerr = abs(float(loss.detach()) - float(r.loss))
    worst, whole = grad_check(cfg, m.arena.grad, r.leaf, precision, r.stages)
    print(f"{name} {precision} {route}: loss error {lerr:.3e} (gate {LOSS_TOL[precision]:.0e}), "
          f"worst per-tensor gradient relative L2 {worst:.3e}")
    assert lerr < LOSS_TOL[precision], (name, precision, route, lerr)


@pytest.mark.parametrize("name,precision", [("i224", "bf16"), ("i100", "fp16")])
def test_rejected_forward_leaves_every_buffer_untouched(name, precision):
    """vitseg_forward through the C ABI, everything guard-banded: an I % 64 != 0 config in a 16-bit precision returns
    ESHAPE before any launch -- the NaN-filled logits, the mask and the workspace come back byte for byte as they went in."""
    cfg, B = _cfg(name)
    S = cfg.image_size
    n = _lib.param_count(cfg)
    arena = guarded((n,), torch.float32, torch.randn(n, device=DEV) * 0.02, name="arena")
    shadow = guarded((n,), torch.bfloat16 if precision == "bf16" else torch.float16, "nan", name="shadow arena")
    x = guarded((B, 3, S, S), torch.float32, torch.rand(B, 3, S, S, device=DEV), name="x")
    ws = guarded(_lib.query_workspace(cfg, B, _lib.F32), torch.uint8, "nan", name="workspace")
    logits = guarded((B, cfg.num_classes, S, S), torch.float32, "nan", name="logits")
    mask = guarded((B, S, S), torch.uint8, "nan", name="mask")
    torch.cuda.synchronize()
    snap = snapshot(x, arena, shadow, ws, logits, mask)
    rc = _lib.lib().vitseg_forward(C.byref(_lib.CConfig.from_config(cfg)), arena.data_ptr(), shadow.data_ptr(),
                                   x.data_ptr(), B, PREC[precision], logits.data_ptr(), mask.data_ptr(), ws.data_ptr(),
                                   ws.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == _lib.ESHAPE and b"multiple of 64" in _lib.lib().vitseg_last_error()
    check(x, arena, shadow, ws, logits, mask)
    unchanged(snap)


# ---------------------------------------------------------------- dispatcher switches
# ViT-B layer at batch 11: Mt = 11 * 197 = 2167 >= 2048 rows with 3D = 2304 and D = 768 multiples of 256, so under
# no_small the 16-bit linears take gemm_p8 (fc2, o_proj) and gemm_h16p (QKV, fc1) and the fp32 ones gemm_f32p.
VITB = (2, 16, 768, 1, 12, 224, 3072, 11)


class _Case:
    def __init__(self, c, seed):
        self.cfg = ViTSegConfig(*c[:5], image_size=c[5], intermediate_size=c[6])
        self.B = c[7]
        self.sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(self.cfg, seed=seed).items()}
        self.x = torch.from_numpy(synth.make_images(self.cfg, self.B, seed=seed))
        self._ref = None

    def ref(self):
        if self._ref is None:
            torch.set_num_threads(16)
            with torch.no_grad():
                self._ref = O.forward(self.x.double(), {k: v.double() for k, v in self.sd.items()}, self.cfg)
        return self._ref

    def logits(self, precision, **opts):
        m = _model(self.cfg, precision, self.sd).eval()
        with _lib.option("no_small", 1):
            olds = {k: _lib.get_option(k) for k in opts}
            try:
                for k, v in opts.items():
                    _lib.set_option(k, v)
                with torch.no_grad():
                    out = m(self.x.to(DEV))
                torch.cuda.synchronize()
            finally:
                for k, v in olds.items():
                    _lib.set_option(k, v)
        return out.cpu()


@pytest.fixture(scope="module")
def switch_cases():
    return {"vitb": _Case(VITB, 12), "a5": _Case(CASES["a5"]["c"], 5)}


# gn sets the column-group width of the tile visit order of the round-1 tile kernels (gemm_tile.hip launch_one: the patch and head
# GEMMs of the fp32 large route, every 16-bit linear at a5); f32p_noinl runs gemm_f32p's epilogues at each tile's end instead
# of inline.  Neither changes what any output element sums or in which order: bitwise equal to the default.
@pytest.mark.parametrize("case,precision,opt,value", [
    ("vitb", "fp32", "gn", 1), ("vitb", "fp32", "gn", 3), ("vitb", "fp32", "gn", 8),
    ("a5", "bf16", "gn", 1), ("a5", "bf16", "gn", 2), ("a5", "fp16", "gn", 4), ("a5", "fp32", "gn", 16),
    ("vitb", "fp32", "f32p_noinl", 1),
])
def test_switch_changes_order_not_bits(switch_cases, case, precision, opt, value):
    c = switch_cases[case]
    assert torch.equal(c.logits(precision, **{opt: value}), c.logits(precision))


# no_p8 / no_h16p route the 16-bit linears of the ViT-B layer back to the round-1 / gemm_p8 kernels; bf16_tiles forces the
# round-1 tile shape (1: 128 x 128, 2: 256 x 128, 3: 256 x 256) at a5, where the round-1 kernels run by shape.  Each must
# meet the oracle gate of the default path, and every pair here is also bitwise equal to the default (measured): none of
# these kernels splits K, and each accumulates an output element in fp32 over the same 32 x 32 x 16 MFMA steps in
# ascending K with the same epilogue -- the tile shape and persistence decide which block computes an element, not the
# order of its sum.
ALT = [("vitb", "bf16", "no_p8", 1), ("vitb", "fp16", "no_p8", 1), ("vitb", "bf16", "no_h16p", 1),
       ("vitb", "fp16", "no_h16p", 1), ("a5", "bf16", "bf16_tiles", 1), ("a5", "bf16", "bf16_tiles", 2),
       ("a5", "bf16", "bf16_tiles", 3), ("a5", "fp16", "bf16_tiles", 3)]


@pytest.mark.parametrize("case,precision,opt,value", ALT)
def test_switch_alternate_kernel_meets_the_oracle_gate(switch_cases, case, precision, opt, value):
    c = switch_cases[case]
    alt, base = c.logits(precision, **{opt: value}), c.logits(precision)
    ref = c.ref()
    e_alt, e_base = (alt.double() - ref).abs().max().item(), (base.double() - ref).abs().max().item()
    print(f"{case} {precision} {opt}={value}: error {e_alt:.3e}, default {e_base:.3e}, "
          f"bitwise equal to default: {torch.equal(alt, base)}")
    assert e_base < TOL[precision] and e_alt < TOL[precision], (e_alt, e_base)
    assert torch.equal(alt, base)


def test_no_dropmask_bf16_training_meets_the_same_oracle():
    """bf16 training at a7_thin (Np = 256, a multiple of 128: the attention-dropout keep bits come from precomputed words,
    attention_dropmask.hip) with dropout 0.1, and the same step under no_dropmask (one hash per element).  The keep decisions
    are the same -- tests/test_gpu_backward.py::test_attention_backward_bf16 pins the words against tests/dropout_ref.py --
    but the arithmetic is not: with words the forward kernel rounds the UNSCALED probability to bf16 and applies 1 / (1 - p)
    in the final normalisation (attention_bf16.hip), the hashed path rounds p / (1 - p).  So the two differ in the last bits
    of the 16-bit P (loss 0.6989554 against 0.6989516 here) and bitwise equality is not the contract.  Both must meet the
    bf16 gates against fp64 autograd with the build's masks injected, and each must be closer to that reference than to
    the same step under another seed's masks (a keep decision that differs between the two paths would show there)."""
    from dropout_ref import Masks
    cfg, B = _cfg("a7_thin")
    sd = {k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, seed=7).items()}
    x = torch.from_numpy(synth.make_images(cfg, B, seed=7))
    y = O.resize_target(torch.from_numpy(synth.make_targets(cfg, B, seed=7)), (cfg.image_size, cfg.image_size))
    torch.set_num_threads(16)

    def oracle(seed64):
        leaf = {k: v.double().requires_grad_(True) for k, v in sd.items()}
        masks = Masks(0.1, seed64, B, cfg.num_patches, cfg.num_attention_heads)
        loss = O.ce_loss(O.forward(x.double(), leaf, cfg, drop=masks), y)
        loss.backward()
        return float(loss), leaf

    def flat(g, keys):
        return torch.cat([g[k].detach().cpu().double().flatten() for k in keys])

    from visiontransformer_amd.params import arena_views
    runs = {}
    for flag in (0, 1):
        m = _model(cfg, "bf16", sd, dropout=0.1).train()
        with _lib.option("no_dropmask", flag):
            loss = m.ce_loss(x.to(DEV), y.to(DEV))
            loss.backward()
        torch.cuda.synchronize()
        runs[flag] = (float(loss.detach()), m.arena.grad.detach().clone(), arena_views(cfg, m.arena.grad.detach().cpu()))
    seed64 = (m.dropout_seed * 0x9E3779B97F4A7C15 + 1 * 0x100000001B3 + 0) & (2 ** 64 - 1)   # first training forward
    ref_loss, leaf = oracle(seed64)
    _, other = oracle(seed64 ^ 0x5A5A5A5A)
    keys = sorted(k for k, v in leaf.items() if v.grad is not None and "pooler" not in k)
    right = flat({k: leaf[k].grad for k in keys}, keys)
    wrong = flat({k: other[k].grad for k in keys}, keys)
    for flag, (loss, grad, views) in runs.items():
        assert abs(loss - ref_loss) < LOSS_TOL["bf16"], (flag, loss, ref_loss)
        grad_check(cfg, grad, leaf, "bf16")
        g = flat(views, keys)
        d_right, d_wrong = float((g - right).norm() / right.norm()), float((g - wrong).norm() / wrong.norm())
        print(f"no_dropmask={flag}: loss {loss:.7f} (fp64 {ref_loss:.7f}); whole gradient vs the right masks {d_right:.3e}, "
              f"vs another seed's {d_wrong:.3e}")
        assert d_right < d_wrong, (flag, d_right, d_wrong)
    d = float((flat(runs[0][2], keys) - flat(runs[1][2], keys)).norm() / right.norm())
    print(f"words against hash: whole-gradient relative L2 {d:.3e}")
