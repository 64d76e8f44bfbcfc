"""GPU (-m gpu): every LayerNorm entry point on inputs in which eps, the row mean and the row scale count
(tests/layernorm_cases.py: the designs, the fp64 reference and the derivation of every gate; tests/test_layernorm_cases_cpu.py:
proof on the CPU that a plain fp32 model stays within a quarter of the gates and that every single fault of its list is at
least 8 gates away).  Every comparison is against that fp64 reference, never against another kernel; every buffer is
guard-banded and every output poisoned (tests/guard.py).  One RATIO line per case: the worst |got - ref| / gate per output.

A test is one (entry, design, D); inside it run the rows 1, 5, 67, 261, eps 1e-12, 1e-6, 1e-5 and, for the backward entries, their
modes (branch output or none, p = 0 / 0.25, one gradient slab or three).

Measured on an MI355X, worst |got - ref| / gate per entry point and design over all shapes, eps and modes (270 tests, 6768 cases):
    entry                      design      y / out   dw     db     br     brsum  brsum_own
    layernorm_f32              offset      0.089
    (linear_resln_f32_small:   eps         0.105             (resln: X_out == x bit for bit, H the same bits from all six
     the same four figures)    exact       0 (y == b)         tile variants)
                               outlier     0.158
    layernorm_h16[bf16]        offset / eps / outlier  0.995 / 0.995 / 0.996, exact 0      (the rounding to 16 bits is the gate's u16 |ref|:
    layernorm_h16[fp16]        offset / eps / outlier  0.992 / 0.993 / 0.999, exact 0       up to 1.0 by right, as in the CPU model)
    layernorm_bwd_f32          offset      0.089     0.058  0.091
    (layernorm_bwd_f32_small:  eps         0.024     0.028  0.090
     the same figures)         exact       0.010     0      0
                               outlier     0.097     0.077  0.090
                               null        0.027     0.054  0.100
                               heavy_row   0.034     0.054  0.141
    layernorm_bwd_f32_small    offset                              0.123  0.038  0.102
                               eps                                 0.025  0.021  0.114
                               exact                               0.013  0.014  0.099
                               outlier                             0.132  0.092  0.101
                               null                                0.035  0.011  0.103
                               heavy_row                           0.052  0.025  0.119
    layernorm_bwd_bf16         offset      0.086     0.057  0.001  0.996  0.983  0.022
                               eps         0.024     0.029  0.001  0.993  0.988  0.028
                               exact       0.010     0      0      0.953  0.953  0.082
                               outlier     0.096     0.076  0.001  0.996  0.992  0.002
                               null        0.028     0.050  0.033  0.995  0.986  0.016
                               heavy_row   0.038     0.053  0.050  0.995  0.991  0.042
No gate was widened after the kernels ran.  Whole model at eps = 100 (tests below), error / gate: logits fp32 small 4.6e-7, large
1.0e-6, fp32x3 4.4e-7 / 2e-5; bf16 2.1e-3, 4.6e-3 / 3e-2; fp16 1.9e-4, 4.5e-4 / 2e-3; loss fp32 4.0e-8 / 2e-6, bf16 2.6e-5 / 5e-3;
worst per-tensor gradient fp32 1.5e-6 (small), 2.0e-6 (large) / 2e-4, bf16 3.0e-2 / 0.10.
"""
import pytest
import torch

import layernorm_cases as LC
from guard import check, guarded, snapshot, unchanged
from visiontransformer_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P_DROP = 0.25
NVARIANTS = 5   # tile variants of the small route's GEMM (tests/test_gpu_small.py)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(t, dtype=None, name=None):
    return guarded(tuple(t.shape), dtype or t.dtype, t, device=DEV, name=name)


def _out(shape, dtype=torch.float32, name=None):
    return guarded(shape, dtype, "nan", device=DEV, name=name)


def _after(snap, *outs):
    torch.cuda.synchronize()
    check(*[t for t, _ in snap], *[o for o in outs if o is not None])
    unchanged(snap)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _cpu(t):
    return None if t is None else t.float().cpu()


DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
FORWARD = {"layernorm_f32": "fp32", "layernorm_h16[bf16]": "bf16", "layernorm_h16[fp16]": "fp16", "linear_resln_f32_small": "fp32"}


def _layernorm(entry, c, eps):
    fmt = FORWARD[entry]
    x, w, b = _dev(c.x, name="x"), _dev(c.w, name="w"), _dev(c.b, name="b")
    y = _out((c.rows, c.D), DT[fmt], name="y")
    snap = snapshot(x, w, b)
    L = _lib.lib()
    if fmt == "fp32":
        _lib.check(L.vitseg_op_layernorm_f32(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), c.rows, c.D, eps, _stream()))
    else:
        _lib.check(_lib.symbol("vitseg_op_layernorm_h16")(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), c.rows, c.D, eps,
                                                          1 if fmt == "bf16" else 2, _stream()))
    _after(snap, y)
    return _cpu(y)


def _resln(c, eps):
    """X += A W^T + bias, H = LayerNorm(X), fed so that the sum is the designed row exactly: X = x / 2, A = [x / 2 | random],
    W = [I | 0], bias = 0 (every product is x / 2 or 0, every partial sum exact in any chunking).  X_out == x bit for bit; H
    from every tile variant is the same bits."""
    M, N = c.rows, c.D
    K = (N + 31) // 32 * 32 + 32
    gen = torch.Generator().manual_seed(N + M)
    A = torch.randn(M, K, generator=gen)
    A[:, :N] = c.x * 0.5
    W = torch.zeros(N, K)
    W[torch.arange(N), torch.arange(N)] = 1.0
    L = _lib.lib()
    S = L.vitseg_small_splits(N, K)
    Ad, Wd, bias = _dev(A, name="A"), _dev(W, name="W"), _dev(torch.zeros(N), name="bias")
    lnw, lnb = _dev(c.w, name="lnw"), _dev(c.b, name="lnb")
    first = None
    for v in range(NVARIANTS + 1):
        X, H = _dev(c.x * 0.5, name="X"), _out((M, N), name="H")
        scratch = _out((S * M * N,), name="resln scratch")
        snap = snapshot(Ad, Wd, bias, lnw, lnb)
        with _lib.option("small_variant", v):
            _lib.check(L.vitseg_op_linear_resln_f32_small(Ad.data_ptr(), Wd.data_ptr(), bias.data_ptr(), X.data_ptr(), lnw.data_ptr(),
                                                          lnb.data_ptr(), H.data_ptr(), scratch.data_ptr(), scratch.numel(), M, N, K,
                                                          eps, _stream()))
        _after(snap, X, H, scratch)
        assert torch.equal(X.cpu(), c.x), ("X_out is not the designed row", v)
        if first is None:
            first = H.cpu()
        else:
            assert torch.equal(H.cpu(), first), ("tile variant", v)
    return first


@pytest.mark.parametrize("D", LC.D_FWD)
@pytest.mark.parametrize("design", LC.DESIGNS_FWD)
@pytest.mark.parametrize("entry", list(FORWARD))
def test_forward(entry, design, D):
    """y within its gate of the fp64 reference (exact design: y == b, rounded once for a 16-bit output, bit for bit)"""
    fmt, bad = FORWARD[entry], []
    for rows in LC.ROWS:
        for eps in LC.EPS:
            c, ref = LC.make_case(design, rows, D, eps), LC.reference(design, rows, D, eps)
            y = _resln(c, eps) if entry == "linear_resln_f32_small" else _layernorm(entry, c, eps)
            ratio = LC.worst_ratio(y, ref.y16[fmt] if design == "exact" else ref.y, ref.gate_y(fmt))
            print(f"RATIO {entry} {design} rows{rows}-D{D}-eps{eps:g} y {ratio:.3f}")
            if not ratio <= 1.0:
                bad.append((rows, eps, ratio))
    assert not bad, bad


# entry -> modes (branch output, dropout p, gradient slabs)
BACKWARD = {
    "layernorm_bwd_f32": [(False, 0.0, 1)],
    "layernorm_bwd_bf16": [(False, 0.0, 1), (True, 0.0, 1), (True, P_DROP, 1)],
    "layernorm_bwd_f32_small": [(br, p, s) for s in (1, 3) for br, p in ((False, 0.0), (True, 0.0), (True, P_DROP))],
}


def _backward(entry, c, eps, br, p, splits):
    """one call; out, dw, db, br_out (None where the entry writes none), br_dbias (None without the branch output) on the CPU"""
    R, D = c.rows, c.D
    g16 = entry == "layernorm_bwd_bf16"
    x, w, dres = _dev(c.x, name="x"), _dev(c.w, name="w"), _dev(c.dres, name="dres")
    if splits == 1:
        g = _dev(c.g, torch.bfloat16 if g16 else torch.float32, name="g")
    else:   # row r's gradient sits in slab r mod splits, the other slabs hold 0: a lost slab is a lost row
        slabs = torch.zeros(splits, R, D)
        r = torch.arange(R)
        slabs[r % splits, r] = c.g
        g = _dev(slabs, name="g slabs")
    L = _lib.lib()
    scratch = _out((L.vitseg_op_layernorm_bwd_scratch_floats(R, D),), name="layernorm_bwd scratch")
    out, dw, db = _out((R, D), name="dres_out"), _out((D,), name="dw"), _out((D,), name="db")
    br_out = br_dbias = None
    if br:
        br_dbias = _out((D,), name="br_dbias")
        if g16 or p:
            br_out = _out((R, D), torch.bfloat16 if g16 else torch.float32, name="br_out")
    snap = snapshot(x, w, dres, g)
    if entry == "layernorm_bwd_f32":
        _lib.check(L.vitseg_op_layernorm_bwd_f32(x.data_ptr(), w.data_ptr(), g.data_ptr(), dres.data_ptr(), out.data_ptr(), dw.data_ptr(),
                                                 db.data_ptr(), scratch.data_ptr(), R, D, eps, _stream()))
    elif g16:
        _lib.check(_lib.symbol("vitseg_op_layernorm_bwd_bf16")(
            x.data_ptr(), w.data_ptr(), g.data_ptr(), dres.data_ptr(), out.data_ptr(), dw.data_ptr(), db.data_ptr(), scratch.data_ptr(),
            R, D, eps, _ptr(br_out), _ptr(br_dbias), p, LC.DROP_SEED, LC.STREAM_ID, _stream()))
    else:
        _lib.check(L.vitseg_op_layernorm_bwd_f32_small(
            x.data_ptr(), w.data_ptr(), g.data_ptr(), R * D, splits, dres.data_ptr(), out.data_ptr(), dw.data_ptr(), db.data_ptr(),
            scratch.data_ptr(), R, D, eps, _ptr(br_out), _ptr(br_dbias), p, LC.DROP_SEED, LC.STREAM_ID, _stream()))
    _after(snap, out, dw, db, scratch, br_out, br_dbias)
    return _cpu(out), _cpu(dw), _cpu(db), _cpu(br_out), _cpu(br_dbias)


@pytest.mark.parametrize("D", LC.D_BWD)
@pytest.mark.parametrize("design", LC.DESIGNS_BWD)
@pytest.mark.parametrize("entry", list(BACKWARD))
def test_backward(entry, design, D):
    """dres_out, dw, db, the branch output and its column sums within their gates of the fp64 reference (which takes the
    kernels' own dropout mask, tests/dropout_ref.py); the column sums besides within KC rows u sum |br| of the fp64 sum of the
    branch values the kernel wrote itself (the bf16 form sums the rounded values)."""
    g16 = entry == "layernorm_bwd_bf16"
    fmt, bad = ("bf16" if g16 else "fp32"), []
    for br, p, splits in BACKWARD[entry]:
        mode = ("br" if br else "nobr") + f"-p{p:g}-s{splits}"
        for rows in LC.ROWS:
            for eps in LC.EPS:
                c, ref = LC.make_case(design, rows, D, eps), LC.reference(design, rows, D, eps, p, g16)
                out, dw, db, br_out, br_dbias = _backward(entry, c, eps, br, p, splits)
                r = {"out": LC.worst_ratio(out, ref.out, ref.gate_out), "dw": LC.worst_ratio(dw, ref.dw, ref.gate_dw),
                     "db": LC.worst_ratio(db, ref.db, ref.gate_db)}
                if br:
                    own = out if br_out is None else br_out     # (the small form at p = 0 writes no br_out: the branch takes dres_out)
                    if br_out is not None:
                        r["br"] = LC.worst_ratio(br_out, ref.br, ref.gate_br(fmt))
                    r["brsum"] = LC.worst_ratio(br_dbias, ref.brsum, ref.gate_brsum(fmt))
                    r["brsum_own"] = LC.worst_ratio(br_dbias, own.double().sum(0), LC.own_sum_gate(own))
                print(f"RATIO {entry}[{mode}] {design} rows{rows}-D{D}-eps{eps:g} " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
                bad += [(mode, rows, eps, k, v) for k, v in r.items() if not v <= 1.0]
    assert not bad, bad


# ---------------------------------------------------------------- layer_norm_eps through the whole model
PREC = {"fp32": _lib.F32, "bf16": _lib.BF16, "fp16": _lib.F16, "fp32x3": _lib.F32X3}


@pytest.fixture(scope="module")
def eps_model():
    """the whole-model case of tests/layernorm_cases.py and its fp64 oracle results at eps = MODEL_EPS, computed once"""
    import test_gpu_config_sweep as sweep
    from util import BF16_GRAD_REL
    assert LC.MODEL_TOL == sweep.TOL and LC.MODEL_LOSS_TOL == sweep.LOSS_TOL and LC.MODEL_GRAD_REL["bf16"] == BF16_GRAD_REL
    torch.set_num_threads(16)
    cfg, sd, x, y = LC.whole_model()
    return (cfg, sd, x, y) + LC.oracle_step(cfg, sd, x, y)


def _eps_net(cfg, sd, precision):
    from visiontransformer_amd.model import ViTSegmentationModel
    m = ViTSegmentationModel(cfg.num_classes, cfg.patch_size, cfg.hidden_size, cfg.num_hidden_layers, cfg.num_attention_heads,
                             image_size=cfg.image_size, intermediate_size=cfg.intermediate_size, precision=precision, dropout=0.0,
                             layer_norm_eps=cfg.layer_norm_eps, device=DEV)
    assert m.cfg == cfg
    m.load_state_dict(sd)
    return m


@pytest.mark.parametrize("precision,route", [("fp32", "small"), ("fp32", "large"), ("fp32x3", "large"), ("bf16", "small"),
                                             ("bf16", "large"), ("fp16", "small"), ("fp16", "large")])
def test_whole_model_forward_at_an_eps_that_matters(eps_model, precision, route):
    """logits against the oracle at eps = MODEL_EPS within the gate of tests/test_gpu_config_sweep.py; a 1e-12 at any one
    LayerNorm site would be 8 gates or more away (tests/test_layernorm_cases_cpu.py)"""
    cfg, sd, x, y, logits, loss, leaf, stages = eps_model
    B = LC.MODEL_CFG[7]
    m = _eps_net(cfg, sd, precision).eval()
    with _lib.option("no_small", int(route == "large")):
        assert _lib.forward_route(cfg, B, PREC[precision]) == route
        with torch.no_grad():
            got = m(x.to(DEV))
    torch.cuda.synchronize()
    err = float((got.cpu().double() - logits).abs().max())
    print(f"RATIO whole_model_forward {precision} {route}: logits max-abs error {err:.3e} gate {LC.MODEL_TOL[precision]:.0e} "
          f"ratio {err / LC.MODEL_TOL[precision]:.3f}")
    assert err < LC.MODEL_TOL[precision], err


@pytest.mark.parametrize("precision,route", [("fp32", "small"), ("fp32", "large"), ("bf16", "single")])
def test_whole_model_training_step_at_an_eps_that_matters(eps_model, precision, route):
    """loss and every tensor's gradient against fp64 autograd of the oracle at eps = MODEL_EPS (LOSS_TOL, grad_check)"""
    from util import grad_check
    cfg, sd, x, y, logits, loss, leaf, stages = eps_model
    B = LC.MODEL_CFG[7]
    m = _eps_net(cfg, sd, precision).train()
    with _lib.option("no_small", int(route == "large")):
        if precision == "fp32":
            assert _lib.forward_route(cfg, B, _lib.F32) == route
        got = m.ce_loss(x.to(DEV), y.to(DEV))
        got.backward()
    torch.cuda.synchronize()
    lerr = abs(float(got.detach()) - float(loss))
    worst, whole = grad_check(cfg, m.arena.grad, leaf, precision, stages)
    print(f"RATIO whole_model_training {precision} {route}: loss error {lerr:.3e} gate {LC.MODEL_LOSS_TOL[precision]:.0e}, "
          f"worst per-tensor gradient relative L2 {worst:.3e} gate {LC.MODEL_GRAD_REL[precision]:.0e}")
    assert lerr < LC.MODEL_LOSS_TOL[precision], lerr
