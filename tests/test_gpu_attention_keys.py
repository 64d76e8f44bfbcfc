"""GPU (-m gpu): the attention kernels on inputs in which every single key, query and probed dropout bit carries O(1) of a
compared output (tests/attention_cases.py: the designs, the fp64 reference and the derivation of every gate;
tests/test_attention_cases_cpu.py: proof on the CPU that one lost, doubled or misplaced key / query / bit shows at >= 8 x
the widest gate).  Every comparison is against that fp64 reference, never against another kernel.

Gates, per element (u = 2^-8 bf16, 2^-11 half; A(x) = the sum of the absolute values of the terms of x):
    ctx, dv          3 u A(x)                                  P, the dropout scale and the output are rounded once each
                     (gather: + the reference's own leak, ~3e-9)
    dq, dk uniform   u A1 + 3 u A2 + u |ref|                   + dS rounded once; A1 = 0.125 sum |dS| |k|, A2 = 0.125 sum P Dabs |k|
    dq, dk gather    (1 + u) (64 2^-24 + [p > 0] (2 u + 4 2^-24)) A2 + A1          the exact value is 0: only the fp32
                     summation order of delta against dP (and, under dropout, the rounded scale inside the stored context) is left
    dbias_qkv        the column sum of the gates above + Mt 2^-24 sum_rows |ref|   (fp32 column sums of the unrounded gradients)
    fp32 entries     the controls of the designs: 2e-5 (the project's fp32 attention gate) in place of 3 u / 4 u / u
    lse              see LSE_GATE below
"""
import pytest
import torch

import attention_cases as AC
from guard import check, guarded, snapshot, unchanged
from visiontransformer_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P_DROP = 0.25
STREAM_ID = AC.DROP_LAYER * 8 + 1
DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}

LSE_GATE = AC.LSE_GATE   # per design, with the measured errors it comes from (tests/attention_cases.py)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(t, dtype=None, name=None):
    """guard-banded device copy of a CPU tensor (tests/guard.py)"""
    return guarded(tuple(t.shape), dtype or t.dtype, t, device=DEV, name=name)


def _out(shape, dtype=torch.float32, fill="nan", name=None):
    return guarded(shape, dtype, fill, device=DEV, name=name)


def _after(snap, *outs):
    """after a call: every guard (inputs and outputs) intact, every input bitwise unchanged"""
    torch.cuda.synchronize()
    check(*[t for t, _ in snap], *[o for o in outs if o is not None])
    unchanged(snap)


def _ids(shapes):
    return [f"B{b}-Np{n}-A{a}" for b, n, a in shapes]


# entry -> (symbol, input format, output format, trailing integer arguments, shapes)
FORWARD = {
    "attention_bf16": ("vitseg_op_attention_bf16", "bf16", "bf16", (), AC.SHAPES),
    "attention_f16": ("vitseg_op_attention_f16", "fp16", "fp16", (), AC.SHAPES),
    "attention_h16_small[bf16]": ("vitseg_op_attention_h16_small", "fp32", "bf16", (0,), AC.SHAPES_SHORT),
    "attention_h16_small[fp16]": ("vitseg_op_attention_h16_small", "fp32", "fp16", (1,), AC.SHAPES_SHORT),
    "attention_f32": ("vitseg_op_attention_f32", "fp32", "fp32", (), AC.SHAPES),
    "attention_f32_small": ("vitseg_op_attention_f32_small", "fp32", "fp32", (), AC.SHAPES_SHORT),
    "attention_f32x3": ("vitseg_op_attention_f32x3", "fp32", "fp32", (), AC.SHAPES),
}
FORWARD_CASES = [pytest.param(e, *s, id=f"{e}-B{s[0]}-Np{s[1]}-A{s[2]}") for e, row in FORWARD.items() for s in row[4]]


@pytest.mark.parametrize("design", AC.DESIGNS)
@pytest.mark.parametrize("entry,B,Np,A", FORWARD_CASES)
def test_forward(entry, B, Np, A, design):
    """Inference forward of every attention entry point: ctx within 3 u A(ctx) of the fp64 reference -- in the gather design
    3 u |v_pi(i)| (the matched key's value row or nothing) + the leak, in the uniform designs 3 u |ref| = 1.2 % (bf16), where a lost
    heavy key is 20 % (N = 1025) to 98 % (N = 5) of its channel."""
    fn, fin, fout, extra, _ = FORWARD[entry]
    c, ref = AC.make_case(design, B, Np, A), AC.reference(design, B, Np, A)
    qd = _dev(c.qkv, DT[fin], name="qkv")
    ctx = _out((c.Mt, c.D), DT[fout], name="ctx")
    snap = snapshot(qd)
    _lib.check(getattr(_lib.lib(), fn)(qd.data_ptr(), ctx.data_ptr(), B, Np, A, *extra, _stream()))
    _after(snap, ctx)
    ratio = AC.worst_ratio(ctx.float().cpu(), ref.ctx, ref.gates(fout)["ctx"])
    print(f"RATIO {entry} {design} B{B}-Np{Np}-A{A} ctx {ratio:.3f}")
    assert ratio <= 1.0, ratio


def _dropped_rows(c, ctx):
    """gather: [B, A, N] bool, the (image, head, query) whose context row is nothing but the leak (kept rows hold M v with an
    integer row v != 0, i.e. at least 1 somewhere)"""
    out = torch.zeros(c.B, c.A, c.N, dtype=torch.bool)
    for b in range(c.B):
        rows = AC.token_rows(c.B, c.Np, b)
        out[b] = (ctx[rows].reshape(c.N, c.A, 64).abs().amax(-1) < 0.5).T
    return out


def _has_256(c, ctx, mask):
    """heavy_key: [B, A, N, 64] bool, the outputs (i, c) that hold their heavy key: ctx_ic = (kept_i + 255 keep(i, j*_c)) M / N
    lies above the half-way mark (kept_i + 127.5) M / N"""
    out = torch.zeros(c.B, c.A, c.N, 64, dtype=torch.bool)
    for b in range(c.B):
        rows = AC.token_rows(c.B, c.Np, b)
        got = ctx[rows].reshape(c.N, c.A, 64).transpose(0, 1)                 # [A, N, 64]
        half = (mask[b].sum(-1) + 127.5 * mask.max()) / c.N                   # [A, N]: sum_j M_ij = kept_i M
        out[b] = got > half[..., None]
    return out


TRAIN = {
    "attention_bwd_bf16": ("bf16", AC.SHAPES, ("p0", "hash", "words")),
    "attention_bwd_f32": ("fp32", AC.SHAPES, ("p0",)),
    "attention_bwd_f32_small": ("fp32", AC.SHAPES_SHORT, ("p0", "hash")),
}
TRAIN_CASES = [pytest.param(e, m, *s, id=f"{e}-{m}-B{s[0]}-Np{s[1]}-A{s[2]}") for e, (_, shapes, modes) in TRAIN.items()
               for m in modes for s in shapes if m != "words" or s[1] % 128 == 0]


def _run_pair(entry, mode, c, fmt):
    """one call of a training pair; ctx, lse, dqkv, dbias (or None) as CPU tensors"""
    B, Np, A = c.B, c.Np, c.A
    p = 0.0 if mode == "p0" else P_DROP
    dt = DT[fmt]
    qd, dd = _dev(c.qkv, dt, name="qkv"), _dev(c.dctx, dt, name="dctx")
    ctx = _out((c.Mt, c.D), dt, name="ctx")
    lse = _out((B * A * c.N,), name="lse")
    dqkv = _out((c.Mt, 3 * c.D), dt, name="dqkv")
    snap = snapshot(qd, dd)
    dbias = None
    L = _lib.lib()
    if entry == "attention_bwd_bf16":
        scr = _out((L.vitseg_attention_bwd_scratch_floats(B, Np, A),), name="attention_bwd scratch")
        mw = _out((L.vitseg_attention_dropmask_bytes(B, Np, A),), torch.uint8, name="dropmask words") if mode == "words" else None
        dbias = _out((3 * c.D,), name="dbias_qkv")
        _lib.check(L.vitseg_op_attention_bwd_bf16(qd.data_ptr(), dd.data_ptr(), ctx.data_ptr(), lse.data_ptr(), scr.data_ptr(),
                                                  dqkv.data_ptr(), B, Np, A, p, AC.DROP_SEED, STREAM_ID,
                                                  mw.data_ptr() if mw is not None else None, dbias.data_ptr(), _stream()))
        _after(snap, ctx, lse, scr, dqkv, mw, dbias)
    elif entry == "attention_bwd_f32":
        scr = _out((B * A * c.N,), name="attention_bwd scratch")
        _lib.check(L.vitseg_op_attention_bwd_f32(qd.data_ptr(), dd.data_ptr(), ctx.data_ptr(), lse.data_ptr(), scr.data_ptr(),
                                                 dqkv.data_ptr(), B, Np, A, _stream()))
        _after(snap, ctx, lse, scr, dqkv)
    else:
        _lib.check(L.vitseg_op_attention_bwd_f32_small(qd.data_ptr(), dd.data_ptr(), ctx.data_ptr(), lse.data_ptr(),
                                                       dqkv.data_ptr(), B, Np, A, p, AC.DROP_SEED, STREAM_ID, _stream()))
        _after(snap, ctx, lse, dqkv)
    return (ctx.float().cpu().double(), lse.cpu().double().view(B, A, c.N), dqkv.float().cpu().double(),
            None if dbias is None else dbias.cpu().double())


@pytest.mark.parametrize("design", AC.DESIGNS)
@pytest.mark.parametrize("entry,mode,B,Np,A", TRAIN_CASES)
def test_training_pair(entry, mode, B, Np, A, design):
    """Forward (ctx, lse) + backward (dq | dk | dv, dbias_qkv) of the three training pairs against the fp64 reference, which takes the
    kernels' own dropout masks (tests/dropout_ref.py, seed and stream id of test_attention_backward_bf16).  mode: p0 = no dropout,
    hash = p 0.25 hashed per element, words = p 0.25 through precomputed mask words (Np % 128 == 0).  Gates: the module docstring.
    Under dropout the kept / dropped PATTERN is asserted besides: gather -- the set of empty context rows is the set of
    dropped (query, own key) bits, N bits per head; heavy_key -- the set of outputs (i, c) without their 256 is the set of
    dropped bits (i, j*_c), N x 64 per head.

    lse: uniform designs log2 N exactly, held to the project's fp32 gate 2e-5 (measured 6.0e-7 at worst; N - 1 keys would be
    >= 1.4e-3 off); gather 64 log2 e = 92.3, fp32 spacing 7.6e-6: measured 2.93e-5 (bwd_f32), 2.17e-5 (bwd_f32_small), 1.23e-6
    (bwd_bf16), gate 4 x 2.93e-5."""
    fmt = TRAIN[entry][0]
    p = 0.0 if mode == "p0" else P_DROP
    c, ref = AC.make_case(design, B, Np, A), AC.reference(design, B, Np, A, p)
    ctx, lse, dqkv, dbias = _run_pair(entry, mode, c, fmt)
    tag = f"{entry}[{mode}] {design} B{B}-Np{Np}-A{A}"
    gates = ref.gates(fmt)
    got = {"ctx": ctx, "dq": dqkv[:, :c.D], "dk": dqkv[:, c.D:2 * c.D], "dv": dqkv[:, 2 * c.D:]}
    ratios = {name: AC.worst_ratio(got[name], ref.part(name), gates[name]) for name in AC.OUTPUTS}
    lse_err = float((lse - ref.lse).abs().max())
    print(f"RATIO {tag} " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()) + f" lse_err {lse_err:.2e} lse {lse_err / LSE_GATE[design]:.3f}")
    if dbias is not None:
        want = ref.dqkv.sum(0)
        g = torch.cat([gates[n].sum(0) for n in ("dq", "dk", "dv")]) + c.Mt * 2.0 ** -24 * ref.dqkv.abs().sum(0)
        r = AC.worst_ratio(dbias, want, g)
        print(f"RATIO {tag} dbias {r:.3f}")
        assert r <= 1.0, ("dbias_qkv", r)
    if p and design == "gather":
        on = torch.stack([torch.stack([ref.mask[b, h][torch.arange(c.N), c.perm[b, h]] for h in range(A)]) for b in range(B)])
        assert torch.equal(_dropped_rows(c, ctx), on == 0), "the empty context rows are not the dropped (query, key) bits"
    if p and design == "heavy_key":
        want = torch.stack([torch.stack([ref.mask[b, h][:, c.heavy[b, h]] > 0 for h in range(A)]) for b in range(B)])
        assert torch.equal(_has_256(c, ctx, ref.mask), want), "the outputs without their heavy key are not the dropped bits"
    for name in AC.OUTPUTS:
        assert ratios[name] <= 1.0, (name, ratios[name])
    assert lse_err < LSE_GATE[design], lse_err
