"""GPU (-m gpu): the K-sliced GEMM paths at and either side of their slice counts, through the C ABI, against fp64.

Many GEMMs cut the reduction into slices, write fp32 partials into a scratch buffer and sum them with a second kernel.  The
slice count is an integer function of the shape (csrc/gemm_dispatch.hip, splitk.hip, gemm_p8.hip) and fixes the grid, the
stride between partials, the reducing loop and the scratch size, so a kernel can be wrong at one count and right at its
neighbours.  Every case here (tests/splitk_cases.py) is named after its count and asserts it (vitseg_dbg_gemm_slices), brings a
NaN-poisoned scratch of EXACTLY the queried size between guards, checks its inputs unchanged, compares with the fp64 product
of the same (rounded) operands under the tolerance formulas of test_gpu_ops.py, and runs twice for identical bits (the
reduce has a fixed order).  The largest error / bound ratio of each family is printed at the end (-s)."""
import numpy as np
import pytest
import torch

import splitk_cases as SC
from guard import check, guarded, snapshot, unchanged
from oracle import vitseg_oracle as O
from visiontransformer_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for fam in sorted(RATIOS):
        print(f"\nsplitk max error/bound [{fam}]: {RATIOS[fam][0]:.3f} at {RATIOS[fam][1]}", end="")
    print()


def _ratio(fam, err, bound, what):
    """records err / bound (tensors or floats) for the family and returns the largest ratio"""
    r = float((torch.as_tensor(err) / torch.as_tensor(bound)).max())
    if fam not in RATIOS or r > RATIOS[fam][0]:
        RATIOS[fam] = (r, what)
    return r


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


def _dev(t, dtype=None, name=None):
    return guarded(tuple(t.shape), dtype or t.dtype, t, device=DEV, name=name)


def _out(shape, dtype=torch.float32, fill="nan", name=None):
    return guarded(shape, dtype, fill, device=DEV, name=name)


def _after(snap, *outs):
    torch.cuda.synchronize()
    check(*[t for t, _ in snap if t is not None], *outs)
    unchanged(snap)


def _poison_left(scratch):
    """True when no byte of the NaN-poisoned scratch was written"""
    return bool((scratch.view(-1).view(torch.uint8) == 0xFF).all())


def _ptr(t):
    return t.data_ptr() if t is not None else None


# ------------------------------------------------------------------ weight gradients (both operands token-major)
def _wgrad_bf16_run(dYd, Xd, zeros, M, N, K):
    L = _lib.lib()
    n = L.vitseg_op_wgrad_bf16_scratch_floats(M, N, K)
    dW, scratch = _out((M, N), name="dW"), _out((n,), name="wgrad scratch (exactly the queried size)")
    snap = snapshot(dYd, Xd, zeros)
    _lib.check(L.vitseg_op_wgrad_bf16(dYd.data_ptr(), Xd.data_ptr(), dW.data_ptr(), scratch.data_ptr(), zeros.data_ptr(),
                                      M, N, K, _stream()))
    _after(snap, dW, scratch)
    return dW, n


def _wgrad_bf16_case(fam, path, s, M, N, K):
    assert _lib.gemm_slices(path, M, N, K) == s, "the case moved to another slice count"
    dY = _rand(K, M, seed=K).to(torch.bfloat16)
    X = _rand(K, N, seed=N + 3, scale=0.5).to(torch.bfloat16)
    ref = dY.double().T @ X.double()
    scale = float((dY.abs().double().T @ X.abs().double()).max())
    bound = 4e-7 * scale + 1e-5
    dYd, Xd = _dev(dY, name="dY"), _dev(X, name="X")
    zeros = _out((256,), torch.uint8, "zero", name="zero page")
    dW, n = _wgrad_bf16_run(dYd, Xd, zeros, M, N, K)
    assert n >= s * M * N
    err = (dW.cpu().double() - ref).abs().max().item()
    print(f"{fam} {s} slices ({M}, {N}, {K}): err {err:.3e} bound {bound:.3e}")
    _ratio(fam, err, bound, (s, M, N, K))
    assert err < bound, (err, bound)
    dW2, _ = _wgrad_bf16_run(dYd, Xd, zeros, M, N, K)
    assert torch.equal(dW, dW2)
    return dYd, Xd, zeros, dW, ref, bound


@pytest.mark.parametrize("s,M,N,K", SC.WGRAD_TT)
def test_wgrad_bf16_tt_slices(s, M, N, K):
    """gemm_tt.hip (128x128, split over grid.y, balanced slices) + splitk_reduce."""
    _wgrad_bf16_case("wgrad bf16 128x128", SC.P_WGRAD_BF16_TT, s, M, N, K)


@pytest.mark.parametrize("s,M,N,K", SC.WGRAD_P8)
def test_wgrad_bf16_p8_slices(s, M, N, K):
    """gemm_p8.hip in its T-form (256x256, an even number of K steps per slice: ksteps = 8 s + 1 leaves trailing slices empty,
    which must store zeros over the poison), and the same shape on the 128x128 kernel under the switch no_p8."""
    dYd, Xd, zeros, dW, ref, bound = _wgrad_bf16_case("wgrad bf16 8-phase", SC.P_WGRAD_BF16_P8, s, M, N, K)
    with _lib.option("no_p8", 1):
        assert _lib.gemm_slices(SC.P_WGRAD_BF16_P8, M, N, K) == 0
        s_tt = _lib.gemm_slices(SC.P_WGRAD_BF16_TT, M, N, K)
        assert s_tt >= 1
        dW_tt, n = _wgrad_bf16_run(dYd, Xd, zeros, M, N, K)
        assert n >= s_tt * M * N
    err = (dW_tt.cpu().double() - ref).abs().max().item()
    _ratio("wgrad bf16 128x128", err, bound, (s_tt, M, N, K))
    assert err < bound, (err, bound)
    assert (dW - dW_tt).abs().max().item() < bound


@pytest.mark.parametrize("s,M,N,K", SC.WGRAD_F32)
def test_wgrad_f32_slices(s, M, N, K):
    """launch_wgrad_f32 (gemm_tile.hip with both operands T-form, 32-deep K steps) + splitk_reduce, through vitseg_op_wgrad_f32."""
    assert _lib.gemm_slices(SC.P_WGRAD_F32, M, N, K) == s, "the case moved to another slice count"
    q, run = _lib.splitk_symbol("vitseg_op_wgrad_f32_scratch_floats"), _lib.splitk_symbol("vitseg_op_wgrad_f32")
    dY, X = _rand(K, M, seed=K), _rand(K, N, seed=N + 3, scale=0.5)
    ref = dY.double().T @ X.double()
    bound = 4e-7 * float((dY.abs().double().T @ X.abs().double()).max()) + 1e-6
    dYd, Xd = _dev(dY, name="dY"), _dev(X, name="X")
    n = q(M, N, K)
    assert n == s * M * N
    outs = []
    for _ in range(2):
        dW, scratch = _out((M, N), name="dW"), _out((n,), name="wgrad scratch (exactly the queried size)")
        snap = snapshot(dYd, Xd)
        _lib.check(run(dYd.data_ptr(), Xd.data_ptr(), dW.data_ptr(), scratch.data_ptr(), M, N, K, _stream()))
        _after(snap, dW, scratch)
        assert s == 1 or not torch.isnan(scratch).any()       # every slice stored its whole partial
        outs.append(dW)
    err = (outs[0].cpu().double() - ref).abs().max().item()
    print(f"wgrad f32 {s} slices ({M}, {N}, {K}): err {err:.3e} bound {bound:.3e}")
    _ratio("wgrad f32", err, bound, (s, M, N, K))
    assert err < bound, (err, bound)
    assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------ linears: whole-GEMM split and trailing rows by split-K
FMT = {"bf16": (torch.bfloat16, 2 ** -8), "fp16": (torch.float16, 2 ** -11)}


def _gelu_grad64(u):
    return 0.5 * (1 + torch.erf(u / 2 ** 0.5)) + u * torch.exp(-0.5 * u * u) / (2 * np.pi) ** 0.5


def _drop_rows_np(M, N, p, seed, stream):
    from dropout_ref import Masks
    mk = Masks(p, seed, 1, 1, 1)
    keep = mk._keep(stream, np.arange(M)[:, None], np.arange(N)[None, :])
    return torch.from_numpy(np.where(keep, mk.scale, np.float32(0)).astype(np.float32))


class _Linear:
    """One linear layer C = epi(A W^T + bias) in `kind` (f32 / x3 / bf16 / fp16) with its fp64 reference and bound; run() calls
    the entry that takes a scratch (vitseg_op_linear_f32_thin / vitseg_op_linear_h16_ex) and returns (C, aux, colsum)."""

    def __init__(self, kind, M, N, K, epi, extra=""):
        self.kind, self.M, self.N, self.K, self.epi, self.extra = kind, M, N, K, epi, extra
        self.h16 = kind in FMT
        self.dt, self.ulp = FMT[kind] if self.h16 else (torch.float32, 0.0)
        A, W = _rand(M, K, seed=M + K), _rand(N, K, seed=N + 1, scale=0.05)
        if self.h16:
            A, W = A.to(self.dt).float(), W.to(self.dt).float()
        if "spike" in extra:   # tiny, subnormal-half and large magnitudes in one row (test_linear_f32x3_is_fp32_grade)
            A[0, :4] = torch.tensor([1e-6, -3e-5, 2.5e3, -7.0])
        bias = _rand(N, seed=7, scale=0.1)
        self.p, self.seed, self.stream_id = (0.1, 0x1234ABCD, 13) if "drop" in extra else (0.0, 0, 0)
        acc = A.double() @ W.double().T
        self.scale_el = A.abs().double() @ W.abs().double().T
        self.scale = float(self.scale_el.max())
        self.acc_b = acc + bias.double()
        self.Ad, self.Wd = _dev(A, self.dt, name="A"), _dev(W, self.dt, name="W")
        self.bd, self.Ud, self.R = _dev(bias, name="bias"), None, None
        if epi == 2:
            self.R = _rand(M, N, seed=11)
            y = self.acc_b * _drop_rows_np(M, N, self.p, self.seed, self.stream_id).double() if self.p else self.acc_b
            self.ref = self.R.double() + y
        elif epi == 5:
            U = _gelu_grad64(_rand(M, N, seed=12).double()).float().to(self.dt)
            self.Ud, self.bd = _dev(U, name="gelu'"), None
            self.ref = acc * U.double()
        else:
            self.ref = O.gelu_erf(self.acc_b) if epi == 1 else self.acc_b

    def run(self, thin_rows, scratch, capacity=None):
        L = _lib.lib()
        M, N, K, epi = self.M, self.N, self.K, self.epi
        out_dt = torch.float32 if epi == 2 else self.dt
        C = _dev(self.R, name="C") if epi == 2 else _out((M, N), out_dt, name="C")
        Rp = C.data_ptr() if epi == 2 else _ptr(self.Ud)          # in-place residual, as the forward uses it
        aux = _out((M, N), self.dt, name="aux") if "aux" in self.extra else None
        cs_out = cs_scr = None
        cap = scratch.numel() if capacity is None else capacity
        snap = snapshot(self.Ad, self.Wd, self.bd, self.Ud)
        if self.h16:
            if epi == 5 and self.kind == "bf16":
                cs_out = _out((N,), name="colsum")
                cs_scr = _out((L.vitseg_op_colsum_scratch_floats(M, N),), name="colsum scratch")
            _lib.check(L.vitseg_op_linear_h16_ex(
                self.Ad.data_ptr(), self.Wd.data_ptr(), _ptr(self.bd), Rp, C.data_ptr(), _ptr(aux), M, N, K, epi,
                int(self.kind == "fp16"), thin_rows, scratch.data_ptr(), cap, self.p, self.seed, self.stream_id, _ptr(cs_out),
                _ptr(cs_scr), _stream()))
        else:
            _lib.check(_lib.splitk_symbol("vitseg_op_linear_f32_thin")(
                self.Ad.data_ptr(), self.Wd.data_ptr(), _ptr(self.bd), Rp, C.data_ptr(), _ptr(aux), M, N, K, epi,
                int(self.kind == "x3"), thin_rows, scratch.data_ptr(), cap, self.p, self.seed, self.stream_id, _stream()))
        _after(snap, C, aux, scratch, cs_out, cs_scr)
        return C, aux, cs_out

    def verify(self, fam, what, C, aux, cs_out):
        got, ref, scale = C.float().cpu().double(), self.ref, self.scale
        err = (got - ref).abs()
        if self.kind == "x3":        # test_linear_f32x3_is_fp32_grade: 1e-6 of sum |a||w| per element
            bound = 1e-6 * (self.scale_el + 1e-3)
        elif self.kind == "f32":
            bound = torch.tensor(4e-7 * scale + 1e-6)
        elif self.epi == 2:          # fp32 output of 16-bit operands
            bound = torch.tensor(4e-7 * scale * (1.2 if self.p else 1.0) + 1e-5)
        else:                        # one rounding to the 16-bit format
            bound = self.ulp * ref.abs() + 4e-7 * scale + 2e-6
        r = _ratio(fam, err, bound, what)
        print(f"{fam} {what}: max err/bound {r:.3f}")
        assert bool((err < bound).all()), (what, float(err.max()), r)
        if aux is not None:
            dref = _gelu_grad64(self.acc_b)
            assert ((aux.float().cpu().double() - dref).abs() <= self.ulp * dref.abs() + 4e-7 * scale + 2e-6).all()
        if cs_out is not None:
            tol = 4 * 2.0 ** -9 * (ref ** 2).sum(dim=0).sqrt() + 4e-7 * scale * self.M ** 0.5
            assert ((cs_out.cpu().double() - ref.sum(dim=0)).abs() <= tol).all()


def _whole_cases():
    for kind in ("f32", "x3", "bf16", "fp16"):
        for s, M, N, K, epi in SC.WHOLE[64 if kind in FMT else 32]:
            yield pytest.param(kind, s, M, N, K, epi, id=f"{kind}-{s}sl-{M}x{N}x{K}-epi{epi}")


@pytest.mark.parametrize("kind,s,M,N,K,epi", list(_whole_cases()))
def test_whole_gemm_split(kind, s, M, N, K, epi):
    """A linear of at most 128 output tiles and K >= 512 runs on min(8, K / kstep / 4) K slices as a whole when the scratch holds
    slices * M * N floats: capacity exactly that.  0 slices (K below 512, 129 tiles): the path does not apply, the result is
    right and the scratch is not touched."""
    h16 = kind in FMT
    assert _lib.gemm_slices(SC.P_WHOLE_H16 if h16 else SC.P_WHOLE_F32, M, N, K) == s, "the case moved to another slice count"
    lin = _Linear(kind, M, N, K, epi)
    # vitseg_op_linear_h16_ex lends its scratch with thin_rows > 0 only; rows after a ragged body never qualify as thin rows, so
    # where the whole split does not apply the GEMM runs unsliced
    thin = 0 if not h16 else (1 if (M - 1) % 128 else 2)
    outs = []
    for _ in range(2):
        scratch = _out((max(s, 1) * M * N,), name="scratch (exactly slices * M * N)")
        C, aux, cs = lin.run(thin, scratch)
        if s:
            assert not torch.isnan(scratch).any()         # every slice stored its whole partial
        else:
            assert _poison_left(scratch)
        outs.append(C)
    lin.verify(f"whole split {kind}", (s, M, N, K, epi), outs[0], None, None)
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("kind", ["f32", "x3", "bf16", "fp16"])
@pytest.mark.parametrize("epi", [0, 2])
def test_whole_gemm_split_falls_back_one_float_short(kind, epi):
    """Capacity one float below slices * M * N: the router runs the GEMM unsliced, the answer agrees and the scratch keeps its
    poison."""
    M, N, K = 300, 768, 1024
    h16 = kind in FMT
    s = _lib.gemm_slices(SC.P_WHOLE_H16 if h16 else SC.P_WHOLE_F32, M, N, K)
    assert s == (4 if h16 else 8)
    lin = _Linear(kind, M, N, K, epi)
    thin = 1 if h16 else 0          # the body of 299 rows is ragged: no thin-row launch either
    full = _out((s * M * N,), name="scratch")
    C, _, _ = lin.run(thin, full)
    assert not torch.isnan(full).any()
    lin.verify(f"whole split {kind}", (s, M, N, K, epi), C, None, None)
    short = _out((s * M * N - 1,), name="scratch, one float short")
    C1, _, _ = lin.run(thin, short)
    assert _poison_left(short)
    lin.verify(f"unsliced {kind}", (0, M, N, K, epi), C1, None, None)


def _thin_cases():
    epis = {"f32": [(0, ""), (1, ""), (2, "")], "x3": [(0, ""), (1, ""), (2, "")], "fp16": [(0, ""), (1, ""), (2, "")],
            "bf16": [(0, ""), (1, "aux"), (2, "drop"), (5, "")]}
    for kind in ("f32", "x3", "bf16", "fp16"):
        kstep = 64 if kind in FMT else 32
        body = 768 if kind in FMT else 384     # whole tiles of the body kernel: 256 rows for 16-bit operands, 128 for fp32
        rows = [1, 63, 64]
        for i, (s, K) in enumerate(SC.THIN_K[kstep]):
            epi, extra = epis[kind][i % len(epis[kind])]
            yield pytest.param(kind, s, body, rows[i % 3], 768 if K > 2048 else 776, K, epi, extra,
                               id=f"{kind}-{s}sl-K{K}-rows{rows[i % 3]}-epi{epi}{extra}")
        for j, (epi, extra) in enumerate(epis[kind]):     # every epilogue at one count, every row count at it
            yield pytest.param(kind, 4, body, rows[j % 3], 1544, 4 * 4 * kstep, epi, extra,
                               id=f"{kind}-4sl-rows{rows[j % 3]}-epi{epi}{extra}")
        yield pytest.param(kind, 0, body, 65, 768, 1024, 0, "", id=f"{kind}-rows65")
    yield pytest.param("bf16", 4, 2048, 8, 768, 1024, 2, "drop", id="bf16-4sl-persistent-body")


@pytest.mark.parametrize("kind,s,body,rows,N,K,epi,extra", list(_thin_cases()))
def test_thin_rows_split(kind, s, body, rows, N, K, epi, extra):
    """The last `rows` rows after a body of whole tiles on clamp(K / kstep / 4, 1, 16) K slices of the 128x128 kernel + the
    reducing epilogue (launch_thin_rows), the body on its own kernel.  The scratch has the 16 * 64 * N floats the callers size
    it with.  K below 256 or more than 64 rows: the path does not apply, the result is right, the scratch untouched."""
    h16 = kind in FMT
    M = body + rows
    if rows <= 64:   # (the count is a function of K; 65 rows are refused by the router whatever it is)
        assert _lib.gemm_slices(SC.P_THIN_H16 if h16 else SC.P_THIN_F32, M, N, K) == s, "the case moved to another slice count"
    # the whole-GEMM split would take precedence if its slices fitted the scratch
    sp = _lib.gemm_slices(SC.P_WHOLE_H16 if h16 else SC.P_WHOLE_F32, M, N, K)
    assert sp == 0 or sp * M * N > 16 * 64 * N
    lin = _Linear(kind, M, N, K, epi, extra)
    outs = []
    with _lib.option("no_ragged_p8", 1):    # a ragged row tile that fits the persistent kernel's last round would ride along instead
        for _ in range(2):
            scratch = _out((16 * 64 * N,), name="thin scratch")
            C, aux, cs = lin.run(rows, scratch)
            used = s * rows * N
            flat = scratch.view(-1)
            assert not torch.isnan(flat[:used]).any()                   # every slice stored its rows
            assert _poison_left(flat[used:]) if used < flat.numel() else True
            outs.append((C, aux, cs))
    lin.verify(f"thin rows {kind}", (s, M, N, K, epi, extra), *outs[0])
    for a, b in zip(outs[0], outs[1]):
        assert a is None or torch.equal(a, b)


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_thin_rows_fall_back_when_the_scratch_is_short(kind):
    """A scratch below slices * rows * N floats is never written: the rows run with the body."""
    h16 = kind in FMT
    body, rows, N, K = (768 if h16 else 384), 64, 776, 1024
    s = _lib.gemm_slices(SC.P_THIN_H16 if h16 else SC.P_THIN_F32, body + rows, N, K)
    lin = _Linear(kind, body + rows, N, K, 0)
    with _lib.option("no_ragged_p8", 1):
        exact = _out((s * rows * N,), name="thin scratch (exactly slices * rows * N)")
        C, _, _ = lin.run(rows, exact)
        assert not torch.isnan(exact).any()
        lin.verify(f"thin rows {kind}", (s, body + rows, N, K, 0, "exact"), C, None, None)
        short = _out((s * rows * N - 1,), name="thin scratch, one float short")
        C1, _, _ = lin.run(rows, short)
        assert _poison_left(short)
        lin.verify(f"unsliced {kind}", (0, body + rows, N, K, 0, "short"), C1, None, None)
