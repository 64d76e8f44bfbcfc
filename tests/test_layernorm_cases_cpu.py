"""CPU (-m "not gpu"): the gates of tests/layernorm_cases.py can tell right from wrong.

1. A plain fp32 two-pass model of the kernels' arithmetic (fp32 mean, subtract, fp32 variance, 1 / sqrt(var + eps), the backward
   as backward.hip writes it) stays within 0.25 of every gate, for every design, shape and eps, in two summation orders: as
   the kernels sum (four values a vector, the lane's vectors one after the other, a 64-lane tree), and the most sequential
   order a wave-per-row kernel can take (each lane one value after the other, then lane after lane: a chain of up to 95).
   ONE chain over all D values is left out on purpose: its error grows with D itself (measured at K = 4: 2.96 gates at D = 2048, outlier design),
   the gates' log2 D form rightly refuses it, and no kernel of this family sums so.
   Worst ratios: y 0.232, out 0.182, dw 0.097, db 0.169, br 0.182, brsum 0.095, brsum_own 0.158.  An output rounded to 16
   bits may use the u16 |ref| of its gate in full: y 0.999, br 0.996, brsum 0.992 at worst, asserted <= 1.
2. Each single fault of MUTANTS lands at 8 x the gate or more in the design named beside it -- at every D, row count and eps
   tried there, not at one lucky shape (measured ranges beside each).
3. layer_norm_eps through the whole model: the oracle itself shows that the whole-model test of
   tests/test_gpu_layernorm_cases.py can see an eps replaced by 1e-12 at any ONE LayerNorm site.
"""
import math

import numpy as np
import pytest
import torch

import layernorm_cases as LC

F = np.float32


def _tree(s):
    """sum over the last axis by halving (a power-of-two length)"""
    while s.shape[-1] > 1:
        h = s.shape[-1] // 2
        s = s[..., :h] + s[..., h:]
    return s[..., 0]


def rowsum(t, order, nvl):
    """fp32 sum over the columns of t [R, D] as one wave can sum a row that lies across its 64 lanes (lane l holds vectors l, l + 64,
    ...): "lane64" as the kernels do, (a + b) + (c + d) per vector, the lane's vectors one after the other, a 64-lane tree; "seq"
    the most sequential form such a kernel can take, every lane one value after the other and then lane after lane (a chain
    of 4 NV + 63 <= 95 additions).  One chain over all D values is not tried: its error grows with D itself, which no log2 D
    bound covers, and a row kernel that summed so would rightly fail these gates."""
    R, D = t.shape
    pad = np.zeros((R, 256 * nvl), F)
    pad[:, :D] = t
    v = pad.reshape(R, nvl, 64, 4)
    s = np.zeros((R, 64), F)
    if order == "seq":
        for i in range(nvl):
            for e in range(4):
                s = s + v[:, i, :, e]
        tot = np.zeros(R, F)
        for l in range(64):
            tot = tot + s[:, l]
        return tot
    v = (v[..., 0] + v[..., 1]) + (v[..., 2] + v[..., 3])
    for i in range(nvl):
        s = s + v[:, i]
    return _tree(s)


def colsum(t, order, skip=None):
    """fp32 sum over the rows of t [R, D]: "seq" row after row; "lane64": four waves take every fourth row, then (0 + 1) + (2 + 3)"""
    rows = [r for r in range(t.shape[0]) if r != skip]
    if order == "seq":
        s = np.zeros(t.shape[1], F)
        for r in rows:
            s = s + t[r]
        return s
    part = np.zeros((4, t.shape[1]), F)
    for k, r in enumerate(rows):
        part[k % 4] = part[k % 4] + t[r]
    return (part[0] + part[1]) + (part[2] + part[3])


def _bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a)).bfloat16().float().numpy()


def _round(a, fmt):
    if fmt == "fp32":
        return a
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.bfloat16() if fmt == "bf16" else t.half()).float().numpy()


def model(c, order="lane64", mut=None, p=0.0, fmt="fp32", g16=False):
    """The kernels' fp32 arithmetic on case c with at most one fault `mut` (a key of MUTANTS); fmt: the 16-bit format of y
    and br ("fp32": none).  Returns y, out, dw, db, br, brsum as fp32 arrays."""
    x, w, b, g, dres = (t.numpy().astype(F) for t in (c.x, c.w, c.b, c.g, c.dres))
    if g16:
        g = _bf16(g)
    R, D = x.shape
    nvl = (D // 4 + 63) // 64
    eps = F(c.eps)
    if mut == "eps_1e-12":
        eps = F(1e-12)
    elif mut == "eps_0":
        eps = F(0.0)
    lanes = np.ones(D, F)
    if mut == "drop_last":
        lanes[D - 4:] = 0
    elif mut == "dup_last":
        lanes[D - 4:] = 2
    rs = lambda t: rowsum((t * lanes).astype(F), order, nvl)
    with np.errstate(all="ignore"):
        n = F(256 * nvl) if mut == "pad_mean" else F(D)
        mean = (rs(x) / n)[:, None]
        d = x - mean
        if mut == "onepass":
            var = rs(x * x) / F(D) - mean[:, 0] * mean[:, 0]
        else:
            var = rs(d * d) / (F(D - 1) if mut == "unbiased" else F(D))
        rstd = (F(1) / (np.sqrt(var) + eps) if mut == "eps_outside" else F(1) / np.sqrt(var + eps))[:, None]
        if mut == "prev_row_stats":
            mean, rstd = np.roll(mean, 1, 0), np.roll(rstd, 1, 0)
            d = x - mean
        y = _round(d * rstd * w + b, fmt)
        xhat = d * rstd
        gw = g * w
        c1 = F(0) if mut == "no_c1" else (rs(gw) / F(D))[:, None]
        c2 = F(0) if mut == "no_c2" else (rs(gw * xhat) / F(D))[:, None]
        dx = rstd * (gw - c1 - xhat * c2)
        out = dx if mut == "no_dres" else dres + dx
        skip = R - 1 if mut == "lost_row" and R > 1 else None
        dw = colsum(g * (x if mut == "dw_x" else xhat), order, skip)
        db = colsum(g, order, skip)
        mask = (LC.kernel_mask(p, R, D) if p else torch.ones(R, D)).numpy().astype(F)
        br = mask * out
        if mut == "br_drop_res":
            br = dx + mask * dres
        elif mut == "br_before_dres":
            br = mask * dx
        br16 = _round(br, fmt)
        brsum = colsum(br if mut == "brsum_unrounded" else br16, order, skip)
    return dict(y=y, out=out.astype(F), dw=dw, db=db, br=br16, brsum=brsum)


def ratios(c, m, p=0.0, fmt="fp32", g16=False):
    ref = LC.reference(c.design, c.rows, c.D, c.eps, p, g16)
    r = {"y": LC.worst_ratio(m["y"], ref.y16[fmt] if c.design == "exact" else ref.y, ref.gate_y(fmt)),
         "out": LC.worst_ratio(m["out"], ref.out, ref.gate_out),
         "dw": LC.worst_ratio(m["dw"], ref.dw, ref.gate_dw),
         "db": LC.worst_ratio(m["db"], ref.db, ref.gate_db),
         "br": LC.worst_ratio(m["br"], ref.br, ref.gate_br(fmt)),
         "brsum": LC.worst_ratio(m["brsum"], ref.brsum, ref.gate_brsum(fmt))}
    own = torch.from_numpy(m["br"])
    r["brsum_own"] = LC.worst_ratio(m["brsum"], own.double().sum(0), LC.own_sum_gate(own))
    return r


WORST = {}


@pytest.mark.parametrize("D", LC.D_FWD)
@pytest.mark.parametrize("design", LC.DESIGNS_BWD)
def test_fp32_model_stays_within_a_quarter_of_every_gate(design, D):
    backward = D in LC.D_BWD
    if not backward and design not in LC.DESIGNS_FWD:
        return   # the backward takes no row above 1024 values
    worst = {}
    for rows in LC.ROWS:
        for eps in LC.EPS:
            c = LC.make_case(design, rows, D, eps)
            for order in ("seq", "lane64"):
                for p, fmt, g16 in ((0.0, "fp32", False), (0.25, "fp32", False), (0.25, "bf16", True), (0.0, "fp16", False)):
                    r = ratios(c, model(c, order, None, p, fmt, g16), p, fmt, g16)
                    for k, v in r.items():
                        if (backward and fmt != "fp16") or k == "y":   # (half is an output format of the forward alone)
                            # a 16-bit output is rounded once more: up to u16 |ref| of its gate is that rounding's by right
                            k = k + "[16]" if fmt != "fp32" and k in ("y", "br", "brsum") else k
                            worst[k] = max(worst.get(k, 0.0), v)
                if design == "exact":   # the deviation is exactly 0: y is b, bit for bit, in either order
                    assert np.array_equal(model(c, order)["y"], np.broadcast_to(c.b.numpy(), (rows, D)))
    print("MODEL", design, D, " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for k, v in worst.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
        assert v <= (1.0 if k.endswith("[16]") else 0.25), (k, v)


# fault -> (the design that must show it at >= 8 gates, the outputs it may show in).  Beside each: the smallest .. largest ratio over MUT_D x MUT_ROWS x eps
# (inf: a non-finite output, or an output that has to be exact and is not).
MUTANTS = {
    "onepass": ("offset", ("y",)),                       # 99 .. inf
    "unbiased": ("eps", ("y",)),                         # 90 .. 556
    "eps_outside": ("eps", ("y", "out")),                # 1.6e6 .. 2.0e6
    "eps_1e-12": ("eps", ("y", "out")),                  # 1.7e6 .. 2.0e6 (where eps is not 1e-12 itself)
    "eps_0": ("eps", ("y", "out")),                      # 1.7e6 .. 2.0e6
    "pad_mean": ("exact", ("y",)),                       # inf: y is not b (ragged D only: 64 NV 4 lanes = D otherwise)
    "drop_last": ("exact", ("y",)),                      # inf
    "dup_last": ("exact", ("y",)),                       # inf
    "prev_row_stats": ("offset", ("y", "out")),          # 3e10 .. 4e18
    "no_c1": ("null", ("out",)),                         # 5.1e4 .. 5.3e4
    "no_c2": ("null", ("out",)),                         # 4.7e4 .. 5.0e4
    "no_dres": ("null", ("out",)),                       # 3.1e5 .. 5.6e5
    "dw_x": ("offset", ("dw",)),                         # 4.1e3 .. 1.0e4
    "lost_row": ("heavy_row", ("dw", "db", "brsum")),    # 5.2e4 .. 8.4e5
    "br_drop_res": ("heavy_row", ("br",)),               # inf: a dropped element is not 0 (p = 0.25)
    "br_before_dres": ("null", ("br",)),                 # 3.1e5 .. 5.4e5
    "brsum_unrounded": ("heavy_row", ("brsum_own",)),    # 155 .. 3.1e3 (the bf16 form alone)
}
MUT_D, MUT_ROWS = (192, 320, 1024), (5, 67)   # 192 and 320 are ragged (48 and 80 vectors against 64 lanes)


@pytest.mark.parametrize("mut", list(MUTANTS))
def test_every_single_fault_is_eight_gates_away(mut):
    design, outputs = MUTANTS[mut]
    bf16 = mut == "brsum_unrounded"
    p, fmt, g16 = (0.25, "bf16", True) if bf16 or mut == "br_drop_res" else (0.0, "fp32", False)
    best = 0.0
    for D in MUT_D:
        if mut == "pad_mean" and D % 256 == 0:
            continue
        for rows in MUT_ROWS:
            for eps in LC.EPS:
                if mut == "eps_1e-12" and eps == 1e-12:
                    continue
                c = LC.make_case(design, rows, D, eps)
                r = ratios(c, model(c, "lane64", mut, p, fmt, g16), p, fmt, g16)
                here = max(r[k] for k in outputs)
                print("MUTANT", mut, design, f"D{D} rows{rows} eps{eps:g}", " ".join(f"{k} {r[k]:.3g}" for k in outputs))
                # the fault shows at EVERY shape and eps of its design, not at one lucky one
                assert here >= 8.0, (mut, D, rows, eps, r)
                best = max(best, here)
    assert best >= 8.0


@pytest.mark.parametrize("site", range(len(LC.MODEL_SITES)), ids=LC.MODEL_SITES)
def test_whole_model_case_sees_a_wrong_eps_at_any_single_site(site):
    """The whole-model test compares with the oracle at eps = MODEL_EPS under the gates of tests/test_gpu_config_sweep.py.  Its
    power, shown on the oracle alone: 1e-12 at this ONE site, MODEL_EPS at the other four, moves the logits by >= 8 x the widest
    logits gate (bf16: 3e-2) and some tensor's loss gradient by >= 8 x the widest gradient gate (bf16: 0.10 relative L2).
    Measured: logits 0.70 / 1.14 / 0.96 / 0.54 / 2.43 (gate 0.24), gradient 573 / 25 / 53 / 10.9 / 30.6 (gate 0.8), sites in MODEL_SITES order."""
    torch.set_num_threads(8)
    cfg, sd, x, y = LC.whole_model()
    logits, _, leaf, _ = _oracle_right()
    wrong, _, wleaf, _ = LC.oracle_step(cfg, sd, x, y, wrong_site=site)
    move = float((wrong - logits).abs().max())
    gmove = max(float((wleaf[k].grad - v.grad).norm() / v.grad.norm()) for k, v in leaf.items()
                if v.grad is not None and "pooler" not in k and v.grad.norm() >= 1e-7)
    print(f"EPS-SITE {LC.MODEL_SITES[site]}: logits move {move:.3g}, gradient move {gmove:.3g}")
    assert move >= 8 * max(LC.MODEL_TOL.values()), move
    assert gmove >= 8 * max(LC.MODEL_GRAD_REL.values()), gmove


_RIGHT = []


def _oracle_right():
    if not _RIGHT:
        _RIGHT.append(LC.oracle_step(*LC.whole_model()))
    return _RIGHT[0]
