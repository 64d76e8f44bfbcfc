"""LayerNorm inputs in which eps, the row mean and the row scale count, the fp64 reference they are compared with, and the
gates derived from the roundings an fp32 two-pass kernel is allowed (a plain helper module, imported like util.py;
tests/test_layernorm_cases_cpu.py proves the designs and the gates, tests/test_gpu_layernorm_cases.py runs the kernels).

Operation (x [rows, D], w, b [D], upstream gradient g, residual gradient dres, all per row r):
    mu = mean(x),  var = mean((x - mu)^2),  rstd = (var + eps)^-1/2,  xhat = (x - mu) rstd,  y = xhat w + b
    gw = g w,  c1 = mean(gw),  c2 = mean(gw xhat),  out = dres + rstd (gw - c1 - xhat c2)       ("dx + dres")
    dw = sum_r g xhat,  db = sum_r g,  br = mask out (mask = keep / (1 - p), tests/dropout_ref.py),  brsum = sum_r br
eps is taken as the kernels receive it: rounded to fp32.  An entry that reads g as bf16 is compared with the reference of
the ROUNDED g (Reference(..., g16=True)), so the rounding of the input is no error of the kernel.

Designs (make_case(design, rows, D, eps); every random part is seeded by the design and the shape):
offset     row r has mean m_r from {0, 1, -1, 1e2, -1e2, 1e4, -1e4} (r mod 7) and spread 2^k, k = -10 .. 5 (r mod 16): a
           one-pass variance, statistics of the neighbouring row, anything an absolute gate hides on a small row.
eps        entries +-a_r, as many + as -: mean exactly 0, variance exactly a_r^2, a_r^2 = eps / 100, eps, 100 eps (r mod 3).
           Well conditioned; an ignored, hard-coded or misplaced eps, a backward that recomputes rstd with another one.
exact      constant rows c_r from {0, 0.5, -2, 64}: every partial sum is exact in fp32 in any order, the deviation is exactly 0
           and y == b bit for bit; w = +-2^j and gw = g w built from pairs +-v + c so that mean(gw) and gw - mean(gw) are exact,
           out = dres + eps^-1/2 (gw - c).  0 x inf where eps is lost, a mean over a padded lane count, masked lanes that leak.
outlier    one channel per row is +-2^10, the rest N(0, 1); its column walks over 0, 3, 4, 255, 256, D - 1 and the last column
           of the last whole group of 64 vectors.
null       g = 1 / w (gw constant), g = xhat / w (gw = xhat), and their sum (r mod 3): dx = 0 in exact arithmetic, the output
           is dres + rounding -- the c1 and c2 reductions alone.  |w| in [0.5, 1.5], a third of them negative.
heavy_row  column c of g and of dres carries +-2^8 in ONE row h_c, N(0, 1) elsewhere; h_c walks over the first and last row and,
           for every block of the backward's grid (8 rows a block: backward.hip lnb_blocks below 64 x CUs rows), the four
           rows its waves start with and the last row of its share.  A row lost or counted twice in dw, db or brsum is 2^8 / sqrt(rows) of
           the column, not 1e-5 of max |dw|.

Gates, per element, u = 2^-24, L = log2 D.  The fp32 mean is off by at most dmu = u L mean|x_r| (a D-term sum across 64 lanes,
relative to the sum of the absolute values); every deviation x - mu~ carries that shift, s = dmu rstd in units of xhat.
The shift leaves the variance alone to first order (the deviations sum to 0) and adds dmu^2 to it: rstd is off by
rho = RHO u + s^2 / 2 relatively ("a few u": the variance's own sum, the division, the root and the reciprocal; s^2 / 2 is the
term the first-order form lacks, it counts only where a row is ill conditioned).
    y      K (s |w| + rho |xhat w| + u |ref|)                    the form u (L mean|x| rstd |w| + RHO |xhat w| + |ref|) + the s^2 term
           + u16 |ref| for a 16-bit output (u16 = 2^-8 bf16, 2^-11 half; + 2^-25 for half, which has no digits below 2^-24)
    out    K (rstd s (|c2| + |xhat c1|)                           the shift through xhat: c2 moves by c1 s, xhat c2 by s c2 + xhat c1 s
              + 3 rho S                                           rstd enters three times (the factor, xhat, and xhat inside c2)
              + 4 u S                                             the cancellation: S = rstd (|gw| + |c1| + |xhat c2|), four roundings
              + u L rstd (mean|gw| + |xhat| mean|gw xhat|)        the c1 / c2 sums, relative to the sums of their absolute values
              + u |dres| + u |ref|)
    dw     sum_r K |g| (s + (rho + u) |xhat|) + KC rows u sum_r |g xhat|     db     KC rows u sum_r |g|
    br     mask gate(out) + (u + u16) |br|                        brsum  sum_r gate(br) + KC rows u sum_r |br|
The bf16 form sums the ROUNDED branch values: besides the gate above its brsum is held to the fp64 column sum of the br it
wrote itself, within KC rows u sum_r |br| (brsum_own), which is what tells the rounded sum from the unrounded one.
exact design: every partial sum is exact, so s = 0 there and y has no gate at all (y == b, rounded once for a 16-bit output).
A u16 |ref| is the rounding's by right: a 16-bit output reaches 1.0 of its gate where an fp32 one stays below a quarter.
The open constants are fixed from the CPU fp32 model of tests/test_layernorm_cases_cpu.py, never from a kernel, at 4 x its
worst ratio or the next round number above:
    K = 5    how many of the bounds' worst cases add up.  At K = 1 the model's worst is 1.16 (y, outlier design, D = 512, the
             lane-after-lane order: the mean of a row with one channel of 2^10, small |xhat| beside it) -> 4.6 -> 5.
    RHO = 8  the "few u" of rstd; with K, 40 u of |xhat w|.
    KC = 4   column sums: rows u sum |term| is the bound of ONE chain of rows - 1 additions; at KC = 1 the model's worst is 0.68
             (db, 5 rows in one chain) -> 2.7 -> 4.
With these the model's worst ratios are y 0.232, out 0.182, dw 0.097, db 0.169, br 0.182, brsum 0.095, brsum_own 0.158.
A row whose mean dwarfs its spread (offset: 1e4 against 2^-10) is legitimately ill conditioned: s > 1, its gate says so.
"""
import math
from functools import lru_cache

import numpy as np
import torch

U = 2.0 ** -24
U16 = {"fp32": 0.0, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
K = 5.0
KC = 4.0
RHO = 8.0
FLOOR16 = {"fp32": 0.0, "bf16": 0.0, "fp16": 2.0 ** -25}   # half the spacing of the subnormal halves: no digits below it
EPS = (1e-12, 1e-6, 1e-5)
DESIGNS_FWD = ("offset", "eps", "exact", "outlier")
DESIGNS_BWD = DESIGNS_FWD + ("null", "heavy_row")
D_BWD = (64, 192, 320, 512, 704, 768, 1024)     # one whole and one ragged D / 4 per vectors-per-lane class (1, 2, 3, 4)
D_FWD = D_BWD + (1280, 2048)                    # the forward's fifth class (8 vectors per lane)
ROWS = (1, 5, 67, 261)
DROP_SEED, DROP_LAYER, DROP_SITE = 0x1234ABCD, 5, 2   # tests/test_gpu_small.py test_layernorm_backward_small_slabs_and_branch_outputs
STREAM_ID = DROP_LAYER * 8 + DROP_SITE


def f32(eps):
    return float(np.float32(eps))


def edge_columns(D):
    nv = D // 4
    cols = [0, 3, 4, 255, 256, D - 1, 4 * (nv // 64 * 64) - 1]
    return sorted({c for c in cols if 0 <= c < D})


def edge_rows(rows):
    """first, last, and per block of the backward's grid (G = ceil(rows / 8) blocks, block b: rows [b R / G, (b + 1) R / G)) the
    rows its four waves start with and the last row of its share"""
    G = (rows + 7) // 8
    out = [0, rows - 1]
    for b in range(G):
        lo, hi = b * rows // G, (b + 1) * rows // G
        out += [r for r in (lo, lo + 1, lo + 2, lo + 3, hi - 1) if lo <= r < hi]
    seen, uniq = set(), []
    for r in out:
        if r not in seen:
            seen.add(r)
            uniq.append(r)
    return uniq


class Case:
    """x, g, dres [rows, D], w, b [D]: fp32 tensors; heavy [D] (heavy_row: the heavy row of column c) or None"""

    def __init__(self, design, rows, D, eps):
        self.design, self.rows, self.D, self.eps = design, rows, D, eps
        self.heavy = None


def _w(gen, D):
    """|w| in [0.5, 1.5], every third entry (of a random order) negative"""
    w = 0.5 + torch.rand(D, generator=gen)
    w[torch.randperm(D, generator=gen)[:D // 3]] *= -1.0
    return w


@lru_cache(maxsize=64)
def make_case(design, rows, D, eps=1e-12):
    c = Case(design, rows, D, eps)
    gen = torch.Generator().manual_seed(10007 * DESIGNS_BWD.index(design) + 31 * D + rows + int(-math.log10(eps)))
    randn = lambda *s: torch.randn(*s, generator=gen)
    r = torch.arange(rows)
    c.w, c.b = _w(gen, D), randn(D) * 0.5
    c.x, c.g, c.dres = randn(rows, D), randn(rows, D), randn(rows, D)
    if design == "offset":
        m = torch.tensor([0.0, 1.0, -1.0, 1e2, -1e2, 1e4, -1e4])[r % 7]
        s = 2.0 ** ((r % 16).double() - 10.0)
        c.x = (m[:, None].double() + s[:, None] * c.x.double()).float()
    elif design == "eps":
        a = (torch.tensor([0.01, 1.0, 100.0], dtype=torch.float64)[r % 3] * f32(eps)).sqrt().float()
        sg = torch.ones(rows, D)
        for i in range(rows):
            sg[i, torch.randperm(D, generator=gen)[:D // 2]] = -1.0
        c.x = a[:, None] * sg
    elif design == "exact":
        c.x = torch.tensor([0.0, 0.5, -2.0, 64.0])[r % 4][:, None].expand(rows, D).contiguous()
        c.w = torch.tensor([0.5, -1.0, 2.0, 1.0, -0.5, -2.0])[torch.randint(0, 6, (D,), generator=gen)]
        v = torch.randint(-8, 9, (rows, D // 2), generator=gen).float() * 0.5
        cr = torch.tensor([0.0, 1.0, -0.5])[r % 3][:, None]
        gw = torch.empty(rows, D)
        for i in range(rows):
            p = torch.randperm(D, generator=gen)
            gw[i, p[:D // 2]] = v[i] + cr[i]
            gw[i, p[D // 2:]] = -v[i] + cr[i]
        c.g = gw / c.w            # exact: w is a power of two
        c.dres = (c.dres * 8).round() / 8
    elif design == "outlier":
        cols = edge_columns(D)
        col = torch.tensor([cols[i % len(cols)] for i in range(rows)])
        c.x[r, col] = 1024.0 * torch.where(c.x[r, col] < 0, -1.0, 1.0)
    elif design == "null":
        c.x = c.x + 0.3
        xd = c.x.double()
        d = xd - xd.mean(1, keepdim=True)
        xhat = d / ((d * d).mean(1, keepdim=True) + f32(eps)).sqrt()
        k = (r % 3)[:, None]
        gw = torch.where(k == 0, torch.ones_like(xhat), torch.where(k == 1, xhat, 1.0 + xhat))
        c.g = (gw / c.w.double()).float()
    elif design == "heavy_row":
        c.x = c.x + 0.3
        e = edge_rows(rows)
        c.heavy = torch.tensor([e[(i + D) % len(e)] for i in range(D)])
        col = torch.arange(D)
        for t in (c.g, c.dres):
            t[c.heavy, col] = 256.0 * torch.where(t[c.heavy, col] < 0, -1.0, 1.0)
    else:
        raise ValueError(design)
    return c


@lru_cache(maxsize=64)
def kernel_mask(p, rows, D):
    """keep / (1 - p) of the kernels' counter-based generator for rows 0 .. rows - 1 of the hidden-dropout stream STREAM_ID,
    fp64 [rows, D] (Masks.rows speaks the reference's layout: one image of rows - 1 patches, its CLS token -- kernel row
    rows - 1 -- first)"""
    from dropout_ref import Masks
    m = Masks(p, DROP_SEED, 1, rows - 1, 1).rows(DROP_LAYER, DROP_SITE, (1, rows, D))[0]
    return torch.cat([m[1:], m[:1]]).double()


class Reference:
    """fp64 outputs (y, mean, rstd, out, dw, db, br, brsum) and the gate ingredients of one case"""

    def __init__(self, case, p=0.0, g16=False):
        c = self.case = case
        eps = f32(c.eps)
        x, w, b, dres = c.x.double(), c.w.double(), c.b.double(), c.dres.double()
        g = c.g.bfloat16().double() if g16 else c.g.double()
        D, R = c.D, c.rows
        self.mean = x.mean(1, keepdim=True)
        d = x - self.mean
        self.rstd = 1.0 / ((d * d).mean(1, keepdim=True) + eps).sqrt()
        self.xhat = xhat = d * self.rstd
        self.y = xhat * w + b
        self.y16 = {"fp32": self.y, "bf16": self.y.float().bfloat16().double(), "fp16": self.y.float().half().double()}
        gw = g * w
        c1, c2 = gw.mean(1, keepdim=True), (gw * xhat).mean(1, keepdim=True)
        self.dx = self.rstd * (gw - c1 - xhat * c2)
        self.out = dres + self.dx
        self.dw, self.db = (g * xhat).sum(0), g.sum(0)
        self.mask = kernel_mask(p, R, D) if p else torch.ones(R, D, dtype=torch.float64)
        self.br = self.mask * self.out
        self.brsum = self.br.sum(0)
        # ---- gates (module docstring)
        L = math.log2(D)
        s = U * L * x.abs().mean(1, keepdim=True) * self.rstd
        if c.design == "exact":   # every partial sum of a constant row is exact: no shift, and y is held to b itself
            s = torch.zeros_like(s)
        rho = RHO * U + 0.5 * s * s
        self.gate_y32 = K * (s * w.abs() + rho * (xhat * w).abs() + U * self.y.abs())
        S = self.rstd * (gw.abs() + c1.abs() + (xhat * c2).abs())
        self.gate_out = K * (self.rstd * s * (c2.abs() + (xhat * c1).abs()) + 3 * rho * S + 4 * U * S
                             + U * L * self.rstd * (gw.abs().mean(1, keepdim=True) + xhat.abs() * (gw * xhat).abs().mean(1, keepdim=True))
                             + U * dres.abs() + U * self.out.abs())
        self.gate_dw = (K * g.abs() * (s + (rho + U) * xhat.abs())).sum(0) + KC * R * U * (g * xhat).abs().sum(0)
        self.gate_db = KC * R * U * g.abs().sum(0)

    def gate_y(self, fmt="fp32"):
        if self.case.design == "exact":   # y == b, rounded once for a 16-bit output, bit for bit
            return torch.zeros_like(self.y)
        return self.gate_y32 + U16[fmt] * self.y.abs() + FLOOR16[fmt]

    def gate_br(self, fmt="fp32"):
        return self.mask * self.gate_out + (U + U16[fmt]) * self.br.abs()

    def gate_brsum(self, fmt="fp32"):
        return self.gate_br(fmt).sum(0) + KC * self.case.rows * U * self.br.abs().sum(0)


@lru_cache(maxsize=16)
def reference(design, rows, D, eps=1e-12, p=0.0, g16=False):
    return Reference(make_case(design, rows, D, eps), p, g16)


def own_sum_gate(br):
    """gate of a column sum against the fp64 sum of the very values that were summed: KC rows u sum_r |br|"""
    return KC * br.shape[0] * U * br.double().abs().sum(0)


def worst_ratio(got, ref, gate):
    """max |got - ref| / gate over the elements (an element with gate 0 must be exact; a non-finite output is infinitely far)"""
    err = (torch.as_tensor(got).double() - ref).abs()
    if not torch.isfinite(err).all():
        return math.inf
    ratio = torch.where(gate > 0, err / gate.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return float(ratio.max())


# ---- layer_norm_eps through the whole model -------------------------------------------------------------------------------------
# One small config (C, P, D, L, A, S, I, B) of the kind tests/test_gpu_config_sweep.py uses, with an eps that matters: the
# residual stream's variance is 6 (embeddings) to 43 (layer 1) once the encoder weights of visiontransformer_amd.synth are
# scaled by MODEL_WS, eps = 100 is of that order, and the seg head scaled by MODEL_HS carries the difference to the logits.
# tests/test_layernorm_cases_cpu.py proves on the oracle that 1e-12 in place of MODEL_EPS at any ONE of the five LayerNorm sites
# moves the logits and the loss gradient by 8 gates of every precision or more.
MODEL_CFG = (2, 16, 128, 2, 2, 64, 256, 2)
MODEL_EPS, MODEL_WS, MODEL_HS, MODEL_SEED = 100.0, 8.0, 3.0, 11
MODEL_SITES = ("layers.0.layernorm_before", "layers.0.layernorm_after", "layers.1.layernorm_before", "layers.1.layernorm_after",
               "layernorm")   # in the order the oracle's forward calls layer_norm
MODEL_TOL = {"fp32": 2e-5, "fp32x3": 2e-5, "fp16": 2e-3, "bf16": 3e-2}   # tests/test_gpu_config_sweep.py TOL (logits, max-abs)
MODEL_LOSS_TOL = {"fp32": 2e-6, "bf16": 5e-3}                             # ... LOSS_TOL
MODEL_GRAD_REL = {"fp32": 2e-4, "bf16": 0.10}                             # tests/util.py grad_check: per-tensor relative L2


def whole_model():
    """cfg (layer_norm_eps = MODEL_EPS), state dict, images, targets of the whole-model eps test"""
    from oracle import vitseg_oracle as O
    from visiontransformer_amd import synth
    from visiontransformer_amd.config import ViTSegConfig
    c = MODEL_CFG
    cfg = ViTSegConfig(*c[:5], image_size=c[5], intermediate_size=c[6], layer_norm_eps=MODEL_EPS)
    sd = {}
    for k, v in synth.make_state_dict(cfg, seed=MODEL_SEED).items():
        scale = 1.0 if "layernorm" in k else MODEL_HS if k.startswith("seg_head") else MODEL_WS
        sd[k] = torch.from_numpy(v) * scale
    x = torch.from_numpy(synth.make_images(cfg, c[7], seed=MODEL_SEED))
    y = O.resize_target(torch.from_numpy(synth.make_targets(cfg, c[7], seed=MODEL_SEED)), (cfg.image_size, cfg.image_size))
    return cfg, sd, x, y


def oracle_step(cfg, sd, x, y, wrong_site=None):
    """fp64 forward + CE loss + autograd of the oracle; wrong_site k: LayerNorm call k (MODEL_SITES) runs with eps 1e-12, the
    others with cfg's.  Returns logits, loss, leaf (parameters with .grad), stages."""
    from oracle import vitseg_oracle as O
    real, calls = O.layer_norm, [0]

    def layer_norm(t, w, b, eps=1e-12):
        k = calls[0]
        calls[0] += 1
        return real(t, w, b, 1e-12 if k == wrong_site else eps)

    leaf = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    stages = {}
    O.layer_norm = layer_norm
    try:
        logits = O.forward(x.double(), leaf, cfg, stages=stages)
    finally:
        O.layer_norm = real
    assert calls[0] == len(MODEL_SITES), calls
    loss = O.ce_loss(logits, y)
    loss.backward()
    return logits.detach(), loss.detach(), leaf, stages
