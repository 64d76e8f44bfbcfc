"""Attention inputs in which every single key, query and probed dropout bit carries O(1) of a compared output, the fp64
reference they are compared with, and the gates derived from the roundings a kernel is allowed (a plain helper module,
imported like util.py; tests/test_attention_cases_cpu.py proves the designs, tests/test_gpu_attention_keys.py runs the kernels).

Layout: q | k | v rows as the kernels read them -- patch token t of image b in row b Np + t, the CLS token of image b in row
B Np + b, i.e. token index N - 1 = Np of its image ("CLS last").  Every value is exact in bf16 AND in IEEE half, so a 16-bit
kernel sees the numbers the reference sees.  Every design draws its random parts per (image, head): a kernel that takes a
row from the neighbouring head or image reads different numbers.

gather        keys = distinct random +-1 rows, q_i = 8 k_pi(i) for a random permutation pi, v integer rows in [-8, 8], dctx
              integer rows in [-4, 4].  Score of the matched key 64, of any other at most 42: query i puts all but ~1e-10 of
              its weight on key pi(i), every key is the target of exactly one query.
              ctx_i = M v_pi(i),  dv_pi(i) = M dctx_i,  dq = dk = 0,  lse = 64 log2 e   (M = keep / (1 - p) of the pair)
heavy_key     q = 0 (uniform P = 1 / N), k random +-1, v = 1 except v[j*_c, c] = 256 for one heavy key per channel c,
              dctx_i = e_(i mod 64).  ctx_ic = (sum_j M_ij + 255 M_ij*_c) / N: the heavy key is 255 / (N + 255) of channel c.
heavy_query   k = 0, q random +-1, v_j = e_(j mod 64), dctx = 0 except dctx[i*_c, c] = 256 for one heavy query per channel.
              dv_jc = 256 M_(i*_c)j / N: the heavy query is all of column c of dv, and of dk's.
The heavy keys / queries of a pair are the EDGE SET first (tokens 0, 1, N - 2, N - 1 = CLS, and b - 1, b, b + 1 for every
multiple b of 32 below N), filled up with random others; where the set is longer than 64 the pairs of a launch start at
different places of it.

Gates (u = one unit of the last place of the format, twice its rounding error: 2^-8 bf16, 2^-11 half).  The reference returns, next
to each output, the sum of the ABSOLUTE values of its terms; with one relative rounding (<= u) each for P, the dropout scale
and the output,
    |ctx - ref|  <=  3 u  sum_j P~_ij |v_jc|                                   (= 3 u |ref| in the uniform designs: one sign)
    |dv  - ref|  <=  3 u  sum_i P~_ij |dO_ic|
and for dS_ij = P_ij (dP_ij M_ij - delta_i), delta_i = dO_i . O_i taken from the STORED context (the three roundings above
reach it, |d delta_i| <= 3 u Dabs_i, Dabs_i = sum_c |dO_ic| sum_j P~_ij |v_jc|) and dS rounded once more,
    |dq  - ref|  <=  0.125 sum_j (u |dS_ij| + 3 u P_ij Dabs_i) |k_jc|  +  u |ref|
    |dk  - ref|  <=  0.125 sum_i (u |dS_ij| + 3 u P_ij Dabs_i) |q_ic|  +  u |ref|
In the uniform designs (sums of one sign, or one dominant term on a 1 / N background) these are 3 u ... 4 u of the output,
1.6 % for bf16, against the 20 % ... 100 % a lost heavy key or query moves it.
In the gather design nothing but the dropout scale and the output is rounded (P = 1 and the products are small integers),
so ctx and dv keep the 3 u bound on the matched term, plus the reference's own LEAK taken whole: the ~1e-10 of weight a query
puts off its key is below the smallest half and is formed from exponents near 92, where fp32 resolves 7.6e-6, so a kernel owes
no digits of it (slack: the largest off-key weight of a row / column x max |v| / max |dctx| x 1 / (1 - p), about 3e-9).
dq, dk (exact value: 0 but for the ~1e-10 leak) are held to what can be left of dP_i,pi(i) M - delta_i:  both are sums of the same 64 exact products dctx_ic v_pi(i)c, so at p = 0 they differ by the fp32
summation order at most, 64 2^-24 sum_c |dctx v|; at p > 0 the scale M is applied to the sum on one side and, rounded with the
stored context (two roundings of the format, four of fp32), to every term on the other: (2 u + 4 2^-24) M sum_c |dctx v| more.
    |dq_i|, |dk_pi(i)|  <=  (1 + u) 0.125 max|k|, max|q| (64 2^-24 + [p > 0] (2 u + 4 2^-24)) M sum_c |dctx_ic v_pi(i)c|
                            + the leak's own terms taken whole, 0.125 sum_j |dS_ij| |k_jc|
(the factor 1 + u: the residue itself is rounded to the output format).
fp32 entries are the control of the designs: u = 0 in the design-specific terms, and the project's fp32 gate 2e-5 relative to the
same sums of absolute values in place of 3 u / 4 u (fp32 accumulation over up to 1025 keys, exp2 and the log-sum-exp's last bit).
"""
import math
from functools import lru_cache

import torch

LOG2E = 1.4426950408889634
U = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11, "fp32": 0.0}
F32_GATE = 2e-5            # tests/test_gpu_small.py test_attention_small_forward_and_backward_for_training
# log-sum-exp (fp32, log2 domain): that test's 2e-5 holds in the uniform designs (lse = log2 N <= 10; measured on an MI355X
# 6.0e-7 at worst, where a lost key is >= 1.4e-3).  In the gather design lse = 92.3, where fp32 resolves 7.6e-6 and the fp32
# kernels reach it through a 64-step fp32 chain: measured 2.93e-5 (vitseg_op_attention_bwd_f32), 2.17e-5 (..._f32_small),
# 1.23e-6 (..._bwd_bf16), with the uniform designs ruling out a lost key -> 4 x the measured 2.93e-5.
LSE_GATE = {"gather": 1.17e-4, "heavy_key": 2e-5, "heavy_query": 2e-5}
DROP_SEED, DROP_LAYER = 0xBEEF1234, 3   # tests/test_gpu_backward.py test_attention_backward_bf16: stream id 3 * 8 + 1

# (B, Np, A): either side of the 32 / 128 / 256 blockings; the short-sequence kernels end at N = 400
SHAPES = [(1, 4, 1), (2, 31, 2), (3, 127, 1), (1, 129, 3), (2, 196, 3), (2, 255, 2), (1, 257, 1), (1, 1024, 2)]
SHAPES_SHORT = SHAPES[:6] + [(2, 200, 3), (1, 399, 1)]
ALL_SHAPES = SHAPES + SHAPES_SHORT[6:]
DESIGNS = ("gather", "heavy_key", "heavy_query")


def edge_set(N):
    """tokens a blocked kernel is most likely to lose: both ends (N - 1 is the CLS token) and either side of every 32"""
    e = [0, 1, N - 2, N - 1]
    for b in range(32, N, 32):
        e += [b - 1, b, b + 1]
    return sorted({t for t in e if 0 <= t < N})


def token_rows(B, Np, b):
    """rows of image b's N tokens in kernel order (CLS last)"""
    return list(range(b * Np, (b + 1) * Np)) + [B * Np + b]


class Case:
    """qkv [Mt, 3 D], dctx [Mt, D] (fp32 tensors of exactly representable values) + what the design knows about itself:
    perm [B, A, N] (gather: the key of query i) or heavy [B, A, 64] (the heavy key / query of channel c)."""

    def __init__(self, design, B, Np, A):
        self.design, self.B, self.Np, self.A = design, B, Np, A
        self.N, self.D, self.Mt = Np + 1, 64 * A, B * Np + B
        self.qkv = torch.zeros(self.Mt, 3 * self.D)
        self.dctx = torch.zeros(self.Mt, self.D)
        self.perm = self.heavy = None

    def put(self, b, h, part, x):   # part 0 / 1 / 2 = q / k / v, 3 = dctx; x [N, 64]
        rows = token_rows(self.B, self.Np, b)
        if part == 3:
            self.dctx[rows, 64 * h:64 * h + 64] = x
        else:
            self.qkv[rows, part * self.D + 64 * h:part * self.D + 64 * h + 64] = x

    def get(self, b, h, part):
        rows = token_rows(self.B, self.Np, b)
        if part == 3:
            return self.dctx[rows, 64 * h:64 * h + 64].double()
        return self.qkv[rows, part * self.D + 64 * h:part * self.D + 64 * h + 64].double()


def _signs(g, n):
    return (torch.randint(0, 2, (n, 64), generator=g) * 2 - 1).float()


def _distinct_keys(g, N):
    """N random +-1 rows whose pairwise dot products stay at or below 42 (so the matched score leads by >= 22)"""
    k = _signs(g, N)
    for _ in range(64):
        gram = k @ k.T - 64.0 * torch.eye(N)
        bad = (torch.triu(gram, 1) > 42).any(dim=0).nonzero().flatten()
        if not len(bad):
            return k
        k[bad] = _signs(g, len(bad))
    raise AssertionError("no well-separated keys: change the seed")


def _heavy_tokens(g, N, start):
    """64 tokens, one per channel: the edge set from `start` on in a random order, then random others, cycled if N < 64"""
    e = edge_set(N)
    e = e[start % len(e):] + e[:start % len(e)]
    head = e[:64]
    head = [head[i] for i in torch.randperm(len(head), generator=g).tolist()]
    rest = [t for t in range(N) if t not in set(head)]
    rest = [rest[i] for i in torch.randperm(len(rest), generator=g).tolist()]
    lst = (head + rest)[:64]
    return torch.tensor([lst[c % len(lst)] for c in range(64)])


@lru_cache(maxsize=None)
def make_case(design, B, Np, A):
    c = Case(design, B, Np, A)
    N = c.N
    g = torch.Generator().manual_seed(1000 * DESIGNS.index(design) + 7 * Np + 3 * A + B)
    if design == "gather":
        c.perm = torch.zeros(B, A, N, dtype=torch.long)
    else:
        c.heavy = torch.zeros(B, A, 64, dtype=torch.long)
    for b in range(B):
        for h in range(A):
            if design == "gather":
                k = _distinct_keys(g, N)
                pi = torch.randperm(N, generator=g)
                c.perm[b, h] = pi
                c.put(b, h, 0, 8.0 * k[pi])
                c.put(b, h, 1, k)
                c.put(b, h, 2, torch.randint(-8, 9, (N, 64), generator=g).float())
                c.put(b, h, 3, torch.randint(-4, 5, (N, 64), generator=g).float())
                continue
            hv = _heavy_tokens(g, N, 64 * (b * A + h))
            c.heavy[b, h] = hv
            ch = torch.arange(64)
            if design == "heavy_key":
                c.put(b, h, 1, _signs(g, N))
                v = torch.ones(N, 64)
                v[hv, ch] = 256.0
                c.put(b, h, 2, v)
                c.put(b, h, 3, torch.eye(64)[torch.arange(N) % 64])
            else:
                c.put(b, h, 0, _signs(g, N))
                c.put(b, h, 2, torch.eye(64)[torch.arange(N) % 64])
                do = torch.zeros(N, 64)
                do[hv, ch] = 256.0
                c.put(b, h, 3, do)
    return c


@lru_cache(maxsize=None)
def kernel_masks(p, B, Np, A):
    """dropout factors keep / (1 - p) of the kernels' counter-based generator, fp64 [B, A, N, N] in KERNEL token order"""
    from dropout_ref import Masks
    N = Np + 1
    m = Masks(p, DROP_SEED, B, Np, A).attn(DROP_LAYER, (B, A, N, N)).double()   # reference order: CLS first
    idx = torch.cat([torch.arange(1, N), torch.tensor([0])])
    return m[:, :, idx][:, :, :, idx].contiguous()


OUTPUTS = ("ctx", "dq", "dk", "dv")


def pair_reference(q, k, v, do, mask=None, with_abs=True):
    """fp64 attention of one (image, head): q, do [Nq, 64], k, v [Nk, 64], mask [Nq, Nk] (dropout factors) or None.
    ctx, lse (log2 domain) and the autograd gradients of sum(ctx * do); `abs`: the sums of absolute values the gates need."""
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    sc = q @ k.T * 0.125
    P = torch.softmax(sc, dim=-1)
    Pm = P if mask is None else P * mask
    o = Pm @ v
    (o * do).sum().backward()
    if not with_abs:
        return dict(ctx=o.detach(), lse=torch.logsumexp(sc.detach(), dim=-1) * LOG2E, dq=q.grad, dk=k.grad, dv=v.grad)
    with torch.no_grad():
        oabs = Pm @ v.abs()
        dS = P * ((do @ v.T) * (1.0 if mask is None else mask) - (do * o).sum(-1, keepdim=True))
        pd = P * (do.abs() * oabs).sum(-1, keepdim=True)
        out = dict(ctx=o.detach(), lse=torch.logsumexp(sc, dim=-1) * LOG2E, dq=q.grad, dk=k.grad, dv=v.grad,
                   abs=dict(ctx=oabs, dv=Pm.T @ do.abs(),
                            dq1=0.125 * dS.abs() @ k.abs(), dq2=0.125 * pd @ k.abs(),
                            dk1=0.125 * dS.abs().T @ q.abs(), dk2=0.125 * pd.T @ q.abs()))
    return out


def mutated_pair(case, b, h, mask, mutate=None):
    """pair_reference of pair (b, h) as a kernel with ONE fault would compute it; every output keeps its full [N, 64] shape
    (lse: [N]).  In the gather design a key read TWICE leaves ctx and the gradients as they are (two halves of the same row)
    and shows in lse alone, which moves by exactly 1; the heavy_key design shows it in ctx.
    mutate = (kind, token[, key]): "delete_key" (the key is never read), "dup_key" (read twice), "neighbour_key" (k and v rows
    taken from the next head, or the next image where there is one head), "delete_query" (its ctx row stays 0, it adds
    nothing to dk / dv), "flip_bit" (the dropout bit of (query token, key))."""
    N = case.N
    q, k, v, do = (case.get(b, h, part) for part in range(4))
    m = None if mask is None else mask.clone()
    qi, ki = list(range(N)), list(range(N))
    if mutate is not None:
        kind, t = mutate[0], mutate[1]
        if kind == "delete_key":
            ki.remove(t)
        elif kind == "dup_key":
            ki.append(t)
        elif kind == "neighbour_key":
            b2, h2 = (b, (h + 1) % case.A) if case.A > 1 else ((b + 1) % case.B, h)
            assert (b2, h2) != (b, h), "no neighbour"
            k[t], v[t] = case.get(b2, h2, 1)[t], case.get(b2, h2, 2)[t]
        elif kind == "delete_query":
            qi.remove(t)
        elif kind == "flip_bit":
            m[t, mutate[2]] = m.max() - m[t, mutate[2]]
        else:
            raise ValueError(kind)
    r = pair_reference(q[qi], k[ki], v[ki], do[qi], None if m is None else m[qi][:, ki], with_abs=False)
    out = {}
    for name, idx in (("ctx", qi), ("dq", qi), ("dk", ki), ("dv", ki)):
        full = torch.zeros(N, 64, dtype=torch.float64)
        full.index_add_(0, torch.tensor(idx), r[name])   # a key read twice collects both gradients
        out[name] = full
    out["lse"] = torch.full((N,), math.nan, dtype=torch.float64)   # a lost query has none
    out["lse"][qi] = r["lse"]
    return out


class Reference:
    """The whole launch: ctx [Mt, D], lse [B, A, N] (kernel order), dqkv [Mt, 3 D], and `abs` in the same shapes."""

    def __init__(self, case, p=0.0):
        c = self.case = case
        self.p = p
        self.mask = kernel_masks(p, c.B, c.Np, c.A) if p else None
        self.ctx = torch.zeros(c.Mt, c.D, dtype=torch.float64)
        self.dqkv = torch.zeros(c.Mt, 3 * c.D, dtype=torch.float64)
        self.lse = torch.zeros(c.B, c.A, c.N, dtype=torch.float64)
        self.abs = {k: torch.zeros(c.Mt, c.D, dtype=torch.float64) for k in ("ctx", "dv", "dq1", "dq2", "dk1", "dk2")}
        self.offtarget = 0.0     # gather: the largest weight a query puts anywhere but on its key (before dropout)
        self.offtarget_col = 0.0  # ... and the largest weight a key collects from the queries that are not its own
        self.margin = math.inf   # gather: the smallest lead of the matched score
        for b in range(c.B):
            rows = token_rows(c.B, c.Np, b)
            for h in range(c.A):
                sl = slice(64 * h, 64 * h + 64)
                r = pair_reference(*(c.get(b, h, part) for part in range(4)), None if self.mask is None else self.mask[b, h])
                self.ctx[rows, sl] = r["ctx"]
                self.lse[b, h] = r["lse"]
                for i, name in enumerate(("dq", "dk", "dv")):
                    self.dqkv[rows, i * c.D + 64 * h:i * c.D + 64 * h + 64] = r[name]
                for name, val in r["abs"].items():
                    self.abs[name][rows, sl] = val
                if c.design == "gather":
                    q, k = c.get(b, h, 0), c.get(b, h, 1)
                    sc = q @ k.T * 0.125
                    on = torch.zeros(c.N, c.N, dtype=torch.bool)
                    on[torch.arange(c.N), c.perm[b, h]] = True
                    self.margin = min(self.margin, float((sc[on][:, None] - sc.masked_fill(on, -math.inf)).min()))
                    off = torch.softmax(sc, -1).masked_fill(on, 0.0)
                    self.offtarget = max(self.offtarget, float(off.sum(-1).max()))
                    self.offtarget_col = max(self.offtarget_col, float(off.sum(0).max()))

    def part(self, name):
        D = self.case.D
        return self.ctx if name == "ctx" else self.dqkv[:, ("dq", "dk", "dv").index(name) * D:][:, :D]

    def gates(self, fmt):
        """elementwise gates [Mt, D] of ctx, dq, dk, dv for an entry whose 16-bit format is `fmt` ("fp32": the control)"""
        u, ab = U[fmt], self.abs
        r3, r1 = (3 * u, u) if u else (F32_GATE, F32_GATE)
        g = {"ctx": r3 * ab["ctx"], "dv": r3 * ab["dv"]}
        if self.case.design == "gather":
            c, m = self.case, 1.0 / (1.0 - self.p)
            g["ctx"] = g["ctx"] + self.offtarget * float(c.qkv[:, 2 * c.D:].abs().max()) * m
            g["dv"] = g["dv"] + self.offtarget_col * float(c.dctx.abs().max()) * m
            z = (1 + u) * (64 * 2.0 ** -24 + ((2 * u + 4 * 2.0 ** -24) if self.p else 0.0))
            g["dq"] = z * ab["dq2"] + ab["dq1"]
            g["dk"] = z * ab["dk2"] + ab["dk1"]
        else:
            g["dq"] = r1 * ab["dq1"] + r3 * ab["dq2"] + r1 * self.part("dq").abs()
            g["dk"] = r1 * ab["dk1"] + r3 * ab["dk2"] + r1 * self.part("dk").abs()
        return g


@lru_cache(maxsize=None)
def reference(design, B, Np, A, p=0.0):
    return Reference(make_case(design, B, Np, A), p)


def worst_ratio(got, ref, gate):
    """max |got - ref| / gate over the elements (an element with gate 0 must be exact)"""
    err = (got.double() - ref).abs()
    assert torch.isfinite(err).all(), "non-finite output"
    ratio = torch.where(gate > 0, err / gate.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return float(ratio.max())
