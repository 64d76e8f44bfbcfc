"""CPU: the attention designs of tests/attention_cases.py proved on the fp64 reference alone, at every shape of
tests/test_gpu_attention_keys.py -- the values are exact in both 16-bit formats, the preconditions of the gather design hold,
the reference gives the closed-form answers, and a kernel with ONE fault (a key lost, read twice or taken from the neighbouring
head, a query lost, a dropout bit flipped) would move a compared output by at least 8 x its widest (bf16) gate."""
import math

import pytest
import torch

import attention_cases as AC

P_DROP = 0.25
NEED = 8.0          # a single fault must show at this many times the gate
RANDOM_OTHERS = 32  # subjects per shape besides the whole edge set


def _ids(shapes):
    return [f"B{b}-Np{n}-A{a}" for b, n, a in shapes]


@pytest.mark.parametrize("design", AC.DESIGNS)
@pytest.mark.parametrize("B,Np,A", AC.ALL_SHAPES, ids=_ids(AC.ALL_SHAPES))
def test_values_are_exact_in_both_16bit_formats(design, B, Np, A):
    c = AC.make_case(design, B, Np, A)
    for t in (c.qkv, c.dctx):
        assert torch.equal(t.to(torch.bfloat16).float(), t) and torch.equal(t.to(torch.float16).float(), t)
    assert c.qkv.shape == (B * Np + B, 3 * 64 * A) and c.dctx.shape == (B * Np + B, 64 * A)


@pytest.mark.parametrize("B,Np,A", AC.ALL_SHAPES, ids=_ids(AC.ALL_SHAPES))
def test_gather_preconditions_and_closed_form(B, Np, A):
    c = AC.make_case("gather", B, Np, A)
    N = c.N
    for p in (0.0, P_DROP):
        ref = AC.reference("gather", B, Np, A, p)
        assert ref.margin >= 16.0, ref.margin          # the design gives >= 22
        assert ref.offtarget < 1e-8, ref.offtarget     # ... and < 3e-10
        assert (ref.lse - 64 * AC.LOG2E).abs().max().item() < 1e-8
        for b in range(B):
            for h in range(A):
                k, v, do, pi = c.get(b, h, 1), c.get(b, h, 2), c.get(b, h, 3), c.perm[b, h]
                assert len({tuple(r) for r in k.tolist()}) == N, "keys are not distinct"
                assert sorted(pi.tolist()) == list(range(N))
                assert torch.equal(c.get(b, h, 0), 8 * k[pi])
                # the kept / dropped pattern is read off all-zero rows: no v or dctx row may be zero by itself
                assert bool(v.abs().sum(-1).min() > 0) and bool(do.abs().sum(-1).min() > 0)
                m = torch.ones(N, dtype=torch.float64) if not p else ref.mask[b, h][torch.arange(N), pi]
                rows = AC.token_rows(B, Np, b)
                sl = slice(64 * h, 64 * h + 64)
                want_dv = torch.zeros(N, 64, dtype=torch.float64)
                want_dv[pi] = m[:, None] * do
                tiny = 1e-8 * 8 / (1 - p)
                assert (ref.ctx[rows, sl] - m[:, None] * v[pi]).abs().max().item() < tiny
                assert (ref.part("dv")[rows, sl] - want_dv).abs().max().item() < tiny
                assert ref.part("dq")[rows, sl].abs().max().item() < 1e-4 and ref.part("dk")[rows, sl].abs().max().item() < 1e-4
        if p:
            on = torch.stack([torch.stack([ref.mask[b, h][torch.arange(N), c.perm[b, h]] for h in range(A)]) for b in range(B)])
            assert set(on.unique().tolist()) <= {0.0, float(ref.mask.max())}
            if N > 30:
                assert 0 < int((on == 0).sum()) < on.numel()   # both kinds of row are there to be told apart


@pytest.mark.parametrize("design", ["heavy_key", "heavy_query"])
@pytest.mark.parametrize("B,Np,A", AC.ALL_SHAPES, ids=_ids(AC.ALL_SHAPES))
def test_uniform_designs_closed_form_and_edge_cover(design, B, Np, A):
    c = AC.make_case(design, B, Np, A)
    N = c.N
    ref = AC.reference(design, B, Np, A, 0.0)
    assert (ref.lse - math.log2(N)).abs().max().item() < 1e-12
    heavy_somewhere = set(c.heavy.flatten().tolist())
    assert set(AC.edge_set(N)) <= heavy_somewhere, sorted(set(AC.edge_set(N)) - heavy_somewhere)
    assert N - 1 in AC.edge_set(N)   # the CLS token
    for b in range(B):
        rows = AC.token_rows(B, Np, b)
        for h in range(A):
            sl, hv, ch = slice(64 * h, 64 * h + 64), c.heavy[b, h], torch.arange(64)
            if N >= 64:
                assert len(set(hv.tolist())) == 64
            if design == "heavy_key":
                v = c.get(b, h, 2)
                assert torch.equal(v[hv, ch], torch.full((64,), 256.0, dtype=torch.float64)) and int((v == 256).sum()) == 64
                assert (ref.ctx[rows, sl] - (N + 255.0) / N).abs().max().item() < 1e-12
            else:
                do = c.get(b, h, 3)
                assert int((do != 0).sum()) == 64
                want = torch.zeros(N, 64, dtype=torch.float64)
                want[:, ch] = 256.0 / N                    # dv_jc = P (1 / N) x the heavy query's 256, for EVERY key j
                assert (ref.part("dv")[rows, sl] - want).abs().max().item() < 1e-12
    # the gates of the uniform designs stay a few per cent of the output (bf16: at most 4 u = 1.6 %)
    g = ref.gates("bf16")
    for name in ("ctx", "dv"):
        refp = ref.part(name).abs()
        nz = refp > 0
        assert float((g[name][nz] / refp[nz]).max()) <= 4 * AC.U["bf16"] + 1e-12


def _subjects(N, seed):
    edge = AC.edge_set(N)
    rest = [t for t in range(N) if t not in set(edge)]
    g = torch.Generator().manual_seed(seed)
    pick = [rest[i] for i in torch.randperm(len(rest), generator=g)[:RANDOM_OTHERS].tolist()]
    return edge + pick


def _moved(case, ref, b, h, mutate, gates):
    """largest |mutated - base| / gate over the compared outputs of pair (b, h)"""
    rows, sl = AC.token_rows(case.B, case.Np, b), slice(64 * h, 64 * h + 64)
    mut = AC.mutated_pair(case, b, h, None if ref.mask is None else ref.mask[b, h], mutate)
    worst = 0.0
    for name in AC.OUTPUTS:
        worst = max(worst, AC.worst_ratio(mut[name], ref.part(name)[rows, sl], gates[name][rows, sl]))
    have = ~torch.isnan(mut["lse"])
    return max(worst, float((mut["lse"] - ref.lse[b, h])[have].abs().max()) / AC.LSE_GATE[case.design])


@pytest.mark.parametrize("B,Np,A", AC.ALL_SHAPES, ids=_ids(AC.ALL_SHAPES))
def test_gather_single_faults_show(B, Np, A):
    """every key and every query (the whole edge set + 32 others where N is larger) is lost, doubled, swapped with the
    neighbour's once; the dropout bit of every such query's own key is flipped once.  (A key read twice shows in lse alone,
    which moves by 1: the two halves of the weight meet the same value row.  The heavy_key design shows it in ctx.)"""
    c = AC.make_case("gather", B, Np, A)
    ref0, refp = AC.reference("gather", B, Np, A, 0.0), AC.reference("gather", B, Np, A, P_DROP)
    g0, gp = ref0.gates("bf16"), refp.gates("bf16")
    kinds = ["delete_key", "dup_key", "delete_query"] + (["neighbour_key"] if B * A > 1 else [])
    for n, t in enumerate(_subjects(c.N, Np)):
        b, h = divmod(n % (B * A), A)
        for kind in kinds:
            assert _moved(c, ref0, b, h, (kind, t), g0) >= NEED, (kind, t, b, h)
        assert _moved(c, refp, b, h, ("flip_bit", t, int(c.perm[b, h, t])), gp) >= NEED, ("flip_bit", t, b, h)
    # the unmutated pair is its own reference
    assert _moved(c, ref0, 0, 0, None, g0) == 0.0


@pytest.mark.parametrize("B,Np,A", AC.ALL_SHAPES, ids=_ids(AC.ALL_SHAPES))
def test_uniform_single_faults_show(B, Np, A):
    """every heavy key (heavy_key) and heavy query (heavy_query) among the edge set + 32 others: lost, doubled, swapped / lost;
    a dropout bit (random query, heavy key) flipped"""
    ck, cq = AC.make_case("heavy_key", B, Np, A), AC.make_case("heavy_query", B, Np, A)
    rk0, rkp, rq0 = (AC.reference("heavy_key", B, Np, A, 0.0), AC.reference("heavy_key", B, Np, A, P_DROP),
                     AC.reference("heavy_query", B, Np, A, 0.0))
    gk0, gkp, gq0 = rk0.gates("bf16"), rkp.gates("bf16"), rq0.gates("bf16")
    gen = torch.Generator().manual_seed(Np)
    tested_k, tested_q = set(), set()
    for t in _subjects(ck.N, Np + 1):
        for case, tested in ((ck, tested_k), (cq, tested_q)):
            pairs = [(b, h) for b in range(B) for h in range(A) if t in case.heavy[b, h].tolist()]
            if not pairs:
                continue                 # a random other that is heavy nowhere: not a probe of this design
            b, h = pairs[0]
            tested.add(t)
            if case is ck:
                for kind in ["delete_key", "dup_key"] + (["neighbour_key"] if B * A > 1 else []):
                    assert _moved(ck, rk0, b, h, (kind, t), gk0) >= NEED, (kind, t, b, h)
                i = int(torch.randint(0, ck.N, (1,), generator=gen))
                assert _moved(ck, rkp, b, h, ("flip_bit", i, t), gkp) >= NEED, ("flip_bit", i, t, b, h)
            else:
                assert _moved(cq, rq0, b, h, ("delete_query", t), gq0) >= NEED, ("delete_query", t, b, h)
    assert set(AC.edge_set(ck.N)) <= tested_k and set(AC.edge_set(cq.N)) <= tested_q


def test_deleting_a_heavy_token_at_N_130():
    """the figures the designs were chosen by: at N = 130 a lost heavy key takes 66 % of its channel of the context, a lost
    heavy query all of its column of dv"""
    B, Np, A = 1, 129, 3
    ck, cq = AC.make_case("heavy_key", B, Np, A), AC.make_case("heavy_query", B, Np, A)
    rows = AC.token_rows(B, Np, 0)
    t = int(ck.heavy[0, 0, 5])
    mut = AC.mutated_pair(ck, 0, 0, None, ("delete_key", t))
    base = AC.reference("heavy_key", B, Np, A).ctx[rows, 0:64]
    ch = (ck.heavy[0, 0] == t).nonzero().flatten()
    rel = ((mut["ctx"] - base).abs() / base)[:, ch]
    assert 0.6 < float(rel.min()) and float(rel.max()) < 0.7, (float(rel.min()), float(rel.max()))
    t = int(cq.heavy[0, 0, 5])
    mut = AC.mutated_pair(cq, 0, 0, None, ("delete_query", t))
    base = AC.reference("heavy_query", B, Np, A).part("dv")[rows, 0:64]
    ch = (cq.heavy[0, 0] == t).nonzero().flatten()
    assert float(mut["dv"][:, ch].abs().max()) == 0.0 and float(base[:, ch].min()) > 1.9
