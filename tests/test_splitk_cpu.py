"""CPU (-m "not gpu"): the slice counts of the K-sliced GEMM paths (csrc/gemm_dispatch.hip, splitk.hip, gemm_p8.hip) as host
arithmetic -- vitseg_dbg_gemm_slices reports what the launches use, no device needed (256 compute units assumed, as an MI355X has).

A slice count fixes the grid, the stride between partials, the reducing kernel's loop and the scratch a caller must bring, so:
the public size queries cover what the launch of the same shape writes; the slices tile the K steps; the workspace sizes that
contain these queries stay what they were; and the shapes tests/test_gpu_splitk.py runs still sit on the count they are named
after."""
import os

import numpy as np
import pytest

import splitk_cases as SC
from visiontransformer_amd import _lib
from visiontransformer_amd.config import ViTSegConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# multiples of 8 up to 1024: of 256 (8-phase kernel), of 128 only, of neither; one either side of a tile edge
DIMS = (8, 64, 120, 128, 136, 192, 256, 264, 384, 512, 576, 768, 1000, 1024)
KS = sorted(set(range(1, 4201)) | {b * t for b in range(1, 65) for t in (197, 1025, 785)})


def _slices(path, M, N, K):
    return _lib.gemm_slices(path, M, N, K)


def _sweep(check):
    bad = []
    for M in DIMS:
        for N in DIMS:
            for K in KS:
                if not check(M, N, K):
                    bad.append((M, N, K))
    return bad


def test_wgrad_bf16_scratch_query_covers_the_launch():
    """vitseg_op_wgrad_bf16_scratch_floats(M, N, K) floats hold the partials of whichever kernel vitseg_op_wgrad_bf16 picks:
    slices * M * N, remainder of K below one 64-row step included (the query used to count whole steps only: (128, 136, 500)
    launches 2 slices, the query sized 1)."""
    q = _lib.lib().vitseg_op_wgrad_bf16_scratch_floats

    def covered(M, N, K):
        tt, p8 = _slices(SC.P_WGRAD_BF16_TT, M, N, K), _slices(SC.P_WGRAD_BF16_P8, M, N, K)
        assert (tt > 0) != (p8 > 0), (M, N, K, tt, p8)       # exactly one kernel takes a valid shape
        return q(M, N, K) >= (tt + p8) * M * N

    bad = _sweep(covered)
    assert not bad, (len(bad), bad[:8])
    with _lib.option("no_p8", 1):   # the switch moves every shape onto the 128x128 kernel: the same scratch must do
        for M, N in ((256, 256), (768, 768), (256, 1024), (1024, 1024), (768, 512)):
            for K in KS:
                assert _slices(SC.P_WGRAD_BF16_P8, M, N, K) == 0
                assert q(M, N, K) >= _slices(SC.P_WGRAD_BF16_TT, M, N, K) * M * N, (M, N, K)


def test_wgrad_f32_scratch_query_covers_the_launch():
    q = _lib.splitk_symbol("vitseg_op_wgrad_f32_scratch_floats")
    bad = _sweep(lambda M, N, K: q(M, N, K) >= _slices(SC.P_WGRAD_F32, M, N, K) * M * N >= M * N)
    assert not bad, (len(bad), bad[:8])


def test_slice_layouts_tile_the_k_steps():
    """The two layouts, restated in splitk_cases.py, over every swept shape: the slices tile [0, ksteps) without overlap; the
    balanced layout (gemm_tile.hip, gemm_tt.hip) gives every slice >= 4 K steps; the 8-phase layout leaves slices empty on some
    shapes (recorded), the headline training batch's 768x768 gradients among them."""
    empty = {}
    for M in DIMS:
        for N in DIMS:
            for K in KS:
                for path, kstep in ((SC.P_WGRAD_F32, 32), (SC.P_WGRAD_BF16_TT, 64)):
                    n, ksteps = _slices(path, M, N, K), SC.ceil_div(K, kstep)
                    if n:
                        lay = SC.balanced_layout(ksteps, n)
                        assert SC.tiles_exactly(lay, ksteps), (path, M, N, K)
                        assert n == 1 or min(b - a for a, b in lay) >= 4, (path, M, N, K, n)
                n = _slices(SC.P_WGRAD_BF16_P8, M, N, K)
                if n:
                    ksteps = SC.ceil_div(K, 64)
                    lay = SC.p8_layout(ksteps, n)
                    assert SC.tiles_exactly(lay, ksteps), (M, N, K)
                    assert n == 1 or ksteps // n >= 8, (M, N, K, n)       # "at least 8 K steps per slice" on average
                    e = SC.empty_slices(lay)
                    if e:
                        empty[(M, N, K)] = e
    for K in KS:   # thin rows and whole-GEMM split: functions of K (and of the tile count) on the balanced layout
        for path, kstep in ((SC.P_THIN_F32, 32), (SC.P_THIN_H16, 64), (SC.P_WHOLE_F32, 32), (SC.P_WHOLE_H16, 64)):
            n = _slices(path, 256, 768, K)
            assert 0 <= n <= (8 if path in (SC.P_WHOLE_F32, SC.P_WHOLE_H16) else 16)
            if n:
                assert K % kstep == 0 and K >= 256
                lay = SC.balanced_layout(K // kstep, n)
                assert SC.tiles_exactly(lay, K // kstep) and min(b - a for a, b in lay) >= 4, (path, K)
    assert empty, "the sweep holds shapes with empty 8-phase slices"
    assert all(e == list(range(e[0], e[0] + len(e))) and e[-1] == _slices(SC.P_WGRAD_BF16_P8, *mnk) - 1 for mnk, e in empty.items())
    assert empty[(768, 768, 64 * 1025)] == [27]           # 1025 steps on 28 slices of 38
    assert (768, 768, 3600) in empty or _slices(SC.P_WGRAD_BF16_P8, 768, 768, 3600) != 28
    print(f"{len(empty)} swept shapes have empty 8-phase slices; up to {max(len(e) for e in empty.values())} of them, e.g. "
          f"{sorted(empty)[:4]}")
    for M, N, K in SC.P8_EMPTY:
        n = _slices(SC.P_WGRAD_BF16_P8, M, N, K)
        assert SC.empty_slices(SC.p8_layout(SC.ceil_div(K, 64), n)), (M, N, K)


def test_gpu_cases_sit_on_the_counts_they_are_named_after():
    for path, cases in ((SC.P_WGRAD_BF16_TT, SC.WGRAD_TT), (SC.P_WGRAD_BF16_P8, SC.WGRAD_P8), (SC.P_WGRAD_F32, SC.WGRAD_F32)):
        for s, M, N, K in cases:
            assert _slices(path, M, N, K) == s, (path, s, M, N, K)
    for s, M, N, K in SC.WGRAD_TT:
        assert _slices(SC.P_WGRAD_BF16_P8, M, N, K) == 0
    with _lib.option("no_p8", 1):
        for s, M, N, K in SC.WGRAD_P8:
            assert _slices(SC.P_WGRAD_BF16_P8, M, N, K) == 0 and _slices(SC.P_WGRAD_BF16_TT, M, N, K) >= 1
    for kstep, path in ((32, SC.P_WHOLE_F32), (64, SC.P_WHOLE_H16)):
        for s, M, N, K, _ in SC.WHOLE[kstep]:
            assert _slices(path, M, N, K) == s, (path, s, M, N, K)
        assert {s for s, *_ in SC.WHOLE[kstep]} >= set(range(4 if kstep == 32 else 2, 9)) | {0}
    for kstep, path in ((32, SC.P_THIN_F32), (64, SC.P_THIN_H16)):
        for s, K in SC.THIN_K[kstep]:
            assert _slices(path, 4100, 768, K) == s, (path, s, K)
    # the counts the issue of this test names for production shapes
    assert _slices(SC.P_WGRAD_BF16_TT, 192, 192, 64 * 197) == 49 and _slices(SC.P_WGRAD_BF16_P8, 768, 768, 65600) == 28
    assert _slices(99, 128, 128, 512) == 0 and _slices(SC.P_WGRAD_F32, 0, 128, 512) == 0


def test_workspace_sizes_are_what_they_were():
    """tests/golden/workspace/workspace.npz (tools/make_golden_workspace.py, written before the bf16 weight-gradient query
    counted a remainder of K as a step): every training and inference workspace size, every precision, unchanged."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "workspace", "workspace.npz"))
    fields = ("num_classes", "patch_size", "hidden_size", "num_hidden_layers", "num_attention_heads", "image_size",
              "intermediate_size", "num_channels")
    assert z["train"].shape == z["query"].shape == (len(z["configs"]), len(z["batches"]), len(z["precisions"]))
    assert z["train"][:160, :, :2].size == 2560 and int((z["train"] > 0).sum()) > 400
    bad = []
    for i, row in enumerate(z["configs"]):
        cfg = ViTSegConfig(**{k: int(v) for k, v in zip(fields, row)})
        for j, b in enumerate(z["batches"]):
            for k, p in enumerate(z["precisions"]):
                for name, fn in (("train", _lib.train_workspace), ("query", _lib.query_workspace)):
                    try:
                        got = fn(cfg, int(b), int(p))
                    except (ValueError, RuntimeError):
                        got = 0
                    if got != int(z[name][i, j, k]):
                        bad.append((name, cfg, int(b), int(p), int(z[name][i, j, k]), got))
    assert not bad, (len(bad), bad[:4])
