"""CPU (-m "not gpu"): the shape domain of the workspace queries.  Every config that `check_config` (csrc/plan.hpp)
accepts must be refused by `vitseg_query_workspace` / `vitseg_train_workspace` exactly when a documented per-precision or
training limit says so (include/vitseg.h), and accepted otherwise.  A query that says OK for a config
the launches cannot run hands the caller a partial launch sequence later (16-bit GEMMs step K in 64-value slices: before
the query checked it, I = 224 passed the bf16 query and failed at layer 0's fc2)."""
import ctypes as C
import random

import pytest

from visiontransformer_amd import _lib
from visiontransformer_amd.config import ViTSegConfig

PRECISIONS = (_lib.F32, _lib.BF16, _lib.F16, _lib.F32X3)


def _rejected_infer(cfg, precision):
    return precision in (_lib.BF16, _lib.F16) and cfg.intermediate_size % 64 != 0


def _rejected_train(cfg, precision):
    return (_rejected_infer(cfg, precision) or cfg.num_classes > 32 or cfg.hidden_size > 1024)


def _grid(n, seed):
    """n configs inside check_config's domain: P any multiple of 4, S = g * P with g from 1 (S = P) up, I any multiple of
    4 (also <= D), C in [1, 255], D = 64 * A up to 2048.  The corners are always in."""
    rng = random.Random(seed)
    out = [(1, 4, 1, 1, 4, 1), (255, 32, 32, 2, 4, 2), (33, 16, 17, 1, 2048 + 4, 1), (32, 16, 16, 1, 1024 + 64, 3),
           (2, 16, 16, 4, 224, 2), (2, 12, 2, 8, 100, 1), (150, 16, 4, 32, 2304, 1)]
    while len(out) < n:
        C = rng.choice([1, 2, 3, 17, 32, 33, 150, 255])
        P = 4 * rng.randint(1, 8)
        A = rng.randint(1, 32)
        g = rng.randint(1, 16)
        I = 4 * rng.randint(1, 1024)
        B = rng.randint(1, 8)
        out.append((C, P, A, g, I, B))
    return [(ViTSegConfig(C, P, 64 * A, 1, A, image_size=g * P, intermediate_size=I), B) for C, P, A, g, I, B in out]


CASES = _grid(160, seed=2026)


@pytest.mark.parametrize("k", range(0, len(CASES), 16))
def test_query_workspace_rejects_exactly_the_documented_configs(k):
    for cfg, B in CASES[k:k + 16]:
        assert _lib.param_count(cfg) > 0          # inside check_config's domain
        for precision in PRECISIONS:
            if _rejected_infer(cfg, precision):
                with pytest.raises(ValueError, match="intermediate_size"):
                    _lib.query_workspace(cfg, B, precision)
            else:
                assert _lib.query_workspace(cfg, B, precision) > 0, (cfg, B, precision)


@pytest.mark.parametrize("k", range(0, len(CASES), 16))
def test_train_workspace_rejects_exactly_the_documented_configs(k):
    for cfg, B in CASES[k:k + 16]:
        for precision in (_lib.F32, _lib.BF16):
            if _rejected_train(cfg, precision):
                with pytest.raises(ValueError):
                    _lib.train_workspace(cfg, B, precision)
            else:
                assert _lib.train_workspace(cfg, B, precision) > 0, (cfg, B, precision)
        for precision in (_lib.F16, _lib.F32X3):    # inference formats: EINVAL, not a shape error
            with pytest.raises(RuntimeError, match="training runs in"):
                _lib.train_workspace(cfg, B, precision)


def test_other_input_sizes_apply_the_same_limits():
    """The `_at` queries (interpolated position embeddings) check the limits on the input's derived config."""
    for cfg, B in CASES[:48]:
        for scale in (1, 2):
            size = cfg.image_size * scale
            for precision in PRECISIONS:
                if _rejected_infer(cfg, precision):
                    with pytest.raises(ValueError):
                        _lib.query_workspace(cfg, B, precision, image_size=size)
                else:
                    assert _lib.query_workspace(cfg, B, precision, image_size=size) > 0
            for precision in (_lib.F32, _lib.BF16):
                if _rejected_train(cfg, precision):
                    with pytest.raises(ValueError):
                        _lib.train_workspace(cfg, B, precision, image_size=size)
                else:
                    assert _lib.train_workspace(cfg, B, precision, image_size=size) > 0


def test_limit_edges():
    """Each limit on both sides of its edge."""
    def cfg(C=2, A=2, I=256):
        return ViTSegConfig(C, 16, 64 * A, 1, A, image_size=64, intermediate_size=I)
    for I, ok16 in ((192, True), (196, False), (224, False), (256, True), (100, False), (64, True), (4, False)):
        for precision in (_lib.BF16, _lib.F16):
            if ok16:
                assert _lib.query_workspace(cfg(I=I), 2, precision) > 0
                assert precision == _lib.F16 or _lib.train_workspace(cfg(I=I), 2, precision) > 0
            else:
                with pytest.raises(ValueError, match="multiple of 64"):
                    _lib.query_workspace(cfg(I=I), 2, precision)
        assert _lib.query_workspace(cfg(I=I), 2, _lib.F32) > 0 and _lib.train_workspace(cfg(I=I), 2, _lib.F32) > 0
    assert _lib.train_workspace(cfg(C=32), 1, _lib.F32) > 0
    with pytest.raises(ValueError, match="32 classes"):
        _lib.train_workspace(cfg(C=33), 1, _lib.F32)
    assert _lib.train_workspace(cfg(A=16, I=4096), 1, _lib.BF16) > 0
    with pytest.raises(ValueError, match="hidden_size <= 1024"):
        _lib.train_workspace(cfg(A=17, I=4096), 1, _lib.BF16)
    assert _lib.query_workspace(cfg(C=255, A=32, I=8192), 1, _lib.BF16) > 0   # inference keeps the whole domain


def test_layer_norm_eps_domain():
    """`check_config` takes any finite eps >= 0 (0 as torch.nn.LayerNorm does, -0.0 is 0) and refuses a NaN, an infinite or a
    negative one with VITSEG_EINVAL -- in every query that checks a config, before anything is sized or launched."""
    import dataclasses
    import math
    base = ViTSegConfig(2, 16, 128, 2, 2, image_size=64, intermediate_size=256)
    for eps in (0.0, -0.0, 1e-45, 1e-12, 1e-6, 1e-5, 1.0, 100.0, 3.0e38):
        cfg = dataclasses.replace(base, layer_norm_eps=eps)
        assert _lib.param_count(cfg) == _lib.param_count(base)
        assert _lib.query_workspace(cfg, 2, _lib.BF16) == _lib.query_workspace(base, 2, _lib.BF16)
        assert _lib.train_workspace(cfg, 2, _lib.F32) == _lib.train_workspace(base, 2, _lib.F32)
    for eps in (math.nan, math.inf, -math.inf, -1e-45, -1e-12, -1.0):
        cfg = dataclasses.replace(base, layer_norm_eps=eps)
        for query in (lambda: _lib.param_count(cfg), lambda: _lib.query_workspace(cfg, 2, _lib.F32),
                      lambda: _lib.query_workspace(cfg, 2, _lib.F16, image_size=128), lambda: _lib.train_workspace(cfg, 2, _lib.BF16)):
            with pytest.raises(RuntimeError, match="layer_norm_eps"):
                query()
        c = _lib.CConfig.from_config(cfg)
        n = C.c_size_t(0)
        assert _lib.lib().vitseg_param_count(C.byref(c), C.byref(n)) == _lib.EINVAL


@pytest.mark.parametrize("precision", [_lib.F32, _lib.BF16])
def test_backward_refuses_bad_loss_arguments_before_any_launch(precision):
    """`vitseg_backward` needs exactly one of `target` (fused CE) and `grad_logits`, and `loss` with `target`.  Both
    precisions refuse a violation with VITSEG_EINVAL before anything reaches the device, so fake non-null pointers and a
    large enough workspace size exercise the checks here."""
    cfg = ViTSegConfig(2, 16, 128, 1, 2, image_size=64, intermediate_size=256)
    B = 1
    ws_bytes = _lib.train_workspace(cfg, B, precision)
    c = _lib.CConfig.from_config(cfg)
    fake = C.c_void_p(1 << 20)
    L = _lib.lib()
    for target, grad_logits, loss in ((None, None, None), (fake, None, None)):
        rc = L.vitseg_backward(C.byref(c), fake, fake, fake, B, precision, 0.0, 0, target, 0, grad_logits, fake, loss, 1.0,
                               None, fake, ws_bytes, None)
        assert rc == _lib.EINVAL, (rc, L.vitseg_last_error())
        msg = L.vitseg_last_error().decode()
        assert ("exactly one of target" in msg) if target is None else ("loss output pointer" in msg), msg
