"""The K-sliced GEMM paths (csrc/gemm_dispatch.hip): plain Python restatements of the two slice layouts and the shapes of
tests/test_gpu_splitk.py, each named after the slice count it is there for (a plain helper module, imported like util.py).

tests/test_splitk_cpu.py checks the restatements' contract and that every listed case still gets its count from the router
(vitseg_dbg_gemm_slices, host arithmetic at 256 compute units); the GPU test checks the kernels against fp64.
"""

# enum vitseg_slices_path (include/vitseg.h)
P_WHOLE_F32, P_WHOLE_H16, P_THIN_F32, P_THIN_H16, P_WGRAD_F32, P_WGRAD_BF16_TT, P_WGRAD_BF16_P8 = range(7)


def ceil_div(a, b):
    return -(-a // b)


def balanced_layout(ksteps, n):
    """gemm_tile.hip / gemm_tt.hip: slice s of n walks the K steps [ksteps * s / n, ksteps * (s + 1) / n)."""
    return [(ksteps * s // n, ksteps * (s + 1) // n) for s in range(n)]


def p8_layout(ksteps, n):
    """gemm_p8.hip, T-form: every slice walks an EVEN number of K steps, ceil(ksteps / n) rounded up; slice s starts at
    s * that and ends at ksteps at the latest (token rows beyond K read as zeros).  A slice that starts at or past ksteps
    is empty: it must still store a zero partial."""
    per = (ceil_div(ksteps, n) + 1) & ~1
    return [(min(s * per, ksteps), min((s + 1) * per, ksteps)) for s in range(n)]


def tiles_exactly(layout, ksteps):
    """the slices cover [0, ksteps) in order, without gap or overlap"""
    pos = 0
    for a, b in layout:
        if a != pos or b < a:
            return False
        pos = b
    return pos == ksteps


def empty_slices(layout):
    return [s for s, (a, b) in enumerate(layout) if a == b]


# ---- bf16 weight gradient dW[M, N] over K token rows, 128x128 T-form kernel (gemm_tt.hip): (slices, M, N, K) ----
# slices = min(1024 / tiles, ceil(K / 64) / 4).  Per K-bound count s: K = 256 s, 256 s + 1 (a last step of one row) and a K with
# ceil(K / 64) = 4 s whose last step is ragged (256 s - 12: the shapes on which the size query used to be one slice short).
# M or N is not a multiple of 256, or K < 1024: the 8-phase kernel does not take them.
def _triple(s, M, N):
    return [(s, M, N, 256 * s), (s, M, N, 256 * s + 1), (s, M, N, 256 * s - 12)]


WGRAD_TT = (_triple(1, 128, 136) + _triple(2, 128, 136) + _triple(3, 192, 576) + _triple(4, 192, 576) + _triple(5, 128, 136)
            + _triple(8, 264, 128) + _triple(16, 128, 136) + _triple(49, 192, 192) + [
    (49, 192, 192, 64 * 197),        # ViT-Tiny over 64 x 197 tokens
    (16, 1000, 1024, 6000),          # the tile cap: 64 tiles -> 1024 / 64 slices although K has 94 steps
    (3, 192, 576, 15 * 64),          # 4 s + 3 K steps: slices of 5, 5, 5 steps
    (5, 136, 128, 23 * 64 - 63),     # 4 s + 3 steps and a last step of one row
    (4, 256, 256, 1023),             # whole 256x256 tiles, but K < 1024
    (3, 8, 8, 800),                  # less than one fragment of rows and columns
])

# ---- the same on the 8-phase 256x256 kernel (gemm_p8.hip, T-form): M and N multiples of 256, K >= 1024 ----
# slices = min(256 / tiles, ceil(K / 64) / 8); ksteps = 8 s + 1 with s >= 6 leaves the last slice empty
WGRAD_P8 = [
    (1, 3072, 3072, 1030),           # 144 tiles
    (2, 256, 256, 1024),
    (4, 256, 512, 2050),
    (7, 768, 3072, 56 * 64),         # 36 tiles; 8 s steps exactly
    (7, 768, 3072, 3600),            # 57 steps: 6 slices of 10, the 7th empty
    (7, 768, 3072, 56 * 64 + 1),     # one row past a step (57 steps again: an empty slice AND a one-row step)
    (9, 768, 2304, 4700),            # 27 tiles
    (28, 768, 768, 224 * 64),        # 9 tiles
    (28, 768, 768, 14400),           # 225 steps: 28 slices of 10 steps hold 280; slices 23 .. 27 are empty
    (28, 768, 768, 224 * 64 + 1),
    (28, 768, 768, 65600),           # the headline training batch: 1025 steps, 28 slices of 38, the last one empty
]
P8_EMPTY = {(768, 3072, 3600), (768, 3072, 56 * 64 + 1), (768, 768, 14400), (768, 768, 224 * 64 + 1), (768, 768, 65600)}

# ---- fp32 weight gradient (gemm_tile.hip, both operands T-form; 32-deep K steps): slices = min(1024 / tiles, ceil(K / 32) / 4) ----
def _triple32(s, M, N):
    return [(s, M, N, 128 * s), (s, M, N, 128 * s + 1), (s, M, N, 128 * s - 5)]


WGRAD_F32 = (_triple32(1, 128, 136) + _triple32(2, 128, 136) + _triple32(3, 192, 576) + _triple32(8, 264, 128)
             + _triple32(31, 192, 192) + [
    (16, 1000, 1024, 2100),          # the tile cap: 64 tiles, 66 K steps
    (3, 192, 576, 15 * 32),          # 4 s + 3 K steps
    (5, 4, 4, 700),                  # a 4 x 4 output
    (5, 4, 136, 23 * 32 - 31),       # ... 4 rows, 4 s + 3 steps, a last step of one row
    (28, 768, 768, 3600),            # 36 tiles
])

# ---- whole-GEMM split of a small linear (<= 128 output tiles, K >= 512): slices = min(8, K / kstep / 4) ----
# (slices, M, N, K, epilogue): epilogue 0 bias, 1 GELU, 2 in-place residual.  0 slices: the path does not apply.
WHOLE = {
    32: [(4, 300, 768, 512, 0), (5, 129, 192, 640, 1), (6, 1, 768, 768, 2), (7, 788, 384, 896, 0), (8, 129, 768, 1024, 2),
         (8, 197, 768, 3072, 1),           # the cap: 24 slices' worth of K
         (0, 300, 768, 480, 0),            # K just below 512
         (4, 16384, 128, 512, 2),          # 128 output tiles
         (0, 16385, 128, 512, 0)],         # 129
    64: [(2, 300, 768, 512, 0), (3, 129, 192, 768, 1), (4, 1, 768, 1024, 2), (5, 788, 384, 1280, 0), (6, 129, 768, 1536, 2),
         (7, 300, 192, 1792, 1), (8, 129, 768, 2048, 0),
         (8, 197, 768, 3072, 2),           # the cap
         (0, 300, 768, 448, 0),            # K just below 512
         (2, 16384, 128, 512, 2),          # 128 output tiles
         (0, 16385, 128, 512, 0)],         # 129
}

# ---- trailing rows by split-K (the CLS rows): slices = clamp(K / kstep / 4, 1, 16) for K >= 256, K % kstep == 0 ----
# (slices, K): fp32 / x3 with 32-deep steps start at 2 slices (K = 256)
THIN_K = {
    32: [(2, 256), (4, 512), (15, 1920), (16, 2048), (16, 3072), (0, 224)],
    64: [(1, 256), (2, 512), (4, 1024), (15, 3840), (16, 4096), (16, 6144), (0, 192)],   # 16-bit K is a multiple of 64
}
