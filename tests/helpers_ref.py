"""fp64 CPU references of the embedding, seg-head and training helper kernels (tests/test_gpu_helpers.py), each written from the
model's definition with torch / numpy calls -- not from a kernel's index arithmetic -- and checked among themselves without a
GPU by tests/test_helpers_ref_cpu.py.  Also the shapes both files use, and the input generators.

Layouts (include/vitseg.h): token rows are patches first (row b * Np + t), the CLS rows B * Np + b after them; feature maps
are token-major [B * g * g, channels]; a 3x3 weight is [N, 9 * channels] with k = (ky, kx, channel); the patch weight is
[D, Cin * P * P] with k = (c, py, px)."""
import numpy as np
import torch
import torch.nn.functional as F

from dropout_ref import Masks

MID = 256   # seg_head.0 output channels

# ---- shapes: the smallest that cross every boundary the code names (see the tests' docstrings) ----
PATCH_SHAPES = [(2, 3, 4, 3, 64), (1, 3, 4, 12, 64), (2, 1, 8, 3, 192), (2, 3, 12, 2, 64), (1, 3, 16, 3, 132),
                (2, 3, 32, 2, 64)]                                   # (B, Cin, P, g, D)
CONV_SHAPES = [(2, 3, 64, 256), (1, 1, 64, 256), (3, 12, 64, 256), (2, 14, 192, 256)]     # (B, g, channels, N)
CONV_DGRAD_SHAPES = [(2, 3, 256, 64), (3, 12, 256, 192)]
CONV_LARGE_SHAPE = (4, 32, 256, 256)                                 # M = 4096, K = 2304: the 256x128 16-bit kernel
HEAD_SHAPES = [(2, 9, 2), (1, 197, 17), (3, 5, 1), (1, 7, 40)]       # (B, Np, C)
HEAD_BWD_SHAPES = [(2, 9, 2), (1, 13, 17), (1, 16383, 3), (1, 16384, 3), (2, 8200, 32)]
COLSUM_F32_SHAPES = [(1, 4, 4), (63, 20, 24), (257, 260, 260), (4096, 768, 768), (4097, 768, 768), (4353, 72, 80)]   # (M, N, ld)
COLSUM_BF16_SHAPES = [(255, 64, 64), (256, 192, 200), (513, 2304, 2304)]
EMBED_BWD_SHAPES = [(1, 4, 64), (3, 9, 192), (2, 196, 100)]          # (B, Np, D)
TRANSPOSE_SHAPES = [(64, 64, 64, 64), (130, 72, 80, 192), (197, 200, 200, 256), (9, 8, 8, 64)]   # (R, C, ldin, Rpad)
TRANSPOSE_LAYERS_SHAPES = [(2, 64, 192), (2, 72, 136)]               # (L, D, I): [3D, D] [D, D] [I, D] [D, I] per layer
DROPOUT_SHAPES = [(5, 64, 0.1), (197, 192, 0.5), (4100, 1024, 0.1)]  # (rows, cols, p)
IM2COL3_SHAPES = [(2, 3, 64), (1, 1, 8), (3, 12, 72), (2, 14, 192)]  # (B, g, D)
IM2COL_PATCH_SHAPES = [(2, 3, 4, 3), (1, 3, 16, 3), (2, 1, 8, 3), (2, 3, 12, 2)]   # (B, Cin, P, g)


# ---- inputs ----
def ints(*shape, lo, hi, seed):
    """integers of [lo, hi] as fp32: exact in fp32, bf16 and IEEE half (|v| <= 256), and so are their products and sums
    while these stay below 2^24"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def gauss(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


# ---- gathers ----
def im2col3x3(H, B, g):
    """[B * g * g, 9 * D] rows of the zero-padded 3x3 neighbourhoods of the token-major map H [B * g * g, D], k = (ky, kx, d)"""
    D = H.shape[1]
    x = H.view(B, g, g, D).permute(0, 3, 1, 2)
    cols = F.unfold(x, 3, padding=1)                       # [B, D * 9, g * g], k = (d, ky, kx)
    return cols.view(B, D, 9, g * g).permute(0, 3, 2, 1).reshape(B * g * g, 9 * D)


def im2col_patch(img, P):
    """[B * g * g, Cin * P * P] patch rows of the NCHW image, k = (c, py, px)"""
    cols = F.unfold(img, P, stride=P)                      # [B, Cin * P * P, g * g]
    return cols.transpose(1, 2).reshape(-1, cols.shape[1])


# ---- the embeddings ----
def patch_embed(img, Wp, bp, pos, cls, P):
    """X [B * (Np + 1), D] in fp64: Conv2d(Cin, D, P, stride P) on the image, one row per patch, + pos[1 + t]; the CLS rows
    cls + pos[0] (modeling_vit.py ViTEmbeddings)"""
    B, Cin = img.shape[:2]
    D = Wp.shape[0]
    y = F.conv2d(img.double(), Wp.double().view(D, Cin, P, P), bp.double(), stride=P)   # [B, D, g, g]
    rows = y.flatten(2).transpose(1, 2) + pos.double()[1:].unsqueeze(0)                 # [B, Np, D]
    cls_rows = (cls.double() + pos.double()[0]).expand(B, D)
    return torch.cat([rows.reshape(-1, D), cls_rows], 0)


def embed_bwd(dX, B, Np):
    """(dpos [Np + 1, D], dcls [D]) in fp64: autograd of X = cat(patch rows + pos[1:], cls + pos[0])"""
    D = dX.shape[1]
    patch = torch.zeros(B, Np, D, dtype=torch.float64)
    pos = torch.zeros(Np + 1, D, dtype=torch.float64, requires_grad=True)
    cls = torch.zeros(D, dtype=torch.float64, requires_grad=True)
    X = torch.cat([(patch + pos[1:]).reshape(B * Np, D), (cls + pos[0]).expand(B, D)], 0)
    dpos, dcls = torch.autograd.grad(X, [pos, cls], dX.double())
    return dpos, dcls


# ---- seg_head.0 ----
def conv3x3(H, W, bias, B, g, relu):
    """[B * g * g, N] in fp64: Conv2d(channels, N, 3, padding=1) (+ ReLU) on the token-major map H, weight [N, 9 * channels]"""
    C, N = H.shape[1], W.shape[0]
    x = H.double().view(B, g, g, C).permute(0, 3, 1, 2)
    w = W.double().view(N, 3, 3, C).permute(0, 3, 1, 2)
    y = F.conv2d(x, w, None if bias is None else bias.double(), padding=1)
    if relu:
        y = torch.relu(y)
    return y.permute(0, 2, 3, 1).reshape(B * g * g, N)


def conv3x3_input_grad(dF, W0, B, g):
    """[B * g * g, D] in fp64: autograd of conv3x3(H, W0) with respect to H, given dF [B * g * g, N]"""
    D = W0.shape[1] // 9
    H = torch.zeros(B * g * g, D, dtype=torch.float64, requires_grad=True)
    return torch.autograd.grad(conv3x3(H, W0, None, B, g, False), H, dF.double())[0]


def conv_dgrad_weight(W0):
    """Wd [D, 9 * N]: Wd[d][t][o] = W0[o][8 - t][d], the weight with which the input gradient of the conv is itself a conv"""
    N = W0.shape[0]
    D = W0.shape[1] // 9
    return W0.view(N, 9, D).flip(1).permute(2, 1, 0).reshape(D, 9 * N).contiguous()


# ---- seg_head.2 ----
def head1x1(Fm, W2, b2, B, Np):
    """Z [B, C, Np] in fp64: Conv2d(256, C, 1) on the token-major F [B * Np, 256]"""
    C = W2.shape[0]
    x = Fm.double().view(B, Np, MID).permute(0, 2, 1).unsqueeze(-1)
    return F.conv2d(x, W2.double().view(C, MID, 1, 1), b2.double()).squeeze(-1)


def head1x1_bwd(dZ, Fm, W2, B, Np):
    """(dFpre [B * Np, 256], dW2 [C, 256], db2 [C]) in fp64: autograd of conv1x1(relu(Fpre)) given dZ [B, C, Np], with
    F = relu(Fpre) handed in.  Where the F handed in is negative (never so in the model; the tests plant some) it keeps its
    value in the product and passes no gradient, as at zero."""
    C = W2.shape[0]
    Fpre = Fm.double().clone().requires_grad_(True)
    act = torch.relu(Fpre) + Fpre.detach().clamp(max=0.0)
    W = W2.double().clone().requires_grad_(True)
    b = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    Z = F.conv2d(act.view(B, Np, MID).permute(0, 2, 1).unsqueeze(-1), W.view(C, MID, 1, 1), b).squeeze(-1)
    return torch.autograd.grad(Z, [Fpre, W, b], dZ.double())


# ---- dropout, transposes, rounding ----
def dropout_keep(rows, cols, p, seed, stream):
    """(keep [rows, cols] bool, scale float32) of the hidden-dropout mask (tests/dropout_ref.py)"""
    mk = Masks(p, seed, 1, 1, 1)
    return mk._keep(stream, np.arange(rows)[:, None], np.arange(cols)[None, :]), mk.scale, int(mk.thresh)


def dropout_rows(src, p, seed, stream):
    """float32 numpy: keep ? src * scale : 0, one fp32 multiply"""
    keep, scale, _ = dropout_keep(src.shape[0], src.shape[1], p, seed, stream)
    return np.where(keep, src.numpy().astype(np.float32) * scale, np.float32(0)).astype(np.float32)


def transpose_pad(x, C, Rpad):
    """[C, Rpad]: the first C columns of x [R, ld] transposed, zeros in columns R .. Rpad - 1"""
    out = torch.zeros(C, Rpad, dtype=x.dtype)
    out[:, :x.shape[0]] = x[:, :C].t()
    return out


def half_ulp(ref, dtype):
    """half a unit in the last place of `dtype` (bf16 / IEEE half) at |ref|, elementwise in fp64"""
    mant, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    _, e = torch.frexp(ref.abs().clamp(min=2.0 ** emin))    # |ref| = m * 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(ref), e - 1 - mant - 1)


def bf16_ties(n, seed):
    """n fp32 values exactly halfway between two neighbouring bf16 numbers (low 16 bits 0x8000), both parities of the kept
    bit and both signs: round-to-nearest-even must go down for an even kept mantissa and up for an odd one"""
    rng = np.random.default_rng(seed)
    hi = rng.integers(0x3C00, 0x4400, n).astype(np.uint32)                          # bf16 bit patterns of 2^-7 .. 2^9
    hi[1::2] |= np.uint32(0x8000)                                                   # every other one negative
    return torch.from_numpy(((hi << np.uint32(16)) | np.uint32(0x8000)).view(np.float32).copy())
