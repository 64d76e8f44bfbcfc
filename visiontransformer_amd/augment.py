"""Training augmentation on the device: flips, quarter turns, rotation, scale / translate jitter and colour jitter of a
batch of images TOGETHER with their label maps, in one launch of `vitseg_augment` (csrc/augment.hip).

The reference's datasets apply `Resize` + `ToTensor` and nothing else (model/CE/classes.py:60-89), so a trainer sees the same
pixels every epoch.  Here the random draw happens on the host (`Augmenter.sample`, a few numbers per sample), is turned
into one Q16 integer affine matrix per sample and plane (`matrices`, through the library's `vitseg_augment_matrix`) and one
3x4 colour matrix per sample (`colour`), and the kernel does the rest: bilinear image warp, colour matrix + clamp, nearest
label warp.  All coordinate arithmetic is integer and every fp32 operation is rounded on its own, so the result is
reproducible to the bit (tests/augment_ref.py restates it in numpy).

Out-of-frame pixels: `border="edge"` repeats the frame's edge; `border="constant"` writes `fill` into the image and
`fill_label` into the label maps -- with the fused cross-entropy's `ignore_index` as `fill_label` those pixels do not count.
The binary PAED targets are recomputed from the WARPED mask (`paed_binary`, vitseg_sdf), so the signed distances stay exact
after a rotation.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

_BORDERS = {"constant": _lib.AUGMENT_CONSTANT, "edge": _lib.AUGMENT_EDGE}
_QUARTER = np.array(((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)))   # exact (cos, sin) of k quarter turns
_GREY = np.array((0.299, 0.587, 0.114))                                    # Rec.601 luma


def _default_rank() -> int:
    import torch.distributed as dist
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


def _pair(v, what) -> Tuple[int, int]:
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError(f"{what} must be an int or (h, w), got {v!r}")
        return int(v[0]), int(v[1])
    return int(v), int(v)


class Augmenter:
    """Random paired augmentation for one model input size.

    hflip / vflip: probabilities of a horizontal / vertical flip.  rot90: draw 0..3 quarter turns (counter-clockwise, as
    `np.rot90(m, k)`).  rotate: degrees, the angle is uniform in [-rotate, rotate].  scale = (lo, hi): zoom factor, uniform
    (> 1 enlarges the content).  translate: the sampling window shifts by a uniform fraction of the frame in
    [-translate, translate] along each axis.  brightness / contrast / saturation: each factor is uniform in
    [max(0, 1 - v), 1 + v].  Rotation and scale act about the centre, in the frame's normalised coordinates (a source of
    another shape is stretched onto the square as `Preprocessor` stretches it).  `fill`: the image value outside the frame
    per channel, in the output's [0, 1] units; `fill_label`: the label written there."""

    def __init__(self, image_size: int, device="cuda:0", seed: int = 0, hflip: float = 0.5, vflip: float = 0.0,
                 rot90: bool = False, rotate: float = 0.0, scale: Sequence[float] = (1.0, 1.0), translate: float = 0.0,
                 brightness: float = 0.0, contrast: float = 0.0, saturation: float = 0.0, border: str = "edge",
                 fill: Sequence[float] = (0.0, 0.0, 0.0), fill_label: Optional[int] = None):
        self.S = int(image_size)
        if self.S < 1:
            raise ValueError(f"image_size must be positive, got {image_size}")
        self.device = torch.device(device)
        self.seed = int(seed)
        if border not in _BORDERS:
            raise ValueError(f'border must be "edge" or "constant", got {border!r}')
        for name, p in (("hflip", hflip), ("vflip", vflip)):
            if not 0.0 <= float(p) <= 1.0:
                raise ValueError(f"{name} is a probability, got {p}")
        lo, hi = (float(v) for v in scale)
        if not 0.0 < lo <= hi:
            raise ValueError(f"scale must be (lo, hi) with 0 < lo <= hi, got {tuple(scale)}")
        for name, v in (("rotate", rotate), ("translate", translate), ("brightness", brightness), ("contrast", contrast),
                        ("saturation", saturation)):
            if not float(v) >= 0.0:
                raise ValueError(f"{name} must be >= 0, got {v}")
        if len(tuple(fill)) != 3:
            raise ValueError(f"fill must hold one value per channel, got {fill!r}")
        self.hflip, self.vflip, self.rot90 = float(hflip), float(vflip), bool(rot90)
        self.rotate, self.scale, self.translate = float(rotate), (lo, hi), float(translate)
        self.brightness, self.contrast, self.saturation = float(brightness), float(contrast), float(saturation)
        self.border, self.fill = border, tuple(float(v) for v in fill)
        self.fill_label = None if fill_label is None else int(fill_label)
        self.rank = _default_rank()
        self.calls = 0

    @property
    def has_colour(self) -> bool:
        """Whether `apply` passes a colour table: with no colour jitter configured the kernel skips the step."""
        return self.brightness > 0 or self.contrast > 0 or self.saturation > 0

    # ---- the random draw -------------------------------------------------------------------------------------------------
    def sample(self, n: int, key: Optional[Sequence[int]] = None) -> dict:
        """The draw of `n` samples as a plain dict of numpy arrays: hflip, vflip (bool), quarter (int64 0..3), angle
        (degrees), scale, tx, ty, brightness, contrast, saturation (float64).  The generator is
        `np.random.Generator(PCG64(SeedSequence([seed, *key])))`, so a draw depends on (seed, key) alone, never on call
        order; the default key is (rank, calls) with `calls` counting the default-keyed draws of this object.  Every
        field is always drawn, so switching one transformation on or off leaves the others' draws as they were."""
        if key is None:
            key = (self.rank, self.calls)
            self.calls += 1
        rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence([self.seed, *[int(k) for k in key]])))
        n = int(n)
        u = rng.random((2, n))
        quarter = rng.integers(0, 4, n)
        angle = rng.uniform(-1.0, 1.0, n) * self.rotate
        scale = rng.uniform(self.scale[0], self.scale[1], n)
        shift = rng.uniform(-1.0, 1.0, (2, n)) * self.translate
        col = rng.uniform(-1.0, 1.0, (3, n))
        factor = lambda v, r: np.maximum(0.0, 1.0 + v * r)
        return dict(hflip=u[0] < self.hflip, vflip=u[1] < self.vflip,
                    quarter=quarter.astype(np.int64) if self.rot90 else np.zeros(n, np.int64),
                    angle=angle, scale=scale, tx=shift[0], ty=shift[1], brightness=factor(col[0], self.brightness),
                    contrast=factor(col[1], self.contrast), saturation=factor(col[2], self.saturation))

    # ---- parameters -> tables ---------------------------------------------------------------------------------------------
    @staticmethod
    def affine(params: dict) -> np.ndarray:
        """float64 [n, 6]: the normalised 2x3 affine of every sample, output unit square -> source unit square:
        q = c + R(quarter * 90 + angle) (p - c) / scale + (tx, ty) with c = (0.5, 0.5), then u -> 1 - u for a horizontal
        and v -> 1 - v for a vertical flip (the flips act on the source axes).  Quarter turns and flips are exact."""
        quarter = _QUARTER[np.asarray(params["quarter"], np.int64) % 4]
        cq, sq = quarter[:, 0], quarter[:, 1]
        ang = np.radians(np.asarray(params["angle"], np.float64))
        ca, sa = np.cos(ang), np.sin(ang)
        c, s = cq * ca - sq * sa, sq * ca + cq * sa
        sc = np.asarray(params["scale"], np.float64)
        a00, a01, a10, a11 = c / sc, -s / sc, s / sc, c / sc
        a02 = 0.5 - (a00 + a01) * 0.5 + np.asarray(params["tx"], np.float64)
        a12 = 0.5 - (a10 + a11) * 0.5 + np.asarray(params["ty"], np.float64)
        h, v = np.asarray(params["hflip"], bool), np.asarray(params["vflip"], bool)
        a00, a01, a02 = np.where(h, -a00, a00), np.where(h, -a01, a01), np.where(h, 1.0 - a02, a02)
        a10, a11, a12 = np.where(v, -a10, a10), np.where(v, -a11, a11), np.where(v, 1.0 - a12, a12)
        return np.ascontiguousarray(np.stack([a00, a01, a02, a10, a11, a12], axis=1))

    def matrices(self, params: dict, src_hw, dst_hw) -> np.ndarray:
        """int64 [n, 6]: the Q16 matrices of `params` for one (source, output) size pair, through vitseg_augment_matrix."""
        (sh, sw), (dh, dw) = _pair(src_hw, "src_hw"), _pair(dst_hw, "dst_hw")
        aff = self.affine(params)
        out = np.empty((aff.shape[0], 6), np.int64)
        fn, pa, po = _lib.symbol("vitseg_augment_matrix"), aff.ctypes.data, out.ctypes.data
        for i in range(aff.shape[0]):   # one call per sample: 48 bytes in, 48 bytes out
            rc = fn(pa + 48 * i, sh, sw, dh, dw, po + 48 * i)
            if rc:
                _lib.check(rc)
        return out

    @staticmethod
    def colour(params: dict) -> np.ndarray:
        """float32 [n, 12]: one 3x4 matrix per sample, composed in float64: brightness (v * b), then contrast about 0.5
        (c (v - 0.5) + 0.5), then saturation towards the Rec.601 grey (s v + (1 - s) grey(v))."""
        b, c, s = (np.asarray(params[k], np.float64) for k in ("brightness", "contrast", "saturation"))
        # the saturation's 3x3 acts on c * b * v + 0.5 (1 - c): its rows scale the gain and sum over the offset
        sat = s[:, None, None] * np.eye(3) + (1.0 - s)[:, None, None] * _GREY[None, None, :]
        out = np.empty((len(b), 3, 4), np.float64)
        out[:, :, :3] = sat * (c * b)[:, None, None]
        out[:, :, 3] = sat.sum(axis=2) * (0.5 * (1.0 - c))[:, None]
        return out.reshape(-1, 12).astype(np.float32)

    # ---- the launch -------------------------------------------------------------------------------------------------------
    def _launch(self, images: torch.Tensor, M_img: np.ndarray, colour: Optional[np.ndarray], planes) -> tuple:
        """images on the device: uint8 [n, H, W, 3] or float32 [n, 3, H, W]; planes: [(mask [n, h, w] on the device,
        matrices int64 [n, 6], (oh, ow), out dtype)].  One upload of all the matrices, one of the colour table, one launch."""
        u8 = images.dtype == torch.uint8
        n = int(images.shape[0])
        H, W = (int(images.shape[1]), int(images.shape[2])) if u8 else (int(images.shape[2]), int(images.shape[3]))
        S, dev = self.S, self.device
        tab = torch.from_numpy(np.ascontiguousarray(np.concatenate([M_img] + [p[1] for p in planes]), np.int64)).to(dev)
        ctab = None if colour is None else torch.from_numpy(np.ascontiguousarray(colour, np.float32)).to(dev)
        x = torch.empty((n, 3, S, S), dtype=torch.float32, device=dev)
        descs = (_lib.CAugmentMask * max(len(planes), 1))()
        outs = []
        for i, (m, _, (oh, ow), dt) in enumerate(planes):
            y = torch.empty((n, oh, ow), dtype=dt, device=dev)
            outs.append(y)
            descs[i] = _lib.CAugmentMask(m.data_ptr(), tab.data_ptr() + (i + 1) * n * 48, y.data_ptr(),
                                         int(m.dtype == torch.long), int(dt == torch.long), int(m.shape[1]),
                                         int(m.shape[2]), oh, ow)
        scale = 255.0 if u8 else 1.0   # the kernel takes the fill in the source's units
        fill = (C.c_float * 3)(*[v * scale for v in self.fill])
        with torch.cuda.device(dev):
            _lib.check(_lib.symbol("vitseg_augment")(
                images.data_ptr(), _lib.AUGMENT_U8_NHWC if u8 else _lib.AUGMENT_F32_NCHW, n, H, W, S, S, tab.data_ptr(),
                None if ctab is None else ctab.data_ptr(), x.data_ptr(), descs, len(planes), _BORDERS[self.border], fill,
                self.fill_label if self.fill_label is not None else 0, torch.cuda.current_stream(dev).cuda_stream))
        return x, outs

    def _images(self, images) -> torch.Tensor:
        if isinstance(images, np.ndarray):
            images = torch.from_numpy(np.ascontiguousarray(images))
        ok_u8 = images.dtype == torch.uint8 and images.dim() == 4 and images.shape[-1] == 3
        ok_f32 = images.dtype == torch.float32 and images.dim() == 4 and images.shape[1] == 3
        if not (ok_u8 or ok_f32):
            raise ValueError(f"expected uint8 [n, H, W, 3] or float32 [n, 3, H, W] images, got {images.dtype} "
                             f"{tuple(images.shape)}")
        return images.to(self.device, non_blocking=True).contiguous()

    def apply(self, images, masks=None, params: Optional[dict] = None, mask_size=None, mask_dtype=torch.uint8):
        """(x, y): images uint8 [n, H, W, 3] or float32 [n, 3, H, W] -> x float32 [n, 3, S, S]; masks uint8 / int64
        [n, h, w] of any size -> y `mask_dtype` (torch.uint8 or torch.long) [n, *mask_size] (default (S, S)), warped by
        the same draw; y is None without masks.  `params`: a dict as `sample` returns (default: a fresh draw).  The colour
        step runs when the object has any colour jitter configured (`has_colour`)."""
        images = self._images(images)
        n = int(images.shape[0])
        if params is None:
            params = self.sample(n)
        src_hw = tuple(images.shape[1:3]) if images.dtype == torch.uint8 else tuple(images.shape[2:4])
        planes = []
        if masks is not None:
            if self.border == "constant" and self.fill_label is None:
                raise ValueError('border="constant" with masks needs fill_label (the label of out-of-frame pixels)')
            if mask_dtype not in (torch.uint8, torch.long):
                raise ValueError("mask_dtype must be torch.uint8 or torch.long")
            if isinstance(masks, np.ndarray):
                masks = torch.from_numpy(np.ascontiguousarray(masks))
            if masks.dim() != 3 or masks.dtype not in (torch.uint8, torch.long) or int(masks.shape[0]) != n:
                raise ValueError(f"expected uint8 / int64 [n, h, w] masks for {n} images, got {masks.dtype} "
                                 f"{tuple(masks.shape)}")
            masks = masks.to(self.device, non_blocking=True).contiguous()
            size = _pair(self.S if mask_size is None else mask_size, "mask_size")
            planes.append((masks, self.matrices(params, tuple(masks.shape[1:]), size), size, mask_dtype))
        x, ys = self._launch(images, self.matrices(params, src_hw, (self.S, self.S)),
                             self.colour(params) if self.has_colour else None, planes)
        return x, (ys[0] if ys else None)

    def paed_binary(self, images, masks, params: Optional[dict] = None):
        """The binary PAED trainer's batch from un-augmented images and masks: (x, mask float32 [n, 1, S, S] of 0 / 1,
        sdf_ext, sdf_int float32 [n, S, S]).  masks: [n, h, w] or [n, 1, h, w], non-zero = mask pixel.  The signed-distance
        targets are recomputed from the WARPED mask (vitseg_sdf), so they are exact for the augmented sample."""
        from .sdf import _launch as sdf_launch
        if isinstance(masks, np.ndarray):
            masks = torch.from_numpy(np.ascontiguousarray(masks))
        if masks.dim() == 4 and masks.shape[1] == 1:
            masks = masks[:, 0]
        if masks.dim() != 3:
            raise ValueError(f"expected [n, h, w] or [n, 1, h, w] masks, got {tuple(masks.shape)}")
        if self.border == "constant" and self.fill_label not in (0, 1):
            raise ValueError('border="constant" on a binary mask needs fill_label 0 or 1')
        masks = (masks.to(self.device, non_blocking=True) != 0).to(torch.uint8)
        x, m = self.apply(images, masks, params=params, mask_size=self.S, mask_dtype=torch.uint8)
        sdf_ext, sdf_int = sdf_launch(m, True)
        return x, m[:, None].float(), sdf_ext, sdf_int
