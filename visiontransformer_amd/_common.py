"""What the host side of the mask modules (regions, clean, polygons, centerlines, confidence, metrics) and the evaluation's
reports share: the argument checks, each a ValueError before anything reaches the library, and the CSV writer."""
from __future__ import annotations

import csv
import math

import numpy as np


def is_integer(v, lo: int, hi: int) -> bool:
    """Whether `v` is an integer (Python's or numpy's; a bool is not) in lo..hi."""
    return not isinstance(v, bool) and isinstance(v, (int, np.integer)) and lo <= int(v) <= hi


def integer(name: str, v, lo: int, hi: int, span: str = "") -> int:
    """`v` as an int when `is_integer`; the refusal states the range as `span` (default "lo..hi")."""
    if not is_integer(v, lo, hi):
        raise ValueError(f"{name} must be an integer in {span or f'{lo}..{hi}'}, got {v!r}")
    return int(v)


def label_values(name: str, values, empty_ok: bool = False, background=None) -> list:
    """A sequence of distinct label values 0..255 as a list of ints; `background`, when given, must not be among them."""
    values = list(values)
    if (not values and not empty_ok) or not all(is_integer(c, 0, 255) for c in values):
        raise ValueError(f"{name} must be label values in 0..255, got {values}")
    values = [int(c) for c in values]
    if len(set(values)) != len(values) or background in values:
        what = "distinct" if background is None else f"distinct and must not hold the background {background}"
        raise ValueError(f"{name} must be {what}, got {values}")
    return values


def connectivity(c) -> None:
    if c not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {c}")


def pixel_size(v) -> float:
    ps = float(v)
    if not ps > 0 or math.isinf(ps):
        raise ValueError(f"pixel_size must be a positive finite number, got {v!r}")
    return ps


def write_csv(path: str, columns, rows) -> None:
    with open(path, mode="w", newline="") as f:
        w = csv.writer(f)
        w.writerow(columns)
        w.writerows(rows)
