"""Seeded trials for the fuzz of grouped and truncated split / join
transposes: geometry, scalar size and n come from ``fuzz_util.draw_cfg`` as it
is (its split and join flavours), the keep set from ``fuzz_util._draw_keep``
on a generator of its own."""

from __future__ import annotations

import numpy as np

import fuzz_util
from pencilarrays_amd import native

FLAVOURS = ("split", "join", "split_keep", "join_keep", "join_keep_scale")
KIND_OF = {4: "f32", 8: "f64", 16: "c128"}
ALPHAS = [1.0 / 3.0, -2.5, 0.5]


def draw(flavour: str, index: int):
    """(cfg, kind, n, direction, keep, fill, alpha) of trial ``index``."""
    base = "split" if flavour.startswith("split") else "join"
    t = fuzz_util.draw_cfg(base, index)
    direction = native.SOA_SPLIT if base == "split" else native.SOA_JOIN
    keep, fill, alpha = None, native.FILL_ZERO, None
    if "keep" in flavour:
        rng = np.random.default_rng([0x50A, FLAVOURS.index(flavour), index])
        keep = fuzz_util._draw_keep(rng, t.cfg[0], index)
        # the oracle masks with explicit ranges
        keep = tuple((N, 0) if k is None else k
                     for k, N in zip(keep, t.cfg[0]))
        fill = native.FILL_ZERO if rng.random() < 0.6 else native.FILL_NONE
    if flavour.endswith("scale"):
        alpha = ALPHAS[index % len(ALPHAS)]
    return t.cfg, KIND_OF[t.elem], t.n, direction, keep, fill, alpha


def trial_ids(count: int):
    return [(fl, i) for fl in FLAVOURS for i in range(count)]
