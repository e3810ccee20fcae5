"""Tiled and x8 self-ensemble inference as ONE mechanism: a table of *views* of the (padded) image, one gather kernel, batched network
calls, one blend kernel (csrc/views.hip: rcot_view_gather, rcot_view_blend).

A view is a window of the image under one of the 8 dihedral maps of the reference's ``data_augmentation`` (util/image_utils.py:133-163).
Overlapping tiles are views of several windows under the identity; the geometric self-ensemble — the mean of aug^-1(T(aug(x))) over the
8 maps, the "+" rows of restoration tables — is 8 views of one window; both at once is their product.  The network runs on runs of
consecutive views of one shape (tiles of one size are the natural batch), and the blend kernel puts every restored view back through the
inverse map, weighted by a separable window that ramps across the overlap, so that neighbouring tiles — whose outputs disagree where
they overlap, Restormer's transposed attention takes its statistics over the whole tile — meet without a step.

This module is host logic only (numpy; torch is imported where tensors are made): nothing here needs a device to import.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Tuple

import numpy as np

WINDOWS = ("uniform", "linear", "cosine")
ENSEMBLE_MODES = {1: (0,), 8: (0, 1, 4, 5, 2, 3, 6, 7)}       # the shape-keeping maps first: the views of one shape are consecutive


class ViewPlan(NamedTuple):
    """The views of one request: windows of Th x Tw at ys x xs of an H x W image, each under every map of ``modes``; view index
    (k * len(ys) + iy) * len(xs) + ix.  ``ov_y`` / ``ov_x``: the overlap of neighbouring windows in a regular step (0 with one window)."""
    H: int
    W: int
    ys: Tuple[int, ...]
    xs: Tuple[int, ...]
    Th: int
    Tw: int
    modes: Tuple[int, ...]
    ov_y: int
    ov_x: int

    @property
    def n_views(self) -> int:
        return len(self.modes) * len(self.ys) * len(self.xs)

    def shape_classes(self):
        """[(first view, view count, rows, columns)]: the runs of consecutive views of one shape"""
        per, runs = len(self.ys) * len(self.xs), []
        for k, m in enumerate(self.modes):
            shape = (self.Tw, self.Th) if m & 2 else (self.Th, self.Tw)
            if runs and runs[-1][2:] == shape:
                runs[-1] = (runs[-1][0], runs[-1][1] + per, *shape)
            else:
                runs.append((k * per, per, *shape))
        return runs


def plan(H: int, W: int, tile: int = 0, overlap: int = 32, mult: int = 8, ensemble: int = 1) -> ViewPlan:
    """The windows of ``tester.restore(net, x, tile, overlap, mult)`` — ``tile`` and the step rounded down to ``mult``, origins clamped to
    H - tile, windows of min(tile, H) x min(tile, W); tile 0 (or a tile that holds the image): one window, the whole image — under the
    maps of ``ensemble`` (1: the identity; 8: all)."""
    if ensemble not in ENSEMBLE_MODES:
        raise ValueError(f"ensemble {ensemble!r}: expected 1 or 8")
    modes = ENSEMBLE_MODES[ensemble]
    if not tile or (tile >= H and tile >= W):
        return ViewPlan(H, W, (0,), (0,), H, W, modes, 0, 0)
    tile = max(mult, tile // mult * mult)
    step = max(mult, (tile - overlap) // mult * mult)
    ys = tuple(sorted({min(y, max(H - tile, 0)) for y in range(0, H, step)}))
    xs = tuple(sorted({min(c, max(W - tile, 0)) for c in range(0, W, step)}))
    Th, Tw = min(tile, H), min(tile, W)
    return ViewPlan(H, W, ys, xs, Th, Tw, modes, max(Th - step, 0) if len(ys) > 1 else 0, max(Tw - step, 0) if len(xs) > 1 else 0)


def window_taps(T: int, overlap: int, kind: str) -> Optional[np.ndarray]:
    """The T taps of one axis of the blending window, float32 (computed in fp64); None for "uniform" (equal weights).
    r_i = min(1, (i + 1) / (ov + 1), (T - i) / (ov + 1)): 1 in the interior, a ramp of ov steps at either end that sums to 1 with the
    neighbouring tile's across an overlap of ov pixels; "linear" is r itself, "cosine" 0.5 - 0.5 cos(pi r) (a Hann ramp, same sum)."""
    if kind not in WINDOWS:
        raise ValueError(f"window {kind!r}: expected one of {WINDOWS}")
    if kind == "uniform":
        return None
    return _taps64(T, overlap, kind).astype(np.float32)


def _taps64(T: int, overlap: int, kind: str) -> np.ndarray:
    ov = max(int(overlap), 0)
    i = np.arange(T, dtype=np.float64)
    r = np.minimum(1.0, np.minimum((i + 1.0) / (ov + 1.0), (T - i) / (ov + 1.0)))
    return r if kind == "linear" else 0.5 - 0.5 * np.cos(math.pi * r)


def restore_views(net, x, plan: ViewPlan, window: str = "uniform", tile_batch: int = 1):
    """x float [B, C, H, W] on the network's device -> the blend of ``net`` on the views of ``plan``, image by image: rcot_view_gather,
    ``net`` on runs of at most ``tile_batch`` consecutive views of one shape (0: a whole shape class per call), rcot_view_blend with the
    taps of ``window`` over the plan's overlaps.  No torch arithmetic: allocation and device-to-device placement only."""
    import torch
    be = net.be
    B, C, H, W = x.shape
    if (H, W) != (plan.H, plan.W):
        raise ValueError(f"the plan is for {plan.H} x {plan.W}, the image is {H} x {W}")
    if tile_batch < 0:
        raise ValueError(f"tile_batch {tile_batch}: expected 0 (a whole shape class per call) or a positive count")
    wy, wx = window_taps(plan.Th, plan.ov_y, window), window_taps(plan.Tw, plan.ov_x, window)
    if wy is not None:
        wy, wx = torch.from_numpy(wy).to(be.device), torch.from_numpy(wx).to(be.device)
    geom = (plan.ys, plan.xs, plan.modes, plan.Th, plan.Tw)
    x = x.contiguous()
    out = be.empty(B, C, H, W)
    per = C * plan.Th * plan.Tw
    views, restored = be.empty(plan.n_views, per), be.empty(plan.n_views, per)
    for b in range(B):
        be.view_gather(x[b], *geom, out=views)
        for first, count, rows, cols in plan.shape_classes():
            src, dst = (t[first:first + count].view(count, C, rows, cols) for t in (views, restored))
            run = count if tile_batch == 0 else min(tile_batch, count)
            for a in range(0, count, run):
                dst[a:a + run].copy_(net(src[a:a + run]))
        be.view_blend(restored, H, W, *geom, wy, wx, out=out[b])
    return out
