"""Landmark localisation kernels (csrc/landmark.hip): heatmap loss (sigmoid Dice + BCE), sliding-window aggregation in sigmoid space, heatmap metrics
(soft-argmax coordinates, per-map Dice) and the Wing loss of the coordinate head.

Part of the ctypes front of ``libcinema_hip.so`` (see ``cinema_amd/hip/__init__.py``); everything here is re-exported there, so callers write
``hip.<name>``."""
from __future__ import annotations

import torch

from cinema_amd.hip import HipLibraryError, _check, _dev, _empty, _empty_like, _p, _stream, load

__all__ = ['LANDMARK_MAX_BLOCKS', 'head_wing', 'heatmap_metrics', 'landmark_loss_bwd', 'landmark_loss_fwd', 'landmark_window_accumulate',
           'landmark_window_finish']

LANDMARK_MAX_BLOCKS = 64  # = CINEMA_LANDMARK_MAX_BLOCKS of include/cinema_hip.h (partial rows per sample of the loss forward's slab)


def _f32c(*ts: torch.Tensor) -> bool:
    return all(t.dtype == torch.float32 and t.is_contiguous() for t in ts)


def landmark_loss_fwd(logits_rows: torch.Tensor, labels: torch.Tensor, batch: int):  # noqa: ANN201
    """-> (out4 = [loss, bce, dice, 0], coef) for fp32 rows [batch*vox, c] and fp32 channels-first labels (batch, c, *spatial)."""
    _dev(logits_rows, labels)
    if not _f32c(logits_rows, labels) or logits_rows.dim() != 2 or labels.numel() != logits_rows.numel():
        raise HipLibraryError("landmark_loss: contiguous fp32 logits rows [b*vox, c] and fp32 channels-first labels of as many elements")
    rows, c = logits_rows.shape
    slab = _empty(batch * LANDMARK_MAX_BLOCKS * (3 * c + 1), dtype=torch.float32, device=logits_rows.device)
    out4 = _empty(4, dtype=torch.float32, device=logits_rows.device)
    coef = _empty(batch * c * 2, dtype=torch.float32, device=logits_rows.device)
    _check(load().cinema_landmark_loss_fwd(logits_rows.data_ptr(), labels.data_ptr(), batch, rows // batch, c, slab.data_ptr(), out4.data_ptr(),
                                           coef.data_ptr(), _stream()), "landmark_loss_fwd")
    return out4, coef


def landmark_loss_bwd(logits_rows: torch.Tensor, labels: torch.Tensor, batch: int, coef: torch.Tensor, upstream: torch.Tensor | None) -> torch.Tensor:
    """d loss / d logits rows [batch*vox, c] (times ``upstream[0]``) from the coefficients of :func:`landmark_loss_fwd`."""
    _dev(logits_rows, labels, coef, upstream)
    rows, c = logits_rows.shape
    d = _empty_like(logits_rows)
    _check(load().cinema_landmark_loss_bwd(logits_rows.data_ptr(), labels.data_ptr(), batch, rows // batch, c, coef.data_ptr(), _p(upstream), d.data_ptr(),
                                           _stream()), "landmark_loss_bwd")
    return d


def landmark_window_accumulate(window_rows: torch.Tensor, patch: tuple, start: tuple, size: tuple, prob_sum: torch.Tensor, count: torch.Tensor) -> None:
    """Add sigmoid(window_rows) (fp32 [prod(patch), c], channels last) into prob_sum [prod(size), c] / count [prod(size)] at offset ``start``
    (2-D windows use a leading unit axis)."""
    _dev(window_rows, prob_sum, count)
    if not _f32c(window_rows, prob_sum, count):
        raise HipLibraryError("landmark_window_accumulate: contiguous fp32 tensors")
    p3, z3 = [(1,) * (3 - len(t)) + tuple(int(v) for v in t) for t in (patch, size)]
    s3 = (0,) * (3 - len(start)) + tuple(int(v) for v in start)
    _check(load().cinema_landmark_window_accumulate(window_rows.data_ptr(), window_rows.shape[1], *p3, *s3, *z3, prob_sum.data_ptr(), count.data_ptr(),
                                                    _stream()), "landmark_window_accumulate")


def landmark_window_finish(prob_sum: torch.Tensor, count: torch.Tensor) -> torch.Tensor:
    """-> fp32 [c, n_voxels] = log(p / (1 - p)) of p = prob_sum / count (channels first; +inf where p rounds to 1)."""
    _dev(prob_sum, count)
    n, c = prob_sum.shape
    out = _empty((c, n), dtype=torch.float32, device=prob_sum.device)
    _check(load().cinema_landmark_window_finish(prob_sum.data_ptr(), count.data_ptr(), c, n, out.data_ptr(), _stream()), "landmark_window_finish")
    return out


def heatmap_metrics(logits: torch.Tensor, labels: torch.Tensor, beta: float = 1000.0) -> torch.Tensor:
    """logits / labels fp32 (b, c, w, h) contiguous -> fp32 [b, c, 8]: soft-argmax E[x], E[y] of sigmoid(logits), of labels, then I, P, G and the
    Dice loss of the map (``cinema_heatmap_metrics``)."""
    _dev(logits, labels)
    if not _f32c(logits, labels) or logits.dim() != 4 or logits.shape != labels.shape:
        raise HipLibraryError("heatmap_metrics: contiguous fp32 logits and labels of one shape (b, c, w, h)")
    b, c, w, h = logits.shape
    out = _empty((b, c, 8), dtype=torch.float32, device=logits.device)
    _check(load().cinema_heatmap_metrics(logits.data_ptr(), labels.data_ptr(), b, c, w, h, float(beta), out.data_ptr(), _stream()), "heatmap_metrics")
    return out


def head_wing(pred: torch.Tensor, label: torch.Tensor, scales: torch.Tensor | None = None, w: float = 10.0, epsilon: float = 2.0,
              rel: bool = True) -> tuple:
    """-> (out5 = [loss, landmark wing, rel-dist wing, landmark MAE, rel-dist MAE], d loss / d pred) for contiguous fp32 [b, n] tensors (``rel``: n == 6)."""
    _dev(pred, label, scales)
    if not _f32c(pred, label) or pred.dim() != 2 or pred.shape != label.shape or (scales is not None and (not _f32c(scales) or scales.shape != pred.shape)):
        raise HipLibraryError("head_wing: contiguous fp32 predictions, labels (and scales) of one shape [b, n]")
    out, d = _empty(5, dtype=torch.float32, device=pred.device), _empty_like(pred)
    _check(load().cinema_head_wing(pred.data_ptr(), label.data_ptr(), _p(scales), pred.shape[0], pred.shape[1], float(w), float(epsilon), int(rel),
                                   out.data_ptr(), d.data_ptr(), _stream()), "head_wing")
    return out, d
