"""The small metric helpers the reference's evaluation / inference scripts import from ``cinema.metric`` (``cinema/metric.py:14-146``).

``stability_score`` and ``get_volumes`` of device tensors count voxels with ``cinema_seg_metric_counts`` (one pass over the channels-first logits, the same
kernel :func:`cinema_amd.segmentation.train.segmentation_metrics` uses); the scalar formulas (ejection fraction, its region, coefficient of variance) are
host arithmetic on whatever the caller passes (floats, numpy arrays, tensors), as in the reference.  ``heatmap_argmax`` / ``heatmap_soft_argmax``
(exported from the package root, ``cinema/__init__.py:5``) are plain tensor functions; the landmark evaluation itself computes its soft-argmax coordinates
in ``cinema_heatmap_metrics`` (:func:`cinema_amd.segmentation.landmark.train.landmark_detection_metrics`)."""

from __future__ import annotations

import numpy as np
import torch

# <= 40 %: reduced EF, > 55 %: normal EF, in between: borderline EF (cinema/metric.py:14-16)
REDUCED_EF = 40
NORMAL_EF = 55


def _counts(logits: torch.Tensor, labels: torch.Tensor | None = None) -> torch.Tensor:
    from cinema_amd import hip as K

    if labels is None:
        labels = torch.zeros((logits.shape[0], *logits.shape[2:]), dtype=torch.int32, device=logits.device)
    return K.seg_metric_counts(logits.float().contiguous(), labels.to(torch.int32).contiguous()).to(torch.float32)  # (batch, n_classes, 6)


def stability_score(logits: torch.Tensor, threshold: float = 0.0, threshold_offset: float = 1.0) -> torch.Tensor:
    """IoU of the masks ``logits - mean_c(logits) >= threshold +/- threshold_offset`` per (sample, class), NaN where the low-threshold mask is empty
    (reference ``stability_score``, ``cinema/metric.py:19-42``, through monai ``compute_iou``).  The kernel implements the reference's defaults
    (threshold 0, offset 1), which is how every call site uses it."""
    if threshold != 0.0 or threshold_offset != 1.0:
        raise NotImplementedError("cinema_amd stability_score: the reference's defaults (threshold 0, offset 1) only")
    c = _counts(logits)
    hi, lo, both = c[..., 3], c[..., 4], c[..., 5]
    return torch.where(lo > 0, both / (hi + lo - both).clamp_min(1e-30), torch.full_like(lo, float("nan")))


def heatmap_argmax(heatmap: torch.Tensor) -> torch.Tensor:
    """(batch, 3, w, h) -> (batch, 6) integer coordinates (x0, y0, x1, y1, x2, y2) of the maximum of each of the three maps
    (reference ``cinema/metric.py:45-59``)."""
    b, c, w, h = heatmap.shape
    flat = heatmap.reshape(b, c, w * h).argmax(dim=2)
    return torch.stack((flat // h, flat % h), dim=2).reshape(b, 2 * c)


def heatmap_soft_argmax(heatmap: torch.Tensor, beta: float = 1000.0) -> torch.Tensor:
    """Expected coordinate under softmax(beta * heatmap) over the map, truncated to integers: (batch, 3, w, h) -> (batch, 6)
    (reference ``cinema/metric.py:62-81``).  The expectation separates: E[x] = sum_x x * sum_y p(x, y), E[y] likewise."""
    b, c, w, h = heatmap.shape
    prob = torch.softmax(heatmap.reshape(b, c, w * h) * beta, dim=2).reshape(b, c, w, h)
    ex = (prob.sum(dim=3) * torch.arange(w, device=heatmap.device)).sum(dim=2)
    ey = (prob.sum(dim=2) * torch.arange(h, device=heatmap.device)).sum(dim=2)
    return torch.stack((ex, ey), dim=2).reshape(b, 2 * c).to(torch.long)


def get_volumes(mask: torch.Tensor, spacing: tuple) -> torch.Tensor:
    """Volume in ml of every class of a mask (batch, n_classes, ...) (reference ``cinema/metric.py:84-96``): the plain sum over the spatial axes on
    either device, so soft or multi-hot masks and all-zero voxels give the reference's numbers (a voxel-count kernel would call an all-zero voxel class 0)."""
    vol = float(np.prod([float(s) for s in spacing])) / 1000.0
    return mask.sum(dim=tuple(range(2, mask.ndim))) * vol


def _quantile(d: torch.Tensor, q: float) -> torch.Tensor:
    """torch.quantile's default (linear interpolation between the two nearest order statistics) from one sort; no size limit."""
    s, _ = torch.sort(d)
    pos = q * (s.numel() - 1)
    lo = int(pos)
    hi = min(lo + 1, s.numel() - 1)
    return s[lo] + (s[hi] - s[lo]) * (pos - lo)


def hausdorff_distance_95(pred_label: torch.Tensor, true_label: torch.Tensor, n_classes: int, spacing: tuple, percentile: float = 95.0) -> torch.Tensor:
    """Symmetric 95th-percentile Hausdorff distance of every foreground class: label maps (batch, *spatial) with 2 or 3 spatial axes -> (batch, n_classes)
    (reference ``cinema/segmentation/train.py:262-267`` -> monai ``compute_hausdorff_distance(percentile=95, spacing=spacing)``).  monai's algorithm, restated
    (the package is absent: parity UNPINNED, cross-checked against scipy in the tests): surface = mask XOR binary_erosion(mask); directed distances = Euclidean
    distance transform of the other surface's complement, read at this surface's voxels; per direction the 95 % quantile (linear interpolation), then the
    maximum of the two.  Both surfaces empty -> NaN, exactly one empty -> inf (what monai's inf-filled distance maps produce).  Surfaces come from
    ``cinema_mask_edges``, nearest-surface distances from ``cinema_min_dist``; the variable-length point lists are built with ``torch.nonzero`` (this is the
    evaluation path: one host round trip per class is fine)."""
    from cinema_amd import hip as K

    nd = pred_label.dim() - 1
    c = n_classes + 1
    ep = K.mask_edges(pred_label.to(torch.int32).contiguous(), c)
    et = K.mask_edges(true_label.to(torch.int32).contiguous(), c)
    sp = torch.tensor([float(v) for v in spacing][:nd], dtype=torch.float32, device=pred_label.device)
    out = torch.full((pred_label.shape[0], n_classes), float("nan"), dtype=torch.float32, device=pred_label.device)

    def points(e: torch.Tensor) -> torch.Tensor:
        p = torch.nonzero(e).to(torch.float32) * sp
        return torch.nn.functional.pad(p, (0, 3 - nd)).contiguous()

    for b in range(pred_label.shape[0]):
        for k in range(1, c):
            pa, pb = points(ep[b, k]), points(et[b, k])
            if pa.shape[0] == 0 and pb.shape[0] == 0:
                continue
            if pa.shape[0] == 0 or pb.shape[0] == 0:
                out[b, k - 1] = float("inf")
                continue
            q = percentile / 100.0
            out[b, k - 1] = torch.maximum(_quantile(K.min_dist(pa, pb), q), _quantile(K.min_dist(pb, pa), q))
    return out


def ejection_fraction(edv, esv):  # noqa: ANN001, ANN201
    """(EDV - ESV) / EDV x 100 (reference ``cinema/metric.py:99-112``)."""
    return (edv - esv) / edv * 100.0


def coefficient_of_variance(x: np.ndarray, y: np.ndarray) -> float:
    """Coefficient of variance of two measurements (reference ``cinema/metric.py:115-130``)."""
    s2 = (x - y) ** 2 / 2
    m = (x + y) / 2
    return float(np.sqrt(np.mean(s2 / m**2)))


def get_ef_region(x: float) -> int:
    """0 reduced (<= 40), 1 borderline (<= 55), 2 normal (reference ``cinema/metric.py:133-146``)."""
    if x <= REDUCED_EF:
        return 0
    if x <= NORMAL_EF:
        return 1
    return 2
