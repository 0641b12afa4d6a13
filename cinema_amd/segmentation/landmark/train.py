"""Landmark detection by heatmaps (interface of the reference ``cinema/segmentation/landmark/train.py``): ConvUNetR predicts one heatmap per landmark; the
loss is sigmoid soft Dice + BCE against soft Gaussian labels; evaluation reads soft-argmax coordinates and per-landmark Dice.

The loss, the sliding-window aggregation and the metrics are HIP kernels (``csrc/landmark.hip``).  Not rebuilt: ``load_dataset`` /
``LandmarkDetectionDataset`` and the hydra ``main`` (data loading and the control plane are outside this build for every task)."""

from __future__ import annotations

from functools import partial

import torch

from cinema_amd import hip as K
from cinema_amd.segmentation.train import (  # noqa: F401  (get_segmentation_model: re-exported, as the reference imports it from here)
    SegTrainStep,
    get_segmentation_model,
    segmentation_eval,
    segmentation_eval_dataloader,
    segmentation_loss,
    segmentation_loss_tensors,
)


class _LandmarkLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits: torch.Tensor, labels: torch.Tensor):  # noqa: ANN001, ANN205
        b, c = logits.shape[0], logits.shape[1]
        rows = logits.detach().float().movedim(1, -1).contiguous().reshape(-1, c)  # channels-last rows (layout only)
        lab = labels.detach().float().contiguous()  # channels-first, read as is by the kernels
        out4, coef = K.landmark_loss_fwd(rows, lab, b)
        ctx.save_for_backward(rows, lab, coef)
        ctx.shape, ctx.dtype = tuple(logits.shape), logits.dtype
        return out4[0].clone(), out4[1].clone(), out4[2].clone()

    @staticmethod
    def backward(ctx, g_loss, g_bce, g_dice):  # noqa: ANN001, ANN205
        rows, lab, coef = ctx.saved_tensors
        b, c = ctx.shape[0], ctx.shape[1]
        if g_bce is not None and bool((g_bce != 0).any()) or g_dice is not None and bool((g_dice != 0).any()):
            raise NotImplementedError("only the total loss is differentiable (the metrics are reported values)")
        up = g_loss.reshape(1).float().contiguous()
        d = K.landmark_loss_bwd(rows, lab, b, coef, up)
        return d.reshape(b, *ctx.shape[2:], c).movedim(-1, 1).to(ctx.dtype), None


def _landmark_detection_loss(logits: torch.Tensor, labels: torch.Tensor) -> tuple:
    """monai ``DiceLoss(include_background=True)`` of sigmoid(logits) + ``BCEWithLogitsLoss`` against soft heatmap labels (reference ``train.py:109-132``).

    ``logits`` (batch, n_landmarks, ...), ``labels`` (batch, n_landmarks, ...) float; returns (loss, {"bce_loss", "dice_loss", "loss"})."""
    if tuple(logits.shape) != tuple(labels.shape):
        raise ValueError(f"logits {tuple(logits.shape)} and labels {tuple(labels.shape)} do not match")
    loss, bce, dice = _LandmarkLoss.apply(logits, labels)
    return loss, {"bce_loss": bce.detach(), "dice_loss": dice.detach(), "loss": loss}


landmark_detection_loss = partial(segmentation_loss, loss_fn=_landmark_detection_loss)
landmark_detection_loss_tensors = partial(segmentation_loss_tensors, loss_fn=_landmark_detection_loss)


class LandmarkTrainStep(SegTrainStep):
    """One optimisation step of the landmark-detection fine-tuning loop (reference ``cinema/train.py:85-168`` with ``landmark_detection_loss``): the fused
    step of :class:`SegTrainStep` (clip, layer-decay AdamW, data parallelism, ``replay=True`` through ``cinema_amd.replay.RecordedLandmarkStep``) with the
    heatmap loss.  Labels ``{view}_label`` are float heatmaps (batch, n_landmarks, *image_size)."""

    loss_tensors = staticmethod(landmark_detection_loss_tensors)
    recorded_step = "RecordedLandmarkStep"


# ---------------------------------------------------------------------------------------------------------------------
# evaluation path (reference train.py:135-295)
# ---------------------------------------------------------------------------------------------------------------------
def landmark_detection_forward(model, image_dict: dict, patch_size_dict: dict, amp_dtype: torch.dtype | None = None, window_batch: int = 8) -> dict:  # noqa: ANN001, ARG001
    """Logits per view, (1, n_landmarks, *image_size), with a sliding window over the ONE view whose image is larger than its patch size (reference
    ``train.py:135-208``): the windows' sigmoid probabilities are averaged where windows overlap and returned as ``log(p / (1 - p))`` (+inf where the mean
    rounds to 1, as in the reference); the other views' outputs are the same of their window-mean probability.

    MI355X path: windows go through the model ``window_batch`` at a time (eval mode: samples are independent), ``cinema_landmark_window_accumulate`` adds
    each window's sigmoid in grid order, ``cinema_landmark_window_finish`` forms the logits.  ``amp_dtype`` is accepted for signature compatibility."""
    from cinema_amd.transform import get_patch_grid, patch_grid_sample

    for view, image in image_dict.items():
        if any(s < p for s, p in zip(image.shape[2:], patch_size_dict[view])):
            raise ValueError(f"For view {view}, image size {image.shape[2:]} is smaller than patch size {patch_size_dict[view]}.")
    views = list(image_dict.keys())
    need_patch = {v: tuple(image_dict[v].shape[2:]) != tuple(patch_size_dict[v]) for v in views}
    if not any(need_patch.values()):
        with torch.no_grad():
            return model(image_dict)
    if sum(need_patch.values()) > 1:
        raise ValueError(f"Only support patching on one view for now, but got {need_patch}.")
    batch_size = image_dict[views[0]].shape[0]
    if batch_size != 1:
        raise ValueError(f"Expected batch size 1 for patching, but got {batch_size}.")

    view_p = next(v for v, need in need_patch.items() if need)
    image = image_dict[view_p][0]  # (channel, *image_size)
    size = tuple(image.shape[1:])
    patch = tuple(patch_size_dict[view_p])
    starts = get_patch_grid(image_size=size, patch_size=patch, patch_overlap=tuple(s // 2 for s in patch))
    patches = patch_grid_sample(image, starts, patch)  # (n_patches, channel, *patch)
    n_patches = patches.shape[0]
    dev = image.device
    n_vox = 1
    for s in size:
        n_vox *= int(s)

    sums: dict = {}  # view -> (prob_sum [n_vox, c], count [n_vox], spatial size)
    with torch.no_grad():
        for i0 in range(0, n_patches, window_batch):
            chunk = patches[i0:i0 + window_batch]
            nb = chunk.shape[0]
            feed = {v: chunk if v == view_p else image_dict[v].expand(nb, *image_dict[v].shape[1:]) for v in views}
            out = model(feed)
            for v in views:
                lg = out[v].float()
                c = lg.shape[1]
                o_size = size if v == view_p else tuple(lg.shape[2:])
                if v not in sums:
                    nv = n_vox if v == view_p else lg[0, 0].numel()
                    sums[v] = (K.zeros((nv, c), torch.float32, dev), K.zeros((nv,), torch.float32, dev), o_size)
                rows = lg.movedim(1, -1).contiguous().reshape(nb, -1, c)  # channels-last rows per window (layout only)
                for j in range(nb):
                    # the patched view: the window at its grid start; any other view: its full image in every window (the mean over windows)
                    at = tuple(int(s) for s in starts[i0 + j]) if v == view_p else (0,) * len(o_size)
                    K.landmark_window_accumulate(rows[j], patch if v == view_p else o_size, at, o_size, sums[v][0], sums[v][1])
    return {v: K.landmark_window_finish(ps, cn).reshape(1, -1, *o_size) for v, (ps, cn, o_size) in sums.items()}


def landmark_detection_coords_metrics(pred_labels: torch.Tensor, true_labels: torch.Tensor, spacing: tuple) -> dict:
    """Coordinates (batch, 6) = (x1, y1, x2, y2, x3, y3) -> per-sample metrics of shape (batch,): the coordinates and the distances of the three landmarks
    in physical units and their mean (reference ``train.py:211-254``)."""
    d = []
    for i in range(3):
        dx = (pred_labels[:, 2 * i] - true_labels[:, 2 * i]) * spacing[0]
        dy = (pred_labels[:, 2 * i + 1] - true_labels[:, 2 * i + 1]) * spacing[1]
        d.append(torch.sqrt(dx**2 + dy**2))
    metrics = {}
    for name, t in (("pred", pred_labels), ("true", true_labels)):
        for i in range(3):
            metrics[f"{name}_x{i + 1}"] = t[:, 2 * i]
            metrics[f"{name}_y{i + 1}"] = t[:, 2 * i + 1]
    for i in range(3):
        metrics[f"distance{i + 1}"] = d[i]
    metrics["mean_distance"] = (d[0] + d[1] + d[2]) / 3
    return metrics


def landmark_detection_metrics(logits: torch.Tensor, labels: torch.Tensor, spacing: tuple) -> dict:
    """Per-sample evaluation metrics (reference ``train.py:257-288``): soft-argmax coordinates (softmax at beta = 1000 over each map, truncated to integers)
    of sigmoid(logits) and of the labels, their distances, and ``landmark_{i}_dice_score`` = 1 - monai ``DiceLoss(include_background=True,
    reduction="none")``.  One workgroup per map of ``cinema_heatmap_metrics`` reads both maps once."""
    out = K.heatmap_metrics(logits.detach().float().contiguous(), labels.detach().float().contiguous())  # (batch, n_landmarks, 8)
    b = logits.shape[0]
    metrics = landmark_detection_coords_metrics(pred_labels=out[..., 0:2].reshape(b, -1).to(torch.long),
                                                true_labels=out[..., 2:4].reshape(b, -1).to(torch.long), spacing=spacing)
    dice_loss = out[..., 7]
    if dice_loss.shape != (b, 3):
        raise ValueError(f"Invalid dice shape: {dice_loss.shape}")
    for i in range(1, 4):
        metrics[f"landmark_{i}_dice_score"] = 1.0 - dice_loss[:, i - 1]
    return metrics


# the reference's evaluation goes through segmentation_forward (softmax aggregation over windows), not landmark_detection_forward; reproduced as is
# (evaluation images are padded to the patch size, so no windows are cut there)
landmark_detection_eval = partial(segmentation_eval, metrics_fn=landmark_detection_metrics)
landmark_detection_eval_dataloader = partial(segmentation_eval_dataloader, metrics_fn=landmark_detection_metrics)
