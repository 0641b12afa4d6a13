"""Host-side checks of the landmark localisation modules (reference cinema/segmentation/landmark/train.py, cinema/regression/landmark/train.py): the import
surface, the relative-distance matrix, the Wing constant and the coordinate metrics against hand-computed values."""

from __future__ import annotations

import math

import numpy as np
import pytest
import torch


def test_reference_landmark_imports_resolve_to_cinema_amd() -> None:
    import cinema
    from cinema.regression.landmark.train import (  # noqa: F401
        LandmarkRegTrainStep,
        WingLoss,
        get_coords_from_batch,
        get_relative_distances,
        landmark_regression_eval_dataloader,
        landmark_regression_loss,
    )
    from cinema.segmentation.landmark.train import (  # noqa: F401
        LandmarkTrainStep,
        _landmark_detection_loss,
        get_segmentation_model,
        landmark_detection_coords_metrics,
        landmark_detection_eval,
        landmark_detection_eval_dataloader,
        landmark_detection_forward,
        landmark_detection_loss,
        landmark_detection_metrics,
    )
    from cinema_amd.regression.landmark import train as reg
    from cinema_amd.segmentation.landmark import train as seg

    assert cinema.segmentation.landmark.train is seg and cinema.regression.landmark.train is reg
    assert WingLoss is reg.WingLoss and LandmarkTrainStep is seg.LandmarkTrainStep
    from cinema_amd.segmentation.train import segmentation_eval, segmentation_loss

    # the reference's partials: the loss through segmentation_loss, the evaluation through segmentation_eval (softmax aggregation, a reference quirk)
    assert landmark_detection_loss.func is segmentation_loss and landmark_detection_loss.keywords["loss_fn"] is _landmark_detection_loss
    assert landmark_detection_eval.func is segmentation_eval and landmark_detection_eval.keywords["metrics_fn"] is landmark_detection_metrics


def test_relative_distances_hand_computed() -> None:
    from cinema_amd.regression.landmark.train import get_relative_distances

    coords = torch.tensor([[10.0, 20.0, 30.0, 40.0, 50.0, 0.0], [0.0, 0.0, 2.0, 0.0, 0.0, 4.0]])
    # point 1 minus the midpoint of points 2 and 3, and so on
    want = torch.tensor([[10 - 40.0, 20 - 20.0, 30 - 30.0, 40 - 10.0, 50 - 20.0, 0 - 30.0], [-1.0, -2.0, 2.0, -2.0, -1.0, 4.0]])
    assert torch.equal(get_relative_distances(coords), want)
    assert get_relative_distances(coords.double()).dtype == torch.float64


def test_wing_constant_and_cpu_formula() -> None:
    from cinema_amd.regression.landmark.train import WingLoss

    wl = WingLoss()
    assert wl.w == 10 and wl.epsilon == 2
    assert wl.c == pytest.approx(10 - 10 * math.log(6.0), rel=1e-12) and wl.c == pytest.approx(-7.917594692280549, rel=1e-12)
    assert WingLoss(w=4, epsilon=1).c == pytest.approx(4 - 4 * math.log(5.0), rel=1e-12)
    pred = torch.tensor([[0.0, 3.0, 15.0]])
    true = torch.tensor([[0.0, 1.0, 0.0]])
    # e = 0 -> 0; e = 2 < 10 -> 10 log 2; e = 15 >= 10 -> 15 - c
    want = (0.0 + 10 * math.log(2.0) + 15 - (10 - 10 * math.log(6.0))) / 3
    assert float(wl(pred, true)) == pytest.approx(want, rel=1e-6)


def test_coords_metrics_hand_computed() -> None:
    from cinema_amd.segmentation.landmark.train import landmark_detection_coords_metrics

    pred = torch.tensor([[3, 4, 10, 10, 0, 0], [1, 1, 1, 1, 1, 1]])
    true = torch.tensor([[0, 0, 10, 10, 6, 8], [1, 1, 1, 1, 1, 1]])
    m = landmark_detection_coords_metrics(pred, true, (1.0, 1.0))
    assert list(m) == ["pred_x1", "pred_y1", "pred_x2", "pred_y2", "pred_x3", "pred_y3", "true_x1", "true_y1", "true_x2", "true_y2", "true_x3", "true_y3",
                       "distance1", "distance2", "distance3", "mean_distance"]
    assert torch.allclose(m["distance1"], torch.tensor([5.0, 0.0]))
    assert torch.allclose(m["distance2"], torch.tensor([0.0, 0.0]))
    assert torch.allclose(m["distance3"], torch.tensor([10.0, 0.0]))
    assert torch.allclose(m["mean_distance"], torch.tensor([5.0, 0.0]))
    assert torch.equal(m["pred_x3"], pred[:, 4]) and torch.equal(m["true_y1"], true[:, 1])
    # anisotropic spacing scales x and y separately
    m2 = landmark_detection_coords_metrics(pred.float(), true.float(), (2.0, 0.5))
    assert float(m2["distance1"][0]) == pytest.approx(math.hypot(6.0, 2.0))
    assert float(m2["distance3"][0]) == pytest.approx(math.hypot(12.0, 4.0))


def test_coords_from_batch_uses_the_heatmap_maxima() -> None:
    from cinema_amd.regression.landmark.train import get_coords_from_batch

    label = torch.zeros(2, 3, 8, 6)
    pts = [[(1, 2), (7, 5), (0, 0)], [(4, 4), (3, 1), (6, 2)]]
    for b, row in enumerate(pts):
        for c, (x, y) in enumerate(row):
            label[b, c, x, y] = 1.0
    coords, scales = get_coords_from_batch({"lax_2c_image": torch.zeros(2, 1, 8, 6), "lax_2c_label": label}, "lax_2c")
    assert torch.equal(scales, torch.tensor([[8, 6, 8, 6, 8, 6]]))
    want = torch.tensor([[x for p in row for x in p] for row in pts], dtype=torch.float32) / torch.tensor([8.0, 6.0, 8.0, 6.0, 8.0, 6.0])
    assert torch.allclose(coords, want)
    assert np.all(coords.numpy() <= 1.0)
