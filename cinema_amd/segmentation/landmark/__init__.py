"""Landmark detection by heatmaps with ConvUNetR on the HIP path (interface of the reference ``cinema/segmentation/landmark``)."""
