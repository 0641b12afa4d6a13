"""Landmark localisation by coordinate regression with ConvViT on the HIP path (interface of the reference ``cinema/regression/landmark``)."""
