"""Unpooling (PyG 1.4.3 nn.unpool): knn_interpolate on the native engine."""
from .knn_interpolate import knn_interpolate

__all__ = ["knn_interpolate"]
