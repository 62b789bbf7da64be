from .autoencoder import InnerProductDecoder, GAE, VGAE
from .graph_unet import GraphUNet

__all__ = ["InnerProductDecoder", "GAE", "VGAE", "GraphUNet"]
