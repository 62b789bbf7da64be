from .autoencoder import InnerProductDecoder, GAE, VGAE

__all__ = ["InnerProductDecoder", "GAE", "VGAE"]
