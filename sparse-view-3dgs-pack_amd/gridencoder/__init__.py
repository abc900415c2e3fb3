"""`gridencoder` stand-in (DNGaussian/gridencoder: `from gridencoder import GridEncoder`, encoding.py:63-69): the
multi-resolution hash / tiled grid encoder, served by libgsplat_hip.so (csrc/gs_encoding.hip).  No CPU fallback."""
from .grid import GridEncoder, _grid_encode, grid_encode  # noqa: F401

__all__ = ["GridEncoder", "grid_encode", "_grid_encode"]
