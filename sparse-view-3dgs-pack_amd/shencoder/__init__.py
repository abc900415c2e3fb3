"""`shencoder` stand-in (DNGaussian/shencoder: `from shencoder import SHEncoder`, encoding.py:59-61): the Cartesian
real spherical harmonics up to degree 8, served by libgsplat_hip.so (csrc/gs_encoding.hip).  No CPU fallback."""
from .sphere_harmonics import SHEncoder, sh_encode  # noqa: F401

__all__ = ["SHEncoder", "sh_encode"]
