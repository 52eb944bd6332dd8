"""pcodec_amd -- MI355X-native (gfx950 / HIP) implementation of pcodec's chunk encode / decode path.

The Python layer mirrors the reference's `pcodec` module (pco_python/src/{config,standalone,wrapped}.rs):
ChunkConfig / ModeSpec / DeltaSpec / PagingSpec / Progress, `standalone.simple_*` and `wrapped.{FileCompressor,
FileDecompressor}`, plus `paged` (the batched wrapped writer on torch device tensors), all routed through the C ABI of libpco_gfx.so (include/pco_gfx.h).  There is no CPU codec in this package.
"""
from .config import ChunkConfig, ChunkSpec, DeltaSpec, ModeSpec, PagingSpec, Progress  # noqa: F401
from . import paged, standalone, wrapped  # noqa: F401

__all__ = ["ChunkConfig", "ChunkSpec", "DeltaSpec", "ModeSpec", "PagingSpec", "Progress", "paged", "standalone", "wrapped"]
