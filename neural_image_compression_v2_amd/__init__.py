"""MI355X (gfx950) native implementation of the grid + positional-encoding + MLP coordinate-network hot path
of 21K1113/Neural_Image_Compression_V2.

Modules mirror the reference's files for this path (same function names and argument meaning):
``fp_def``, ``utils``, ``models``, ``positional_encoding``, ``var2`` (settings), ``image_compression`` (driver-level
functions), plus ``fused`` (geometry descriptors + autograd glue) and ``distributed`` (sample-sharded data
parallel step over RCCL).  All arithmetic runs in libnicv2_hip.so (C ABI: include/nicv2_hip.h); there is no
CPU or eager-torch fallback - importing the package works anywhere, calling it needs a HIP device.
"""
__version__ = "0.1.0"

from . import _lib  # noqa: F401


def library_path() -> str:
    return _lib.LIB_PATH


_HASHGRID_NAMES = ("HashGeometry", "HashGridField", "HashGridFieldBatch", "hash_batch_forward", "hash_batch_forward_backward", "hash_batch_forward_source", "hash_batch_groups",
                   "hash_batch_forward_p16", "hash_batch_groups_p16", "hash_batch_forward_backward_points", "hash_batch_point_order",
                   "hash_batch_forward_points_lod", "hash_batch_forward_backward_points_lod", "hash_batch_points_grad",
                   "hash_batch_forward_backward_points_grad", "hash_encode_points_grad_lod", "hash_fused_points_grad_lod",
                   "hash_encode_points_grad_lod_noisy", "hash_fused_forward_backward_points_grad_lod", "hash_batch_points_grad_lod",
                   "hash_batch_forward_backward_points_grad_lod", "hash_fused_forward_backward_points_weighted", "hash_mip_weights")


def __getattr__(name):
    """the hash-grid field classes and the batched wrappers, from ``hashgrid`` on first use (importing the package stays light)"""
    if name in _HASHGRID_NAMES:
        from . import hashgrid
        return getattr(hashgrid, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
