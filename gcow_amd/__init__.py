"""gcow_amd -- MI355X-native ZFP-style gradient codec (drop-in for fpgasystems/gcow's sw/ encoder/decoder).

The product is libgcow.so (gcow_amd/lib, C ABI in include/gcow.h): hand-written gfx950 HIP kernels behind the
reference's sw/ call surface. This package is the Python host binding: ctypes over the C ABI, torch for device
memory, streams and torch.distributed (RCCL).
"""
from ._ffi import GcowError, GcowParams, load  # noqa: F401

__all__ = ["GcowError", "GcowParams", "load", "codec", "dist", "TensorListRoundtrip", "roundtrip_tensors",
           "roundtrip_gradients", "TensorListRelative", "roundtrip_tensors_relative", "roundtrip_gradients_relative",
           "TensorListFitted", "rate_table_tensors", "roundtrip_tensors_fitted", "roundtrip_gradients_fitted",
           "TensorListFittedPerTensor", "rate_tables_tensors", "fit_device_batch",
           "roundtrip_tensors_fitted_per_tensor", "roundtrip_gradients_fitted_per_tensor"]


def __getattr__(name):
    # codec / dist import torch; keep `import gcow_amd` light for the C-ABI-only callers.
    if name in ("codec", "dist"):
        import importlib
        return importlib.import_module("." + name, __name__)
    if name in ("TensorListRoundtrip", "roundtrip_tensors", "roundtrip_gradients", "TensorListRelative",
                "roundtrip_tensors_relative", "roundtrip_gradients_relative", "TensorListFitted",
                "rate_table_tensors", "roundtrip_tensors_fitted", "roundtrip_gradients_fitted",
                "TensorListFittedPerTensor", "rate_tables_tensors", "fit_device_batch",
                "roundtrip_tensors_fitted_per_tensor", "roundtrip_gradients_fitted_per_tensor"):
        import importlib
        return getattr(importlib.import_module(".codec", __name__), name)
    raise AttributeError(name)
