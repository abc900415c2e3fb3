"""Loads the product library csrc/libgsplat_hip.so (prefix ``gs_``).

There is deliberately no fallback: if the HIP library has not been built, or the process has no
GPU, every operator raises.
"""
import ctypes as C
import os
import threading

# torch must be loaded BEFORE the library: both link libamdhip64 and have to share ONE HIP runtime (the
# streams and device pointers handed across the C ABI come from torch).  Loading the library first would
# bind it to a second copy of the runtime and every launch would fail with hipErrorNoDevice.
import torch  # noqa: F401,E402

from .capi import CApi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "csrc", "libgsplat_hip.so")

_lock = threading.Lock()
_api = None


def hip_api():
    global _api
    if _api is None:
        with _lock:
            if _api is None:
                _api = CApi(LIB_PATH, "gs_")
    return _api


def stream_of(t):
    """The current stream of t's device as the C ABI takes it; None for a tensor that is not on the GPU (the CPU oracle's
    entries take no stream).  A caller that hands device pointers on must have rejected CPU tensors before."""
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream) if t.is_cuda else None


def gpu_tensors(what, tensors, dtypes=(torch.float32,), contiguous=False):
    """The input check of the small-kernel modules, after their shape checks: EVERY tensor's device, then every tensor's dtype
    (dtypes=None: devices only).  contiguous: -> the tensors, contiguous.  A module whose order is tensor by tensor calls it
    once per tensor."""
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError("%s expects CUDA(HIP) tensors - there is no CPU path" % what)
    if dtypes is not None:
        for t in tensors:
            if t.dtype not in dtypes:
                raise RuntimeError("%s: fp32 only (got %s)" % (what, t.dtype))
    return [t.contiguous() for t in tensors] if contiguous else None
