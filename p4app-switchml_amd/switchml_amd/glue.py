"""The torch side of every wrapper: streams, tensor checks and the pointer
tables the C ABI takes.  Tensors are torch CUDA (HIP) tensors or pinned host
memory; torch is imported on first use, not with the package."""
import ctypes

from .abi import BFLOAT16, FLOAT16, FLOAT32


def _torch():
    import torch
    return torch


def _stream(stream, like=None):
    """The HIP stream to launch on: the given one, else torch's current
    stream of `like`'s device (else of the current device)."""
    torch = _torch()
    if stream is None:
        dev = like.device if like is not None and getattr(like, "is_cuda", False) else None
        stream = torch.cuda.current_stream(dev)
    return ctypes.c_void_p(stream.cuda_stream)


def _dev(t, dtype, name):
    torch = _torch()
    if not isinstance(t, torch.Tensor) or not (t.is_cuda or t.is_pinned()):
        raise TypeError(f"{name} must be a CUDA (HIP) tensor or pinned host memory (read by the "
                        "kernel over PCIe) — the HIP path has no CPU fallback")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return ctypes.c_void_p(t.data_ptr())


def _opt(t, dtype, name):
    """_dev of an optional tensor: None stays None (a NULL pointer)."""
    return None if t is None else _dev(t, dtype, name)


def _ptr_table(planes, dtype, name, raw: bool = False):
    """The void* array of a list of tensors of `dtype`; with `raw`, an entry
    that is no tensor is a plane exposing data_ptr() / numel() only (a peer's
    mapped plane) and is taken as it is."""
    torch = _torch()
    return (ctypes.c_void_p * len(planes))(*[
        p.data_ptr() if raw and not isinstance(p, torch.Tensor) else _dev(p, dtype, name).value for p in planes])


def _float_type(dtype, name):
    """sml_data_type_t of a float bucket's torch dtype: fp32, or one of the
    16-bit types the kernels convert (the sml_*_typed entry points)."""
    torch = _torch()
    code = {torch.float32: FLOAT32, torch.float16: FLOAT16, torch.bfloat16: BFLOAT16}.get(dtype)
    if code is None:
        raise TypeError(f"{name} must be float32, float16 or bfloat16, got {dtype}")
    return code
