"""Long RDMA messages (include/switchml_messages.h): the plane kernels with one
exponent per message of msg_numel elements, any multiple of MSG_NUMEL_STEP up
to MSG_NUMEL_MAX.  The argument shapes are those of planes.py's exponents,
quantize_pack, dequantize and roundtrip_loopback, with msg_numel in place of
packet_numel."""
from __future__ import annotations

from .abi import MSG_NUMEL_MAX, MSG_NUMEL_STEP, call, lib
from .glue import _dev, _float_type, _opt, _stream, _torch
from .planes import typed_slice_table


def msg_numel_supported(msg_numel: int) -> bool:
    return 0 <= msg_numel < 2 ** 32 and bool(lib().sml_msg_numel_supported(msg_numel))


def _num_msgs(numel: int, msg_numel: int) -> int:
    if not msg_numel_supported(msg_numel):
        raise ValueError(f"msg_numel must be a multiple of {MSG_NUMEL_STEP} in {MSG_NUMEL_STEP}..{MSG_NUMEL_MAX}, "
                         f"got {msg_numel}")
    return -(-numel // msg_numel)


def msg_exponents(x, msg_numel: int, out=None, stream=None):
    torch = _torch()
    if out is None:
        out = torch.empty(_num_msgs(x.numel(), msg_numel), dtype=torch.int8, device=x.device)
    call("sml_msg_exponents", _dev(x, x.dtype, "x"), _float_type(x.dtype, "x"), x.numel(), msg_numel,
         _dev(out, torch.int8, "exps"), _stream(stream, x))
    return out


def msg_quantize_pack(x, msg_numel: int, num_workers: int = 1, global_exps=None, payload=None, exps_out=None,
                      want_exps: bool = True, flags: int = 0, stream=None):
    """Returns (payload int32[B*M] (BE words unless FLAG_PAYLOAD_LE), exps int8[B] or None)."""
    torch = _torch()
    B = _num_msgs(x.numel(), msg_numel)
    if payload is None:
        payload = torch.empty(B * msg_numel, dtype=torch.int32, device=x.device)
    if global_exps is None and want_exps and exps_out is None:
        exps_out = torch.empty(B, dtype=torch.int8, device=x.device)
    call("sml_msg_quantize_pack", _dev(x, x.dtype, "x"), _float_type(x.dtype, "x"), x.numel(), msg_numel, num_workers,
         _opt(global_exps, torch.int8, "global_exps"), _dev(payload, torch.int32, "payload"),
         _opt(exps_out, torch.int8, "exps_out"), flags, _stream(stream, x))
    return payload, (global_exps if global_exps is not None else exps_out)


def msg_dequantize(payload, exps, numel: int, msg_numel: int, num_workers: int = 1, out=None, flags: int = 0,
                   stream=None, out_dtype=None):
    """K4 into `out`, or into a new bucket of `out_dtype` (default fp32)."""
    torch = _torch()
    if out is None:
        out = torch.empty(numel, dtype=out_dtype or torch.float32, device=payload.device)
    elif out_dtype is not None and out.dtype != out_dtype:
        raise TypeError(f"out is {out.dtype}, out_dtype {out_dtype}")
    call("sml_msg_dequantize", _dev(payload, torch.int32, "payload"), _dev(exps, torch.int8, "exps"), numel, msg_numel,
         num_workers, _dev(out, out.dtype, "out"), _float_type(out.dtype, "out"), flags, _stream(stream, payload))
    return out


def msg_roundtrip_loopback(x, msg_numel: int, num_workers: int = 1, out=None, payload=None, exps_out=None,
                           flags: int = 0, stream=None):
    torch = _torch()
    if out is None:
        out = torch.empty_like(x)
    call("sml_msg_roundtrip_loopback", _dev(x, x.dtype, "x"), _dev(out, x.dtype, "out"), _float_type(x.dtype, "x"),
         x.numel(), msg_numel, num_workers, _opt(payload, torch.int32, "payload"),
         _opt(exps_out, torch.int8, "exps_out"), flags, _stream(stream, x))
    return out


def msg_roundtrip_loopback_batch(slices, msg_numel: int, num_workers: int = 1, flags: int = 0, stream=None):
    """planes.roundtrip_loopback_batch with msg_numel in place of packet_numel
    (include/switchml_msg_batch.h): `slices` is a list of (x, out) tensor
    pairs, and slice i gets exactly msg_roundtrip_loopback(x_i, out=out_i)."""
    arr, st = typed_slice_table(slices, stream)
    call("sml_msg_roundtrip_loopback_batch", arr, len(slices), msg_numel, num_workers, flags, st)
