"""Process-wide tuning knobs (each returns the previous value) and two probes:
the streaming copy the bench takes as the HBM ceiling, the stall tests inject."""
import ctypes

from .abi import call, lib
from .glue import _stream


def set_grid_limit(max_workgroups: int) -> int:
    return int(lib().sml_set_grid_limit(max_workgroups))


def set_payload_nt_threshold(nbytes: int) -> int:
    """Payload planes (and K4 / round-trip outputs) of at least `nbytes`
    bytes take non-temporal stores (default 64 MiB, a quarter of the Infinity
    Cache; 2**64-1 = never, 0 = always); returns the previous threshold."""
    return int(lib().sml_set_payload_nt_threshold(nbytes))


def set_quantize_tile_slices(slices: int) -> int:
    """Slices of 256 elements per K1/K2/K3 wave tile: 4, 2 or 1 for every
    kernel (never below P/256), or 0 = the default, 2 slices for every kernel
    (never below P/256); returns the previous setting."""
    return int(lib().sml_set_quantize_tile_slices(slices))


def set_stream_tile_slices(slices: int) -> int:
    """Slices of 256 elements per K4 / fused round-trip wave tile: 4 or 2,
    or 0 = the default; returns the previous setting."""
    return int(lib().sml_set_stream_tile_slices(slices))


def set_xcd_chunk(chunk: int) -> int:
    """Workgroups per contiguous run on one XCD (0 = plain order); returns the previous value."""
    return int(lib().sml_set_xcd_chunk(chunk))


def stream_copy(src, dst, stream=None):
    """Measurement probe: non-temporal tile copy (src/dst same byte size)."""
    nbytes = src.numel() * src.element_size()
    call("sml_stream_copy", ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()), nbytes,
         _stream(stream, src))
    return dst


def debug_stall(microseconds: int, stream=None):
    """Fault injection for tests: keep `stream` busy for `microseconds` of
    device wall-clock time (<= 60 s), then end (sml_debug_stall)."""
    call("sml_debug_stall", int(microseconds), _stream(stream))
