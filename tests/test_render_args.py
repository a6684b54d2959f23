"""Argument checks that need no GPU: pnrt_create reads PNRT_BATCH_BYTES before it
touches a device, and PathTracer.render checks its frame numbers before it
calls into the library."""
import ctypes
import os

import pytest

from pnraytracing_amd import _native as N
from pnraytracing_amd.tracer import PathTracer

PNRT_E_ARG = -1
REJECTED = ["3e9", "abc", "-1", "", "12x", " 12", "12 ", "+5", "0x10", "1.5", "18446744073709551616"]


@pytest.mark.parametrize("text", REJECTED)
def test_create_refuses_misspelt_batch_bytes(text):
    """Decimal digits only and a value that fits 64 bits: strtoull's reading of
    `3e9` as a 3-byte cap, or of `abc` as no cap, is PNRT_E_ARG instead."""
    lib = N.device_lib()
    ctx = ctypes.c_void_p()
    old = os.environ.get("PNRT_BATCH_BYTES")
    os.environ["PNRT_BATCH_BYTES"] = text
    try:
        rc = lib.pnrt_create(0, ctypes.byref(ctx))
    finally:
        if old is None:
            del os.environ["PNRT_BATCH_BYTES"]
        else:
            os.environ["PNRT_BATCH_BYTES"] = old
    assert rc == PNRT_E_ARG and not ctx.value


@pytest.mark.parametrize("text", ["0", "3000000000", "18446744073709551615"])
def test_create_accepts_decimal_batch_bytes(text):
    """... and a well-formed value is not what fails the call (without a GPU it
    fails later, with PNRT_E_HIP)."""
    lib = N.device_lib()
    ctx = ctypes.c_void_p()
    os.environ["PNRT_BATCH_BYTES"] = text
    try:
        rc = lib.pnrt_create(0, ctypes.byref(ctx))
    finally:
        del os.environ["PNRT_BATCH_BYTES"]
    if ctx.value:
        lib.pnrt_destroy(ctx)
    assert rc != PNRT_E_ARG


@pytest.mark.parametrize("first,n", [(2**32 + 5, 1), (2**32, 1), (-1, 1), (0, 2**32), (0, -1)])
def test_render_refuses_frame_numbers_outside_uint32(first, n):
    pt = PathTracer.__new__(PathTracer)          # no context: the check comes before any library call
    with pytest.raises(ValueError):
        pt.render(first, n)
