"""Device buffers for the raw-ABI GPU tests: outputs between 0xA5 guard bands, inputs at a byte shift.

One convention: a guarded buffer holds `front` bytes, the payload and at least `guard` bytes, all 0xA5 before the call; the
kernel is handed buf.ptr + front, and read_guarded checks every byte before and behind the payload.  Each test file keeps
its own guard size and its own shifts and passes them in."""
import numpy as np

from oflibnumpy_amd import device as dev
from oflibnumpy_amd import _native as nat


def guarded(nbytes, guard, front=0):
    """a buffer of front + nbytes + guard bytes, every byte 0xA5"""
    buf = dev.DeviceBuffer(front + nbytes + guard)
    nat.check(nat.load().ofl_memset(buf.ptr, 0xA5, buf.nbytes, None))
    return buf


def place(arr, shift=0):
    """the bytes of a host array in device memory, `shift` bytes into a fresh buffer -> (buffer, address)"""
    arr = np.ascontiguousarray(arr)
    buf = dev.DeviceBuffer(arr.nbytes + shift)
    nat.check(nat.load().ofl_upload(buf.ptr + shift, arr.ctypes.data, arr.nbytes, None))
    dev.sync()
    return buf, buf.ptr + shift


def read_guarded(buf, front, size, guard, dtype, shape):
    """the `size` payload bytes `front` bytes into a guarded buffer, once the bytes around them are seen to be intact"""
    raw = buf.to_host((buf.nbytes,), np.uint8)
    assert (raw[:front] == 0xA5).all() and (raw[front + size:] == 0xA5).all() and raw[front + size:].size >= guard, "guard bytes"
    return raw[front:front + size].copy().view(dtype).reshape(shape)
