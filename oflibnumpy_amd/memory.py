"""Device and pinned-host memory of the resident layer: the HBM recycling pool, `DeviceBuffer` and views into memory that
somebody else owns, downloads into a pool of page-locked host blocks -- and the three small helpers every launch wrapper
shares (`_lib`, `_ptr`, `_size_query`).

SINGLE-STREAM: a recycled buffer is handed out as soon as Python drops it, which is only safe while all work is queued on
one stream (see device.py).
"""
import ctypes
import weakref

import numpy as np

from . import _native as nat


def _lib():
    nat.ensure_device()
    return nat.load()


def _ptr(buf):
    """The address of a buffer or view; None (a null pointer: "not given") stays None."""
    return buf.ptr if buf is not None else None


def _size_query(entry, *args):
    """One of the library's ofl_*_bytes entries, which answer through a trailing size_t pointer -> int."""
    n = ctypes.c_size_t(0)
    nat.check(entry(*args, ctypes.byref(n)))
    return n.value


def sync(stream=None):
    nat.check(_lib().ofl_stream_sync(stream))


class _Pool:
    """Size-bucketed free lists: hipFree synchronises the device, so chained operations recycle
    their intermediates instead of returning them to the driver."""

    def __init__(self):
        self.free = {}
        self.cached_bytes = 0
        self.limit = 64 << 30

    def take(self, nbytes):
        lst = self.free.get(nbytes)
        if lst:
            self.cached_bytes -= nbytes
            return lst.pop()
        p = ctypes.c_void_p()
        try:
            nat.check(_lib().ofl_malloc(ctypes.byref(p), nbytes))
        except nat.NativeError:
            self.trim()
            nat.check(_lib().ofl_malloc(ctypes.byref(p), nbytes))
        return p.value

    def give(self, ptr, nbytes):
        if self.cached_bytes + nbytes > self.limit:
            nat.load().ofl_free(ptr)
            return
        self.free.setdefault(nbytes, []).append(ptr)
        self.cached_bytes += nbytes

    def trim(self):
        lib = nat.load()
        for lst in self.free.values():
            for p in lst:
                lib.ofl_free(p)
        self.free.clear()
        self.cached_bytes = 0


_pool = _Pool()


def empty_cache():
    _pool.trim()


def _release(ptr, nbytes):
    try:
        _pool.give(ptr, nbytes)
    except Exception:       # interpreter shutdown
        pass


_PINNED_MIN = 1 << 20        # results below 1 MiB stay pageable


def _download(ptr, shape, dtype, stream=None):
    """Device memory at `ptr` -> a fresh array (what to_host of a buffer or a view does)."""
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    if nbytes >= _PINNED_MIN:
        out = _pinned_pool.array(shape, dtype)
        if out is not None:
            nat.check(_lib().ofl_download_async(out.ctypes.data, ptr, nbytes, stream))
            nat.check(_lib().ofl_stream_sync(stream))
            return out
    out = np.empty(shape, dtype)
    if out.nbytes:
        nat.check(_lib().ofl_download(out.ctypes.data, ptr, out.nbytes, stream))
    return out


class _Span:
    """What a DeviceBuffer and a _BufferView share: an address `ptr` and a length `nbytes` in device memory."""

    __slots__ = ()

    def to_host(self, shape, dtype, stream=None):
        """Download into a fresh array.  Large results land in page-locked memory from a recycling pool (a DMA at link
        speed; a pageable destination of fresh pages costs 2-3 x as long in page faults) -- the array owns its block and
        returns it to the pool when it is garbage-collected."""
        return _download(self.ptr, shape, dtype, stream)

    def view(self, offset, nbytes):
        """`nbytes` bytes from byte `offset` on -- rows r0..r1 of a field, field k of a batch -- as a _BufferView that keeps
        this object alive."""
        return _BufferView(self.ptr + offset, nbytes, owner=self)


class DeviceBuffer(_Span):
    """A block of HBM owned by this process (ofl_malloc / pooled)."""

    __slots__ = ("ptr", "nbytes", "_fin", "__weakref__")

    def __init__(self, nbytes):
        self.nbytes = max(int(nbytes), 16)
        self.ptr = _pool.take(self.nbytes)
        self._fin = weakref.finalize(self, _release, self.ptr, self.nbytes)

    @classmethod
    def from_host(cls, arr, stream=None):
        arr = np.ascontiguousarray(arr)
        buf = cls(arr.nbytes)
        if arr.nbytes:
            nat.check(_lib().ofl_upload(buf.ptr, arr.ctypes.data, arr.nbytes, stream))
            # the source array may be a temporary: make the (possibly staged) copy complete now
            nat.check(_lib().ofl_stream_sync(stream))
        return buf

    @classmethod
    def zeros(cls, nbytes, stream=None):
        buf = cls(nbytes)
        nat.check(_lib().ofl_memset(buf.ptr, 0, buf.nbytes, stream))
        return buf


class _BufferView(_Span):
    """An address and a length in memory that somebody else owns: part of a DeviceBuffer, or memory of another framework that a
    field has adopted.  `owner` is whatever keeps that memory alive; it travels with the view, so that every field or image
    that shares the view (relabel, scaling, an exported view) holds the owner too.  A view has no finaliser: the recycling pool
    never receives its pointer."""

    __slots__ = ("ptr", "nbytes", "owner")

    def __init__(self, ptr, nbytes, owner=None):
        self.ptr, self.nbytes, self.owner = ptr, int(nbytes), owner


class PinnedArray:
    """A NumPy view of page-locked host memory (ofl_host_alloc): transfers from / to it are asynchronous DMA."""

    def __init__(self, shape, dtype):
        self.shape, self.dtype = tuple(int(v) for v in shape), np.dtype(dtype)
        self.nbytes = max(int(np.prod(self.shape)) * self.dtype.itemsize, 16)
        p = ctypes.c_void_p()
        nat.check(_lib().ofl_host_alloc(ctypes.byref(p), self.nbytes))
        self.ptr = p.value
        self._fin = weakref.finalize(self, nat.load().ofl_host_free, self.ptr)
        buf = (ctypes.c_char * self.nbytes).from_address(self.ptr)
        self.array = np.frombuffer(buf, dtype=self.dtype, count=int(np.prod(self.shape))).reshape(self.shape)


class _PinnedBlock:
    __slots__ = ("ptr", "nbytes", "__weakref__")

    def __init__(self, ptr, nbytes):
        self.ptr, self.nbytes = ptr, nbytes


class _PinnedPool:
    """Page-locked host blocks for downloads, recycled by size (hipHostMalloc of 66 MB takes milliseconds)."""

    def __init__(self, limit=8 << 30):
        self.free, self.in_use, self.limit = {}, 0, limit

    def _give(self, ptr, nbytes):
        try:
            self.in_use -= nbytes
            self.free.setdefault(nbytes, []).append(ptr)
        except Exception:       # interpreter shutdown
            pass

    def array(self, shape, dtype):
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape)) * dtype.itemsize
        if self.in_use + nbytes > self.limit:
            return None
        lst = self.free.get(nbytes)
        if lst:
            ptr = lst.pop()
        else:
            p = ctypes.c_void_p()
            try:
                nat.check(_lib().ofl_host_alloc(ctypes.byref(p), nbytes))
            except nat.NativeError:
                return None
            ptr = p.value
        self.in_use += nbytes
        block = _PinnedBlock(ptr, nbytes)
        weakref.finalize(block, self._give, ptr, nbytes)
        buf = (ctypes.c_char * nbytes).from_address(ptr)
        buf._block = block                      # the array's base keeps the block alive
        return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)


_pinned_pool = _PinnedPool()

