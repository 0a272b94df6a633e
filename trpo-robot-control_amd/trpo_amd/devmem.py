"""Device memory and streams for the device-resident loop (Context.act_dev and its kin), with ctypes on the HIP
runtime the library itself loaded (trpo_amd.runtime_path()): every buffer is known to the one runtime in the
process.  No torch, no further dependency.

    st = Stream(device=0)
    obs = DeviceArray.from_host(np.zeros((8, 15)), device=0)
    mean = DeviceArray((8, 3), np.float64, device=0)
    ctx.act_dev(obs, mean, seed=1, stream=st, sample=False)
    st.synchronize(); mean.to_host()
"""
import ctypes as C

import numpy as np

import trpo_amd

_DTYPES = {np.dtype(np.float64): "<f8", np.dtype(np.float32): "<f4", np.dtype(np.uint8): "|u1"}
_H2D, _D2H, _D2D = 1, 2, 3            # hipMemcpyKind

_rt = None


def runtime():
    """The process's libamdhip64, as the library resolved it."""
    global _rt
    if _rt is None:
        R = C.CDLL(trpo_amd.runtime_path())
        R.hipGetErrorString.restype = C.c_char_p
        R.hipGetErrorString.argtypes = [C.c_int]
        R.hipSetDevice.argtypes = [C.c_int]
        R.hipGetDevice.argtypes = [C.POINTER(C.c_int)]
        R.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        R.hipFree.argtypes = [C.c_void_p]
        R.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        R.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        R.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        R.hipHostMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
        R.hipHostFree.argtypes = [C.c_void_p]
        R.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
        R.hipStreamSynchronize.argtypes = [C.c_void_p]
        R.hipStreamDestroy.argtypes = [C.c_void_p]
        _rt = R
    return _rt


def _chk(rc, what):
    if rc != 0:
        raise trpo_amd.TRPOError("%s failed: HIP error %d (%s)" % (what, rc, runtime().hipGetErrorString(rc).decode()))


def _device(device):
    if device is None or device < 0:
        d = C.c_int(0)
        _chk(runtime().hipGetDevice(C.byref(d)), "hipGetDevice")
        return d.value
    return int(device)


class Stream:
    """A non-blocking HIP stream.  handle: the hipStream_t as an integer."""

    def __init__(self, device=None):
        self.device = _device(device)
        R = runtime()
        _chk(R.hipSetDevice(self.device), "hipSetDevice")
        h = C.c_void_p()
        _chk(R.hipStreamCreateWithFlags(C.byref(h), 1), "hipStreamCreateWithFlags")     # hipStreamNonBlocking
        self.handle = h.value

    def synchronize(self):
        _chk(runtime().hipStreamSynchronize(self.handle), "hipStreamSynchronize")

    def close(self):
        if self.handle:
            runtime().hipStreamSynchronize(self.handle)
            runtime().hipStreamDestroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def stream_handle(stream):
    """None, a Stream or an integer hipStream_t -> the handle (None: the callee's own stream)."""
    if stream is None:
        return None
    return stream.handle if isinstance(stream, Stream) else int(stream)


class PinnedArray:
    """Page-locked host memory as a numpy array (.array): the source or target of a copy that is to be
    asynchronous."""

    def __init__(self, shape, dtype=np.float64):
        self.array = None
        dt = np.dtype(dtype)
        shape = (int(shape),) if np.isscalar(shape) else tuple(int(s) for s in shape)
        nbytes = max(int(np.prod(shape)) * dt.itemsize, 1)
        p = C.c_void_p()
        _chk(runtime().hipHostMalloc(C.byref(p), nbytes, 0), "hipHostMalloc")
        self._p = p.value
        self.array = np.frombuffer((C.c_char * nbytes).from_address(self._p), dt, int(np.prod(shape))).reshape(shape)

    def close(self):
        if getattr(self, "_p", None):
            self.array = None
            runtime().hipHostFree(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceArray:
    """A C-contiguous array in device memory: float64, float32 or uint8.  ptr is its device address; view()
    gives an element-offset window into the same allocation (the owner must outlive it, and is kept alive by
    it); __cuda_array_interface__ describes it to any consumer of that protocol."""

    def __init__(self, shape, dtype=np.float64, device=None, _base=None, _ptr=None):
        self.dtype = np.dtype(dtype)
        if self.dtype not in _DTYPES:
            raise TypeError("DeviceArray holds float64, float32 or uint8, not %s" % self.dtype)
        self.shape = (int(shape),) if np.isscalar(shape) else tuple(int(s) for s in shape)
        self.size = int(np.prod(self.shape))
        self.nbytes = self.size * self.dtype.itemsize
        self._base = _base
        if _base is not None:
            self.device, self.ptr = _base.device, _ptr
            return
        self.device = _device(device)
        R = runtime()
        _chk(R.hipSetDevice(self.device), "hipSetDevice")
        p = C.c_void_p()
        _chk(R.hipMalloc(C.byref(p), max(self.nbytes, 1)), "hipMalloc")
        self.ptr = p.value
        _chk(R.hipMemset(self.ptr, 0, max(self.nbytes, 1)), "hipMemset")

    @classmethod
    def from_host(cls, a, device=None):
        a = np.ascontiguousarray(a)
        out = cls(a.shape, a.dtype, device)
        out.copy_from_host(a)
        return out

    def copy_from_host(self, a, stream=None):
        """Synchronous without a stream; on a stream the copy is enqueued (asynchronous from a PinnedArray's
        array) and `a` must stay alive until the stream has run it."""
        a = np.ascontiguousarray(a, self.dtype)
        if a.size != self.size:
            raise ValueError("host array of %d elements for a device array of %d" % (a.size, self.size))
        R = runtime()
        _chk(R.hipSetDevice(self.device), "hipSetDevice")
        if stream is None:
            _chk(R.hipMemcpy(self.ptr, a.ctypes.data, self.nbytes, _H2D), "hipMemcpy")
        else:
            _chk(R.hipMemcpyAsync(self.ptr, a.ctypes.data, self.nbytes, _H2D, stream_handle(stream)), "hipMemcpyAsync")

    def copy_from_device(self, src, stream=None):
        if src.nbytes != self.nbytes:
            raise ValueError("device copy of %d bytes into %d" % (src.nbytes, self.nbytes))
        R = runtime()
        _chk(R.hipSetDevice(self.device), "hipSetDevice")
        if stream is None:
            _chk(R.hipMemcpy(self.ptr, src.ptr, self.nbytes, _D2D), "hipMemcpy")
        else:
            _chk(R.hipMemcpyAsync(self.ptr, src.ptr, self.nbytes, _D2D, stream_handle(stream)), "hipMemcpyAsync")

    def to_host(self, out=None, stream=None):
        """The contents as a numpy array; with a stream the copy into `out` is only enqueued there."""
        if out is None:
            out = np.empty(self.shape, self.dtype)
        if out.dtype != self.dtype or out.size != self.size or not out.flags.c_contiguous:
            raise ValueError("to_host needs a C-contiguous %s array of %d elements" % (self.dtype, self.size))
        R = runtime()
        _chk(R.hipSetDevice(self.device), "hipSetDevice")
        if stream is None:
            _chk(R.hipMemcpy(out.ctypes.data, self.ptr, self.nbytes, _D2H), "hipMemcpy")
        else:
            _chk(R.hipMemcpyAsync(out.ctypes.data, self.ptr, self.nbytes, _D2H, stream_handle(stream)),
                 "hipMemcpyAsync")
        return out

    def view(self, offset, shape):
        """`shape` elements from element `offset` of this array (no bounds beyond the array's own)."""
        shape = (int(shape),) if np.isscalar(shape) else tuple(int(s) for s in shape)
        if offset < 0 or offset + int(np.prod(shape)) > self.size:
            raise ValueError("view [%d, +%d) leaves the array's %d elements" % (offset, int(np.prod(shape)), self.size))
        return DeviceArray(shape, self.dtype, _base=self._base or self, _ptr=self.ptr + offset * self.dtype.itemsize)

    @property
    def __cuda_array_interface__(self):
        return dict(shape=self.shape, typestr=_DTYPES[self.dtype], data=(self.ptr, False), version=3, strides=None)

    def close(self):
        if self._base is None and getattr(self, "ptr", None):
            runtime().hipFree(self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def device_pointer(a, dtype, shape, what):
    """The device address of `a`, any object with __cuda_array_interface__, after checking its element type,
    C-contiguity and shape (`shape` may hold -1 for a free leading extent; the element count must match)."""
    try:
        cai = a.__cuda_array_interface__
    except AttributeError:
        raise TypeError("%s must expose __cuda_array_interface__ (a DeviceArray, a torch tensor on the GPU)" % what)
    dt = np.dtype(dtype)
    if np.dtype(cai["typestr"]) != dt:
        raise TypeError("%s has element type %s, expected %s" % (what, cai["typestr"], dt))
    shp = tuple(int(s) for s in cai["shape"])
    strides = cai.get("strides")
    if strides is not None:
        want, acc = [], dt.itemsize
        for s in reversed(shp):
            want.append(acc)
            acc *= s
        if tuple(strides) != tuple(reversed(want)) and int(np.prod(shp)) > 1:
            raise ValueError("%s is not C-contiguous" % what)
    if int(np.prod(shp)) != int(np.prod(shape)):
        raise ValueError("%s has shape %s, expected %s" % (what, shp, tuple(shape)))
    return int(cai["data"][0])
