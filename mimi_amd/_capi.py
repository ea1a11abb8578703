"""ctypes binding of libmimi_hip.so (include/mimi_hip.h).  There is no CPU fallback:
if the library is missing or no HIP device is visible, calls raise."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np

from . import _header
from . import build as _build

_lib = None


def _read_header():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mimi_hip.h")
    try:
        with open(path) as f:
            return _header.parse(f.read())
    except OSError as e:
        raise RuntimeError(f"{path} cannot be read ({e.strerror}): the binding is derived from it, and the build needs it too") from e


# The header is the binding's only source: prototypes, struct layouts, enumerators and the ABI version are read from it here,
# at import (no compiler, no library load); a new entry is an edit of the header and of nothing in this file.
HEADER = _read_header()
EXPORTS = list(HEADER.functions)
# the enumerators without their MIMI_HIP_ prefix: ABI.MAT_J2, ABI.DOMAIN_INFO_NNZ, ...
ABI = SimpleNamespace(**{name[len("MIMI_HIP_"):]: value for name, value in HEADER.enums.items()})


class Material(C.Structure):
    _fields_ = HEADER.structs["mimi_hip_material"]


class DomainTables(C.Structure):
    _fields_ = HEADER.structs["mimi_hip_domain_tables"]


class BSplinePatch(C.Structure):
    _fields_ = HEADER.structs["mimi_hip_bspline_patch"]


class ContactTables(C.Structure):
    _fields_ = HEADER.structs["mimi_hip_contact_tables"]


class PressureTables(C.Structure):
    _fields_ = HEADER.structs["mimi_hip_pressure_tables"]


class SplineBody(C.Structure):
    _fields_ = HEADER.structs["mimi_hip_spline_body"]


def _header_abi_version():
    return HEADER.defines["MIMI_HIP_ABI_VERSION"]


def library_path():
    return _build.LIB


def lib():
    """Load libmimi_hip.so (building it if hipcc is around and the file is stale)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("MIMI_HIP_LIBRARY") or _build.LIB      # (another build of the same sources: timing experiments)
    import shutil
    if path == _build.LIB and (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        _build.build()          # no-op unless a source or the header is newer than the library
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: run `python -m mimi_amd.build` (hipcc --offload-arch=gfx950). "
            "mimi_amd has no CPU fallback.")
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64.so.7; when it is
    # loaded first our NEEDED entry resolves to that same copy (same soname), and device
    # pointers / streams can be shared with torch.  Loading ours first would hand torch a
    # runtime it was not built against.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(path)
    expected = _header_abi_version()
    if L.mimi_hip_abi_version() != expected:
        raise RuntimeError(f"{path} has ABI version {L.mimi_hip_abi_version()}, include/mimi_hip.h declares {expected}: "
                           "rebuild with `python -m mimi_amd.build`")
    for name, (restype, argtypes) in HEADER.functions.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def check(status):
    """non-zero status -> RuntimeError carrying the library's message (the reference throws
    std::runtime_error -> Python RuntimeError through pybind11, utils/print.hpp:47-56)."""
    if status != 0:
        raise RuntimeError(lib().mimi_hip_last_error().decode())


def ptr(x, dtype=None):
    """void* of a numpy array (host) or a torch tensor (host or device) or None.  dtype: what the C side reads
    ("float64", "int32", "int64"); a buffer of another type raises instead of being reinterpreted."""
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        assert x.flags.c_contiguous
        if dtype is not None and x.dtype != np.dtype(dtype):
            raise TypeError(f"expected a {dtype} array, got {x.dtype}")
        return x.ctypes.data_as(C.c_void_p)
    if hasattr(x, "data_ptr"):
        assert x.is_contiguous()
        if dtype is not None and str(x.dtype).split(".")[-1] != dtype:
            raise TypeError(f"expected a {dtype} tensor, got {x.dtype}")
        return C.c_void_p(x.data_ptr())
    if isinstance(x, int):
        return C.c_void_p(x)
    raise TypeError(type(x))


def fptr(x):
    """ptr() of a float64 buffer (u, r, CSR values)"""
    return ptr(x, "float64")


def torch_stream_of(*buffers):
    """cuda_stream of torch's current stream on the device of the first CUDA tensor among `buffers`, else None: a handle
    that was never given a stream launches on it, so that what torch enqueued on these tensors before the call (zero
    fills, copies) is ordered before the kernels, and what it enqueues afterwards behind them."""
    for b in buffers:
        if b is not None and hasattr(b, "is_cuda") and b.is_cuda:
            import torch
            s = torch.cuda.current_stream(b.device).cuda_stream
            return s if s else STREAM_NULL       # torch's default stream is the device's null stream (handle 0)
    return None


STREAM_NULL = 2 ** 64 - 1        # MIMI_HIP_STREAM_NULL of include/mimi_hip.h


class Handle:
    """What the front-ends of the library's handles share: `_h` (None until the handle exists), the stream rules and the
    release.  `_prefix` names the C entries: mimi_hip_<_prefix>_set_stream / _synchronize / _destroy."""
    _prefix = None
    _h = None

    def _fn(self, name):
        return getattr(lib(), f"mimi_hip_{self._prefix}_{name}")

    def _handle(self):
        if self._h is None:
            raise RuntimeError("Prepare() has not been called")
        return self._h

    def SetStream(self, stream):
        """launch on `stream` (a hipStream_t as an int); 0 / None: back to following torch's current stream for CUDA
        tensors and the handle's own stream for host buffers"""
        self._user_stream = bool(stream)
        self._user_stream_value = int(stream) if stream else 0
        check(self._fn("set_stream")(self._handle(), C.c_void_p(stream) if stream else None))

    def _follow_torch(self, *buffers):
        # ordering with the caller's torch work (zero fills of r / A, copies of u): see torch_stream_of.  A handle that
        # was never given a stream launches on torch's current stream when it gets CUDA tensors
        if getattr(self, "_user_stream", False):
            return
        s = torch_stream_of(*buffers)
        if s is not None or getattr(self, "_followed", None):
            check(self._fn("set_stream")(self._handle(), C.c_void_p(s) if s else None))
            self._followed = s

    def Synchronize(self):
        check(self._fn("synchronize")(self._handle()))

    def __del__(self):
        try:
            if self._h is not None:
                self._fn("destroy")(self._h)
                self._h = None
        except Exception:
            pass

    def _sized_query(self, name, dtype):
        """the C entries that list values (out == NULL: count only): ask for the size, allocate, ask again"""
        n = C.c_int64(0)
        check(self._fn(name)(self._handle(), None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=dtype)
        check(self._fn(name)(self._handle(), ptr(out), out.size, C.byref(n)))
        return out


def fill_face_tables(t, patch, axis, side, quadrature_order, element_box=None, empty="no boundary faces in this element box"):
    """the fields ContactTables and PressureTables share, from splines.face_tables; returns the arrays the caller keeps
    alive while the C side reads them"""
    from . import splines
    # (a rational patch raises here: face_tables builds B-spline tables only)
    dofs, N, dN, weight = splines.face_tables(patch, axis, side, quadrature_order, element_box)
    if len(dofs) == 0:
        raise RuntimeError(empty)
    x_ref = np.ascontiguousarray(patch.control_points, dtype=np.float64)
    t.dim = patch.dim
    t.n_faces, t.n_dof = dofs.shape
    t.n_quad = weight.shape[1]
    t.n_nodes = patch.n_nodes
    t.dofs, t.N, t.dN_dxi, t.weight = dofs.ctypes.data, N.ctypes.data, dN.ctypes.data, weight.ctypes.data
    t.x_ref = x_ref.ctypes.data
    return [dofs, N, dN, weight, x_ref]
