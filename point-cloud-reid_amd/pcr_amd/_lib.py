"""ctypes binding of libpcr_hip.so (include/pcr.h).  There is NO fallback: if the library is
missing or a call fails, a RuntimeError is raised."""
import ctypes
import os

import torch  # must be imported before the library so that libamdhip64.so.7 resolves to torch's copy

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# (PCR_LIB_TAG: a diagnostic build made by pcr_amd/build.py under the same variable, e.g. libpcr_hip_tune.so)
_TAG = os.environ.get("PCR_LIB_TAG", "")
SO_PATH = os.path.join(_HERE, "lib", "libpcr_hip%s.so" % ("_" + _TAG if _TAG else ""))
_lib = None

ABI_VERSION = 17


class PcrError(RuntimeError):
    pass


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise PcrError(
                "libpcr_hip.so is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `python point-cloud-reid_amd/pcr_amd/build.py`; there is no CPU fallback." % SO_PATH)
        lib = ctypes.CDLL(SO_PATH)
        if lib.pcr_abi_version() != ABI_VERSION:
            raise PcrError("libpcr_hip.so ABI %d != binding %d: rebuild" % (lib.pcr_abi_version(), ABI_VERSION))
        for name, sig in abi.SIGNATURES.items():         # every prototype of include/pcr.h, once
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = abi.prototype(sig)
            if sig[0] == "s":
                setattr(run, name, _checked(name))
        if os.environ.get("PCR_STREAM_MIN_BLOCKS"):      # launch policy of the train-dense kernels (include/pcr.h)
            lib.pcr_set_stream_min_blocks(int(os.environ["PCR_STREAM_MIN_BLOCKS"]))
        _lib = lib
    return _lib


def _checked(name):
    def call(*args):
        status = getattr(load(), name)(*args)            # through load(), so that whoever substitutes it sees the call
        if status != 0:
            raise PcrError("%s failed: %s" % (name, _lib.pcr_status_string(status).decode()))
    return call


class _Run:
    """`run.pcr_x(args...)`: `load().pcr_x(args...)`, raising PcrError on a nonzero status.  load() puts one callable per
    status-returning entry point on the instance; this hook only serves the first use before the library is loaded."""

    def __getattr__(self, name):
        if _lib is not None or name not in abi.SIGNATURES:
            raise AttributeError(name)
        load()
        return getattr(self, name)


run = _Run()


def stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    if t is None:
        return ctypes.c_void_p(0)
    return ctypes.c_void_p(t.data_ptr())


def _p(t):
    """address for a pointer FIELD of a parameter block (the blocks hold plain addresses; None = NULL)"""
    return None if t is None else t.data_ptr()


def _c8(n):
    return (n + 7) // 8 * 8


def _c32(n):
    return (n + 31) // 32 * 32


def _f32(*shape, device):
    return torch.empty(shape, dtype=torch.float32, device=device)


def _i32(*shape, device):
    return torch.empty(shape, dtype=torch.int32, device=device)


def check(status, what):
    if status != 0:
        raise PcrError("%s failed: %s" % (what, load().pcr_status_string(status).decode()))


def require_cuda(*tensors):
    """device tensors only (no CPU fallback), all on the CURRENT device: the launch goes to the current device's
    stream (mmdet3d.ops switches to the tensor's device first, as the reference's KNN wrapper does)"""
    current = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise PcrError("pcr_amd ops run only on an MI355X device tensor (got %s); there is no CPU "
                           "fallback in the product path" % t.device)
        if current is None:                              # (asked once per call: a block's fill passes two dozen tensors)
            current = torch.cuda.current_device()
        if t.device.index != current:
            raise PcrError("tensor on %s but the current device is cuda:%d: call torch.cuda.set_device / "
                           "torch.cuda.device(...) first" % (t.device, current))


def require_f32(*tensors):
    for t in tensors:
        if t is not None and t.dtype != torch.float32:
            raise PcrError("expected a float32 tensor, got %s (the kernels read raw binary32)" % t.dtype)


def require_i32(*tensors):
    """the reference's wrappers read indices through data_ptr<int>() and raise on int64; so do we"""
    for t in tensors:
        if t is not None and t.dtype != torch.int32:
            raise PcrError("expected an int32 index tensor, got %s" % t.dtype)


def refuse(who, what):
    """every refused call is a PcrError that names the entry and the argument (an assert would vanish under python -O)"""
    raise PcrError("%s: %s" % (who, what))


def require(ok, who, what, *args):
    """`what % args`, put together only when the call is refused"""
    if not ok:
        refuse(who, what % args if args else what)


def tensor(t, who, name, dtype, shape=None, numel=None, optional=False, cast_int64=False, copy=False):
    """The argument `name` of `who` as a kernel reads it: a contiguous tensor of `dtype` and of `shape` (None = a dimension
    of any size) or of `numel` elements; returns it.  optional: None passes.  cast_int64: int64 labels, lengths and masks
    are converted to int32 (on the tensor's device).  copy: a strided tensor is made contiguous instead of refused.  What
    is wrong with the argument comes before where it lives: the device is not looked at, `require_cuda` over all the
    arguments follows the last of these."""
    if t is None and optional:
        return None
    if not isinstance(t, torch.Tensor):
        refuse(who, "%s must be a tensor" % name)
    if cast_int64 and t.dtype == torch.int64:
        t = t.to(torch.int32)
    if t.dtype != dtype:
        refuse(who, "%s must be a %s tensor, got %s" % (name, dtype, t.dtype))
    if shape is not None and t.shape != shape:           # (equal: done; otherwise a None may still let it pass)
        ok = t.dim() == len(shape)
        for want, got in zip(shape, t.shape) if ok else ():
            ok = ok and (want is None or want == got)
        if not ok:
            refuse(who, "%s must be (%s), got %s" % (name, ", ".join("*" if n is None else str(n) for n in shape) +
                                                   ("," if len(shape) == 1 else ""), tuple(t.shape)))
    if numel is not None and t.numel() != numel:
        refuse(who, "%s must hold %d elements, got %s" % (name, numel, tuple(t.shape)))
    if not t.is_contiguous():
        if not copy:
            refuse(who, "%s must be contiguous" % name)
        t = t.contiguous()
    return t


def out_tensor(out, who, name, dtype, shape, device):
    """the out= pattern: the caller's buffer held to `tensor`'s checks, or a new uninitialised tensor on `device`"""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    return tensor(out, who, name, dtype, shape=shape)


def require_default_eps(*norms):
    """GroupNorm / LayerNorm kernels use eps = 1e-5 (every norm layer of the ReID configs): anything else is refused
    rather than silently computed with the wrong constant"""
    for n in norms:
        eps = getattr(n, "eps", 1e-5)
        if abs(eps - 1e-5) > 1e-12:
            raise PcrError("%s with eps=%g: the HIP kernels implement eps = 1e-5 only" % (type(n).__name__, eps))
