"""The weight-image cache of the training path: the packed MFMA operand images (pcr_pack_weight*, include/pcr.h section C)
of every conv / linear weight and the zero-padded images of the biases, refreshed by ONE launch per optimizer step, and
the on-the-spot packs that a miss falls back to.  pcr_amd/train_ops.py imports these names; nothing here knows the
training precision -- the callers decide which image they ask for."""
import weakref

import torch

from . import _lib as L
from ._lib import _c8, _c32, _f32
from .abi import pcr_pack_desc


def _dev(t):
    L.require_cuda(t)
    L.require_f32(t)
    return t.contiguous()


def _matrix(w):
    """the (rows, cols) matrix of a linear weight, or of a 1x1 Conv1d / Conv2d weight (rows, cols, 1[, 1])"""
    return w if w.dim() == 2 else w.reshape(w.shape[0], -1)


def _image_floats(rows, cols):
    """-> (floats of the f32 image of a (rows, cols) W, of the image of W^T)"""
    return _c8(cols) * _c32(rows), _c8(rows) * _c32(cols)


class _Images:
    """one registered weight: its matrix shape, the Tensor._version its images hold (-1: none yet), the f32 images of W
    and W^T (two halves of one buffer) and, once they were asked for, the bf16 hi / lo ones (else None)"""
    __slots__ = ("param", "rows", "cols", "version", "wp", "wpT", "wp_bf", "wpT_bf")

    def __init__(self, param, rows, cols, wp, wpT):
        self.param, self.rows, self.cols, self.version = param, rows, cols, -1
        self.wp, self.wpT, self.wp_bf, self.wpT_bf = wp, wpT, None, None

    def matches(self, w):
        return w.dim() == 2 and w.shape[0] == self.rows and w.shape[1] == self.cols and w.is_contiguous()


class _Padded:
    """one bias: the tensor (kept alive), the Tensor._version its zero-padded image holds, the image, the address the
    refresh launch reads it from"""
    __slots__ = ("param", "version", "image", "ptr")

    def __init__(self, param, version, image):
        self.param, self.version, self.image, self.ptr = param, version, image, param.data_ptr()


class _Prepack:
    """Packed images (W and W^T) of every conv / linear weight of a model, refreshed by ONE launch per optimizer step
    (`prepack(model)`, called by the Trainer) instead of one small launch per layer.  Looked up by storage address +
    shape + Tensor._version: a weight that was not registered, or that changed since the refresh, simply misses and is
    packed on the spot."""

    def __init__(self):
        self.key = None
        self.entries = {}          # data_ptr -> _Images
        self.descs = None
        self.ndesc = 0
        self.params = []
        self.biases = {}           # id(bias) -> _Padded
        self.want_bf = set()       # data_ptrs whose bf16 hi / lo images are refreshed too (asked for once: pack_both_bf)

    def build(self, params, biases):
        import numpy as np
        dev = params[0].device
        lib = L.load()
        self.params = params
        old = self.entries
        self.entries = {}
        self.biases = {}
        self.want_bf &= {p.data_ptr() for p in params}
        desc = np.zeros(len(params) + len(biases) + len(self.want_bf),
                        dtype=pcr_pack_desc)
        nbf = 0
        for i, p in enumerate(params):
            rows, cols = _matrix(p).shape
            e = old.get(p.data_ptr())
            if e is not None and e.param is p and e.rows == rows and e.cols == cols:
                e.version = -1         # (a rebuild that only adds bf images keeps the f32 images where they are)
            else:
                n0, n1 = _image_floats(rows, cols)
                out = _f32(n0 + n1, device=dev)
                e = _Images(p, rows, cols, out[:n0], out[n0:])
            desc[i] = (p.data_ptr(), e.wp._base.data_ptr(), rows, cols, 0, 0)
            if p.data_ptr() in self.want_bf:
                b0 = lib.pcr_packed_weight_bf16_floats(rows, cols)
                b1 = lib.pcr_packed_weight_bf16_floats(cols, rows)
                if e.wp_bf is None:
                    ob = _f32(b0 + b1, device=dev)
                    e.wp_bf, e.wpT_bf = ob[:b0], ob[b0:]
                desc[len(params) + len(biases) + nbf] = (p.data_ptr(), e.wp_bf._base.data_ptr(), rows, cols, 1, 0)
                nbf += 1
            else:
                e.wp_bf = e.wpT_bf = None
            self.entries[p.data_ptr()] = e
        for i, b in enumerate(biases):          # cols = 0: a bias, copied into its zero-padded image by the same launch
            out = torch.zeros(_c32(b.numel()), dtype=torch.float32, device=dev)
            desc[len(params) + i] = (b.data_ptr(), out.data_ptr(), b.numel(), 0, 0, 0)
            self.biases[id(b)] = _Padded(b, -1, out)
        self.ndesc = len(desc)
        self.descs = torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
        self.key = tuple(id(p) for p in params) + tuple(id(b) for b in biases)

    def refresh(self, params, biases=(), build_only=False):
        params = [p for p in params if p.is_cuda and p.dim() >= 2 and p.dtype == torch.float32 and p.is_contiguous()]
        biases = [b for b in biases if b.is_cuda and b.dim() == 1 and b.dtype == torch.float32 and b.is_contiguous()]
        if not params:
            return
        if self.key != tuple(id(p) for p in params) + tuple(id(b) for b in biases) or \
                any(e.param.data_ptr() != k for k, e in self.entries.items()) or \
                any(e.param.data_ptr() != e.ptr for e in self.biases.values()) or \
                any((k in self.want_bf) != (e.wp_bf is not None) for k, e in self.entries.items()):
            self.build(params, biases)
            if build_only:
                return
        elif build_only or all(e.version == e.param._version for e in self.entries.values()) and \
                all(e.version == e.param._version for e in self.biases.values()):
            return        # nothing changed since the last refresh (micro-steps of a gradient accumulation)
        L.run.pcr_pack_weights_multi_f32(L.ptr(self.descs), self.ndesc, L.stream_ptr())
        for e in self.entries.values():
            e.version = e.param._version
        for e in self.biases.values():
            e.version = e.param._version

    def lookup_bias(self, v, n):
        e = self.biases.get(id(v))
        if e is None or e.param is not v or e.version != v._version or e.image.numel() != _c32(n):
            return None
        return e.image

    def lookup(self, w):
        e = self.entries.get(w.data_ptr())
        if e is None or e.version != w._version or not e.matches(w):
            return None
        return e.wp, e.wpT

    def lookup_bf(self, w):
        """-> (bf image of W, of W^T) | None (not registered / stale); registers the weight for the NEXT refresh"""
        e = self.entries.get(w.data_ptr())
        if e is None or not e.matches(w):
            return None
        self.want_bf.add(w.data_ptr())
        if e.wp_bf is None or e.version != w._version:
            return None
        return e.wp_bf, e.wpT_bf


# one table per model, owned by the model (dropped with it); `_first_hit` searches the live tables
_PREPACKS = weakref.WeakKeyDictionary()


def _first_hit(lookup, *args):
    """the first answer of `lookup` (a _Prepack method) over the live tables, or None"""
    for t in _PREPACKS.values():
        hit = lookup(t, *args)
        if hit is not None:
            return hit
    return None


def _lookup(w):
    return _first_hit(_Prepack.lookup, w)


def prepack(model, build_only=False):
    """refresh the packed images of every conv / linear weight of `model` in one launch (Trainer.step calls this once
    per iteration, after the previous update); pack_dev / pack_both then hit the cache.  Note for callers that keep an
    autograd graph across iterations: the images are overwritten in place by the next refresh.
    build_only: only (re)build the descriptor table and the image buffers if the set of weights or of requested bf16
    images changed -- allocations and a host-to-device copy, which a stream capture cannot take: the Trainer calls this
    right before it captures an iteration, whose own prepack() then is the one launch and nothing else."""
    mods = [m for m in model.modules()
            if isinstance(m, (torch.nn.Linear, torch.nn.Conv1d, torch.nn.Conv2d)) and m.weight is not None]
    tab = _PREPACKS.get(model)
    if tab is None:
        tab = _PREPACKS[model] = _Prepack()
    tab.refresh([m.weight for m in mods], [m.bias for m in mods if m.bias is not None], build_only=build_only)


def _pack_f32(w, mode):
    """on-the-spot pcr_pack_weight_dev_f32 of a device weight: mode 0 = image of W, 1 = of W^T, 2 = both, side by side
    -> (buffer, floats of the W image)"""
    w = _matrix(_dev(w.detach()))
    rows, cols = w.shape
    n = _image_floats(rows, cols)
    out = _f32(n[0] + n[1] if mode == 2 else n[mode], device=w.device)
    L.run.pcr_pack_weight_dev_f32(w, rows, cols, cols, mode, out, L.stream_ptr())
    return out, n[0]


def pack_dev(w, transpose=False):
    """(rows, cols) device matrix -> packed MFMA A-operand image of W or W^T (weights change every step, so the
    pack runs on the device; inference packs once on the host)"""
    hit = _lookup(w)
    if hit is not None:
        return hit[1] if transpose else hit[0]
    return _pack_f32(w, int(transpose))[0]


def pack_both(w):
    """-> (image of W, image of W^T) from ONE launch (forward and backward operands of a layer)"""
    hit = _lookup(w)
    if hit is not None:
        return hit
    out, n0 = _pack_f32(w, 2)
    return out[:n0], out[n0:]


def _pack_bf(w, transpose):
    """on-the-spot bf16 hi / lo image of a device weight or of its transpose (one small launch)"""
    w = _matrix(_dev(w.detach()))
    rows, cols = w.shape
    out = _f32(L.load().pcr_packed_weight_bf16_floats(*((cols, rows) if transpose else (rows, cols))), device=w.device)
    L.run.pcr_pack_weight_bf16_dev_f32(w, rows, cols, cols, int(transpose), out, L.stream_ptr())
    return out


def pack_both_bf(w):
    """-> (bf16 hi / lo image of W, of W^T): the operands of the fused chains on the bf16 matrix core.  A weight of a
    prepacked model is registered on its first request and refreshed by the one launch per iteration from then on; a
    miss packs on the spot (two small launches)"""
    hit = _first_hit(_Prepack.lookup_bf, w)
    if hit is not None:
        return hit
    return _pack_bf(w, False), _pack_bf(w, True)


def pack_bf_T(w):
    """(rows, cols) device weight -> bf16 hi / lo image of W^T (the dx operand of the bf16 backward), packed on the device:
    one small launch per layer and iteration (the weights change every step)"""
    return _pack_bf(w, True)


_PAD_CACHE = {}            # id(bias) -> _Padded, for the biases that no live table holds


def pad32(v, n):
    """(n) vector -> zero-padded to a multiple of 32 (accumulator seeds are read 16 bytes at a time); cached per
    (tensor, version): a bias is padded once per optimizer step, not once per launch"""
    if v is None:
        return None
    hit = _first_hit(_Prepack.lookup_bias, v, n)          # refreshed with the weights by the one launch per iteration
    if hit is not None:
        return hit
    # keyed by the tensor OBJECT (kept alive by the entry, so its id and storage cannot be recycled under the cache: a
    # (data_ptr, version) key returned another tensor's bias once the allocator had reused the address) and its version
    e = _PAD_CACHE.get(id(v))
    if e is not None and e.param is v and e.image.numel() == _c32(n) and e.image.device == v.device:
        if e.version != v._version:       # updated since (optimizer step): refresh the live part in place, one small copy
            e.image[:n].copy_(v.detach())
            e.version = v._version
        return e.image
    out = torch.zeros(_c32(n), dtype=torch.float32, device=v.device)
    out[:n] = v.detach()
    if len(_PAD_CACHE) > 256:
        _PAD_CACHE.clear()
    _PAD_CACHE[id(v)] = _Padded(v, v._version, out)
    return out
