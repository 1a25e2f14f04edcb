"""Host-side API over libgcow.so for device-resident torch tensors.

Mirrors the reference's codec interface (fpgasystems/gcow sw/include/types.h + zfp.h): the four expert parameters
(minbits, maxbits, maxprec, minexp) and the accuracy / rate / precision setters, `encode` = zfp_compress
(sw/src/zfp.c:10-28) and `decode` = zfp_decompress with libzfp 0.5.5 semantics. torch is used only for device
memory and streams; every byte of codec work runs in the gfx950 kernels of gcow_amd/csrc.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import numbers
from dataclasses import dataclass

import torch

from ._ffi import DTYPE_BF16, DTYPE_FLOAT, GcowError, GcowParams, ZfpInput, check, load

ZFP_MIN_BITS, ZFP_MAX_BITS, ZFP_MAX_PREC, ZFP_MIN_EXP = 1, 16658, 64, -1074
# index_stride of decode_mean for the packed 16-block index (include/gcow.h GCOW_INDEX_PACKED16)
INDEX_PACKED16 = 0x1010


# ------------------------------------------------------------------------------------------- parameters
def accuracy(tolerance: float) -> GcowParams:
    """set_zfp_output_accuracy (sw/src/common.c:6-21)."""
    emin = ZFP_MIN_EXP
    if tolerance > 0:
        _, e = math.frexp(tolerance)
        emin = e - 1
    return GcowParams(ZFP_MIN_BITS, ZFP_MAX_BITS, ZFP_MAX_PREC, emin)


def rate(bits_per_value: float, dims: int) -> GcowParams:
    """libzfp 0.5.5 zfp_stream_set_rate (float, no write-random-access): minbits = maxbits = floor(4^d r + 0.5)."""
    n = 1 << (2 * dims)
    bits = max(int(math.floor(n * bits_per_value + 0.5)), 9)
    return GcowParams(bits, bits, ZFP_MAX_PREC, ZFP_MIN_EXP)


def precision(prec: int) -> GcowParams:
    """libzfp 0.5.5 zfp_stream_set_precision."""
    p = min(prec, ZFP_MAX_PREC) if prec else ZFP_MAX_PREC
    return GcowParams(ZFP_MIN_BITS, ZFP_MAX_BITS, p, ZFP_MIN_EXP)


def expert(minbits: int, maxbits: int, maxprec: int, minexp: int) -> GcowParams:
    return GcowParams(minbits, maxbits, maxprec, minexp)


def is_fixed(p: GcowParams) -> bool:
    return p.minbits == p.maxbits


# ------------------------------------------------------------------------------------------- fields
def field_of(t: torch.Tensor, dims: int | None = None) -> ZfpInput:
    """zfp_input for a 1-4 dim tensor (numpy order: the last axis is x, the fastest)."""
    if t.dim() < 1 or t.dim() > 4:
        raise GcowError("tensors of 1-4 dims are supported, got %d" % t.dim())
    if t.dtype == torch.float32:
        dt = DTYPE_FLOAT
    elif t.dtype == torch.bfloat16:
        dt = DTYPE_BF16
    else:
        raise GcowError("dtype %s not supported (float32, bfloat16)" % t.dtype)
    f = ZfpInput()
    f.dtype = dt
    f.data = t.data_ptr()
    shp = list(reversed(t.shape))
    st = list(reversed(t.stride()))
    names_n = ["nx", "ny", "nz", "nw"]
    names_s = ["sx", "sy", "sz", "sw"]
    for i in range(t.dim()):
        if st[i] == 0 and shp[i] > 1:
            # an expanded / broadcast view: the ABI reads stride 0 as "dense" (sw/src/zfp.c:37-38), which would walk
            # past the tensor's storage
            raise GcowError("stride 0 on a dimension of size %d (expanded view): pass t.contiguous()" % shp[i])
        setattr(f, names_n[i], int(shp[i]))
        setattr(f, names_s[i], int(st[i]))
    return f


def _stream_ptr(stream) -> int:
    if stream is None:
        stream = torch.cuda.current_stream()
    return stream.cuda_stream


def max_output_bytes(shape, p: GcowParams, dtype=torch.float32) -> int:
    t = torch.empty(0)
    f = ZfpInput()
    f.dtype = DTYPE_FLOAT if dtype == torch.float32 else DTYPE_BF16
    shp = list(reversed(shape))
    for i, n in enumerate(shp):
        setattr(f, ["nx", "ny", "nz", "nw"][i], int(n))
    del t
    return load().gcow_max_output_bytes(C.byref(f), C.byref(p))


@dataclass
class Encoded:
    """A compressed stream on the device: `words` (int64 tensor holding little-endian uint64 stream words),
    `bits_dev` (int64[1] device tensor with the unflushed bit count), optional block `index` for parallel decode."""
    words: torch.Tensor
    bits_dev: torch.Tensor
    shape: tuple
    params: GcowParams
    index: torch.Tensor | None = None
    index_stride: int = 0

    @property
    def bits(self) -> int:
        return int(self.bits_dev.item())

    @property
    def nwords(self) -> int:
        return (self.bits + 63) // 64

    def stream(self) -> torch.Tensor:
        """The flushed stream: ceil(bits/64) words (sw/src/stream.c:132-138 + :176-179)."""
        return self.words[: self.nwords]

    def to_bytes(self) -> bytes:
        return self.stream().cpu().numpy().tobytes()


class Encoder:
    """Preallocated encoder for a fixed shape / dtype / params (bench and repeated-bucket use)."""

    def __init__(self, shape, dtype, params: GcowParams, device=None, index_stride: int = 0):
        self.L = load()
        self.shape = tuple(shape)
        self.dtype = dtype
        self.params = params
        self.device = torch.device(device or "cuda")
        f = field_of_shape(self.shape, dtype)
        self.cap = self.L.gcow_max_output_bytes(C.byref(f), C.byref(params))
        if self.cap == 0:
            raise GcowError("unsupported shape %s" % (self.shape,))
        self.words = torch.zeros((self.cap + 7) // 8, dtype=torch.int64, device=self.device)
        self.bits_dev = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.fixed = is_fixed(params)
        if self.fixed:  # fixed rate: the bit count is known on the host; no device write per call
            nb = 1
            for n in self.shape:
                nb *= (n + 3) // 4
            self.bits_dev.fill_(nb * params.maxbits)
        ws = self.L.gcow_encode_workspace_bytes(C.byref(f), C.byref(params))
        self.ws = torch.zeros(max(ws // 8, 1), dtype=torch.int64, device=self.device)
        self.ws_bytes = ws
        self.index_stride = index_stride
        ne = self.L.gcow_index_entries(C.byref(f), index_stride) if index_stride else 0
        self.index = torch.zeros(max(ne, 1), dtype=torch.int64, device=self.device) if index_stride else None

    def __call__(self, x: torch.Tensor, stream=None) -> Encoded:
        if tuple(x.shape) != self.shape or x.dtype != self.dtype:
            raise GcowError("Encoder built for %s %s, got %s %s" % (self.shape, self.dtype, tuple(x.shape), x.dtype))
        if not x.is_cuda:
            raise GcowError("Encoder expects a device tensor")
        f = field_of(x)
        st = self.L.gcow_encode_device(C.byref(f), C.byref(self.params), self.words.data_ptr(), self.cap,
                                       None if self.fixed else self.bits_dev.data_ptr(), self.ws.data_ptr(),
                                       self.ws_bytes,
                                       self.index.data_ptr() if self.index is not None else None,
                                       self.index_stride, _stream_ptr(stream))
        check(st, "gcow_encode_device")
        return Encoded(self.words, self.bits_dev, self.shape, self.params, self.index, self.index_stride)


RESID_COMPOSED, RESID_FUSED_FIXED, RESID_FUSED_VAR = 0, 1, 2  # gcow_encode_residual_path


class ResidualEncoder(Encoder):
    """Preallocated error-feedback encoder (gcow_encode_residual_device) for a 1-D bucket of n values: calling it with
    (x, err) codes y = x + err and leaves err = finite(y - decode(stream)) (err: fp32 device tensor of n values,
    updated in place). `path` says how, for 16-byte aligned tensors (gcow_encode_residual_path): RESID_FUSED_FIXED at
    rate 8 / 16 without an index (one kernel, no workspace), RESID_FUSED_VAR for accuracy, precision and expert sets
    with minbits <= 1 and maxbits >= 160 (the variable-rate encoder's passes on y, the code pass writing err from its
    own coefficients; the encoder's workspace), RESID_COMPOSED for everything else (encoder and decoder composed on
    the device through a workspace that also holds y). A view off 16-byte alignment takes the composed path."""

    def __init__(self, n: int, dtype, params: GcowParams, device=None, index_stride: int = 0):
        super().__init__((int(n),), dtype, params, device, index_stride)
        f = field_of_shape(self.shape, dtype)
        # sized from the parameters alone (aligned tensors assumed): nothing for the fused fixed-rate kernel, the
        # encoder's workspace for the fused variable-rate passes, the composed path's y, encoder workspace and index
        # otherwise; a call whose views turn out off 16-byte alignment is refused where this is too small
        self.ws_bytes = self.L.gcow_encode_residual_workspace_bytes(C.byref(f), C.byref(params))
        self.ws = torch.zeros(max(self.ws_bytes // 8, 1), dtype=torch.int64, device=self.device)
        self.path = self.L.gcow_encode_residual_path(C.byref(f), C.byref(params), None, None,
                                                     self.index.data_ptr() if self.index is not None else None)

    def __call__(self, x: torch.Tensor, err: torch.Tensor, stream=None) -> Encoded:
        if tuple(x.shape) != self.shape or x.dtype != self.dtype:
            raise GcowError("ResidualEncoder built for %s %s, got %s %s" % (self.shape, self.dtype, tuple(x.shape),
                                                                           x.dtype))
        _check_err(x, err)
        f = field_of(x)
        st = self.L.gcow_encode_residual_device(C.byref(f), C.byref(self.params), err.data_ptr(), err.data_ptr(),
                                                self.words.data_ptr(), self.cap,
                                                None if self.fixed else self.bits_dev.data_ptr(), self.ws.data_ptr(),
                                                self.ws_bytes,
                                                self.index.data_ptr() if self.index is not None else None,
                                                self.index_stride, _stream_ptr(stream))
        check(st, "gcow_encode_residual_device")
        return Encoded(self.words, self.bits_dev, self.shape, self.params, self.index, self.index_stride)


def _check_err(x: torch.Tensor, err: torch.Tensor):
    if not (x.is_cuda and x.dim() == 1 and x.is_contiguous()):
        raise GcowError("encode_residual expects a contiguous 1-D device tensor")
    if not (err.is_cuda and err.device == x.device and err.dtype == torch.float32 and err.is_contiguous()
            and err.numel() == x.numel()):
        raise GcowError("encode_residual: err must be a contiguous fp32 tensor of x.numel() values on x's device")


def encode_residual(x: torch.Tensor, err: torch.Tensor, params: GcowParams, index_stride: int = 0,
                    stream=None) -> Encoded:
    """Error feedback: encode y = x + err (x: 1-D contiguous device tensor, fp32 or bf16; one fp32 add per value) and
    update `err` in place to y - decode(stream), non-finite differences as 0 (gcow_encode_residual_device). The
    stream is the one `encode` gives for the fp32 tensor y. Rate 8 / 16 and the variable-rate sets without a budget
    (accuracy, precision) run fused; see ResidualEncoder."""
    _check_err(x, err)
    return ResidualEncoder(x.numel(), x.dtype, params, x.device, index_stride)(x, err, stream)


def roundtrip(x: torch.Tensor, params: GcowParams, out: torch.Tensor | None = None, bits: torch.Tensor | None = None,
              stream=None) -> torch.Tensor:
    """decode(encode(x, params)) in one kernel, without the stream (gcow_roundtrip_device): what the reference's
    training loop does to its flattened gradients. x: contiguous 1-D (or flattened-contiguous) fp32 / bf16 device
    tensor. out: fp32 or bf16 tensor of x.numel() values (default: a new tensor of x's dtype; out=x runs in place; a
    bf16 out is the fp32 decode rounded to nearest even). bits: optional int64[1] device tensor that receives the bit
    length `encode` would report, for callers that log the compression ratio. Returns out."""
    if not (x.is_cuda and x.is_contiguous() and x.dim() >= 1):
        raise GcowError("roundtrip expects a contiguous device tensor")
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise GcowError("roundtrip: dtype %s not supported (float32, bfloat16)" % x.dtype)
    if out is None:
        out = torch.empty_like(x)
    if not (out.is_cuda and out.device == x.device and out.is_contiguous() and out.numel() == x.numel()
            and out.dtype in (torch.float32, torch.bfloat16)):
        raise GcowError("roundtrip: out must be a contiguous fp32 or bf16 tensor of x.numel() values on x's device")
    if bits is not None and not (bits.is_cuda and bits.device == x.device and bits.dtype == torch.int64
                                 and bits.numel() == 1):
        raise GcowError("roundtrip: bits must be a one-element int64 tensor on x's device")
    f = field_of(x.view(-1))
    st = load().gcow_roundtrip_device(C.byref(f), C.byref(params), out.data_ptr(),
                                      DTYPE_BF16 if out.dtype == torch.bfloat16 else DTYPE_FLOAT,
                                      bits.data_ptr() if bits is not None else None, _stream_ptr(stream))
    check(st, "gcow_roundtrip_device")
    return out


RTLIST_ROWS_DWORD, RTLIST_ROWS_NATURAL = 0, 1  # gcow_roundtrip_list_stats.row_rule


class TensorListRoundtrip:
    """roundtrip of the concatenation of a list of tensors, each read and written where it lies
    (gcow_roundtrip_list_device): no torch.cat before the call, no copy per tensor after it. The object owns the host
    plan (pinned) and its device copy; a call rebuilds and re-uploads them (non-blocking, on the call's stream) only
    when the tuple of (data_ptr, numel) of the tensors, the dtypes or the device changes, so a training loop whose
    gradients stay where they are plans once. `rebuilds` counts the plans made; `stats()` says how many chunks of
    2048 blocks run through the direct kernels and how many through the gather kernel. One object serves one stream
    at a time: a rebuild overwrites the device plan in stream order."""

    def __init__(self, params: GcowParams):
        self.L = load()
        self._p = params    # the plan's parameter set (`params` below; a subclass may give that name another meaning)
        self.rebuilds = 0
        self._key = None
        self._h = None      # pinned int64 host plan
        self._d = None      # its device copy
        self._used = 0
        self._uploaded = None  # event after the last upload: the host plan is not rewritten before it

    @property
    def params(self) -> GcowParams:
        return self._p

    @staticmethod
    def _dt(t):
        return DTYPE_BF16 if t == torch.bfloat16 else DTYPE_FLOAT

    def _check(self, tensors, outs):
        ok = (torch.float32, torch.bfloat16)
        if outs is not None and len(outs) != len(tensors):
            raise GcowError("roundtrip_tensors: %d outputs for %d tensors" % (len(outs), len(tensors)))
        dev = None
        for group, what in ((tensors, "tensors"), (outs or [], "outs")):
            for t in group:
                if not isinstance(t, torch.Tensor) or not t.is_cuda:
                    raise GcowError("roundtrip_tensors expects device tensors")
                if t.dtype not in ok:
                    raise GcowError("roundtrip_tensors: dtype %s not supported (float32, bfloat16)" % t.dtype)
                if t.dtype != group[0].dtype:
                    raise GcowError("roundtrip_tensors: %s of mixed dtypes (%s, %s)" % (what, group[0].dtype, t.dtype))
                if not t.is_contiguous():
                    raise GcowError("roundtrip_tensors expects contiguous tensors")
                if dev is None:
                    dev = t.device
                elif t.device != dev:
                    raise GcowError("roundtrip_tensors: tensors on different devices (%s, %s)" % (dev, t.device))
        if outs is not None:
            for t, o in zip(tensors, outs):
                if o.numel() != t.numel():
                    raise GcowError("roundtrip_tensors: an output of %d values for a tensor of %d" % (o.numel(),
                                                                                                     t.numel()))
        return dev if dev is not None else torch.device("cuda", torch.cuda.current_device())

    def _plan(self, tensors, outs, in_dt, out_dt, dev, stream):
        n = len(tensors)
        ins = (C.c_void_p * max(n, 1))(*[t.data_ptr() or None for t in tensors])
        ous = (C.c_void_p * max(n, 1))(*[o.data_ptr() or None for o in outs]) if outs is not None else None
        cnt = (C.c_uint64 * max(n, 1))(*[t.numel() for t in tensors])
        need = self.L.gcow_roundtrip_list_plan_bytes(n, sum(t.numel() for t in tensors))
        words = (need + 7) // 8
        if self._uploaded is not None:
            self._uploaded.synchronize()  # the pinned plan is still the source of a copy in flight
        if self._h is None or self._h.numel() < words or self._d.device != dev:
            self._h = torch.empty(words, dtype=torch.int64).pin_memory()
            self._d = torch.empty(words, dtype=torch.int64, device=dev)
        used = C.c_size_t(0)
        check(self.L.gcow_roundtrip_list_plan(ins, ous, cnt, n, in_dt, out_dt, C.byref(self._p),
                                              self._h.data_ptr(), self._h.numel() * 8, C.byref(used)),
              "gcow_roundtrip_list_plan")
        self._used = int(used.value)
        w = (self._used + 7) // 8
        with torch.cuda.stream(stream):
            self._d[:w].copy_(self._h[:w], non_blocking=True)
            self._uploaded = torch.cuda.Event()
            self._uploaded.record(stream)
        self.rebuilds += 1

    def stats(self):
        """gcow_roundtrip_list_stats of the current plan (None before the first call)."""
        if self._h is None:
            return None
        from ._ffi import RoundtripListStats
        s = RoundtripListStats()
        check(self.L.gcow_roundtrip_list_plan_stats(self._h.data_ptr(), self._used, C.byref(s)),
              "gcow_roundtrip_list_plan_stats")
        return s

    def _prepare(self, tensors, outs, bits, stream):
        """The checks of a call and the plan made current for it -> (tensors, outs, device, stream)."""
        tensors = list(tensors)
        outs = list(outs) if outs is not None else None
        dev = self._check(tensors, outs)
        if bits is not None and not (bits.is_cuda and bits.device == dev and bits.dtype == torch.int64
                                     and bits.numel() == 1):
            raise GcowError("roundtrip_tensors: bits must be a one-element int64 tensor on the tensors' device")
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        in_dt = self._dt(tensors[0].dtype) if tensors else DTYPE_FLOAT
        out_dt = self._dt(outs[0].dtype) if outs else in_dt
        key = (in_dt, out_dt, dev, tuple((t.data_ptr(), t.numel()) for t in tensors),
               tuple(o.data_ptr() for o in outs) if outs is not None else None)
        if key != self._key:
            self._key = None
            self._plan(tensors, outs, in_dt, out_dt, dev, stream)
            self._key = key
        return tensors, outs, dev, stream

    def __call__(self, tensors, outs=None, bits: torch.Tensor | None = None, stream=None):
        tensors, outs, dev, stream = self._prepare(tensors, outs, bits, stream)
        check(self.L.gcow_roundtrip_list_device(self._h.data_ptr(), self._d.data_ptr(), self._used,
                                                C.byref(self._p),
                                                bits.data_ptr() if bits is not None else None, stream.cuda_stream),
              "gcow_roundtrip_list_device")
        return outs if outs is not None else tensors


def roundtrip_tensors(tensors, params: GcowParams, outs=None, bits: torch.Tensor | None = None, stream=None,
                      plan: TensorListRoundtrip | None = None):
    """decode(encode(cat(tensors), params)) written back tensor by tensor, in one or two launches and without the
    concatenation ever existing (gcow_roundtrip_list_device): tensor s receives values start_s .. start_s + n_s - 1
    of codec.roundtrip(torch.cat([t.view(-1) for t in tensors]), params), bit for bit. tensors: contiguous fp32 or
    bf16 device tensors of one dtype on one device (empty ones are skipped). outs: tensors of the same sizes and one
    dtype (fp32 / bf16; bf16 is the fp32 decode rounded to nearest even); None runs in place. bits: optional int64[1]
    device tensor that receives the bit length `encode` of the concatenation would report. plan: a TensorListRoundtrip
    kept by the caller, so that repeated calls on tensors that stay where they are plan once; without it the call
    plans every time. Returns the list of outputs."""
    if plan is None:
        plan = TensorListRoundtrip(params)
    elif plan.params.tuple() != params.tuple():
        raise GcowError("roundtrip_tensors: the plan object was made for %r" % (plan.params,))
    return plan(tensors, outs, bits, stream)


# roundtrip_gradients' plan objects, one per (parameter set, device): visible so that a caller can drop them
# (gradient_plans.clear()) or read their stats()
gradient_plans: dict = {}


def roundtrip_gradients(parameters, params: GcowParams, bits: torch.Tensor | None = None, stream=None,
                        cache: dict | None = None) -> TensorListRoundtrip:
    """The reference's collect_gradients -> compress -> decompress -> assign_gradients
    (hw/models/train_imagenet.py:448-475) as one call: p.grad of every parameter that has one, in iteration order (the
    order collect_gradients concatenates them in), round-tripped in place as one field. The plan object lives in
    `cache` (default: codec.gradient_plans) under the parameter set and device, so a training loop whose .grad tensors
    stay where they are pays for the plan once. Returns the plan object (stats(), rebuilds)."""
    grads = [q.grad for q in parameters if q.grad is not None]
    if cache is None:
        cache = gradient_plans
    dev = grads[0].device if grads else None
    key = (params.tuple(), str(dev))
    plan = cache.get(key)
    if plan is None:
        plan = cache[key] = TensorListRoundtrip(params)
    plan(grads, None, bits, stream)
    return plan


REL_BITS_MAX = 24  # gcow_roundtrip_rel_device's range of rel_bits


class TensorListRelative(TensorListRoundtrip):
    """The round trip of every tensor of a list as a field of its own, under a tolerance relative to that tensor
    (gcow_roundtrip_rel_device): tensor s is coded in accuracy mode with minexp_s = max(emax_s - rel_bits, -94)
    (capped for a maximum in the top binade so that the decode stays finite: include/gcow.h), emax_s the exponent of
    its largest finite magnitude, which the call finds on the device, so that
    |out - t| <= 2^minexp_s < 2^(1 - rel_bits) max|t_s|. Mirrors TensorListRoundtrip: the object owns the pinned host
    plan and its device copy and re-plans only when the pointers, counts, dtypes or device change (the plan depends on
    neither rel_bits nor maxprec); `rebuilds` counts the plans made, `stats()` gives gcow_roundtrip_rel_stats.
    `absmax` is the float32 tensor of the last call's per-tensor maxima (the caller's, or one kept here)."""

    def __init__(self, rel_bits: int, maxprec: int = 64):
        super().__init__(None)
        self.rel_bits, self.maxprec = int(rel_bits), int(maxprec)
        self.absmax = None

    def _plan(self, tensors, outs, in_dt, out_dt, dev, stream):
        n = len(tensors)
        ins = (C.c_void_p * max(n, 1))(*[t.data_ptr() or None for t in tensors])
        ous = (C.c_void_p * max(n, 1))(*[o.data_ptr() or None for o in outs]) if outs is not None else None
        cnt = (C.c_uint64 * max(n, 1))(*[t.numel() for t in tensors])
        need = self.L.gcow_roundtrip_rel_plan_bytes(n, sum(t.numel() for t in tensors))
        words = (need + 7) // 8
        if self._uploaded is not None:
            self._uploaded.synchronize()  # the pinned plan is still the source of a copy in flight
        if self._h is None or self._h.numel() < words or self._d.device != dev:
            self._h = torch.empty(words, dtype=torch.int64).pin_memory()
            self._d = torch.empty(words, dtype=torch.int64, device=dev)
        used = C.c_size_t(0)
        check(self.L.gcow_roundtrip_rel_plan(ins, ous, cnt, n, in_dt, out_dt, self._h.data_ptr(),
                                             self._h.numel() * 8, C.byref(used)), "gcow_roundtrip_rel_plan")
        self._used = int(used.value)
        w = (self._used + 7) // 8
        with torch.cuda.stream(stream):
            self._d[:w].copy_(self._h[:w], non_blocking=True)
            self._uploaded = torch.cuda.Event()
            self._uploaded.record(stream)
        self.rebuilds += 1

    def stats(self):
        """gcow_roundtrip_rel_stats of the current plan (None before the first call)."""
        if self._h is None:
            return None
        from ._ffi import RoundtripRelStats
        s = RoundtripRelStats()
        check(self.L.gcow_roundtrip_rel_plan_stats(self._h.data_ptr(), self._used, C.byref(s)),
              "gcow_roundtrip_rel_plan_stats")
        return s

    def __call__(self, tensors, outs=None, absmax: torch.Tensor | None = None, bits: torch.Tensor | None = None,
                 stream=None):
        tensors = list(tensors)
        outs = list(outs) if outs is not None else None
        dev = self._check(tensors, outs)
        n = len(tensors)
        if bits is not None and not (bits.is_cuda and bits.device == dev and bits.dtype == torch.int64
                                     and bits.numel() == 1):
            raise GcowError("roundtrip_tensors_relative: bits must be a one-element int64 tensor on the tensors' device")
        if absmax is None:
            if self.absmax is None or self.absmax.numel() != n or self.absmax.device != dev:
                self.absmax = torch.zeros(n, dtype=torch.float32, device=dev)
            absmax = self.absmax
        elif not (absmax.is_cuda and absmax.device == dev and absmax.dtype == torch.float32
                  and absmax.is_contiguous() and absmax.numel() == n):
            raise GcowError("roundtrip_tensors_relative: absmax must be a contiguous float32 tensor of len(tensors) "
                            "values on the tensors' device")
        else:
            self.absmax = absmax
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        in_dt = self._dt(tensors[0].dtype) if tensors else DTYPE_FLOAT
        out_dt = self._dt(outs[0].dtype) if outs else in_dt
        key = (in_dt, out_dt, dev, tuple((t.data_ptr(), t.numel()) for t in tensors),
               tuple(o.data_ptr() for o in outs) if outs is not None else None)
        if key != self._key:
            self._key = None
            self._plan(tensors, outs, in_dt, out_dt, dev, stream)
            self._key = key
        check(self.L.gcow_roundtrip_rel_device(self._h.data_ptr(), self._d.data_ptr(), self._used, self.rel_bits,
                                               self.maxprec, absmax.data_ptr() if n else None,
                                               bits.data_ptr() if bits is not None else None, stream.cuda_stream),
              "gcow_roundtrip_rel_device")
        return outs if outs is not None else tensors


def roundtrip_tensors_relative(tensors, rel_bits: int, outs=None, absmax: torch.Tensor | None = None,
                               bits: torch.Tensor | None = None, stream=None,
                               plan: TensorListRelative | None = None, maxprec: int = 64):
    """Every tensor round-tripped where it lies under a tolerance relative to its own largest magnitude
    (gcow_roundtrip_rel_device): tensor s receives codec.roundtrip(t_s, expert(1, 16658, maxprec, minexp_s)) bit for
    bit, minexp_s = max(emax_s - rel_bits, -94) (capped for emax_s = 128: include/gcow.h), with no host
    synchronisation for the maxima. tensors / outs / bits as
    roundtrip_tensors' (bits: the sum of the per-tensor stream lengths). absmax: optional float32[len(tensors)] device
    tensor that receives every tensor's largest finite magnitude (0 for empty, all-zero or all-non-finite tensors);
    without it one is allocated and kept on the plan object (plan.absmax). plan: a TensorListRelative kept by the
    caller. 0 <= rel_bits <= 24. Returns the list of outputs."""
    if plan is None:
        plan = TensorListRelative(rel_bits, maxprec)
    elif (plan.rel_bits, plan.maxprec) != (int(rel_bits), int(maxprec)):
        raise GcowError("roundtrip_tensors_relative: the plan object was made for rel_bits %d, maxprec %d"
                        % (plan.rel_bits, plan.maxprec))
    return plan(tensors, outs, absmax, bits, stream)


def roundtrip_gradients_relative(parameters, rel_bits: int, bits: torch.Tensor | None = None, stream=None,
                                 cache: dict | None = None, maxprec: int = 64) -> TensorListRelative:
    """roundtrip_gradients with a tolerance relative to each gradient tensor: p.grad of every parameter that has one,
    in iteration order, round-tripped in place by roundtrip_tensors_relative. The plan object lives in `cache`
    (default: codec.gradient_plans) under (rel_bits, maxprec, device). Returns it (stats(), rebuilds, absmax)."""
    grads = [q.grad for q in parameters if q.grad is not None]
    if cache is None:
        cache = gradient_plans
    dev = grads[0].device if grads else None
    key = ("relative", int(rel_bits), int(maxprec), str(dev))
    plan = cache.get(key)
    if plan is None:
        plan = cache[key] = TensorListRelative(rel_bits, maxprec)
    plan(grads, None, None, bits, stream)
    return plan


def field_of_shape(shape, dtype) -> ZfpInput:
    f = ZfpInput()
    f.dtype = DTYPE_BF16 if dtype == torch.bfloat16 else DTYPE_FLOAT
    for i, n in enumerate(reversed(tuple(shape))):
        setattr(f, ["nx", "ny", "nz", "nw"][i], int(n))
    return f


def encode(x: torch.Tensor, params: GcowParams, index_stride: int = 0, stream=None) -> Encoded:
    """zfp_compress of a device tensor (1-4 dims, fp32 or bf16, any strides)."""
    if not x.is_cuda:
        raise GcowError("encode expects a device tensor (host arrays: the sw/ drop-in zfp_compress in libgcow.so, see INTEGRATION.md; or codec.HostEncoder for a pinned 1-D bucket)")
    enc = Encoder(x.shape, x.dtype, params, x.device, index_stride)
    L = enc.L
    f = field_of(x)
    st = L.gcow_encode_device(C.byref(f), C.byref(params), enc.words.data_ptr(), enc.cap, enc.bits_dev.data_ptr(),
                              enc.ws.data_ptr(), enc.ws_bytes,
                              enc.index.data_ptr() if enc.index is not None else None, index_stride,
                              _stream_ptr(stream))
    check(st, "gcow_encode_device")
    return Encoded(enc.words, enc.bits_dev, tuple(x.shape), params, enc.index, index_stride)


def decode(enc_or_words, shape=None, params: GcowParams | None = None, index: torch.Tensor | None = None,
           index_stride: int = 0, out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """zfp_decompress (libzfp 0.5.5 semantics) into an fp32 device tensor, or into `out` (fp32; a 1-D out may be bf16:
    the fp32 decode rounded to nearest even, as `.to(torch.bfloat16)`)."""
    if isinstance(enc_or_words, Encoded):
        e = enc_or_words
        words, shape = e.words, e.shape
        if e.params is not None:  # None: a fitted stream (FittedEncoder), decoded under the params the caller read
            params = e.params
        if index is None and e.index is not None:
            index, index_stride = e.index, e.index_stride
    else:
        words = enc_or_words
    if out is None:
        out = torch.empty(tuple(shape), dtype=torch.float32, device=words.device)
    f = field_of(out)
    L = load()
    st = L.gcow_decode_device(C.byref(f), C.byref(params), words.data_ptr(), words.numel() * 8,
                              index.data_ptr() if index is not None else None, index_stride, _stream_ptr(stream))
    check(st, "gcow_decode_device")
    return out


# ------------------------------------------------------------------------------------------- accuracy under a budget
RATE_TABLE_MINEXP_LO, RATE_TABLE_ENTRIES = -154, 288  # include/gcow.h GCOW_RATE_TABLE_*
RATE_TABLE_TILE_VALUES = 4096  # values one workgroup covers per iteration (csrc/kernels.h kRateTableTileValues)


def is_nobudget(p: GcowParams) -> bool:
    """A variable-rate set whose budget truncates no 1-D block (accuracy, precision, expert(<= 1, >= 160, ...)): the
    domain the rate table describes."""
    return p.minbits <= 1 and p.maxbits >= 160


class RateTable:
    """Preallocated rate table (gcow_rate_table_device) for 1-D buckets of n values: calling it with x returns the
    int64[288] device tensor `table` with table[t] = the bit count codec.encode(x, expert(1, 16658, maxprec,
    -154 + t)) reports -- for every t from one pass over x, exact. The range is complete (a smaller minexp than -154
    changes nothing, from 132 on every block is one bit) and the table is non-increasing. No host synchronisation;
    the table and the workspace are allocated once and need no zeroing."""

    def __init__(self, n: int, dtype, device=None):
        self.L = load()
        self.n, self.dtype = int(n), dtype
        self.device = torch.device(device or "cuda")
        f = field_of_shape((self.n,), dtype)
        self.ws_bytes = self.L.gcow_rate_table_workspace_bytes(C.byref(f))
        self.ws = torch.empty(max(self.ws_bytes // 8, 1), dtype=torch.int64, device=self.device)
        self.table = torch.empty(RATE_TABLE_ENTRIES, dtype=torch.int64, device=self.device)

    def __call__(self, x: torch.Tensor, maxprec: int = 64, stream=None,
                 err: torch.Tensor | None = None) -> torch.Tensor:
        """With `err` (fp32, n values): the table of y = x.float() + err, the array encode_residual codes, formed in
        registers (gcow_rate_table_residual_device)."""
        if x.dim() != 1 or x.numel() != self.n or x.dtype != self.dtype:
            raise GcowError("RateTable built for %d %s values, got %s %s" % (self.n, self.dtype, tuple(x.shape),
                                                                            x.dtype))
        if not (x.is_cuda and x.is_contiguous()):
            raise GcowError("rate_table expects a contiguous 1-D device tensor")
        f = field_of(x) if self.n else field_of_shape((0,), self.dtype)
        if err is None:
            check(self.L.gcow_rate_table_device(C.byref(f), int(maxprec), self.table.data_ptr(), self.ws.data_ptr(),
                                                self.ws_bytes, _stream_ptr(stream)), "gcow_rate_table_device")
            return self.table
        if not (err.is_cuda and err.device == x.device and err.dtype == torch.float32 and err.is_contiguous()
                and err.numel() == self.n):
            raise GcowError("rate_table_residual: err must be a contiguous fp32 tensor of x.numel() values on x's "
                            "device")
        check(self.L.gcow_rate_table_residual_device(C.byref(f), err.data_ptr() if self.n else None, int(maxprec),
                                                     self.table.data_ptr(), self.ws.data_ptr(), self.ws_bytes,
                                                     _stream_ptr(stream)), "gcow_rate_table_residual_device")
        return self.table


def rate_table(x: torch.Tensor, maxprec: int = 64, stream=None) -> torch.Tensor:
    """One-shot RateTable: the int64[288] device tensor of stream lengths of the 1-D device tensor x (fp32 / bf16)
    under expert(1, 16658, maxprec, minexp), minexp = -154 .. 133."""
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise GcowError("dtype %s not supported (float32, bfloat16)" % x.dtype)
    return RateTable(x.numel(), x.dtype, x.device)(x, maxprec, stream)


def rate_table_residual(x: torch.Tensor, err: torch.Tensor | None, maxprec: int = 64, stream=None) -> torch.Tensor:
    """The rate table of y = x.float() + err (err: fp32 device tensor of x.numel() values, or None for zeros): entry t
    is the bit count codec.encode_residual(x, err, expert(1, 16658, maxprec, -154 + t)) reports. One pass over x and
    err; y is never written to memory."""
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise GcowError("dtype %s not supported (float32, bfloat16)" % x.dtype)
    return RateTable(x.numel(), x.dtype, x.device)(x, maxprec, stream, err)


def fit_minexp(table, budget_bits: int):
    """gcow_rate_table_fit: -> (minexp, bits), the smallest minexp of the table whose stream length is <= budget_bits
    and that length. Host code: a device tensor is copied once (288 int64, 2.3 KB) -- the only synchronisation of the
    feature; a host tensor, array or list is read as is. GcowError when the budget is below the last entry (one bit
    per block)."""
    if isinstance(table, torch.Tensor):
        table = table.detach().reshape(-1).cpu().tolist()
    vals = [int(v) for v in table]
    if len(vals) != RATE_TABLE_ENTRIES:
        raise GcowError("fit_minexp: a rate table has %d entries, got %d" % (RATE_TABLE_ENTRIES, len(vals)))
    h = (C.c_uint64 * RATE_TABLE_ENTRIES)(*vals)
    me, bits = C.c_int(0), C.c_uint64(0)
    check(load().gcow_rate_table_fit(h, max(int(budget_bits), 0), C.byref(me), C.byref(bits)), "gcow_rate_table_fit")
    return int(me.value), int(bits.value)


def fitted_params(maxprec: int, minexp: int) -> GcowParams:
    """The parameter set a fit stands for: accuracy mode (no bit budget) at that minexp."""
    return GcowParams(ZFP_MIN_BITS, ZFP_MAX_BITS, int(maxprec), int(minexp))


def fit_accuracy(x: torch.Tensor, bits_per_value: float, maxprec: int = 64, stream=None) -> GcowParams:
    """The finest accuracy-mode set whose stream of x (1-D device tensor) takes at most floor(bits_per_value * n) bits:
    expert(1, 16658, maxprec, minexp) with minexp fitted on x's rate table. One pass over x and one 2.3 KB host read,
    where re-encoding until the length fits costs a full encode and a host read per try."""
    budget = int(math.floor(bits_per_value * x.numel()))
    me, _ = fit_minexp(rate_table(x.reshape(-1), maxprec, stream), budget)
    return fitted_params(maxprec, me)


def encode_fitted(x: torch.Tensor, bits_per_value: float, maxprec: int = 64, index_stride: int = 0, stream=None):
    """-> (Encoded, params): x (1-D device tensor) encoded under fit_accuracy(x, bits_per_value, maxprec). Guarantees
    Encoded.bits <= floor(bits_per_value * n): the table entry is the encoder's own bit count."""
    p = fit_accuracy(x, bits_per_value, maxprec, stream)
    return encode(x, p, index_stride, stream), p


# ------------------------------------------------------------------------------------------- the fit on the device
# A gcow_fit record (include/gcow.h) as a device tensor: int64[2], word 0 = minexp (low half, signed) | status << 32,
# word 1 = bits. Its first 4 bytes are the int32 word the fitted calls read.
FIT_WORDS = 2


def new_fit_record(device=None) -> torch.Tensor:
    return torch.zeros(FIT_WORDS, dtype=torch.int64, device=torch.device(device or "cuda"))


def read_fit(fit: torch.Tensor):
    """-> (minexp, status, bits) of a gcow_fit record: the host read of its 16 bytes (a synchronisation when the record
    is on the device)."""
    w0, w1 = (int(v) for v in fit.detach().reshape(-1)[:FIT_WORDS].cpu().tolist())
    me = w0 & 0xFFFFFFFF
    return (me - (1 << 32) if me >> 31 else me), (w0 >> 32) & 0xFFFFFFFF, w1 & ((1 << 64) - 1)


def _budget_u64(budget_bits) -> int:
    return min(max(int(budget_bits), 0), (1 << 64) - 1)


def fit_device(table: torch.Tensor, budget_bits: int, out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """gcow_rate_table_fit_device: the fit of a device rate table (int64[288], one bucket's or a sum over ranks)
    against budget_bits, written to the gcow_fit record `out` (default: a new one) by one small kernel. Nothing is
    read on the host; the record equals fit_minexp's answer with status 0, or the coarsest set (minexp 133) with
    status 1 where fit_minexp raises. Returns the record: pass it to encode_fitted_device / roundtrip_fitted as the
    minexp word, read it with read_fit."""
    if not (isinstance(table, torch.Tensor) and table.is_cuda and table.dtype == torch.int64
            and table.numel() == RATE_TABLE_ENTRIES and table.is_contiguous()):
        raise GcowError("fit_device: table must be a contiguous int64[%d] device tensor" % RATE_TABLE_ENTRIES)
    if out is None:
        out = new_fit_record(table.device)
    if not (out.is_cuda and out.device == table.device and out.dtype == torch.int64 and out.numel() >= FIT_WORDS
            and out.is_contiguous()):
        raise GcowError("fit_device: out must be a contiguous int64[%d] tensor on the table's device" % FIT_WORDS)
    check(load().gcow_rate_table_fit_device(table.data_ptr(), _budget_u64(budget_bits), out.data_ptr(),
                                            _stream_ptr(stream)), "gcow_rate_table_fit_device")
    return out


def _minexp_ptr(word: torch.Tensor, device) -> int:
    if not (isinstance(word, torch.Tensor) and word.is_cuda and word.device == device and word.numel() >= 1
            and word.dtype in (torch.int32, torch.int64) and word.is_contiguous()):
        raise GcowError("minexp_word must be an int32 tensor (or a gcow_fit record from fit_device) on x's device")
    return word.data_ptr()


class FittedEncoder:
    """Accuracy mode under a bit budget with no host read: preallocated rate table, gcow_fit record, stream, bit count,
    index and workspace for 1-D buckets of n values. Calling it with x launches the table pass, the device fit against
    floor(bits_per_value * n) bits and gcow_encode_fitted_device, which takes minexp from the record, and returns an
    Encoded whose `params` is None -- the set is on the device. The call allocates nothing and synchronises nothing,
    so it can be captured into a graph that then follows the data it is replayed on. `fit` is the device record;
    `params()` reads it (the only synchronisation) for codec.decode. The stream is byte for byte
    codec.encode_fitted's whenever the budget can be met (status 0)."""

    def __init__(self, n: int, dtype, bits_per_value: float, maxprec: int = 64, device=None, index_stride: int = 0):
        self.n, self.dtype, self.maxprec = int(n), dtype, int(maxprec)
        self.device = torch.device(device or "cuda")
        self.budget = int(math.floor(bits_per_value * self.n))
        self.table = RateTable(self.n, dtype, self.device)
        self.fit = new_fit_record(self.device)
        # capacity and workspace do not depend on minexp (include/gcow.h): sized from any set of this maxprec
        self.enc = Encoder((self.n,), dtype, fitted_params(self.maxprec, 0), self.device, index_stride)
        self.L = self.enc.L

    def __call__(self, x: torch.Tensor, stream=None) -> Encoded:
        self.table(x, self.maxprec, stream)  # checks x
        fit_device(self.table.table, self.budget, self.fit, stream)
        return _encode_fitted_into(self.enc, x, self.fit, stream)

    def params(self, allow_coarsest: bool = False) -> GcowParams:
        """fitted_params(maxprec, the fitted minexp), from one host read of the record. GcowError when the budget was
        below one bit per block and the coarsest set was taken (status 1), unless allow_coarsest."""
        me, status, _ = read_fit(self.fit)
        if status and not allow_coarsest:
            raise GcowError("budget of %d bits is below one bit per block: the coarsest set was used "
                            "(allow_coarsest=True accepts it)" % self.budget)
        return fitted_params(self.maxprec, me)


def _encode_fitted_into(enc: Encoder, x: torch.Tensor, minexp_word: torch.Tensor, stream=None) -> Encoded:
    if x.dim() != 1 or tuple(x.shape) != enc.shape or x.dtype != enc.dtype:
        raise GcowError("fitted encoder built for %s %s, got %s %s" % (enc.shape, enc.dtype, tuple(x.shape), x.dtype))
    if not (x.is_cuda and x.is_contiguous()):
        raise GcowError("encode_fitted_device expects a contiguous 1-D device tensor")
    f = field_of(x) if x.numel() else field_of_shape((0,), x.dtype)
    st = enc.L.gcow_encode_fitted_device(C.byref(f), enc.params.maxprec, _minexp_ptr(minexp_word, x.device),
                                         enc.words.data_ptr(), enc.cap, enc.bits_dev.data_ptr(), enc.ws.data_ptr(),
                                         enc.ws_bytes, enc.index.data_ptr() if enc.index is not None else None,
                                         enc.index_stride, _stream_ptr(stream))
    check(st, "gcow_encode_fitted_device")
    return Encoded(enc.words, enc.bits_dev, enc.shape, None, enc.index, enc.index_stride)


def encode_fitted_device(x: torch.Tensor, minexp_word: torch.Tensor, maxprec: int = 64, index_stride: int = 0,
                         stream=None) -> Encoded:
    """gcow_encode_fitted_device: x (contiguous 1-D device tensor, fp32 / bf16) encoded under
    expert(1, 16658, maxprec, clamp(minexp_word[0], -154, 133)), the word (an int32 device tensor, or a gcow_fit record
    from fit_device) read on the device when the kernels run. Byte for byte codec.encode under that set. The returned
    Encoded has params None: decode with the params read from the record."""
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise GcowError("dtype %s not supported (float32, bfloat16)" % x.dtype)
    if not x.is_cuda:
        raise GcowError("encode_fitted_device expects a device tensor")
    enc = Encoder((x.numel(),), x.dtype, fitted_params(maxprec, 0), x.device, index_stride)
    return _encode_fitted_into(enc, x, minexp_word, stream)


def _encode_residual_fitted_into(enc: Encoder, x: torch.Tensor, err: torch.Tensor, minexp_word: torch.Tensor,
                                 stream=None) -> Encoded:
    if x.dim() != 1 or tuple(x.shape) != enc.shape:
        raise GcowError("fitted residual encoder built for %s, got %s" % (enc.shape, tuple(x.shape)))
    _check_err(x, err)
    f = field_of(x) if x.numel() else field_of_shape((0,), x.dtype)
    st = enc.L.gcow_encode_residual_fitted_device(C.byref(f), enc.params.maxprec, _minexp_ptr(minexp_word, x.device),
                                                  err.data_ptr(), err.data_ptr(), enc.words.data_ptr(), enc.cap,
                                                  enc.bits_dev.data_ptr(), enc.ws.data_ptr(), enc.ws_bytes,
                                                  enc.index.data_ptr() if enc.index is not None else None,
                                                  enc.index_stride, _stream_ptr(stream))
    check(st, "gcow_encode_residual_fitted_device")
    return Encoded(enc.words, enc.bits_dev, enc.shape, None, enc.index, enc.index_stride)


def encode_residual_fitted_device(x: torch.Tensor, err: torch.Tensor, minexp_word: torch.Tensor, maxprec: int = 64,
                                  index_stride: int = 0, stream=None) -> Encoded:
    """gcow_encode_residual_fitted_device: error feedback under a minexp word in device memory. y = x + err (x:
    contiguous 1-D device tensor, fp32 / bf16; err: fp32, updated in place) is encoded under
    expert(1, 16658, maxprec, clamp(minexp_word[0], -154, 133)), the word (an int32 device tensor, or a gcow_fit record
    from fit_device) read on the device when the kernels run. Stream, bits, index and err are byte for byte
    codec.encode_residual's under that set. x and err must be 16-byte aligned (GcowError otherwise: there is no
    composed fallback). The returned Encoded has params None."""
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise GcowError("dtype %s not supported (float32, bfloat16)" % x.dtype)
    if not x.is_cuda:
        raise GcowError("encode_residual_fitted_device expects a device tensor")
    # capacity and workspace are those of the fp32 field y, and do not depend on minexp
    enc = Encoder((x.numel(),), torch.float32, fitted_params(maxprec, 0), x.device, index_stride)
    return _encode_residual_fitted_into(enc, x, err, minexp_word, stream)


class FittedResidualEncoder:
    """Error feedback under a bit budget with no host read: FittedEncoder for y = x + err. Calling it with (x, err)
    launches the rate table of y (formed in registers, gcow_rate_table_residual_device), the device fit against
    floor(bits_per_value * n) bits and gcow_encode_residual_fitted_device, which codes y under the fitted set and
    leaves err = finite(y - decode(stream)). The budget therefore holds for what is encoded, y, not for x alone.
    Everything is preallocated: the three launches allocate and synchronise nothing and capture into one graph.
    `fit`, `params()` as FittedEncoder's."""

    def __init__(self, n: int, dtype, bits_per_value: float, maxprec: int = 64, device=None, index_stride: int = 0):
        self.n, self.dtype, self.maxprec = int(n), dtype, int(maxprec)
        self.device = torch.device(device or "cuda")
        self.budget = int(math.floor(bits_per_value * self.n))
        self.table = RateTable(self.n, dtype, self.device)
        self.fit = new_fit_record(self.device)
        self.enc = Encoder((self.n,), torch.float32, fitted_params(self.maxprec, 0), self.device, index_stride)
        self.L = self.enc.L

    def __call__(self, x: torch.Tensor, err: torch.Tensor, stream=None) -> Encoded:
        self.table(x, self.maxprec, stream, err)  # checks x and err
        fit_device(self.table.table, self.budget, self.fit, stream)
        return _encode_residual_fitted_into(self.enc, x, err, self.fit, stream)

    params = FittedEncoder.params


def roundtrip_fitted(x: torch.Tensor, fit, maxprec: int = 64, out: torch.Tensor | None = None,
                     bits: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """codec.roundtrip under a set fitted on the device (gcow_roundtrip_fitted_device). `fit` is either a number --
    bits per value: x's rate table and its device fit against floor(fit * n) bits are launched first -- or a minexp
    word (an int32 device tensor or a gcow_fit record). No host read either way. x, out, bits as codec.roundtrip's;
    returns out."""
    if not (x.is_cuda and x.is_contiguous() and x.dim() >= 1):
        raise GcowError("roundtrip_fitted expects a contiguous device tensor")
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise GcowError("roundtrip_fitted: dtype %s not supported (float32, bfloat16)" % x.dtype)
    if out is None:
        out = torch.empty_like(x)
    if not (out.is_cuda and out.device == x.device and out.is_contiguous() and out.numel() == x.numel()
            and out.dtype in (torch.float32, torch.bfloat16)):
        raise GcowError("roundtrip_fitted: out must be a contiguous fp32 or bf16 tensor of x.numel() values on x's "
                        "device")
    if bits is not None and not (bits.is_cuda and bits.device == x.device and bits.dtype == torch.int64
                                 and bits.numel() == 1):
        raise GcowError("roundtrip_fitted: bits must be a one-element int64 tensor on x's device")
    flat = x.view(-1)
    if not isinstance(fit, torch.Tensor):
        budget = int(math.floor(fit * flat.numel()))
        fit = fit_device(rate_table(flat, maxprec, stream), budget, stream=stream)
    f = field_of(flat) if flat.numel() else field_of_shape((0,), x.dtype)
    st = load().gcow_roundtrip_fitted_device(C.byref(f), int(maxprec), _minexp_ptr(fit, x.device), out.data_ptr(),
                                             DTYPE_BF16 if out.dtype == torch.bfloat16 else DTYPE_FLOAT,
                                             bits.data_ptr() if bits is not None else None, _stream_ptr(stream))
    check(st, "gcow_roundtrip_fitted_device")
    return out


# ------------------------------------------------------------------------------------------- bit budget, tensor list
RATE_TABLE_LIST_MAX_GRID = 1024  # workgroups of the table pass over a plan (csrc/kernels.h kRateTableListMaxGrid)


class TensorListFitted(TensorListRoundtrip):
    """Accuracy mode under a bit budget over a tensor list, with no host read: the rate table of the concatenation
    (gcow_rate_table_list_device), the device fit against floor(bits_per_value * N) bits and the fitted round trip
    (gcow_roundtrip_list_fitted_device), every tensor read and written where it lies. Each tensor receives its slice
    of codec.roundtrip_fitted(torch.cat(...), bits_per_value, maxprec), bit for bit. A TensorListRoundtrip planned for
    a set without a block budget: the plan, the table, the workspace, the gcow_fit record and a bit count are
    allocated once (on the first call: the device is the tensors'), so later calls allocate nothing, synchronise
    nothing and capture into a graph that then follows the data it is replayed on. N is known on the host from the
    tensors. `table` and `fit` are the device tensors of the last call, `bits` its int64[1] bit count; `params()`
    reads the record."""

    def __init__(self, bits_per_value: float, maxprec: int = 64):
        super().__init__(fitted_params(maxprec, 0))  # the plan reads neither maxprec nor minexp
        self.bits_per_value, self.maxprec = float(bits_per_value), int(maxprec)
        self.budget = 0
        self.table = self.fit = self.ws = self.bits = None
        self.ws_bytes = 0

    def _buffers(self, dev):
        if self.table is None or self.table.device != dev:
            self.ws_bytes = self.L.gcow_rate_table_list_workspace_bytes(self._h.data_ptr(), self._used)
            self.ws = torch.empty(max(self.ws_bytes // 8, 1), dtype=torch.int64, device=dev)
            self.table = torch.empty(RATE_TABLE_ENTRIES, dtype=torch.int64, device=dev)
            self.fit = new_fit_record(dev)
            self.bits = torch.zeros(1, dtype=torch.int64, device=dev)

    def _table(self, stream):
        check(self.L.gcow_rate_table_list_device(self._h.data_ptr(), self._d.data_ptr(), self._used, self.maxprec,
                                                 self.table.data_ptr(), self.ws.data_ptr(), self.ws_bytes,
                                                 stream.cuda_stream), "gcow_rate_table_list_device")

    def rate_table(self, tensors, stream=None) -> torch.Tensor:
        """The int64[288] device table of the concatenation (codec.rate_table(torch.cat(...), maxprec), exactly). The
        pass reads inputs only: a plan already made for these tensors, with whatever outputs, is used as it is."""
        tensors = list(tensors)
        dev = self._check(tensors, None)
        k = self._key
        same = k is not None and k[2] == dev and k[3] == tuple((t.data_ptr(), t.numel()) for t in tensors) and \
            k[0] == (self._dt(tensors[0].dtype) if tensors else DTYPE_FLOAT)
        if same:
            stream = stream if stream is not None else torch.cuda.current_stream(dev)
        else:
            tensors, _, dev, stream = self._prepare(tensors, None, None, stream)
        self._buffers(dev)
        self._table(stream)
        return self.table

    def run(self, tensors, fit, outs=None, bits: torch.Tensor | None = None, stream=None):
        """__call__ with the budget or the minexp word given per call: `fit` is a number (bits per value: table, fit
        and round trip) or a minexp word / gcow_fit record on the tensors' device (the round trip alone)."""
        tensors, outs, dev, stream = self._prepare(tensors, outs, bits, stream)
        self._buffers(dev)
        if isinstance(fit, torch.Tensor):
            word = _minexp_ptr(fit, dev)
        else:
            self.budget = int(math.floor(fit * sum(t.numel() for t in tensors)))
            self._table(stream)
            fit_device(self.table, self.budget, self.fit, stream)
            word = self.fit.data_ptr()
        check(self.L.gcow_roundtrip_list_fitted_device(self._h.data_ptr(), self._d.data_ptr(), self._used,
                                                       self.maxprec, word,
                                                       (bits if bits is not None else self.bits).data_ptr(),
                                                       stream.cuda_stream), "gcow_roundtrip_list_fitted_device")
        return outs if outs is not None else tensors

    def __call__(self, tensors, outs=None, bits: torch.Tensor | None = None, stream=None):
        return self.run(tensors, self.bits_per_value, outs, bits, stream)

    params = FittedEncoder.params


def _list_fitted_plan(plan, bits_per_value, maxprec, what):
    if plan is None:
        return TensorListFitted(bits_per_value, maxprec)
    if not isinstance(plan, TensorListFitted) or plan.maxprec != int(maxprec):
        raise GcowError("%s: the plan object must be a TensorListFitted of maxprec %d" % (what, int(maxprec)))
    return plan


def rate_table_tensors(tensors, maxprec: int = 64, stream=None, plan: TensorListFitted | None = None) -> torch.Tensor:
    """codec.rate_table of the concatenation of a list of tensors, each read where it lies
    (gcow_rate_table_list_device): the int64[288] device tensor of stream lengths of cat(tensors) under
    expert(1, 16658, maxprec, minexp), minexp = -154 .. 133, exactly. tensors as roundtrip_tensors'. plan: a
    TensorListFitted of this maxprec kept by the caller (the table is its `table`); without it the call plans and
    allocates every time."""
    return _list_fitted_plan(plan, 0.0, maxprec, "rate_table_tensors").rate_table(tensors, stream)


def roundtrip_tensors_fitted(tensors, fit, maxprec: int = 64, outs=None, bits: torch.Tensor | None = None, stream=None,
                             plan: TensorListFitted | None = None):
    """codec.roundtrip_fitted(torch.cat(tensors), fit, maxprec) written back tensor by tensor, without the
    concatenation ever existing (gcow_roundtrip_list_fitted_device). `fit` is a number -- bits per value: the list's
    rate table and its device fit against floor(fit * N) bits are launched first -- or a minexp word (an int32 device
    tensor or a gcow_fit record). No host read either way. tensors / outs / bits as roundtrip_tensors'; plan: a
    TensorListFitted of this maxprec kept by the caller. Returns the list of outputs."""
    if not isinstance(fit, torch.Tensor) and not isinstance(fit, (int, float)):
        raise GcowError("roundtrip_tensors_fitted: fit must be a number of bits per value or a device minexp word")
    bpv = 0.0 if isinstance(fit, torch.Tensor) else fit
    return _list_fitted_plan(plan, bpv, maxprec, "roundtrip_tensors_fitted").run(tensors, fit, outs, bits, stream)


def roundtrip_gradients_fitted(parameters, bits_per_value: float, maxprec: int = 64, bits: torch.Tensor | None = None,
                               stream=None, cache: dict | None = None) -> TensorListFitted:
    """roundtrip_gradients in accuracy mode under a bit budget: p.grad of every parameter that has one, in iteration
    order, round-tripped in place as one field of N values under the finest tolerance whose stream takes at most
    floor(bits_per_value * N) bits -- table, fit and round trip on the device, no host read. The plan object lives in
    `cache` (default: codec.gradient_plans) under ("fitted", bits_per_value, maxprec, device). Returns it (stats(),
    rebuilds, table, fit, bits, params())."""
    grads = [q.grad for q in parameters if q.grad is not None]
    if cache is None:
        cache = gradient_plans
    dev = grads[0].device if grads else None
    key = ("fitted", float(bits_per_value), int(maxprec), str(dev))
    plan = cache.get(key)
    if plan is None:
        plan = cache[key] = TensorListFitted(bits_per_value, maxprec)
    plan(grads, None, bits, stream)
    return plan


# ------------------------------------------------------------------------------------- bit budget, a tensor at a time
MINEXP_FLOOR = -94  # the default floor of a per-tensor fit: gcow_roundtrip_rel_device's, for the same reason


def _fit_records(fits: torch.Tensor, n: int, dev, what: str):
    """-> (pointer, stride in 4-byte words) of per-tensor minexp words: int64[n, 2] gcow_fit records (stride 4) or
    int32[n] packed words (stride 1)."""
    if not (isinstance(fits, torch.Tensor) and fits.is_cuda and fits.device == dev and fits.is_contiguous()):
        raise GcowError("%s: fits must be a contiguous tensor on the tensors' device" % what)
    if fits.dtype == torch.int64 and fits.numel() == FIT_WORDS * n:
        return fits.data_ptr(), 4
    if fits.dtype == torch.int32 and fits.numel() == n:
        return fits.data_ptr(), 1
    raise GcowError("%s: fits must be int64[%d, 2] gcow_fit records or int32[%d] minexp words" % (what, n, n))


def fit_device_batch(tables: torch.Tensor, budgets: torch.Tensor, minexp_floor: int = RATE_TABLE_MINEXP_LO,
                     out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """gcow_rate_table_fit_batch_device: table s (tables: int64[S, 288] on the device) fitted against budgets[s]
    (int64[S] on the device, in bits) over the entries at minexp >= minexp_floor, one workgroup per table and no host
    read. -> `out` (default: new), int64[S, 2]: S gcow_fit records -- row s is what fit_device(tables[s], budgets[s])
    writes when the floor is -154; where no entry fits, (133, status 1, tables[s][287])."""
    if not (isinstance(tables, torch.Tensor) and tables.is_cuda and tables.dtype == torch.int64 and tables.dim() == 2
            and tables.shape[1] == RATE_TABLE_ENTRIES and tables.is_contiguous()):
        raise GcowError("fit_device_batch: tables must be a contiguous int64[S, %d] device tensor" % RATE_TABLE_ENTRIES)
    n = tables.shape[0]
    if not (isinstance(budgets, torch.Tensor) and budgets.is_cuda and budgets.device == tables.device
            and budgets.dtype == torch.int64 and budgets.numel() == n and budgets.is_contiguous()):
        raise GcowError("fit_device_batch: budgets must be a contiguous int64[%d] tensor on the tables' device" % n)
    if out is None:
        out = torch.zeros((n, FIT_WORDS), dtype=torch.int64, device=tables.device)
    if not (out.is_cuda and out.device == tables.device and out.dtype == torch.int64 and out.numel() == FIT_WORDS * n
            and out.is_contiguous()):
        raise GcowError("fit_device_batch: out must be a contiguous int64[%d, %d] tensor on the tables' device"
                        % (n, FIT_WORDS))
    check(load().gcow_rate_table_fit_batch_device(tables.data_ptr() if n else None, n,
                                                  budgets.data_ptr() if n else None, int(minexp_floor),
                                                  out.data_ptr() if n else None, _stream_ptr(stream)),
          "gcow_rate_table_fit_batch_device")
    return out


class TensorListFittedPerTensor(TensorListRelative):
    """Accuracy mode under a bit budget for every tensor of a list, with no host read: tensor s is a field of its own
    (as in TensorListRelative, whose plan this is), with its own rate table (gcow_rate_table_rel_device), its own
    budget of floor(bits_per_value * n_s) bits, its own device fit over minexp >= minexp_floor
    (gcow_rate_table_fit_batch_device) and the round trip under that fit (gcow_roundtrip_rel_fitted_device): tensor s
    receives codec.roundtrip_fitted(t_s, fits[s], maxprec), bit for bit. The loud tensors of a gradient list neither
    decide the quiet ones' tolerance nor take their bits, and the bits of each tensor are bounded.

    The object owns the pinned plan and its device copy, the tables (`tables`, int64[S, 288]), the workspace, the
    gcow_fit records (`fits`, int64[S, 2]: word 0 = minexp | status << 32, word 1 = bits), the device budgets
    (`budgets`, int64[S]) and a bit count (`bits`, int64[1]). They are (re)made and the budgets uploaded only when the
    plan is rebuilt -- pointers, counts, dtypes or device changed -- so later calls allocate nothing, synchronise
    nothing and capture into one graph (a linear chain) that then follows the data it is replayed on. `rebuilds` and
    `stats()` are TensorListRelative's. The default floor of -94 keeps blocks of scale below 2^-98 at precision 0
    (they decode to +0, not to garbage: include/gcow.h); the relative form's cap for maxima in the top binade has no
    counterpart here."""

    def __init__(self, bits_per_value: float, maxprec: int = 64, minexp_floor: int = MINEXP_FLOOR):
        super().__init__(0, maxprec)
        self.bits_per_value, self.minexp_floor = float(bits_per_value), int(minexp_floor)
        self.tables = self.fits = self.budgets = self.ws = self.bits = None
        self.ws_bytes = 0
        self._h_budgets = None

    def _plan(self, tensors, outs, in_dt, out_dt, dev, stream):
        if self._uploaded is not None:
            self._uploaded.synchronize()  # the pinned budgets are still the source of a copy in flight
        super()._plan(tensors, outs, in_dt, out_dt, dev, stream)
        n = len(tensors)
        if self.tables is None or self.tables.shape[0] != n or self.tables.device != dev:
            self.ws_bytes = self.L.gcow_rate_table_rel_workspace_bytes(self._h.data_ptr(), self._used)
            self.ws = torch.empty(max(self.ws_bytes // 8, 1), dtype=torch.int64, device=dev)
            self.tables = torch.empty((n, RATE_TABLE_ENTRIES), dtype=torch.int64, device=dev)
            self.fits = torch.zeros((n, FIT_WORDS), dtype=torch.int64, device=dev)
            self.budgets = torch.zeros(n, dtype=torch.int64, device=dev)
            self.bits = torch.zeros(1, dtype=torch.int64, device=dev)
            self._h_budgets = torch.zeros(n, dtype=torch.int64).pin_memory()
        for s, t in enumerate(tensors):
            self._h_budgets[s] = int(math.floor(self.bits_per_value * t.numel()))
        with torch.cuda.stream(stream):
            self.budgets.copy_(self._h_budgets, non_blocking=True)
            self._uploaded = torch.cuda.Event()
            self._uploaded.record(stream)

    def _current(self, tensors, outs, bits, stream, what):
        tensors = list(tensors)
        outs = list(outs) if outs is not None else None
        dev = self._check(tensors, outs)
        if bits is not None and not (bits.is_cuda and bits.device == dev and bits.dtype == torch.int64
                                     and bits.numel() == 1):
            raise GcowError("%s: bits must be a one-element int64 tensor on the tensors' device" % what)
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        in_dt = self._dt(tensors[0].dtype) if tensors else DTYPE_FLOAT
        out_dt = self._dt(outs[0].dtype) if outs else in_dt
        key = (in_dt, out_dt, dev, tuple((t.data_ptr(), t.numel()) for t in tensors),
               tuple(o.data_ptr() for o in outs) if outs is not None else None)
        if key != self._key:
            self._key = None
            self._plan(tensors, outs, in_dt, out_dt, dev, stream)
            self._key = key
        return tensors, outs, dev, stream

    def _tables(self, n, stream):
        check(self.L.gcow_rate_table_rel_device(self._h.data_ptr(), self._d.data_ptr(), self._used, self.maxprec,
                                                self.tables.data_ptr() if n else None,
                                                self.ws.data_ptr(), self.ws_bytes, stream.cuda_stream),
              "gcow_rate_table_rel_device")

    def rate_tables(self, tensors, stream=None) -> torch.Tensor:
        """The int64[S, 288] device tables: row s is codec.rate_table(t_s, maxprec), exactly (zeros for an empty
        tensor). The pass reads inputs only: a plan already made for these tensors, with whatever outputs, is used as
        it is."""
        tensors = list(tensors)
        dev = self._check(tensors, None)
        k = self._key
        same = k is not None and k[2] == dev and k[3] == tuple((t.data_ptr(), t.numel()) for t in tensors) and \
            k[0] == (self._dt(tensors[0].dtype) if tensors else DTYPE_FLOAT)
        if same:
            stream = stream if stream is not None else torch.cuda.current_stream(dev)
        else:
            tensors, _, dev, stream = self._current(tensors, None, None, stream, "rate_tables_tensors")
        self._tables(len(tensors), stream)
        return self.tables

    def run(self, tensors, fits=None, outs=None, bits: torch.Tensor | None = None, stream=None):
        """__call__ with the fits given per call: None -- tables, fits against the object's budgets, round trip -- or
        per-tensor minexp words on the tensors' device (int64[S, 2] gcow_fit records or int32[S] packed words: the
        round trip alone). Words outside [-154, 133] are clamped."""
        tensors, outs, dev, stream = self._current(tensors, outs, bits, stream, "roundtrip_tensors_fitted_per_tensor")
        n = len(tensors)
        if fits is None:
            self._tables(n, stream)
            fit_device_batch(self.tables, self.budgets, self.minexp_floor, self.fits, stream)
            fits = self.fits
        ptr, stride = _fit_records(fits, n, dev, "roundtrip_tensors_fitted_per_tensor")
        check(self.L.gcow_roundtrip_rel_fitted_device(self._h.data_ptr(), self._d.data_ptr(), self._used,
                                                      self.maxprec, ptr if n else None, stride,
                                                      (bits if bits is not None else self.bits).data_ptr(),
                                                      stream.cuda_stream), "gcow_roundtrip_rel_fitted_device")
        return outs if outs is not None else tensors

    def __call__(self, tensors, outs=None, bits: torch.Tensor | None = None, stream=None):
        return self.run(tensors, None, outs, bits, stream)


def _per_tensor_plan(plan, bits_per_value, maxprec, minexp_floor, what):
    if plan is None:
        return TensorListFittedPerTensor(bits_per_value, maxprec, minexp_floor)
    if not isinstance(plan, TensorListFittedPerTensor) or plan.maxprec != int(maxprec):
        raise GcowError("%s: the plan object must be a TensorListFittedPerTensor of maxprec %d" % (what, int(maxprec)))
    return plan


def rate_tables_tensors(tensors, maxprec: int = 64, stream=None,
                        plan: TensorListFittedPerTensor | None = None) -> torch.Tensor:
    """codec.rate_table of every tensor of a list from one pass, each read where it lies (gcow_rate_table_rel_device):
    the int64[S, 288] device tensor whose row s holds the stream lengths of t_s under
    expert(1, 16658, maxprec, minexp), minexp = -154 .. 133, exactly. tensors as roundtrip_tensors'. plan: a
    TensorListFittedPerTensor of this maxprec kept by the caller (the tables are its `tables`); without it the call
    plans and allocates every time."""
    return _per_tensor_plan(plan, 0.0, maxprec, MINEXP_FLOOR, "rate_tables_tensors").rate_tables(tensors, stream)


def roundtrip_tensors_fitted_per_tensor(tensors, fit, maxprec: int = 64, outs=None, bits: torch.Tensor | None = None,
                                        stream=None, plan: TensorListFittedPerTensor | None = None,
                                        minexp_floor: int = MINEXP_FLOOR):
    """Every tensor round-tripped where it lies under its own fitted tolerance (gcow_roundtrip_rel_fitted_device).
    `fit` is a number -- bits per value: every tensor's rate table and its device fit against floor(fit * n_s) bits
    over minexp >= minexp_floor are launched first -- or per-tensor minexp words on the device (int64[S, 2] gcow_fit
    records or int32[S]). Tensor s receives codec.roundtrip_fitted(t_s, word_s, maxprec) bit for bit; no host read
    either way. tensors / outs / bits as roundtrip_tensors' (bits: the sum of the per-tensor stream lengths). plan: a
    TensorListFittedPerTensor of this maxprec kept by the caller (a number must then be the plan's own
    bits_per_value, and the floor the plan's). Returns the list of outputs."""
    what = "roundtrip_tensors_fitted_per_tensor"
    if isinstance(fit, torch.Tensor):
        return _per_tensor_plan(plan, 0.0, maxprec, minexp_floor, what).run(tensors, fit, outs, bits, stream)
    if not isinstance(fit, (int, float)):
        raise GcowError("%s: fit must be a number of bits per value or device minexp words" % what)
    p = _per_tensor_plan(plan, fit, maxprec, minexp_floor, what)
    if (p.bits_per_value, p.minexp_floor) != (float(fit), int(minexp_floor)):
        raise GcowError("%s: the plan object was made for %g bits per value and floor %d"
                        % (what, p.bits_per_value, p.minexp_floor))
    return p.run(tensors, None, outs, bits, stream)


def roundtrip_gradients_fitted_per_tensor(parameters, bits_per_value: float, maxprec: int = 64,
                                          bits: torch.Tensor | None = None, stream=None, cache: dict | None = None,
                                          minexp_floor: int = MINEXP_FLOOR) -> TensorListFittedPerTensor:
    """roundtrip_gradients under a bit budget per gradient tensor: p.grad of every parameter that has one, in
    iteration order, round-tripped in place, each as a field of its own under the finest tolerance (minexp >=
    minexp_floor) whose stream takes at most floor(bits_per_value * n_s) bits -- tables, fits and round trip on the
    device, no host read. The plan object lives in `cache` (default: codec.gradient_plans) under ("fitted_per_tensor",
    bits_per_value, maxprec, minexp_floor, device). Returns it (stats(), rebuilds, tables, fits, budgets, bits)."""
    grads = [q.grad for q in parameters if q.grad is not None]
    if cache is None:
        cache = gradient_plans
    dev = grads[0].device if grads else None
    key = ("fitted_per_tensor", float(bits_per_value), int(maxprec), int(minexp_floor), str(dev))
    plan = cache.get(key)
    if plan is None:
        plan = cache[key] = TensorListFittedPerTensor(bits_per_value, maxprec, minexp_floor)
    plan(grads, None, bits, stream)
    return plan


# ------------------------------------------------------------------------------ segmented fields: a minexp per tensor
class SegmentPlan:
    """The plan of a segmented field (gcow_seg_plan; include/gcow.h "Segmented fields"): a contiguous buffer of
    sum(counts) values of `dtype` cut into len(counts) tensors in order. It holds no pointers and depends on neither
    maxprec nor the minexp words, so one plan serves every buffer of the shape, the encode and the decode. The host plan
    is `h` (int64, `used` bytes); with `device` its copy `d` is made at once (else by `to`)."""

    def __init__(self, counts, dtype=torch.float32, device=None):
        self.L = load()
        self.counts = tuple(int(c) for c in counts)
        if any(c < 0 for c in self.counts):
            raise GcowError("SegmentPlan: negative count")
        if dtype not in (torch.float32, torch.bfloat16):
            raise GcowError("SegmentPlan: dtype %s not supported (float32, bfloat16)" % dtype)
        self.dtype, self.n = dtype, sum(self.counts)
        ns = len(self.counts)
        need = self.L.gcow_seg_plan_bytes(ns, self.n)
        self.h = torch.zeros((need + 7) // 8, dtype=torch.int64)
        cnt = (C.c_uint64 * max(ns, 1))(*self.counts)
        used = C.c_size_t(0)
        check(self.L.gcow_seg_plan(cnt, ns, DTYPE_BF16 if dtype == torch.bfloat16 else DTYPE_FLOAT, self.h.data_ptr(),
                                   self.h.numel() * 8, C.byref(used)), "gcow_seg_plan")
        self.used = int(used.value)
        self.d = None
        if device is not None:
            self.to(device)

    def to(self, device):
        device = _device_of(device)
        if self.d is None or self.d.device != device:
            self.d = self.h.to(device)
        return self

    def stats(self):
        from ._ffi import SegStats
        s = SegStats()
        check(self.L.gcow_seg_plan_stats(self.h.data_ptr(), self.used, C.byref(s)), "gcow_seg_plan_stats")
        return s

    def segment(self, s: int):
        """-> (vb0, off, n) of tensor s (an empty tensor: those of the next non-empty one, n 0)."""
        a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        check(self.L.gcow_seg_plan_segment(self.h.data_ptr(), self.used, s, C.byref(a), C.byref(b), C.byref(c)),
              "gcow_seg_plan_segment")
        return a.value, b.value, c.value

    def tile(self, t: int):
        """-> (the tensor of tile t's first block, whether the tile is whole blocks of that tensor alone)."""
        a, u = C.c_uint64(0), C.c_int(0)
        check(self.L.gcow_seg_plan_tile(self.h.data_ptr(), self.used, t, C.byref(a), C.byref(u)), "gcow_seg_plan_tile")
        return a.value, bool(u.value)

    def max_output_bytes(self) -> int:
        return self.L.gcow_encode_seg_max_output_bytes(self.h.data_ptr(), self.used)

    def workspace_bytes(self) -> int:
        return self.L.gcow_encode_seg_workspace_bytes(self.h.data_ptr(), self.used)

    def index_entries(self, index_stride: int) -> int:
        return self.L.gcow_encode_seg_index_entries(self.h.data_ptr(), self.used, index_stride)


def _device_of(device) -> torch.device:
    """torch.device(device) with the current device's index for a bare "cuda" (tensors report theirs with one)."""
    device = torch.device(device or "cuda")
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def _seg_plan(plan, counts, dtype, device, what):
    if plan is None:
        return SegmentPlan(counts, dtype, device)
    if not isinstance(plan, SegmentPlan) or plan.counts != tuple(int(c) for c in counts) or plan.dtype != dtype:
        raise GcowError("%s: the plan was made for other counts or another dtype" % what)
    return plan.to(device)


class SegmentedEncoder:
    """Preallocated segmented encoder (gcow_encode_seg_device) for buffers of one shape: plan, stream, bit count, index
    and workspace. Calling it with x (contiguous 1-D device tensor of sum(counts) values) and the per-tensor minexp
    words on x's device (int32[S] packed words, or int64[S, 2] gcow_fit records) launches the encode and returns an
    Encoded whose `params` is None. The stream is the tensors' streams under expert(1, 16658, maxprec,
    clamp(minexp_s, -154, 133)) concatenated bit by bit, what a chain of S encode_append calls leaves; with
    index_stride, index[j] is the bit position of virtual block j * index_stride. Nothing is allocated or read back."""

    def __init__(self, counts, dtype, maxprec: int = 64, device=None, index_stride: int = 0,
                 plan: SegmentPlan | None = None):
        self.device = _device_of(device)
        self.plan = _seg_plan(plan, counts, dtype, self.device, "SegmentedEncoder")
        self.L = self.plan.L
        self.maxprec, self.index_stride = int(maxprec), int(index_stride)
        self.cap = self.plan.max_output_bytes()
        self.words = torch.zeros(max((self.cap + 7) // 8, 1), dtype=torch.int64, device=self.device)
        self.bits_dev = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.ws_bytes = self.plan.workspace_bytes()
        self.ws = torch.zeros(max(self.ws_bytes // 8, 1), dtype=torch.int64, device=self.device)
        ne = self.plan.index_entries(index_stride) if index_stride else 0
        self.index = torch.zeros(max(ne, 1), dtype=torch.int64, device=self.device) if index_stride else None

    def __call__(self, x: torch.Tensor, minexp: torch.Tensor, stream=None) -> Encoded:
        pl = self.plan
        if x.dim() != 1 or x.numel() != pl.n or x.dtype != pl.dtype:
            raise GcowError("segmented encoder built for %d values of %s, got %s %s" % (pl.n, pl.dtype, tuple(x.shape),
                                                                                       x.dtype))
        if not (x.is_cuda and x.is_contiguous() and x.device == self.device):
            raise GcowError("encode_segmented expects a contiguous 1-D tensor on the encoder's device")
        ns = len(pl.counts)
        ptr, stride = _fit_records(minexp, ns, x.device, "encode_segmented")
        check(self.L.gcow_encode_seg_device(pl.h.data_ptr(), pl.d.data_ptr(), pl.used, x.data_ptr() if pl.n else None,
                                            self.maxprec, ptr if ns else None, stride, self.words.data_ptr(),
                                            self.words.numel() * 8, self.bits_dev.data_ptr(), self.ws.data_ptr(),
                                            self.ws.numel() * 8,
                                            self.index.data_ptr() if self.index is not None else None,
                                            self.index_stride, _stream_ptr(stream)), "gcow_encode_seg_device")
        return Encoded(self.words, self.bits_dev, (pl.n,), None, self.index, self.index_stride)


def encode_segmented(x: torch.Tensor, counts, minexp: torch.Tensor, maxprec: int = 64, index_stride: int = 0,
                     stream=None, plan: SegmentPlan | None = None) -> Encoded:
    """One call of a new SegmentedEncoder (which see); plan: a SegmentPlan of these counts and x's dtype kept by the
    caller."""
    return SegmentedEncoder(counts, x.dtype, maxprec, x.device, index_stride, plan)(x, minexp, stream)


def decode_mean_segmented(streams: torch.Tensor, stream_words: int, nstreams: int, counts, minexp: torch.Tensor,
                          maxprec: int = 64, index: torch.Tensor | None = None, index_words: int = 0,
                          index_stride: int = 16, dtype=torch.float32, out: torch.Tensor | None = None, stream=None,
                          plan: SegmentPlan | None = None) -> torch.Tensor:
    """Mean of the decodes of nstreams segmented streams of one shape (gcow_decode_mean_seg_device): stream r at
    streams[r * stream_words:] (2 readable words after the last one), its index (stride 8 or 16, relative to its first
    word) at index[r * index_words:]. minexp on the streams' device: one set for all streams -- int32[S] or gcow_fit
    records int64[S, 2] -- or a set per stream, int32[W, S] or int64[W, S, 2]. Tensor s of `out` (default: new, of
    `dtype`; fp32 or bf16, contiguous, sum(counts) values) receives what decode_mean gives for its n_s values under its
    words, accumulated in fp32 in rank order; bf16 rounds to nearest even in the store. One launch."""
    counts = tuple(int(c) for c in counts)
    n, ns = sum(counts), len(counts)
    if out is None:
        out = torch.empty(n, dtype=dtype, device=streams.device)
    if not (out.is_cuda and out.is_contiguous() and out.numel() == n and out.dtype in (torch.float32, torch.bfloat16)):
        raise GcowError("decode_mean_segmented: out must be a contiguous fp32 / bf16 device tensor of %d values" % n)
    pl = plan.to(out.device) if plan is not None and plan.counts == counts else SegmentPlan(counts, out.dtype, out.device)
    if not (isinstance(minexp, torch.Tensor) and minexp.is_cuda and minexp.is_contiguous()
            and minexp.dtype in (torch.int32, torch.int64)):
        raise GcowError("decode_mean_segmented: minexp must be a contiguous int32 / int64 device tensor")
    per = 1 if minexp.dtype == torch.int32 else 4  # words per tensor
    have = minexp.numel() * (1 if minexp.dtype == torch.int32 else 2)
    if have == ns * per:
        sstride = 0
    elif have == nstreams * ns * per:
        sstride = ns * per
    else:
        raise GcowError("decode_mean_segmented: minexp must hold one set of %d tensors, or one per stream" % ns)
    check(pl.L.gcow_decode_mean_seg_device(pl.h.data_ptr(), pl.d.data_ptr(), pl.used, int(maxprec),
                                           minexp.data_ptr() if ns else None, per, sstride, streams.data_ptr(),
                                           streams.numel() * 8, stream_words, nstreams,
                                           index.data_ptr() if index is not None else None, index_words, index_stride,
                                           out.data_ptr() if n else None,
                                           DTYPE_BF16 if out.dtype == torch.bfloat16 else DTYPE_FLOAT,
                                           _stream_ptr(stream)), "gcow_decode_mean_seg_device")
    return out


class PerTensorFittedEncoder:
    """A bit budget per tensor on the wire, with no host read: calling it with a bucket x (contiguous 1-D device
    tensor) and the counts of its tensors launches the per-tensor rate tables over the bucket's views
    (TensorListFittedPerTensor.rate_tables), the batch fit of every table against floor(bits_per_value * n_s) bits over
    minexp >= minexp_floor, and the segmented encode under the fit records. -> (Encoded, fits): fits is the int64[S, 2]
    tensor of gcow_fit records (`minexp` is word 0: what a receiver needs to decode), and the stream is at most
    sum_s floor(bits_per_value * n_s) bits whenever every status is 0. Buffers are made at the first call for a shape
    (and a bucket address); later calls allocate nothing and synchronise nothing, so the chain captures into one graph
    that follows the data it is replayed on."""

    def __init__(self, bits_per_value: float, maxprec: int = 64, minexp_floor: int = MINEXP_FLOOR):
        self.bits_per_value, self.maxprec, self.minexp_floor = float(bits_per_value), int(maxprec), int(minexp_floor)
        self.lst = TensorListFittedPerTensor(bits_per_value, maxprec, minexp_floor)
        self.enc = None
        self._key = None

    @property
    def fits(self):
        return self.lst.fits

    def __call__(self, x: torch.Tensor, counts, index_stride: int = 0, stream=None):
        counts = tuple(int(c) for c in counts)
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 1 and x.is_contiguous()
                and x.numel() == sum(counts)):
            raise GcowError("PerTensorFittedEncoder expects a contiguous 1-D device tensor of sum(counts) values")
        if stream is None:
            stream = torch.cuda.current_stream(x.device)
        key = (counts, x.dtype, x.device, int(index_stride))
        if key != self._key:
            self.enc = SegmentedEncoder(counts, x.dtype, self.maxprec, x.device, index_stride)
            self._key = key
        views = list(torch.split(x, list(counts))) if counts else []
        lst = self.lst
        lst.rate_tables(views, stream)
        if counts:
            fit_device_batch(lst.tables, lst.budgets, self.minexp_floor, lst.fits, stream)
        fits = lst.fits if counts else torch.zeros((0, FIT_WORDS), dtype=torch.int64, device=x.device)
        return self.enc(x, fits, stream), fits


# ------------------------------------------------------- segmented fields with a residual: error feedback per tensor
def _check_seg_err(x: torch.Tensor, err, what: str, name: str = "err"):
    if not (isinstance(err, torch.Tensor) and err.is_cuda and err.device == x.device and err.dtype == torch.float32
            and err.dim() == 1 and err.numel() == x.numel() and err.is_contiguous()):
        raise GcowError("%s: %s must be a contiguous 1-D float32 tensor of x's size on x's device" % (what, name))


def _check_seg_x(x, pl: SegmentPlan, device, what: str):
    if not (isinstance(x, torch.Tensor) and x.dim() == 1 and x.numel() == pl.n and x.dtype == pl.dtype):
        raise GcowError("%s: built for %d values of %s" % (what, pl.n, pl.dtype))
    if not (x.is_cuda and x.is_contiguous() and x.device == device):
        raise GcowError("%s expects a contiguous 1-D tensor on the plan's device" % what)


class SegmentedRateTables:
    """Preallocated per-tensor rate tables of a segmented field with a carried error (gcow_rate_table_seg_device) for
    buffers of one shape: plan, tables (`tables`, int64[S, 288]) and workspace. Calling it with x and err (fp32, parallel
    to x; None: zeros) launches one pass over the plan's tiles: row s is rate_table_residual(t_s, e_s, maxprec), exactly
    (zeros for an empty tensor). Nothing is allocated or read back."""

    def __init__(self, counts, dtype, maxprec: int = 64, device=None, plan: SegmentPlan | None = None):
        self.device = _device_of(device)
        self.plan = _seg_plan(plan, counts, dtype, self.device, "SegmentedRateTables")
        self.L = self.plan.L
        self.maxprec = int(maxprec)
        ns = len(self.plan.counts)
        self.ws_bytes = self.L.gcow_rate_table_seg_workspace_bytes(self.plan.h.data_ptr(), self.plan.used)
        self.ws = torch.empty(max(self.ws_bytes // 8, 1), dtype=torch.int64, device=self.device)
        self.tables = torch.empty((ns, RATE_TABLE_ENTRIES), dtype=torch.int64, device=self.device)

    def __call__(self, x: torch.Tensor, err: torch.Tensor | None = None, stream=None) -> torch.Tensor:
        pl = self.plan
        _check_seg_x(x, pl, self.device, "rate_tables_segmented")
        if err is not None:
            _check_seg_err(x, err, "rate_tables_segmented")
        ns = len(pl.counts)
        check(self.L.gcow_rate_table_seg_device(pl.h.data_ptr(), pl.d.data_ptr(), pl.used,
                                                x.data_ptr() if pl.n else None,
                                                err.data_ptr() if err is not None and pl.n else None, self.maxprec,
                                                self.tables.data_ptr() if ns else None, self.ws.data_ptr(),
                                                self.ws.numel() * 8, _stream_ptr(stream)),
              "gcow_rate_table_seg_device")
        return self.tables


def rate_tables_segmented(x: torch.Tensor, counts, err: torch.Tensor | None = None, maxprec: int = 64,
                          plan: SegmentPlan | None = None, stream=None) -> torch.Tensor:
    """The rate table of y = x + err of every tensor of a segmented field from one pass (gcow_rate_table_seg_device):
    int64[S, 288] on x's device, row s the stream lengths of t_s + e_s under expert(1, 16658, maxprec, minexp),
    minexp = -154 .. 133, exactly -- what encode_segmented_residual spends on tensor s. err None: zeros, the tables of x
    (rate_tables_tensors' rows). One call of a new SegmentedRateTables; plan: a SegmentPlan kept by the caller."""
    return SegmentedRateTables(counts, x.dtype, maxprec, x.device, plan)(x, err, stream)


class SegmentedResidualEncoder(SegmentedEncoder):
    """SegmentedEncoder with error feedback (gcow_encode_seg_residual_device): calling it with x, err (fp32, parallel
    to x; None: zeros) and the per-tensor minexp words codes y = x + err -- the stream, bit count and index are
    encode_segmented's for the fp32 tensor y -- and writes e' = y - decode(y) (non-finite: +0) for every tensor under
    its own word: into err itself by default, into `err_out` when given (err_out is required with err None). x is only
    read. Nothing is allocated or read back."""

    def __call__(self, x: torch.Tensor, err: torch.Tensor | None, minexp: torch.Tensor,
                 err_out: torch.Tensor | None = None, stream=None) -> Encoded:
        pl = self.plan
        what = "encode_segmented_residual"
        _check_seg_x(x, pl, self.device, what)
        if err is not None:
            _check_seg_err(x, err, what)
        if err_out is None:
            err_out = err
        if err_out is None:
            raise GcowError("%s: err None (zeros) needs err_out" % what)
        _check_seg_err(x, err_out, what, "err_out")
        ns = len(pl.counts)
        ptr, stride = _fit_records(minexp, ns, x.device, what)
        check(self.L.gcow_encode_seg_residual_device(
            pl.h.data_ptr(), pl.d.data_ptr(), pl.used, x.data_ptr() if pl.n else None,
            err.data_ptr() if err is not None and pl.n else None, err_out.data_ptr() if pl.n else None, self.maxprec,
            ptr if ns else None, stride, self.words.data_ptr(), self.words.numel() * 8, self.bits_dev.data_ptr(),
            self.ws.data_ptr(), self.ws.numel() * 8, self.index.data_ptr() if self.index is not None else None,
            self.index_stride, _stream_ptr(stream)), "gcow_encode_seg_residual_device")
        return Encoded(self.words, self.bits_dev, (pl.n,), None, self.index, self.index_stride)


def encode_segmented_residual(x: torch.Tensor, err: torch.Tensor | None, counts, minexp: torch.Tensor,
                              maxprec: int = 64, index_stride: int = 0, err_out: torch.Tensor | None = None,
                              stream=None, plan: SegmentPlan | None = None) -> Encoded:
    """One call of a new SegmentedResidualEncoder (which see): err is updated in place unless err_out is given."""
    return SegmentedResidualEncoder(counts, x.dtype, maxprec, x.device, index_stride, plan)(x, err, minexp, err_out,
                                                                                            stream)


class PerTensorFittedResidualEncoder:
    """PerTensorFittedEncoder with error feedback: calling it with a bucket x, the carried error err (fp32, parallel to
    x, updated in place), the counts and an index stride launches the per-tensor rate tables of y = x + err
    (SegmentedRateTables), the batch fit of every table against floor(bits_per_value * n_s) bits over minexp >=
    minexp_floor, and the segmented residual encode under the fit records. -> (Encoded, fits) as PerTensorFittedEncoder.
    One SegmentPlan serves the tables and the encode. Buffers are made and the budgets uploaded at the first call for
    a shape; later calls allocate nothing and read nothing back, so the chain captures into one graph."""

    def __init__(self, bits_per_value: float, maxprec: int = 64, minexp_floor: int = MINEXP_FLOOR):
        self.bits_per_value, self.maxprec, self.minexp_floor = float(bits_per_value), int(maxprec), int(minexp_floor)
        self.enc = self.tab = self.fits = self.budgets = None
        self._key = None

    def __call__(self, x: torch.Tensor, err: torch.Tensor, counts, index_stride: int = 0, stream=None):
        counts = tuple(int(c) for c in counts)
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 1 and x.is_contiguous()
                and x.numel() == sum(counts)):
            raise GcowError("PerTensorFittedResidualEncoder expects a contiguous 1-D device tensor of sum(counts) values")
        key = (counts, x.dtype, x.device, int(index_stride))
        if key != self._key:
            self.enc = SegmentedResidualEncoder(counts, x.dtype, self.maxprec, x.device, index_stride)
            self.tab = SegmentedRateTables(counts, x.dtype, self.maxprec, x.device, self.enc.plan)
            ns = len(counts)
            self.fits = torch.zeros((ns, FIT_WORDS), dtype=torch.int64, device=x.device)
            self.budgets = torch.tensor([int(math.floor(self.bits_per_value * c)) for c in counts],
                                        dtype=torch.int64).to(x.device)
            self._key = key
        tables = self.tab(x, err, stream)
        if counts:
            fit_device_batch(tables, self.budgets, self.minexp_floor, self.fits, stream)
        return self.enc(x, err, self.fits, None, stream), self.fits


# ------------------------------------------------- segmented fields under a relative tolerance: words from one pass
REL_BITS_MAX = 24


def valid_rel_bits(rel_bits) -> bool:
    """Whether rel_bits is an integer (Python's or numpy's; neither bool nor an integral float) in 0..24: the one test
    of the codec entry points and of compressed_allgather_hook."""
    return (isinstance(rel_bits, numbers.Integral) and not isinstance(rel_bits, bool)
            and 0 <= rel_bits <= REL_BITS_MAX)


def _check_rel_bits(rel_bits, what: str) -> int:
    if not valid_rel_bits(rel_bits):
        raise GcowError("%s: rel_bits must be an integer in 0..%d, got %r" % (what, REL_BITS_MAX, rel_bits))
    return int(rel_bits)


def relative_minexp_segmented(x: torch.Tensor, counts, rel_bits: int, err: torch.Tensor | None = None,
                              absmax: torch.Tensor | None = None, out: torch.Tensor | None = None,
                              plan: SegmentPlan | None = None, stream=None) -> torch.Tensor:
    """The per-tensor minexp words of a relative tolerance over a segmented field, from one pass on the device
    (gcow_seg_rel_minexp_device): word s = max(emax_s - rel_bits, -94) (capped for a maximum in the top binade:
    include/gcow.h), emax_s the exponent of the largest finite |x + err| of tensor s -- the word
    roundtrip_tensors_relative codes tensor s under, and -94 for an empty tensor. x: the bucket, a contiguous 1-D fp32 /
    bf16 device tensor of sum(counts) values; err: fp32, parallel to x, or None for zeros (y = x + err is formed in
    registers, as encode_segmented_residual forms it). absmax: optional float32[S] device tensor that receives the
    maxima (it is the call's workspace; default: new). out: int32[S] (packed words, stride 1; default: new) or an
    int64[S, 2] array of gcow_fit records, of which only word 0 of each record is written. plan: a SegmentPlan of
    these counts and x's dtype kept by the caller; without one every call makes and uploads a new SegmentPlan (a host
    allocation and a copy), so only a call given plan, absmax and out allocates nothing and can be captured, as the
    encoders below call it. No host read; at most three launches. -> out."""
    what = "relative_minexp_segmented"
    rel_bits = _check_rel_bits(rel_bits, what)
    counts = tuple(int(c) for c in counts)
    if not (isinstance(x, torch.Tensor) and x.is_cuda):
        raise GcowError("%s expects a contiguous 1-D tensor on a device" % what)
    pl = _seg_plan(plan, counts, x.dtype, x.device, what)
    _check_seg_x(x, pl, x.device, what)
    if err is not None:
        _check_seg_err(x, err, what)
    ns = len(counts)
    if absmax is None:
        absmax = torch.empty(ns, dtype=torch.float32, device=x.device)
    elif not (isinstance(absmax, torch.Tensor) and absmax.is_cuda and absmax.device == x.device
              and absmax.dtype == torch.float32 and absmax.is_contiguous() and absmax.numel() == ns):
        raise GcowError("%s: absmax must be a contiguous float32 tensor of len(counts) values on x's device" % what)
    if out is None:
        out = torch.empty(ns, dtype=torch.int32, device=x.device)
    ptr, stride = _fit_records(out, ns, x.device, what)
    check(pl.L.gcow_seg_rel_minexp_device(pl.h.data_ptr(), pl.d.data_ptr(), pl.used, x.data_ptr() if pl.n else None,
                                          err.data_ptr() if err is not None and pl.n else None, rel_bits,
                                          absmax.data_ptr() if ns else None, ptr if ns else None, stride,
                                          _stream_ptr(stream)), "gcow_seg_rel_minexp_device")
    return out


class PerTensorRelativeEncoder:
    """A relative tolerance per tensor on the wire, with no host read: calling it with a bucket x (contiguous 1-D
    device tensor) and the counts of its tensors launches the words pass (relative_minexp_segmented) and the segmented
    encode under those words. -> (Encoded, words): words is the int32[S] tensor of per-tensor minexp, what a receiver
    needs to decode (4 bytes per tensor); `absmax` holds the last call's maxima. Buffers and plan are made at the first
    call for a shape; later calls allocate nothing and do nothing on the host between the launches, so the chain
    captures into one graph that follows the data it is replayed on."""

    residual = False

    def __init__(self, rel_bits: int, maxprec: int = 64):
        self.rel_bits, self.maxprec = _check_rel_bits(rel_bits, type(self).__name__), int(maxprec)
        self.enc = self.words = self.absmax = None
        self._key = None

    def _prepare(self, x, counts, index_stride):
        counts = tuple(int(c) for c in counts)
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 1 and x.is_contiguous()
                and x.numel() == sum(counts)):
            raise GcowError("%s expects a contiguous 1-D device tensor of sum(counts) values" % type(self).__name__)
        key = (counts, x.dtype, x.device, int(index_stride))
        if key != self._key:
            make = SegmentedResidualEncoder if self.residual else SegmentedEncoder
            self.enc = make(counts, x.dtype, self.maxprec, x.device, index_stride)
            self.words = torch.zeros(len(counts), dtype=torch.int32, device=x.device)
            self.absmax = torch.zeros(len(counts), dtype=torch.float32, device=x.device)
            self._key = key
        return counts

    def __call__(self, x: torch.Tensor, counts, index_stride: int = 0, stream=None):
        counts = self._prepare(x, counts, index_stride)
        relative_minexp_segmented(x, counts, self.rel_bits, None, self.absmax, self.words, self.enc.plan, stream)
        return self.enc(x, self.words, stream), self.words


class PerTensorRelativeResidualEncoder(PerTensorRelativeEncoder):
    """PerTensorRelativeEncoder with error feedback: calling it with a bucket x, the carried error err (fp32, parallel
    to x, updated in place), the counts and an index stride launches the words pass over y = x + err -- the maxima are
    of the values that are coded -- and the segmented residual encode under those words, which leaves each tensor's
    y - decode(y) in err. -> (Encoded, words) as PerTensorRelativeEncoder. One SegmentPlan serves both calls."""

    residual = True

    def __call__(self, x: torch.Tensor, err: torch.Tensor, counts, index_stride: int = 0, stream=None):
        counts = self._prepare(x, counts, index_stride)
        relative_minexp_segmented(x, counts, self.rel_bits, err, self.absmax, self.words, self.enc.plan, stream)
        return self.enc(x, err, self.words, None, stream), self.words


def stitch(dst: torch.Tensor, dst_bit_offset: int, src: torch.Tensor, src_bits: int, stream=None):
    """OR src_bits bits of src into dst at dst_bit_offset (device words; dst zeroed beyond earlier content)."""
    L = load()
    check(L.gcow_stitch_device(dst.data_ptr(), dst_bit_offset, src.data_ptr(), src_bits, _stream_ptr(stream)),
          "gcow_stitch_device")


def stitch_shards(dst: torch.Tensor, src: torch.Tensor, shard_words: int, lens: torch.Tensor, stream=None):
    """Concatenate len(lens) shard streams (lens: int64 device tensor of bit counts; shard r at src[r * shard_words:])
    bit-exactly into dst (every word of dst is written; one launch, no host sync)."""
    n = lens.numel()
    if src.numel() < n * shard_words:
        raise GcowError("stitch_shards: src holds %d words, %d shards of %d expected" % (src.numel(), n, shard_words))
    check(load().gcow_stitch_shards_device(dst.data_ptr(), dst.numel(), src.data_ptr(), shard_words, lens.data_ptr(),
                                           n, _stream_ptr(stream)), "gcow_stitch_shards_device")
    return dst


def decode_mean(streams: torch.Tensor, stream_words: int, nstreams: int, n: int, params: GcowParams,
                index: torch.Tensor | None = None, index_words: int = 0, index_stride: int = 0,
                out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """Mean of the decodes of nstreams 1-D streams of n values (stream r at streams[r * stream_words:], 2 readable
    words after the last one), accumulated in rank order in fp32 (gcow_decode_mean_device): one launch."""
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=streams.device)
    f = field_of(out)
    check(load().gcow_decode_mean_device(C.byref(f), C.byref(params), streams.data_ptr(), streams.numel() * 8,
                                         stream_words, nstreams,
                                         index.data_ptr() if index is not None else None, index_words, index_stride,
                                         _stream_ptr(stream)), "gcow_decode_mean_device")
    return out


MEANENC_COMPOSED, MEANENC_FUSED_FIXED = 0, 1  # gcow_decode_mean_encode_path


class ReduceEncoder:
    """Preallocated decode + mean + encode (gcow_decode_mean_encode_device) for `nstreams` received streams of one 1-D
    shard of n values under `params_in`: calling it codes their fp32 mean (decode_mean's values) under `params_out`
    (default: params_in) without the mean travelling through memory where the call runs fused. `path`
    (gcow_decode_mean_encode_path, for 16-byte aligned buffers): MEANENC_FUSED_FIXED when both sets are the same rate 8
    / 16 set and no index goes in or out (one kernel, no workspace), else MEANENC_COMPOSED (decode_mean into an fp32
    temporary in the workspace, then the encoder on it). residual=True: calls take `err` (fp32, n values, updated in
    place): y = mean + err is coded and err = finite(y - decode(stream)), as ResidualEncoder does for a bucket. The
    stream, bit count, output index and workspace are allocated once."""

    def __init__(self, n: int, params_in: GcowParams, nstreams: int, params_out: GcowParams | None = None, device=None,
                 residual: bool = False, index_stride_out: int = 0):
        self.L = load()
        self.n, self.nstreams = int(n), int(nstreams)
        self.params_in = params_in
        self.params = params_out if params_out is not None else params_in
        self.device = torch.device(device or "cuda")
        self.residual = bool(residual)
        self.shape = (self.n,)
        f = field_of_shape(self.shape, torch.float32)
        pi, po = C.byref(self.params_in), C.byref(self.params)
        self.cap = self.L.gcow_max_output_bytes(C.byref(f), po) if self.n else 8
        if self.cap == 0:
            raise GcowError("unsupported shard of %d values" % self.n)
        self.words = torch.zeros((self.cap + 7) // 8, dtype=torch.int64, device=self.device)
        self.bits_dev = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.fixed = is_fixed(self.params)
        if self.fixed:  # fixed rate: the bit count is known on the host; no device write per call
            self.bits_dev.fill_((self.n + 3) // 4 * self.params.maxbits)
        self.index_stride = index_stride_out
        ne = self.L.gcow_index_entries(C.byref(f), index_stride_out) if index_stride_out and self.n else 0
        self.index = torch.zeros(max(ne, 1), dtype=torch.int64, device=self.device) if index_stride_out else None
        # the path for aligned buffers: pointers are looked at for presence only (1 = "an index is given")
        self.path = self.L.gcow_decode_mean_encode_path(C.byref(f), pi, po, None, None,
                                                        None if is_fixed(params_in) else 1,
                                                        1 if index_stride_out else None) if self.n else MEANENC_COMPOSED
        ws = self.L.gcow_decode_mean_encode_workspace_bytes(C.byref(f), pi, po)
        if self.n and self.path == MEANENC_COMPOSED and ws == 0:
            # the query decides from the parameter sets alone; an output index sends a rate 8 / 16 call to the
            # composed path: the mean, then the larger of the two inner calls' workspaces
            a256 = lambda v: (v + 255) // 256 * 256
            ws = a256(4 * self.n) + max(a256(self.L.gcow_encode_workspace_bytes(C.byref(f), po)),
                                        self.L.gcow_encode_residual_workspace_bytes(C.byref(f), po))
        self.ws_bytes = ws
        self.ws = torch.zeros(max(ws // 8, 1), dtype=torch.int64, device=self.device)

    def __call__(self, streams: torch.Tensor, stream_words: int, index: torch.Tensor | None = None,
                 index_words: int = 0, index_stride: int = 0, err: torch.Tensor | None = None,
                 stream=None) -> Encoded:
        if not (streams.is_cuda and streams.dtype == torch.int64 and streams.is_contiguous()):
            raise GcowError("ReduceEncoder expects a contiguous int64 device tensor of stream words")
        if self.residual != (err is not None):
            raise GcowError("ReduceEncoder(residual=%s) called %s err" % (self.residual,
                                                                         "with" if err is not None else "without"))
        if err is not None and not (err.is_cuda and err.device == streams.device and err.dtype == torch.float32
                                    and err.is_contiguous() and err.numel() == self.n):
            raise GcowError("ReduceEncoder: err must be a contiguous fp32 tensor of n values on the streams' device")
        f = field_of_shape(self.shape, torch.float32)
        ep = err.data_ptr() if err is not None and self.n else None
        st = self.L.gcow_decode_mean_encode_device(
            C.byref(f), C.byref(self.params_in), streams.data_ptr(), streams.numel() * 8, stream_words, self.nstreams,
            index.data_ptr() if index is not None else None, index_words, index_stride,
            C.byref(self.params), ep, ep, self.words.data_ptr(), self.cap,
            None if self.fixed else self.bits_dev.data_ptr(), self.ws.data_ptr(), self.ws_bytes,
            self.index.data_ptr() if self.index is not None else None, self.index_stride, _stream_ptr(stream))
        check(st, "gcow_decode_mean_encode_device")
        return Encoded(self.words, self.bits_dev, self.shape, self.params, self.index, self.index_stride)


def decode_mean_encode(streams: torch.Tensor, stream_words: int, nstreams: int, n: int, params: GcowParams,
                       index: torch.Tensor | None = None, index_words: int = 0, index_stride: int = 0,
                       out_params: GcowParams | None = None, err: torch.Tensor | None = None,
                       out_index_stride: int = 0, stream=None) -> Encoded:
    """One-shot ReduceEncoder: the stream `encode` gives for decode_mean(streams, ...) under out_params (default:
    params); with `err`, the stream of mean + err, and err updated in place as encode_residual does."""
    enc = ReduceEncoder(n, params, nstreams, out_params, streams.device, err is not None, out_index_stride)
    return enc(streams, stream_words, index, index_words, index_stride, err, stream)


def pack_index16(index8: torch.Tensor, n: int, params: GcowParams, out: torch.Tensor | None = None,
                 stream=None) -> torch.Tensor:
    """The packed 16-block index (gcow_index_pack16_device) of one stream of n values from its index every 8 blocks:
    ceil(n / 64) int64 entries, low 48 bits block 16 c's bit position, high 16 bits block 16 c + 8's offset from it.
    decode_mean(..., index_stride=INDEX_PACKED16) reads it as 8-block chunks."""
    n16 = (n + 63) // 64
    if out is None:
        out = torch.empty(max(n16, 1), dtype=torch.int64, device=index8.device)
    if out.numel() < n16 or index8.numel() < (n + 31) // 32 or not (index8.is_cuda and out.is_cuda):
        raise GcowError("pack_index16: device index of ceil(n / 32) entries and an output of ceil(n / 64)")
    f = field_of_shape((n,), torch.float32)
    check(load().gcow_index_pack16_device(C.byref(f), C.byref(params), index8.data_ptr(), out.data_ptr(),
                                          _stream_ptr(stream)), "gcow_index_pack16_device")
    return out[:n16] if n16 else out[:0]


def fill_normal(out: torch.Tensor, sigma: float = 1e-3, seed: int = 0x67636F77, inject: bool = True, stream=None):
    """Deterministic synthetic gradient bucket on the device (SURVEY 8(d) distribution)."""
    assert out.dtype == torch.float32 and out.is_cuda and out.is_contiguous()
    check(load().gcow_fill_normal_device(out.data_ptr(), out.numel(), sigma, seed, int(inject),
                                         _stream_ptr(stream)), "gcow_fill_normal_device")
    return out


def copy_pattern(x: torch.Tensor, out: torch.Tensor, bits_per_block: int = 64, stream=None):
    """The fixed-rate 1-D encoder's memory access pattern without coding (gcow_copy_pattern_device): the HBM floor
    of that kernel, for bench.py's roofline.copy_ceiling."""
    dt = DTYPE_BF16 if x.dtype == torch.bfloat16 else DTYPE_FLOAT
    if not (x.is_cuda and x.is_contiguous()) or out.numel() * out.element_size() * 8 < x.numel() // 4 * bits_per_block:
        raise GcowError("copy_pattern: contiguous device input and an output of nblocks * bits_per_block bits")
    check(load().gcow_copy_pattern_device(x.data_ptr(), dt, x.numel(), bits_per_block, out.data_ptr(),
                                          _stream_ptr(stream)), "gcow_copy_pattern_device")
    return out


def c3_field(device=None, side: int = 512, seed: int = 21) -> torch.Tensor:
    """SURVEY 8(d) C3 volume on the device: f = sin(6 pi x) cos(4 pi y) sin(2 pi z) + 1e-3 N(0, 1) on the [0, 1)^3
    grid (z slowest), the noise from fill_normal. The bench times this field and the full-size parity test checks the
    same one (copied to the host) against the oracle."""
    import math as _m
    dev = torch.device(device or "cuda")
    g = torch.arange(side, device=dev, dtype=torch.float64) / side
    sx = torch.sin(6 * _m.pi * g).float()
    cy = torch.cos(4 * _m.pi * g).float()
    sz = torch.sin(2 * _m.pi * g).float()
    f = torch.empty(side ** 3, dtype=torch.float32, device=dev)
    fill_normal(f, 1.0, seed=seed, inject=False)
    f = f.view(side, side, side).mul_(1e-3)
    f += sx[None, None, :] * cy[None, :, None] * sz[:, None, None]
    return f.contiguous()


VAR1D_FORMS = {"tile": 0, "range": 1, "single_pass": 2}


@contextlib.contextmanager
def var1d_variant(form: str = "tile", spin: int = -1, stats: bool = False):
    """TEST / MEASUREMENT ONLY: run the 1-D variable-rate encoder in one of its measured-and-not-kept forms inside the
    `with` block (gcow_debug_set_var1d_variant; process-wide, restored to the default tile form on exit)."""
    L = load()
    check(L.gcow_debug_set_var1d_variant(VAR1D_FORMS[form], int(spin), int(bool(stats))),
          "gcow_debug_set_var1d_variant")
    try:
        yield
    finally:
        check(L.gcow_debug_set_var1d_variant(0, -1, 0), "gcow_debug_set_var1d_variant")


# ------------------------------------------------------------------------------------------- zfpy byte streams
def write_header(shape, params: GcowParams, dtype=torch.float32):
    """(header words [3 x uint64 as python ints], header bits) of zfp_write_header(ZFP_HEADER_FULL)."""
    f = field_of_shape(shape, dtype)
    w = (C.c_uint64 * 3)()
    bits = load().gcow_write_header(C.byref(f), C.byref(params), w)
    if not bits:
        raise GcowError("shape %s has no zfp header form" % (tuple(shape),))
    return [int(x) for x in w], int(bits)


def read_header(words):
    """Parse a zfp 0.5.5 header from the first words (host ints, numpy or a tensor) -> (shape, params, bits)."""
    if isinstance(words, torch.Tensor):
        words = words[:3].cpu().tolist()
    w = [int(x) & 0xFFFFFFFFFFFFFFFF for x in list(words)[:3]]
    w += [0] * (3 - len(w))
    arr = (C.c_uint64 * 3)(*w)
    f, p = ZfpInput(), GcowParams()
    bits = load().gcow_read_header(arr, 3, C.byref(f), C.byref(p))
    if not bits:
        raise GcowError("not a zfp 0.5.5 float stream (bad magic, version or type)")
    shape = tuple(n for n in (f.nw, f.nz, f.ny, f.nx) if n)
    return shape, p, int(bits)


def compress_numpy(x: torch.Tensor, tolerance: float = -1, rate: float = -1, precision: int = -1,
                   stream=None) -> torch.Tensor:
    """zfpy.compress_numpy for a device tensor: header + stream, byte-identical to zfpy/libzfp 0.5.5 (returned as an
    int64 device tensor of ceil(bits/64) words). Same keyword semantics as zfpy: exactly one of tolerance / rate /
    precision >= 0 selects the mode."""
    if tolerance >= 0:
        p = accuracy(tolerance)
    elif rate >= 0:
        p = globals()["rate"](rate, x.dim())
    elif precision >= 0:
        p = globals()["precision"](precision)
    else:
        p = expert(ZFP_MIN_BITS, ZFP_MAX_BITS - 1, ZFP_MAX_PREC, ZFP_MIN_EXP)  # zfpy default: lossless-ish expert
    return compress_zfp(x, p, stream)


def compress_zfp(x: torch.Tensor, params: GcowParams, stream=None) -> torch.Tensor:
    if not x.is_cuda:
        raise GcowError("compress_zfp expects a device tensor")
    L = load()
    f = field_of(x)
    cap = L.gcow_max_output_bytes(C.byref(f), C.byref(params)) + 24
    ws_bytes = L.gcow_encode_zfp_workspace_bytes(C.byref(f), C.byref(params))
    out = torch.zeros((cap + 7) // 8, dtype=torch.int64, device=x.device)
    ws = torch.zeros((ws_bytes + 7) // 8, dtype=torch.int64, device=x.device)
    bits = torch.zeros(1, dtype=torch.int64, device=x.device)
    check(L.gcow_encode_device_zfp(C.byref(f), C.byref(params), out.data_ptr(), cap, bits.data_ptr(), ws.data_ptr(),
                                   ws_bytes, _stream_ptr(stream)), "gcow_encode_device_zfp")
    return out[: (int(bits.item()) + 63) // 64]


def decompress_numpy(words: torch.Tensor, out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """zfpy.decompress_numpy for a device stream with a zfp header: shape and mode come from the header."""
    shape, p, hb = read_header(words)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=words.device)
    elif tuple(out.shape) != shape:
        raise GcowError("output shape %s does not match the header's %s" % (tuple(out.shape), shape))
    w = torch.cat([words.reshape(-1), torch.zeros(2, dtype=torch.int64, device=words.device)])
    f = field_of(out)
    check(load().gcow_decode_device_at(C.byref(f), C.byref(p), w.data_ptr(), w.numel() * 8, hb, None, 0,
                                       _stream_ptr(stream)), "gcow_decode_device_at")
    return out


# ------------------------------------------------------------------------------------------- chunked / host paths
def encode_append(x: torch.Tensor, params: GcowParams, words: torch.Tensor, d_base: torch.Tensor,
                  d_total: torch.Tensor, ws: torch.Tensor | None = None, index: torch.Tensor | None = None,
                  index_stride: int = 0, stream=None):
    """Append a variable-rate encode of device tensor x to the stream in `words` whose first d_base[0] bits are
    already written (gcow_encode_device_append); d_total[0] receives the new end. d_base / d_total are int64 device
    tensors (one element each); chunks appended this way equal one encode of their concatenation."""
    L = load()
    f = field_of(x)
    need = L.gcow_encode_workspace_bytes(C.byref(f), C.byref(params))
    if ws is None or ws.numel() * 8 < need:
        ws = torch.empty(max(need // 8, 1), dtype=torch.int64, device=x.device)
    st = L.gcow_encode_device_append(C.byref(f), C.byref(params), words.data_ptr(), words.numel() * 8,
                                     d_base.data_ptr(), d_total.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                     index.data_ptr() if index is not None else None, index_stride,
                                     _stream_ptr(stream))
    check(st, "gcow_encode_device_append")
    return ws


class HostEncoder:
    """Encode a 1-D bucket that starts and ends in pinned host memory (the gradient bucket headed for the NIC,
    BASELINE config 5), with the PCIe copies overlapped: the bucket is cut into `chunks` block-aligned chunks and
    chunk i+1's H2D copy, chunk i's encode and chunk i-1's D2H copy run on three streams at once. Variable rate
    appends each chunk at the device-side end of the previous one (gcow_encode_device_append); fixed rate writes
    chunk i at its known word offset. Only whole 64-bit words that no later chunk touches are copied back early.
    The result is byte-identical to one device encode of the whole bucket."""

    def __init__(self, n: int, dtype, params: GcowParams, chunks: int = 8, device=None):
        self.n, self.dtype, self.params = int(n), dtype, params
        self.device = torch.device(device or "cuda")
        self.fixed = is_fixed(params)
        nb = (self.n + 3) // 4
        # chunks of a multiple of 16 blocks; fixed rate also needs every chunk to start on a 64-bit stream word
        # (written at a byte offset as its own stream): blocks * maxbits % 64 == 0
        align = 16
        if self.fixed:
            g = 64 // math.gcd(int(params.maxbits), 64)
            align = align * g // math.gcd(align, g)
        per = max(align, ((nb + chunks - 1) // chunks + align - 1) // align * align)
        self.bounds = []
        b = 0
        while b < nb:
            e = min(b + per, nb)
            self.bounds.append((4 * b, min(4 * e, self.n)))
            b = e
        self.L = load()
        self.cap = max_output_bytes((self.n,), params, dtype)
        self.words = torch.zeros((self.cap + 7) // 8 + 2, dtype=torch.int64, device=self.device)
        self.bufs = [torch.empty(4 * per, dtype=dtype, device=self.device) for _ in range(2)]
        f = field_of_shape((4 * per,), dtype)
        need = self.L.gcow_encode_workspace_bytes(C.byref(f), C.byref(params))
        self.ws = torch.empty(max(need // 8, 1), dtype=torch.int64, device=self.device)
        k = len(self.bounds)
        self.d_bits = torch.zeros(k + 1, dtype=torch.int64, device=self.device)
        self.h_bits = torch.zeros(k + 1, dtype=torch.int64).pin_memory()
        self.s_h2d, self.s_enc, self.s_d2h = (torch.cuda.Stream(self.device) for _ in range(3))

    def __call__(self, h_in: torch.Tensor, h_out: torch.Tensor) -> int:
        """h_in: pinned host 1-D tensor (n values); h_out: pinned host int64 tensor with room for the stream.
        Returns the stream's bit count; h_out[:ceil(bits / 64)] holds the flushed stream."""
        if h_in.numel() != self.n or h_in.dtype != self.dtype or h_in.is_cuda:
            raise GcowError("HostEncoder built for %d %s host values" % (self.n, self.dtype))
        p = self.params
        k = len(self.bounds)
        ev_h2d = [torch.cuda.Event() for _ in range(k)]
        ev_enc = [torch.cuda.Event() for _ in range(k)]
        done = 0  # words already copied back

        def copy_back(end_word, after):
            nonlocal done
            if end_word > done:
                self.s_d2h.wait_event(after)
                with torch.cuda.stream(self.s_d2h):
                    h_out[done:end_word].copy_(self.words[done:end_word], non_blocking=True)
                done = end_word

        for i, (lo, hi) in enumerate(self.bounds):
            buf = self.bufs[i % 2]
            if i >= 2:
                self.s_h2d.wait_event(ev_enc[i - 2])  # the buffer's previous chunk is encoded
            with torch.cuda.stream(self.s_h2d):
                buf[: hi - lo].copy_(h_in[lo:hi], non_blocking=True)
                ev_h2d[i].record(self.s_h2d)
            self.s_enc.wait_event(ev_h2d[i])
            x = buf[: hi - lo]
            if self.fixed:
                f = field_of(x)
                off = (lo // 4) * p.maxbits // 8
                check(self.L.gcow_encode_device(C.byref(f), C.byref(p), self.words.data_ptr() + off,
                                                self.cap - off, None, None, 0, None, 0,
                                                _stream_ptr(self.s_enc)), "gcow_encode_device")
            else:
                encode_append(x, p, self.words, self.d_bits[i:i + 1], self.d_bits[i + 1:i + 2], self.ws,
                              stream=self.s_enc)
                with torch.cuda.stream(self.s_enc):
                    self.h_bits[i + 1:i + 2].copy_(self.d_bits[i + 1:i + 2], non_blocking=True)
            ev_enc[i].record(self.s_enc)
            if i >= 1:  # chunk i-1's complete words (chunk i only ORs into the word its first bit falls in)
                if self.fixed:
                    end = (self.bounds[i - 1][1] + 3) // 4 * p.maxbits
                else:
                    ev_enc[i - 1].synchronize()
                    end = int(self.h_bits[i])
                copy_back(end // 64, ev_enc[i - 1])
        if self.fixed:
            bits = ((self.n + 3) // 4) * p.maxbits
        else:
            ev_enc[k - 1].synchronize()
            bits = int(self.h_bits[k])
        copy_back((bits + 63) // 64, ev_enc[k - 1])
        self.s_d2h.synchronize()
        return bits
