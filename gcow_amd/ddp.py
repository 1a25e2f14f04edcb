"""torch DDP communication hooks over the gcow codec.

The reference caller (hw/models/train_imagenet.py:446-475, train_resnet_cifar10.py:74-125) all-reduces fp32
gradients with DDP, then copies the flattened gradient vector to the host, runs zfpy compress -> decompress on it
and copies it back (:453, :459-465, :471): the wire carries fp32 and the codec only simulates the loss, with two
PCIe copies per step. Two device-resident replacements:

* `roundtrip_hook` -- the reference's exact semantics (mean all-reduce, then encode -> decode of the reduced
  bucket), on the GPU: no `.cpu()`, no `torch.from_numpy(...).to(device)`.
* `compressed_allgather_hook` -- gradients compressed *before* the wire: each rank encodes its bucket, the
  compressed streams are all-gathered over RCCL, and one launch decodes every rank's stream and averages them
  (gcow_decode_mean_device: acc = 0 + x_0 + x_1 + ... in rank order, then / world). At rate r the wire carries r/32
  of the fp32 bytes per rank.

All register with `ddp_model.register_comm_hook(make_hook_state(hook=hook, ...), hook)` (variable rate and the sharded
hook: the state's exchange group is created by `GcowHookState.setup()`, a collective every rank calls at the same
point). `GcowHookState.codec` defaults to the
device codec (gcow_amd.dist.DeviceCodec); tests inject an oracle-backed codec to run the hook bodies over gloo.

Error feedback (`GcowHookState.error_feedback`, both wire hooks): what the codec truncates from a rank's bucket is
kept on that rank and added to its next step's bucket before encoding, so the sent gradients average over steps to
the meant ones (codec.encode_residual: one fused kernel at rate 8 / 16, and the variable-rate encoder writing the
residual from its own coefficients for accuracy / precision sets, which have no bit budget).

Accuracy mode under a bit budget (`GcowHookState.target_bits`, all three hooks): the tolerance is fitted to a budget
in bits per value from the bucket's rate table (codec.rate_table: the stream length under every minexp from one pass);
roundtrip_hook bounds the budget, the wire hooks track it with a control lagged by one step -- or, with
`GcowHookState.fit_on_device`, compressed_allgather_hook fits the very step it encodes: table, fit and encode run on
the device back to back (codec.fit_device, codec.encode_fitted_device), and the step's streams meet the budget -- with
error feedback too: the table is then of bucket + carried error (codec.rate_table_residual) and the encode is
codec.encode_residual_fitted_device, so the bound holds for what is sent.
"""
import contextlib
import queue
import threading
from dataclasses import dataclass, field
from datetime import timedelta

import torch
import torch.distributed as dist

from . import codec as _codec
from . import dist as gdist
from ._ffi import GcowParams

INDEX_STRIDE = 16  # block index spacing of the round-trip hook's decode (one entry per 16 blocks)
# The sharded hook's index spacing: 8 blocks. decode_mean then runs one lane per 8 blocks (32 fp32 sums per lane, no
# register spills, 5 waves per SIMD): a rank's shard decodes in 0.50 instead of 0.66 ms at W = 8 (accuracy 1e-6,
# 256 Mi values; profiles/r05_dmean_stride8_ab.log) for an index of 1 byte per block instead of 0.5 -- ~6 % more bytes
# in the all-to-all. The all-gather hook gathers every rank's whole index, so it encodes with the same 8-block index
# and sends it packed (codec.pack_index16: the 16-block index's size, the 8-block midpoint as a 16-bit offset), and
# decode_mean reads the packed entries as 8-block chunks.
SHARDED_INDEX_STRIDE = 8


@dataclass
class GcowHookState:
    """Hook state, one per DDP model. `timeout_s` bounds every collective of the variable-rate exchange, which runs
    over a process group of its own. That group is created by `setup()` -- a collective: call it on every rank of
    `process_group`, at the same point of each rank's setup, after init_process_group and before the first backward
    (or build the state with `make_hook_state`, which does). Constructing, copying or `dataclasses.replace`-ing a
    state issues no collective.

    Failure: a rank whose exchange raises stops its comm thread (that bucket's future and every later one fail at
    once) and aborts the exchange group. Over gloo that closes the connections and peers blocked in an exchange
    collective error out at once; over RCCL/NCCL a peer already blocked in a collective only fails when `timeout_s`
    expires (the communicator's watchdog then tears the process group -- and by default the process -- down).

    `error_feedback` (compressed_allgather_hook, compressed_sharded_hook): each rank keeps e = y - decode(encode(y))
    of what it sent (y = its gradient bucket + the e of the step before) and encodes with codec.encode_residual. The
    state holds one fp32 buffer per bucket, zero-initialised, keyed by the bucket's index and numel: a bucket whose
    size changed (DDP rebuilds its buckets after the first iteration) drops the old buffer and starts from zeros
    again. Buckets of equal size that the rebuild permutes are not told apart -- one step's error of the other bucket
    is then added once; `reset_error_feedback()` after the first iteration avoids it. roundtrip_hook raises ValueError
    with the flag set: its loss is applied after the reduction, identically on every rank. Unset (the default):
    nothing changes and encode_residual is never called.

    `compress_mean` (compressed_sharded_hook only; the other two hooks raise ValueError with it set): the second stage
    of the sharded exchange -- the all-gather of the mean shards -- carries streams instead of values. The owner of a
    shard turns its W received pieces straight into the stream of their mean (codec.ReduceEncoder: one kernel at rate
    8 / 16) under `mean_params` (None: `params`), the streams are all-gathered and every rank decodes every shard, the
    owner its own too, so that all ranks hold decode(encode(mean)) bit for bit. With `error_feedback` the owner also
    keeps a second carried error, of its mean shard (keyed by bucket index, "mean" and the shard's numel; cleared by
    reset_error_feedback()). Per rank, n fp32 values at rate 16 then cost 7/8 (2n + 2n) bytes instead of
    7/8 (2n + 4n) at W = 8. The mean is coded from its fp32 values whatever the bucket's dtype: for a bf16 bucket the
    second stage saves bytes only below 16 bits per value. Unset (the default): nothing changes.

    `relative_bits` (roundtrip_hook and compressed_allgather_hook; compressed_sharded_hook raises ValueError with it
    set: its pieces carry no per-tensor exponents): roundtrip_hook -- after the mean all-reduce every parameter's
    gradient in the bucket (bucket.gradients(), views of the buffer) is round-tripped in place as a field of its own,
    in accuracy mode under a tolerance of 2^-relative_bits relative to that gradient's largest magnitude
    (codec.roundtrip_tensors_relative, through the codec's roundtrip_relative, cached per bucket).
    compressed_allgather_hook (_allgather_relative) -- each rank takes its own gradients' maxima in one pass on the
    device, sends one segmented stream coded under the resulting minexp word per gradient and its S int32 words,
    4 bytes per tensor, and every rank decodes and averages the W streams under the W word sets in one launch
    (the codec's encode_relative / decode_mean_per_tensor). Nothing is read on the host but the gathered lengths. The
    bucket's gradients must tile its flat buffer in order. With `error_feedback` the maxima are those of bucket +
    carried error, the values that are coded, and the segmented residual encode leaves each tensor's y - decode(y)
    under its own word in error_buffer(index, ...) (the codec's encode_residual_relative). ValueError, before any
    codec call or collective: with `compress_mean`, `target_bits` or `per_tensor_budget` (both choose the tolerance);
    a value outside 0..24 (bool and float are no integers here: codec.valid_rel_bits); a codec without those methods;
    no initialised process group. In both hooks `params` contributes only its maxprec -- a fixed-rate set, the default
    included, serves as well as a variable-rate one: the exchange is the variable-rate one either way, so setup()
    creates the exchange group whenever the field is set -- and the bucket must be fp32 or bf16. Unset (the default):
    nothing changes.

    `target_bits` (all three hooks): accuracy mode under a bit budget of target_bits bits per value. `params` must be
    a variable-rate set without a block budget (accuracy, precision, expert with minbits <= 1 and maxbits >= 160),
    else ValueError; it supplies maxprec and the first step's minexp. Combined with `relative_bits`: ValueError. The
    tolerance comes from the bucket's rate table (codec.rate_table: the stream length under every minexp from one
    pass) and codec.fit_minexp: the finest minexp whose stream fits.
    roundtrip_hook fits the reduced bucket itself, in the `then` callback (the 2.3 KB host read happens there, off the
    autograd thread), and round-trips it under the fitted set: the bucket is the same on every rank, so is the fit,
    and the simulated stream is never longer than floor(target_bits * n) bits.
    The wire hooks must encode on the autograd thread before the exchange, so their control lags one step: beside the
    encode the hook launches the rate table of the bucket; inside the exchange the table is all-reduced (sum) over the
    exchange group and fitted against world * floor(target_bits * n) bits, and the resulting minexp is kept on the
    state per bucket (keyed like the error buffers, by bucket index and numel) for that bucket's encode and decode in
    the NEXT step. Every rank holds the same summed table and applies the same rule, so every rank uses the same set
    in every step; DDP waits for all bucket futures before the next backward, so the value is in place when the next
    step's hook reads it. The wire hooks therefore TRACK the budget, they do not bound it: a step's streams are fitted
    to the step before, the budget is met by the ranks' total and not by each rank, and with `error_feedback` the
    table is taken of the bucket, not of bucket + carried error. (codec.encode_fitted and roundtrip_hook do bound
    it.) A budget below one bit per block selects the coarsest entry. `mean_params` of `compress_mean` is not fitted.
    `reset_error_feedback()` keeps the fitted values; `reset_rate_fit()` forgets them (the next step uses `params`).
    Unset (the default): nothing changes and rate_table is never called.

    `fit_on_device` (roundtrip_hook and compressed_allgather_hook, only together with `target_bits`; ValueError
    without it): the fit is a kernel (codec.fit_device) and the encode or round trip takes minexp from the 16-byte
    record it writes (codec.encode_fitted_device / roundtrip_fitted), so nothing is read on the host between the table
    pass and the coder. roundtrip_hook: the `then` callback launches table -> fit -> round trip in place and returns;
    no `.cpu()`, `_fits` is not updated, `fit_record(index)` is the device record. compressed_allgather_hook: the
    encode moves from the autograd thread into the exchange, on the side stream: this step's table, its all-reduce
    over the exchange group (world > 1), the fit against world * floor(target_bits * n) bits, the encode under that
    fit and the index packing; the record is read on the host right after the gathered lengths, where the comm thread
    has just waited anyway, and the decode runs under fitted_params(maxprec, minexp). Every rank fits the same summed
    table, so every rank codes under the same set, and the W streams of THIS step total at most
    world * floor(target_bits * n) bits -- the budget is bounded, not tracked, and step 1 is fitted like every other.
    A budget below one bit per block cannot be met: the record's status is 1 and the coarsest set (minexp 133) is
    used, as the lagged control does. The price is latency: table, all-reduce (2.3 KB) and fit now run before the
    encode instead of beside it, and the encode no longer overlaps the autograd thread's work.
    compressed_allgather_hook with `error_feedback` as well: the table is taken of y = bucket + carried error
    (codec.rate_table_residual, y formed in registers), summed and fitted as above, and y is encoded under the record
    by codec.encode_residual_fitted_device, which updates the carried error in place; the error buffer is obtained on
    the autograd thread, everything else runs inside the exchange. The W streams of this step total at most
    world * floor(target_bits * n) bits, and that holds for what is actually sent, y -- where the lagged control fits
    the bucket alone. The codec must also have rate_table_residual and encode_residual_fitted, else ValueError.
    Combined with `compress_mean`, registered with compressed_sharded_hook, or roundtrip_hook with `error_feedback`:
    ValueError -- those encodes are other kernel families. A codec without rate_table,
    fit_device, encode_fitted and roundtrip_fitted: ValueError. Unset (the default): nothing changes.

    `per_tensor_budget` (roundtrip_hook only, and only together with `target_bits`): the budget is per gradient, not
    per bucket. After the mean all-reduce every parameter's gradient in the bucket (bucket.gradients(), views of the
    buffer) is round-tripped in place as a field of its own, under the finest tolerance whose stream takes at most
    floor(target_bits * n_s) bits: one pass writes a rate table per gradient, one kernel fits them all and the round
    trip reads each gradient's minexp from its record (codec.TensorListFittedPerTensor through the codec's
    roundtrip_fitted_per_tensor, cached per bucket). It is always fitted on the device -- nothing is read on the host,
    whatever `fit_on_device` says -- and `fit_record(index)` is the int64[S, 2] tensor of the bucket's records. A quiet
    layer keeps its own tolerance and a loud one cannot take its bits; fits stop at minexp -94 (include/gcow.h).
    `params` supplies maxprec. The bucket must be fp32 or bf16. ValueError: without `target_bits`; with
    `relative_bits` (both choose the tolerance), `error_feedback` or `compress_mean`; registered with
    compressed_sharded_hook, whose pieces carry no per-tensor minexp; a codec without roundtrip_fitted_per_tensor.
    compressed_allgather_hook takes it too (with `target_bits`; _allgather_per_tensor): each rank fits its own
    gradients, sends one segmented stream (a minexp per tensor, read on the device) and its S fit records, 16 bytes
    per tensor, and every rank decodes and averages the W streams under the W sets in one launch. The bucket's
    gradients must tile its flat buffer in order; a codec without encode_per_tensor / decode_mean_per_tensor:
    ValueError. There `error_feedback` combines with it: each rank takes the per-tensor tables of bucket + carried
    error, fits them and codes that sum with the segmented residual encode, which leaves each tensor's y - decode(y)
    under its own fit in error_buffer(index, ...) (the codec's encode_residual_per_tensor; a codec without it:
    ValueError before any codec call or collective). `reset_error_feedback()` forgets those buffers like the others.
    Unset (the default): nothing changes."""
    params: GcowParams = field(default_factory=lambda: _codec.rate(16, 1))
    process_group: object = None
    codec: object = None  # None: gcow_amd.dist.device_codec()
    timeout_s: float = 300.0
    # the state is registered with compressed_sharded_hook (its exchange runs on the comm thread at any rate); set by
    # make_hook_state(hook=compressed_sharded_hook)
    sharded: bool = False
    # error feedback for the wire hooks (class docstring); roundtrip_hook refuses it
    error_feedback: bool = False
    # compressed_sharded_hook: the mean shards travel compressed too (class docstring); the other hooks refuse it
    compress_mean: bool = False
    mean_params: GcowParams | None = None  # the mean's parameter set; None: `params`
    # roundtrip_hook, compressed_allgather_hook: a tolerance relative to each parameter's gradient (class docstring);
    # compressed_sharded_hook refuses it
    relative_bits: int | None = None
    # accuracy mode under a budget of this many bits per value (class docstring)
    target_bits: float | None = None
    # with target_bits: fit on the device, in the step that is encoded (class docstring)
    fit_on_device: bool = False
    # roundtrip_hook with target_bits: a budget per gradient tensor, fitted on the device (class docstring)
    per_tensor_budget: bool = False
    _fit_records: dict = field(default_factory=dict, repr=False)  # bucket index -> the device gcow_fit record
    _fits: dict = field(default_factory=dict, repr=False)  # bucket index -> (numel, fitted minexp)
    _worker: object = field(default=None, repr=False)
    _side: dict = field(default_factory=dict, repr=False)
    _comm_group: object = field(default=None, repr=False)
    _errors: dict = field(default_factory=dict, repr=False)

    def get_codec(self):
        return self.codec or gdist.device_codec()

    def worker(self) -> "_CommWorker":
        if self._worker is None:
            self._worker = _CommWorker(self._abort_comm_group)
        return self._worker

    def needs_comm_group(self) -> bool:
        """A multi-rank state whose hook runs collectives on the comm thread: variable rate (the all-gather hook's
        length exchange), the sharded hook at any rate, or `relative_bits` whatever `params` is (the all-gather hook
        then runs the segmented, variable-rate exchange and takes only maxprec from `params`). The fixed-rate
        all-gather and round-trip hooks issue theirs from the autograd thread on `process_group` and get no extra
        communicator. The state does not know its hook: one registered with roundtrip_hook under variable-rate
        `params` or `relative_bits` gets a group it does not use."""
        return (dist.is_available() and dist.is_initialized() and dist.get_world_size(self.process_group) > 1
                and (self.sharded or self.relative_bits is not None or not _codec.is_fixed(self.params)))

    def setup(self) -> "GcowHookState":
        """Create the exchange's process group (a collective over `process_group`'s ranks; a no-op for a one-rank
        group): the hook's ranks, in a group of their own so that its collectives (issued
        from the comm thread) never interleave with collectives DDP issues on `process_group` from the autograd
        thread (e.g. the find_unused_parameters all-reduce). Idempotent. Returns self."""
        if self._comm_group is None and self.needs_comm_group():
            ranks = dist.get_process_group_ranks(self.process_group or dist.group.WORLD)
            self._comm_group = dist.new_group(ranks=ranks, timeout=timedelta(seconds=self.timeout_s),
                                              use_local_synchronization=True)
        return self

    def comm_group(self):
        """The exchange group created by setup(). Never created lazily: creating it from the comm thread would race
        with process-group creation on the main thread, and creating it in the hook would block the autograd thread
        until every rank reached that bucket."""
        if self._comm_group is None:
            raise RuntimeError("GcowHookState has no exchange group: the variable-rate and sharded exchanges need "
                               "one, created by setup() on every rank before training -- use "
                               "make_hook_state(hook=<the hook>, ...), or GcowHookState(..., sharded=True).setup() "
                               "for compressed_sharded_hook")
        return self._comm_group

    def _abort_comm_group(self, ex):
        g = self._comm_group
        if g is None:
            return
        try:
            g.abort()  # NCCL/RCCL: tears down this rank's communicator (peers fail only at their timeout)
        except Exception:  # noqa: BLE001 -- gloo has no abort; destroying closes its connections
            try:
                dist.destroy_process_group(g)
            except Exception:  # noqa: BLE001
                pass

    def error_buffer(self, index, x: torch.Tensor) -> torch.Tensor:
        """The carried error of bucket `index` for the flattened bucket x: fp32, x.numel() values on x's device, zeros
        at first use and whenever the bucket's size (or device) differs from the buffer kept -- the old one is dropped."""
        e = self._errors.get(index)
        if e is None or e.numel() != x.numel() or e.device != x.device:
            e = self._errors[index] = torch.zeros(x.numel(), dtype=torch.float32, device=x.device)
        return e

    def mean_error_buffer(self, index, numel: int, device) -> torch.Tensor:
        """compress_mean with error_feedback: the carried error of this rank's mean shard of bucket `index`, keyed by
        (index, "mean", numel): fp32 zeros at first use; a shard whose size changed drops the buffer kept before."""
        key = (index, "mean", numel)
        e = self._errors.get(key)
        if e is None or e.device != device:
            for k in [k for k in self._errors if isinstance(k, tuple) and len(k) == 3 and k[:2] == key[:2]]:
                del self._errors[k]
            e = self._errors[key] = torch.zeros(numel, dtype=torch.float32, device=device)
        return e

    def reset_error_feedback(self):
        """Forget every carried error (the next step starts from zeros): after loading a checkpoint, changing the
        codec parameters, or skipping a step whose gradients were discarded."""
        self._errors.clear()

    def check_target(self):
        """ValueError for a `target_bits` the hooks cannot serve (class docstring); nothing when it is unset."""
        if self.target_bits is None:
            if self.fit_on_device:
                raise ValueError("fit_on_device fits target_bits on the device: set target_bits")
            if self.per_tensor_budget:
                raise ValueError("per_tensor_budget gives every gradient target_bits bits per value: set target_bits")
            return
        if not _codec.is_nobudget(self.params) or _codec.is_fixed(self.params):
            raise ValueError("target_bits fits accuracy mode: params must be a variable-rate set without a block "
                             "budget (minbits <= 1, maxbits >= 160), got %r" % (self.params,))
        if self.relative_bits is not None:
            raise ValueError("target_bits and relative_bits both choose the tolerance: set one")

    def step_params(self, index, numel: int) -> GcowParams:
        """The set bucket `index` of `numel` values is coded under in this step: `params`, or with target_bits the
        accuracy-mode set of the minexp fitted in the step before (a bucket whose size changed starts from `params`)."""
        ent = self._fits.get(index) if self.target_bits is not None else None
        if ent is None or ent[0] != numel:
            return self.params
        return _codec.fitted_params(self.params.maxprec, ent[1])

    def reset_rate_fit(self):
        """Forget every fitted minexp (target_bits): the next step codes under `params` again."""
        self._fits.clear()
        self._fit_records.clear()

    def fit_record(self, index):
        """fit_on_device: the gcow_fit record of bucket `index`'s latest step, on the bucket's device (None before its
        first step); codec.read_fit reads it on the host."""
        return self._fit_records.get(index)

    def check_fit_on_device(self, cdc, hook_name: str) -> bool:
        """-> fit_on_device, after ValueError for what the mode cannot be combined with (class docstring)."""
        if not self.fit_on_device:
            return False
        why = None
        resid = self.error_feedback and hook_name == "compressed_allgather_hook" and not self.compress_mean
        if self.error_feedback and not resid:
            why = "error_feedback encodes with the residual form, another kernel family"
        elif self.compress_mean:
            why = "compress_mean encodes the mean with the reduce encoder, another kernel family"
        elif hook_name == "compressed_sharded_hook":
            why = "compressed_sharded_hook decodes the pieces it receives under host parameters in the same exchange"
        if why:
            raise ValueError("fit_on_device is for roundtrip_hook, and for compressed_allgather_hook with or without "
                             "error feedback: " + why)
        missing = [m for m in ("rate_table", "fit_device", "encode_fitted", "roundtrip_fitted") if not hasattr(cdc, m)]
        if missing:
            raise ValueError("fit_on_device needs a codec with %s (gcow_amd.dist.DeviceCodec)" % ", ".join(missing))
        if resid:  # the table of bucket + carried error, and the residual encode under the device record
            missing = [m for m in ("rate_table_residual", "encode_residual_fitted") if not hasattr(cdc, m)]
            if missing:
                raise ValueError("fit_on_device with error_feedback needs a codec with %s "
                                 "(gcow_amd.dist.DeviceCodec)" % ", ".join(missing))
        return True

    def side_stream(self, dev):
        if dev not in self._side:
            self._side[dev] = torch.cuda.Stream(dev)
        return self._side[dev]


def make_hook_state(hook=None, **kw) -> GcowHookState:
    """GcowHookState(**kw).setup() for `hook` (the function the state is registered with; compressed_sharded_hook
    sets `sharded`): call on every rank of the hook's process group at the same point of setup."""
    if hook is not None and getattr(hook, "__name__", "") == "compressed_sharded_hook":
        kw.setdefault("sharded", True)
    return GcowHookState(**kw).setup()


def _done(t: torch.Tensor) -> torch.futures.Future[torch.Tensor]:
    fut = torch.futures.Future()
    fut.set_result(t)
    return fut


def _flat(buf: torch.Tensor):
    flat = buf.reshape(-1)
    return flat, (flat if flat.dtype in (torch.float32, torch.bfloat16) else flat.float())


def _mean_into(cdc, flat: torch.Tensor, *args):
    """decode_mean written straight into the bucket when it is fp32 or bf16 (bf16: the fp32 mean rounded to nearest
    even in the kernel -- no fp32 temporary, no cast pass); other dtypes through an fp32 temporary."""
    if flat.dtype in (torch.float32, torch.bfloat16) and flat.is_contiguous():
        cdc.decode_mean(*args, out=flat)
    else:
        flat.copy_(cdc.decode_mean(*args).to(flat.dtype))


def _encode(state: GcowHookState, cdc, bucket, x: torch.Tensor, stride: int, slot, p: GcowParams | None = None):
    """The wire hooks' encode of the flattened bucket x under p (default: state.params): with state.error_feedback, of
    x plus the bucket's carried error, which is updated in place (the buffer lives on the state, so the exchange never
    reads it)."""
    if p is None:
        p = state.params
    if not state.error_feedback:
        return cdc.encode(x, p, stride, slot=slot)
    index = bucket.index() if hasattr(bucket, "index") else None
    return cdc.encode_residual(x, state.error_buffer(index, x), p, stride, slot=slot)


def _rate_table(state: GcowHookState, cdc, x: torch.Tensor, index):
    """target_bits: launch the rate table of the flattened bucket x (beside the wire hooks' encode, or on the reduced
    bucket in roundtrip_hook); None when the state has no target."""
    if state.target_bits is None:
        return None
    if not hasattr(cdc, "rate_table"):
        raise ValueError("target_bits needs a codec with rate_table (gcow_amd.dist.DeviceCodec)")
    return cdc.rate_table(x, state.params.maxprec, slot=("rate", index))


def _budget(state: GcowHookState, n: int) -> int:
    return int(state.target_bits * n)  # floor: both are >= 0


def _fit_next(state: GcowHookState, table: torch.Tensor, index, n: int, world: int, group):
    """The wire hooks' shared control step, inside the exchange: the ranks' tables summed over the exchange group (the
    length of all W streams under each minexp), fitted against W budgets, and the minexp kept for the bucket's next
    step. The one host read (2.3 KB) blocks the comm thread only. A budget below one bit per block cannot be met:
    the coarsest entry is taken."""
    if world > 1:
        dist.all_reduce(table, group=group)
    h = table.cpu().tolist()
    me, _ = _codec.fit_minexp(h, max(world * _budget(state, n), h[-1]))
    state._fits[index] = (n, me)


_PER_TENSOR_WIRE = ("per_tensor_budget is for roundtrip_hook and compressed_allgather_hook: a stream coded under a "
                    "minexp per tensor needs them on the wire to be decoded, which only the all-gather hook's segmented "
                    "exchange sends")
_RELATIVE_WIRE = ("relative_bits is for roundtrip_hook and compressed_allgather_hook: a stream coded under per-tensor "
                  "exponents needs them on the wire to be decoded, which only the all-gather hook's segmented exchange "
                  "sends; compressed_sharded_hook's pieces carry none")


def roundtrip_hook(state: GcowHookState, bucket) -> torch.futures.Future[torch.Tensor]:
    """Mean all-reduce, then the lossy encode -> decode the reference applies (zfpy), device-resident: one fused
    `roundtrip` call on an fp32 / bf16 bucket when the codec has one, else encode followed by decode."""
    if state.error_feedback:
        raise ValueError("error_feedback is for the wire hooks (compressed_allgather_hook, compressed_sharded_hook): "
                         "roundtrip_hook applies its loss after the reduction, identically on every rank"
                         + (" (per_tensor_budget has no residual form)" if state.per_tensor_budget else ""))
    if state.compress_mean:
        raise ValueError("compress_mean is for compressed_sharded_hook (its all-gather of the mean shards): "
                         "roundtrip_hook puts no mean shard on the wire")
    if state.per_tensor_budget and state.relative_bits is not None:
        raise ValueError("per_tensor_budget (with target_bits) and relative_bits both choose the tolerance: set one")
    state.check_target()
    group = state.process_group
    buf = bucket.buffer()
    cdc = state.get_codec()
    fod = state.check_fit_on_device(cdc, "roundtrip_hook")
    rel = state.relative_bits
    if rel is not None:
        if not hasattr(cdc, "roundtrip_relative"):
            raise ValueError("relative_bits needs a codec with roundtrip_relative (gcow_amd.dist.DeviceCodec)")
        if buf.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("relative_bits takes fp32 or bf16 buckets, got %s" % buf.dtype)
    ptb = state.per_tensor_budget
    if ptb:
        if not hasattr(cdc, "roundtrip_fitted_per_tensor"):
            raise ValueError("per_tensor_budget needs a codec with roundtrip_fitted_per_tensor "
                             "(gcow_amd.dist.DeviceCodec)")
        if buf.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("per_tensor_budget takes fp32 or bf16 buckets, got %s" % buf.dtype)
    world = dist.get_world_size(group)
    fut = dist.all_reduce(buf.div_(world), group=group, async_op=True).get_future()

    def lossy(f):
        t = f.value()[0]
        if ptb:  # each parameter's view of the bucket, in place, under its own budget: tables -> fits -> round trip
            bidx = bucket.index() if hasattr(bucket, "index") else None
            plan = cdc.roundtrip_fitted_per_tensor(bucket.gradients(), state.target_bits,
                                                   maxprec=state.params.maxprec, slot=("per_tensor", bidx))
            state._fit_records[bidx] = getattr(plan, "fits", None)
            return t
        if rel is not None:  # each parameter's view of the bucket, in place, under its own tolerance
            cdc.roundtrip_relative(bucket.gradients(), rel, maxprec=state.params.maxprec,
                                   slot=("rel", bucket.index()))
            return t
        flat, x = _flat(t)
        p = state.params
        bidx = bucket.index() if hasattr(bucket, "index") else None
        if fod:  # table -> fit -> round trip under the record, all on the device: nothing is read here
            rec = cdc.fit_device(_rate_table(state, cdc, x, bidx), _budget(state, x.numel()), slot=("fit", bidx))
            state._fit_records[bidx] = rec
            direct = flat.dtype in (torch.float32, torch.bfloat16) and flat.is_contiguous()
            cdc.roundtrip_fitted(x, rec, p.maxprec, out=flat if direct else x)
            if not direct:
                flat.copy_(x.to(flat.dtype))
            return t
        if state.target_bits is not None:  # the reduced bucket's own table: the same fit on every rank
            table = _rate_table(state, cdc, x, bidx)
            me, _ = _codec.fit_minexp(table, _budget(state, x.numel()))  # host read, in this callback
            p = _codec.fitted_params(p.maxprec, me)
            state._fits[bidx] = (x.numel(), me)
        if hasattr(cdc, "roundtrip") and flat.dtype in (torch.float32, torch.bfloat16) and flat.is_contiguous():
            cdc.roundtrip(x, p, out=flat)  # one kernel, in place, no stream (same bits as the path below)
            return t
        stride = 0 if _codec.is_fixed(p) else INDEX_STRIDE
        # per-bucket buffers: DDP may run several buckets' callbacks before the first one's decode has read its words
        words, _, index = cdc.encode(x, p, stride, slot=("roundtrip", bidx))
        if flat.dtype in (torch.float32, torch.bfloat16) and flat.is_contiguous():
            cdc.decode(words, x.numel(), p, index=index, index_stride=stride, out=flat)  # in place
        else:
            out = cdc.decode(words, x.numel(), p, index=index, index_stride=stride)
            flat.copy_(out.to(flat.dtype))
        return t

    return fut.then(lossy)


class _CommWorker:
    """One FIFO thread per hook state for the variable-rate exchange: its host read of the gathered lengths (which
    size the padded all-gather) blocks this thread only, never the autograd thread, and the collectives it issues
    keep DDP's bucket order on every rank (one queue).

    Fail fast: the first exception stops the worker. That bucket's future and every future queued or submitted after
    it fail at once (DDP raises in its wait instead of hanging on a bucket that never runs), and `on_error` aborts the
    exchange's process group: gloo peers blocked in a collective with this rank error out at once, RCCL peers when
    the group's timeout expires."""

    def __init__(self, on_error=None):
        self.q = queue.Queue()
        self.failed = None
        self.on_error = on_error
        self.t = threading.Thread(target=self._loop, name="gcow-comm", daemon=True)
        self.t.start()

    def _stopped(self):
        return RuntimeError("gcow comm thread stopped after an earlier failure: %r" % (self.failed,))

    def _loop(self):
        while True:
            fn, fut = self.q.get()
            if self.failed is not None:
                if not fut.done():
                    fut.set_exception(self._stopped())
                continue
            try:
                fn(fut)  # completes fut itself, inside its stream context
            except Exception as ex:  # surfaces in DDP's wait on the hook future
                self.failed = ex
                if not fut.done():
                    fut.set_exception(ex)
                if self.on_error is not None:
                    self.on_error(ex)

    def submit(self, fn, fut):
        if self.failed is not None:
            fut.set_exception(self._stopped())
            return fut
        self.q.put((fn, fut))
        return fut


def _bucket_counts(bucket, buf: torch.Tensor, what: str = "per_tensor_budget"):
    """The sizes of the bucket's gradients when they tile its flat buffer in order (pointer arithmetic), else
    ValueError: the segmented stream is cut where the gradients lie. what: the mode that asks, for the message."""
    grads = list(bucket.gradients())
    at, esz = buf.data_ptr(), buf.element_size()
    counts = []
    for g in grads:
        n = g.numel()
        if g.dtype != buf.dtype or (n and (not g.is_contiguous() or g.data_ptr() != at)):
            raise ValueError("%s on the wire: the bucket's gradients must tile its flat buffer in "
                             "order (gradient %d does not lie where the one before it ends)" % (what, len(counts)))
        counts.append(n)
        at += n * esz
    if sum(counts) != buf.numel():
        raise ValueError("%s on the wire: the bucket's gradients cover %d of its %d values"
                         % (what, sum(counts), buf.numel()))
    return counts


def _allgather_per_tensor(state: GcowHookState, bucket) -> torch.futures.Future[torch.Tensor]:
    """compressed_allgather_hook with per_tensor_budget: every rank fits its own gradients -- per-tensor rate tables,
    one batch fit against floor(target_bits * n_s) bits, the segmented encode under the records, with a 16-block index,
    launched on the autograd thread with nothing read back -- so its stream is at most sum_s floor(target_bits * n_s)
    bits whenever every record's status is 0. On the comm thread: the gathered lengths (the one host read), the padded
    all-gather of the words, the all-gather of the index, and the all-gather of each rank's S fit records, 16 bytes per
    tensor: that is the wire format of the per-tensor minexp (word 0 of a record). Then one decode-mean straight into
    the bucket, stream r's tensor s under record (r, s). No table is all-reduced and no minexp reaches the host;
    state.fit_record(index) is this rank's int64[S, 2] records. With state.error_feedback the tables are those of
    bucket + carried error, the encode is the segmented residual form (the codec's encode_residual_per_tensor) and
    state.error_buffer(index, ...) is updated in place; the wire format and the receive side are the same."""
    state.check_target()
    cdc = state.get_codec()
    missing = [m for m in ("encode_per_tensor", "decode_mean_per_tensor") if not hasattr(cdc, m)]
    if missing:
        raise ValueError("per_tensor_budget with compressed_allgather_hook needs a codec with %s "
                         "(gcow_amd.dist.DeviceCodec): %s" % (", ".join(missing), _PER_TENSOR_WIRE))
    if state.error_feedback and not hasattr(cdc, "encode_residual_per_tensor"):
        raise ValueError("error_feedback with per_tensor_budget needs a codec with encode_residual_per_tensor "
                         "(gcow_amd.dist.DeviceCodec): the segmented encode of bucket + carried error that writes "
                         "each tensor's residual under its own fit")
    if not (dist.is_available() and dist.is_initialized()):
        raise ValueError("compressed_allgather_hook with per_tensor_budget needs an initialised process group")
    group = state.process_group
    buf = bucket.buffer()
    if buf.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("per_tensor_budget takes fp32 or bf16 buckets, got %s" % buf.dtype)
    flat = buf.reshape(-1)
    if not flat.is_contiguous() or flat.data_ptr() != buf.data_ptr():
        raise ValueError("per_tensor_budget on the wire takes a contiguous bucket buffer")
    counts = _bucket_counts(bucket, flat)
    world = dist.get_world_size(group)
    slot = bucket.index() if hasattr(bucket, "index") else None
    maxprec = state.params.maxprec
    cgroup = state.comm_group() if world > 1 else group  # raises here, on the autograd thread, without setup()
    if state.error_feedback:  # the buffer is obtained here (zeros at first use, on this stream); it lives on the state
        words, bits, index, fits = cdc.encode_residual_per_tensor(flat, state.error_buffer(slot, flat), counts,
                                                                  state.target_bits, maxprec, INDEX_STRIDE,
                                                                  slot=("per_tensor", slot))
    else:
        words, bits, index, fits = cdc.encode_per_tensor(flat, counts, state.target_bits, maxprec, INDEX_STRIDE,
                                                         slot=("per_tensor", slot))
    state._fit_records[slot] = fits
    return _segmented_exchange(state, cdc, buf, flat, counts, words, bits, index, fits, maxprec, world, cgroup,
                               ("per_tensor", slot))


def _segmented_exchange(state: GcowHookState, cdc, buf, flat, counts, words, bits, index, sets, maxprec, world, cgroup,
                        slot) -> torch.futures.Future[torch.Tensor]:
    """The comm-thread half of the segmented hooks: a rank's segmented stream (words, bits, index at INDEX_STRIDE) and
    its per-tensor sets -- int64[S, 2] fit records, 16 bytes per tensor (minexp | status << 32, bits), or int32[S]
    minexp words, 4 bytes per tensor -- are all-gathered, and one decode-mean writes the bucket, stream r's tensor s
    under set (r, s). The gathered lengths are the one host read."""
    dev = flat.device
    if dev.type == "cuda":
        ev = torch.cuda.Event()
        ev.record()
        side = state.side_stream(dev)
        fut = torch.futures.Future(devices=[dev])
    else:
        ev = side = None
        fut = torch.futures.Future()

    def exchange(fut):
        if side is not None:
            torch.cuda.set_device(dev)
        ctx = torch.cuda.stream(side) if side is not None else contextlib.nullcontext()
        with ctx:
            if side is not None:
                side.wait_event(ev)
                for t in (words, bits, index, sets):
                    t.record_stream(side)
            lens, lens_h = gdist.gather_lengths(bits, dev, cgroup)  # host read: this thread waits, autograd does not
            maxw = max(1, max((b + 63) // 64 for b in lens_h))
            rank = dist.get_rank(cgroup)
            gathered = gdist.allgather_padded(words, (lens_h[rank] + 63) // 64, maxw, cgroup, pad=2)
            ni = index.numel()
            idx = torch.empty(world * ni, dtype=torch.int64, device=dev)
            gdist.allgather_into(idx, index[:ni].contiguous(), cgroup)
            mine = sets.reshape(-1).contiguous()
            recs = torch.empty(world * mine.numel(), dtype=mine.dtype, device=dev)
            gdist.allgather_into(recs, mine, cgroup)
            cdc.decode_mean_per_tensor(gathered, maxw, world, counts, recs, maxprec, idx, ni, INDEX_STRIDE, out=flat,
                                       slot=slot)
            fut.set_result(buf)

    return state.worker().submit(exchange, fut)


def _allgather_relative(state: GcowHookState, bucket) -> torch.futures.Future[torch.Tensor]:
    """compressed_allgather_hook with relative_bits: every rank codes each gradient of the bucket under a tolerance of
    2^-relative_bits of that gradient's own largest magnitude. On the autograd thread, with nothing read back: one pass
    over the bucket leaves a minexp word per gradient (the codec's encode_relative: the words pass, then the segmented
    encode under those words, with a 16-block index). On the comm thread (_segmented_exchange): the gathered lengths,
    the padded all-gather of the streams, the all-gather of the index and the all-gather of each rank's S int32 words --
    the wire format, 4 bytes per tensor -- then one decode-mean straight into the bucket, stream r's tensor s under
    word (r, s). `params` contributes only its maxprec. With state.error_feedback the words are those of bucket +
    carried error, the encode is the segmented residual form (encode_residual_relative) and
    state.error_buffer(index, ...) is updated in place; the wire format and the receive side are the same.
    Every refusal is a ValueError naming relative_bits, raised before any codec call or collective."""
    rel = state.relative_bits
    if state.compress_mean:
        raise ValueError("relative_bits with compress_mean: compress_mean is for compressed_sharded_hook (its "
                         "all-gather of the mean shards); compressed_allgather_hook sends no mean")
    try:
        state.check_target()  # target_bits and relative_bits both choose the tolerance
    except ValueError as ex:
        if "relative_bits" in str(ex):
            raise
        raise ValueError("relative_bits with a budget mode: %s" % ex) from None
    if state.per_tensor_budget:
        raise ValueError("per_tensor_budget (with target_bits) and relative_bits both choose the tolerance: set one")
    if not _codec.valid_rel_bits(rel):
        raise ValueError("relative_bits must be an integer in 0..%d, got %r" % (_codec.REL_BITS_MAX, rel))
    cdc = state.get_codec()
    need = ("encode_relative", "decode_mean_per_tensor") + (("encode_residual_relative",) if state.error_feedback else ())
    missing = [m for m in need if not hasattr(cdc, m)]
    if missing:
        raise ValueError("relative_bits with compressed_allgather_hook%s needs a codec with %s "
                         "(gcow_amd.dist.DeviceCodec)" % (" and error_feedback" if state.error_feedback else "",
                                                          ", ".join(missing)))
    if not (dist.is_available() and dist.is_initialized()):
        raise ValueError("compressed_allgather_hook with relative_bits needs an initialised process group")
    group = state.process_group
    buf = bucket.buffer()
    if buf.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("relative_bits takes fp32 or bf16 buckets, got %s" % buf.dtype)
    flat = buf.reshape(-1)
    if not flat.is_contiguous() or flat.data_ptr() != buf.data_ptr():
        raise ValueError("relative_bits on the wire takes a contiguous bucket buffer")
    counts = _bucket_counts(bucket, flat, "relative_bits")
    world = dist.get_world_size(group)
    slot = bucket.index() if hasattr(bucket, "index") else None
    maxprec = state.params.maxprec
    cgroup = state.comm_group() if world > 1 else group  # raises here, on the autograd thread, without setup()
    if state.error_feedback:  # the buffer is obtained here (zeros at first use, on this stream); it lives on the state
        words, bits, index, mx = cdc.encode_residual_relative(flat, state.error_buffer(slot, flat), counts, rel,
                                                              maxprec, INDEX_STRIDE, slot=("relative", slot))
    else:
        words, bits, index, mx = cdc.encode_relative(flat, counts, rel, maxprec, INDEX_STRIDE, slot=("relative", slot))
    return _segmented_exchange(state, cdc, buf, flat, counts, words, bits, index, mx, maxprec, world, cgroup,
                               ("relative", slot))


def compressed_allgather_hook(state: GcowHookState, bucket) -> torch.futures.Future[torch.Tensor]:
    """Encode locally, all-gather the compressed streams, decode every rank's stream and average (one launch).

    Asynchronous: the hook enqueues and returns, so bucket i's exchange overlaps the backward of the next buckets
    (DDP's point; hw/models/train_imagenet.py:194-195, 219, 224 relies on it). Fixed rate chains encode -> all-gather
    (async_op) -> decode-mean through Future.then. Variable rate needs the gathered lengths on the host to size the
    padded all-gather; that read and the collectives after it run on the state's comm thread (on a side stream that
    waits for the encode), and the returned future completes when the mean is written. Each bucket encodes into its
    own buffers (slot = bucket index), so a later bucket's encode never overwrites a stream still in flight."""
    if state.relative_bits is not None:  # ahead of the checks below: its refusals, compress_mean's too, name the field
        return _allgather_relative(state, bucket)
    if state.compress_mean:
        raise ValueError("compress_mean is for compressed_sharded_hook (its all-gather of the mean shards): "
                         "compressed_allgather_hook decodes every rank's stream on every rank and sends no mean")
    if state.per_tensor_budget:
        return _allgather_per_tensor(state, bucket)
    state.check_target()
    cdc = state.get_codec()
    fod = state.check_fit_on_device(cdc, "compressed_allgather_hook")  # before any collective
    if fod and not (dist.is_available() and dist.is_initialized()):
        # said here, with the state's modes, and not by torch's "default process group" error from the line below
        raise ValueError("compressed_allgather_hook with fit_on_device (error_feedback=%s) encodes inside the "
                         "exchange and needs an initialised process group" % state.error_feedback)
    group = state.process_group
    buf = bucket.buffer()
    world = dist.get_world_size(group)
    flat, x = _flat(buf)
    n = x.numel()
    slot = bucket.index() if hasattr(bucket, "index") else None
    p = state.step_params(slot, n)  # state.params, or with target_bits the set fitted in the step before
    if _codec.is_fixed(p):
        words, _, _ = _encode(state, cdc, bucket, x, 0, slot)
        nw = ((n + 3) // 4 * p.maxbits + 63) // 64
        gathered = torch.zeros(world * nw + 2, dtype=torch.int64, device=x.device)
        fut = gdist.allgather_into_async(gathered[: world * nw], words[:nw].contiguous(), group)

        def finish(f):
            f.wait()
            if gathered.is_cuda:
                # the callback runs on a pool stream; without this the allocator could hand `gathered` to the next
                # bucket's torch.zeros on the autograd stream before the decode below has read it
                gathered.record_stream(torch.cuda.current_stream(gathered.device))
            _mean_into(cdc, flat, gathered, nw, world, n, p)
            return buf

        return fut.then(finish)
    cgroup = state.comm_group() if world > 1 else group  # raises here, on the autograd thread, without setup()
    err = None
    if fod:  # encoded inside the exchange, under this step's own fit
        words = bits = index = table = None
        if state.error_feedback:  # obtained here (zeros at first use, on this stream); it lives on the state
            err = state.error_buffer(slot, x)
    else:
        words, bits, index8 = _encode(state, cdc, bucket, x, SHARDED_INDEX_STRIDE, slot, p)
        index = cdc.pack_index16(index8, n, p)  # what travels: one entry per 16 blocks
        table = _rate_table(state, cdc, x, slot)  # target_bits: this step's lengths, for the next step's set
    dev = x.device
    if dev.type == "cuda":
        ev = torch.cuda.Event()
        ev.record()
        side = state.side_stream(dev)
        fut = torch.futures.Future(devices=[dev])
    else:
        ev = side = None
        fut = torch.futures.Future()

    def exchange(fut):
        nonlocal words, bits, index, p
        if side is not None:
            torch.cuda.set_device(dev)  # this thread's current device: the bucket's, on every LOCAL_RANK
        ctx = torch.cuda.stream(side) if side is not None else contextlib.nullcontext()
        with ctx:
            if side is not None:
                side.wait_event(ev)
                for t in (words, bits, index, table, x if fod else None):  # read on the side stream: kept from the
                    if t is not None:                                      # allocator until then
                        t.record_stream(side)
            rec = None
            if fod:  # this step's table, summed over the ranks, fitted and encoded under on the device
                if err is not None:  # of y = x + e, what is encoded and sent
                    tab = cdc.rate_table_residual(x, err, p.maxprec, slot=("rate", slot))
                else:
                    tab = _rate_table(state, cdc, x, slot)
                if world > 1:
                    dist.all_reduce(tab, group=cgroup)
                rec = cdc.fit_device(tab, world * _budget(state, n), slot=("fit", slot))
                state._fit_records[slot] = rec
                if err is not None:  # e is updated in place: y - decode(stream) under the fitted set
                    words, bits, index8 = cdc.encode_residual_fitted(x, err, rec, p.maxprec, SHARDED_INDEX_STRIDE,
                                                                     slot=slot)
                else:
                    words, bits, index8 = cdc.encode_fitted(x, rec, p.maxprec, SHARDED_INDEX_STRIDE, slot=slot)
                index = cdc.pack_index16(index8, n, p)  # the packing reads no minexp
            elif table is not None:
                _fit_next(state, table, slot, n, world, cgroup)
            lens, lens_h = gdist.gather_lengths(bits, dev, cgroup)  # host read: this thread waits, autograd does not
            if rec is not None:  # the stream has just drained: 16 bytes more, no new wait
                p = _codec.fitted_params(p.maxprec, _codec.read_fit(rec)[0])
            maxw = max(1, max((b + 63) // 64 for b in lens_h))
            rank = dist.get_rank(cgroup)
            gathered = gdist.allgather_padded(words, (lens_h[rank] + 63) // 64, maxw, cgroup, pad=2)
            ni = index.numel()
            idx = torch.empty(world * ni, dtype=torch.int64, device=dev)
            gdist.allgather_into(idx, index[:ni].contiguous(), cgroup)
            _mean_into(cdc, flat, gathered, maxw, world, n, p, idx, ni, _codec.INDEX_PACKED16)
            # completed inside the side-stream context: the future records its event on this stream, so DDP's wait
            # orders its use of the bucket after the mean is written
            fut.set_result(buf)

    return state.worker().submit(exchange, fut)


def _mean_stream(state: GcowHookState, cdc, bidx, pieces, pw, world, lo, hi, pidx, iw, stride, dev, p=None):
    """compress_mean: the stream (words, bits, index) of the mean of this rank's `world` received pieces (coded under
    p; default state.params) under state.mean_params, with error feedback on the mean shard when the state asks for
    it; (None, None, None) for an empty shard. Runs inside the exchange, on the side stream: the carried error and the
    cached encoder's buffers are allocated there."""
    if hi <= lo:
        return None, None, None
    if p is None:
        p = state.params
    mp = state.mean_params or state.params
    ostride = 0 if _codec.is_fixed(mp) else gdist.MEAN_INDEX_STRIDE
    err = None
    if state.error_feedback:
        err = state.mean_error_buffer(bidx, hi - lo, dev)
    slot = ("sharded-mean", bidx)
    if hasattr(cdc, "decode_mean_encode"):
        return cdc.decode_mean_encode(pieces, pw, world, hi - lo, p, pidx, iw, stride, out_params=mp, err=err,
                                      out_index_stride=ostride, slot=slot)
    m = cdc.decode_mean(pieces, pw, world, hi - lo, p, pidx, iw, stride)  # an fp32 temporary
    if err is not None:
        return cdc.encode_residual(m, err, mp, ostride, slot=slot)
    return cdc.encode(m, mp, ostride, slot=slot)


def compressed_sharded_hook(state: GcowHookState, bucket) -> torch.futures.Future[torch.Tensor]:
    """The compressed exchange with a sharded receive side (gcow_amd.dist "sharded receive"): each rank encodes its
    bucket, cuts its stream at the shard boundaries (fixed rate: at b * maxbits; variable rate: at the block index)
    and sends piece r to rank r in one all-to-all; rank r decodes and averages the W pieces of its shard in one launch
    (gcow_decode_mean_device), and an all-gather of the mean shards (in the bucket's dtype: fp32, or bf16 rounded to
    nearest even in the kernel) rebuilds the bucket on every rank. The result is bit-identical to
    compressed_allgather_hook's (the same fp32 sums in rank order); per rank it receives (W - 1) / W of one stream
    instead of W - 1 streams and decodes 1 / W of the values, for an extra all-gather of the mean. Collectives run on
    the state's comm thread over its exchange group (GcowHookState.setup, every rank), on a side stream that waits
    for the encode; the returned future completes when the bucket holds the mean.

    With state.compress_mean the second stage is compressed too (gcow_amd.dist.allgather_mean_streams): the owner
    codes the mean of its pieces without storing it (cdc.decode_mean_encode; a codec without that method composes
    decode_mean and encode), and the bucket ends as decode(encode(mean)) under state.mean_params on every rank."""
    if state.relative_bits is not None:
        raise ValueError(_RELATIVE_WIRE)
    if state.per_tensor_budget:
        raise ValueError(_PER_TENSOR_WIRE)
    state.check_target()
    state.check_fit_on_device(state.get_codec(), "compressed_sharded_hook")
    group = state.process_group
    buf = bucket.buffer()
    world = dist.get_world_size(group)
    flat, x = _flat(buf)
    n = x.numel()
    cdc = state.get_codec()
    bidx = bucket.index() if hasattr(bucket, "index") else None
    p = state.step_params(bidx, n)  # state.params, or with target_bits the set fitted in the step before
    fixed = _codec.is_fixed(p)
    stride = 0 if fixed else SHARDED_INDEX_STRIDE
    cgroup = state.comm_group() if world > 1 else group  # raises here, on the autograd thread, without setup()
    slot = ("sharded", bidx)
    words, bits, index = _encode(state, cdc, bucket, x, stride, slot, p)
    table = _rate_table(state, cdc, x, bidx)  # target_bits: this step's lengths, for the next step's set
    dev = x.device
    if dev.type == "cuda":
        ev = torch.cuda.Event()
        ev.record()
        side = state.side_stream(dev)
        fut = torch.futures.Future(devices=[dev])
    else:
        ev = side = None
        fut = torch.futures.Future()

    def exchange(fut):
        if side is not None:
            torch.cuda.set_device(dev)
        ctx = torch.cuda.stream(side) if side is not None else contextlib.nullcontext()
        with ctx:
            if side is not None:
                side.wait_event(ev)
                for t in (words, bits, index, table):
                    if t is not None:
                        t.record_stream(side)
            if table is not None:
                _fit_next(state, table, bidx, n, world, cgroup)
            if fixed:
                pieces, pw, lo, hi = gdist.shard_pieces_fixed(words, n, p.maxbits, cgroup)
                pidx, iw = None, 0
            else:
                pieces, pw, pidx, iw, lo, hi = gdist.shard_pieces_variable(words, bits, index, n, stride, cgroup)
            direct = flat.dtype in (torch.float32, torch.bfloat16) and flat.is_contiguous()
            shard = flat[lo:hi] if direct else torch.empty(hi - lo, dtype=torch.float32, device=dev)
            if state.compress_mean:
                mwords, mbits, midx = _mean_stream(state, cdc, bidx, pieces, pw, world, lo, hi, pidx, iw, stride, dev,
                                                   p)
                gdist.allgather_mean_streams(flat, mwords, mbits, midx, n, state.mean_params or state.params, cgroup,
                                             cdc)
                fut.set_result(buf)
                return
            if hi > lo:
                cdc.decode_mean(pieces, pw, world, hi - lo, p, pidx, iw, stride, out=shard)
            gdist.allgather_shards(flat, shard if direct else shard.to(flat.dtype), n, cgroup)
            fut.set_result(buf)

    return state.worker().submit(exchange, fut)
