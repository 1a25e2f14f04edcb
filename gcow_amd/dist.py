"""Multi-GPU path: shard a gradient bucket across ranks, encode each shard on its own MI355X, all-gather the
compressed streams over RCCL (torch.distributed backend "nccl" is RCCL on ROCm) into the single-stream layout.

The reference never puts compressed bytes on a wire (its DDP all-reduce runs on fp32 before zfpy,
hw/models/train_imagenet.py:446-475); this is the exchange step north_star asks for.

Fixed rate: every block is maxbits long, so shard r's stream occupies bits [r*S*maxbits, ...) of the full stream;
with S*maxbits a multiple of 64 one all-gather of equal-size shard streams IS the single-GPU stream (byte-identical
to encoding the whole bucket on one GPU).
Variable rate: all-gather the per-rank bit lengths (device tensors), all-gather the streams padded to the longest,
then one launch stitches every shard at its exclusive-prefix bit offset (gcow_stitch_shards_device: the prefix is
taken on the device from the gathered lengths). Per-shard flush padding is dropped: offsets use the unflushed bit
counts. The host reads the gathered lengths once, to size the padded buffers.

The codec work is injectable: every function takes `codec=` (default `DeviceCodec`, the gfx950 kernels), so the
protocol code itself runs unchanged over gloo on CPU tensors with an oracle-backed codec in tests/test_dist_cpu.py.
"""
from __future__ import annotations

from collections import OrderedDict

import torch
import torch.distributed as dist

from ._ffi import GcowError


class DeviceCodec:
    """The codec calls the exchange needs, on device tensors through libgcow.so. Encoders are cached per
    (slot, shape, dtype, params, index stride) so a repeated bucket allocates nothing. Eviction is by idleness, not by
    a fixed count: an entry not used during the last `idle_factor` x (number of cached entries) + `idle_slack` encode
    calls is dropped. A model with B buckets reuses each key every B calls, so its steady-state encoders are never
    evicted however large B is, while the first iteration's encoders (DDP rebuilds its buckets after it: new indices
    and sizes) are released after a few iterations instead of holding their output / index / workspace buffers for
    the life of the process. An evicted encoder's buffers live on while a caller still references them; callers that
    read them on another stream record that stream on them (gcow_amd.ddp does)."""

    def __init__(self, idle_factor: int = 2, idle_slack: int = 8):
        self._enc = OrderedDict()  # key -> [encoder, last tick], least recently used first
        self.idle_factor = max(1, int(idle_factor))
        self.idle_slack = max(0, int(idle_slack))
        self._tick = 0

    def encode(self, x: torch.Tensor, params, index_stride: int = 0, slot=None):
        """-> (words int64 tensor, bits int64[1] tensor on x.device, block index or None). Calls with the same shape,
        params and `slot` reuse (overwrite) one set of output buffers; callers whose streams are still in flight on
        another stream pass distinct slots (the DDP hook: one per bucket)."""
        x = x.reshape(-1)
        e = self._encoder(x, params, index_stride, slot, False)(x if x.is_contiguous() else x.contiguous())
        return e.words, e.bits_dev, e.index

    def encode_residual(self, x: torch.Tensor, err: torch.Tensor, params, index_stride: int = 0, slot=None):
        """Error feedback: `encode` of y = x + err, with `err` (fp32, x.numel() values, on x's device) updated in place
        to y - decode(stream) (codec.encode_residual). Same return value and cache policy as `encode`; the encoders
        are cached apart from `encode`'s (they hold the composed path's workspace)."""
        x = x.reshape(-1)
        e = self._encoder(x, params, index_stride, slot, True)(x if x.is_contiguous() else x.contiguous(), err)
        return e.words, e.bits_dev, e.index

    def _encoder(self, x, params, index_stride, slot, residual):
        from . import codec
        self._tick += 1
        key = (slot, x.numel(), x.dtype, x.device, params.tuple(), index_stride) + (("residual",) if residual else ())
        ent = self._enc.get(key)
        if ent is None:
            enc = codec.ResidualEncoder(x.numel(), x.dtype, params, x.device, index_stride) if residual else \
                codec.Encoder((x.numel(),), x.dtype, params, x.device, index_stride)
            ent = self._enc[key] = [enc, self._tick]
        else:
            ent[1] = self._tick
            self._enc.move_to_end(key)
        self._evict_idle()
        return ent[0]

    def decode_mean_encode(self, streams, stream_words: int, nstreams: int, n: int, params, index=None,
                           index_words: int = 0, index_stride: int = 0, out_params=None, err=None,
                           out_index_stride: int = 0, slot=None):
        """The stream of the mean of nstreams received streams (codec.ReduceEncoder): -> (words, bits, index) as
        `encode` of decode_mean(...) under out_params (default: params) returns them; with `err` (fp32, n values,
        updated in place) as `encode_residual` of that mean. Cached per slot like the encoders."""
        from . import codec
        self._tick += 1
        po = out_params if out_params is not None else params
        key = (slot, n, nstreams, streams.device, params.tuple(), po.tuple(), out_index_stride, err is not None,
               "reduce")
        ent = self._enc.get(key)
        if ent is None:
            ent = self._enc[key] = [codec.ReduceEncoder(n, params, nstreams, po, streams.device, err is not None,
                                                        out_index_stride), self._tick]
        else:
            ent[1] = self._tick
            self._enc.move_to_end(key)
        self._evict_idle()
        e = ent[0](streams, stream_words, index, index_words, index_stride, err)
        return e.words, e.bits_dev, e.index

    def _evict_idle(self):
        limit = self.idle_factor * len(self._enc) + self.idle_slack
        while self._enc:
            key, ent = next(iter(self._enc.items()))
            if self._tick - ent[1] <= limit:
                break
            del self._enc[key]

    def stitch_shards(self, dst, src, shard_words: int, lens, nshards: int):
        from . import codec
        return codec.stitch_shards(dst, src, shard_words, lens[:nshards])

    def decode(self, words, n: int, params, index=None, index_stride: int = 0, out=None):
        from . import codec
        return codec.decode(words, (n,), params, index=index, index_stride=index_stride, out=out)

    def roundtrip(self, x: torch.Tensor, params, out=None):
        """decode(encode(x)) in one kernel without the stream (codec.roundtrip): nothing cached, nothing allocated
        when `out` is given (out=x: in place)."""
        from . import codec
        return codec.roundtrip(x, params, out=out)

    def roundtrip_relative(self, tensors, rel_bits: int, maxprec: int = 64, slot=None):
        """Every tensor of the list round-tripped in place under a tolerance relative to its own largest magnitude
        (codec.roundtrip_tensors_relative). The plan object (pinned plan, device copy, the maxima) is cached per
        (slot, rel_bits, maxprec, device) under the encoders' idleness rule, so a list that stays where it is plans
        once. Returns the tensors."""
        from . import codec
        tensors = list(tensors)
        self._tick += 1
        dev = tensors[0].device if tensors else None
        key = (slot, int(rel_bits), int(maxprec), dev, "relative")
        ent = self._enc.get(key)
        if ent is None:
            ent = self._enc[key] = [codec.TensorListRelative(rel_bits, maxprec), self._tick]
        else:
            ent[1] = self._tick
            self._enc.move_to_end(key)
        self._evict_idle()
        return ent[0](tensors)

    def roundtrip_fitted_per_tensor(self, tensors, bits_per_value: float, maxprec: int = 64, slot=None):
        """Every tensor of the list round-tripped in place under its own bit budget of floor(bits_per_value * n_s)
        bits, fitted on the device (codec.TensorListFittedPerTensor: tables, fits, round trip, no host read). The plan
        object (pinned plan, device copy, tables, records, budgets) is cached per (slot, bits_per_value, maxprec,
        device) under the encoders' idleness rule, so a list that stays where it is plans once. Returns the plan
        object (`fits`, `bits`, `tables`)."""
        from . import codec
        tensors = list(tensors)
        dev = tensors[0].device if tensors else None
        key = (slot, float(bits_per_value), int(maxprec), dev, "fitted_per_tensor")
        plan = self._cached(key, lambda: codec.TensorListFittedPerTensor(bits_per_value, maxprec))
        plan(tensors)
        return plan

    def rate_table(self, x: torch.Tensor, maxprec: int = 64, slot=None) -> torch.Tensor:
        """The rate table of the flattened bucket x (codec.RateTable): int64[288] on x's device, entry t the bits
        `encode` reports under expert(1, 16658, maxprec, -154 + t). The table and workspace are cached per (slot,
        numel, dtype, device) under the encoders' idleness rule; calls with the same key overwrite one table."""
        from . import codec
        x = x.reshape(-1)
        self._tick += 1
        key = (slot, x.numel(), x.dtype, x.device, "rate_table")
        ent = self._enc.get(key)
        if ent is None:
            ent = self._enc[key] = [codec.RateTable(x.numel(), x.dtype, x.device), self._tick]
        else:
            ent[1] = self._tick
            self._enc.move_to_end(key)
        self._evict_idle()
        return ent[0](x if x.is_contiguous() else x.contiguous(), maxprec)

    def rate_table_residual(self, x: torch.Tensor, err: torch.Tensor, maxprec: int = 64, slot=None) -> torch.Tensor:
        """The rate table of y = x + err, the array `encode_residual` codes (codec.rate_table_residual): entry t the
        bits `encode_residual(x, err, expert(1, 16658, maxprec, -154 + t))` reports. x and err are only read. Cached
        as `rate_table`'s, apart from them."""
        from . import codec
        x = x.reshape(-1)
        key = (slot, x.numel(), x.dtype, x.device, "rate_table_residual")
        rt = self._cached(key, lambda: codec.RateTable(x.numel(), x.dtype, x.device))
        return rt(x if x.is_contiguous() else x.contiguous(), maxprec, err=err)

    def _cached(self, key, make):
        self._tick += 1
        ent = self._enc.get(key)
        if ent is None:
            ent = self._enc[key] = [make(), self._tick]
        else:
            ent[1] = self._tick
            self._enc.move_to_end(key)
        self._evict_idle()
        return ent[0]

    def fit_device(self, table: torch.Tensor, budget_bits: int, slot=None) -> torch.Tensor:
        """The fit of a device rate table against budget_bits, on the device (codec.fit_device): -> the gcow_fit
        record, int64[2] on the table's device (codec.read_fit reads it on the host). No host read. The record is
        cached per (slot, device) under the encoders' idleness rule; calls with the same key overwrite one record."""
        from . import codec
        rec = self._cached((slot, table.device, "fit"), lambda: codec.new_fit_record(table.device))
        return codec.fit_device(table, budget_bits, out=rec)

    def encode_fitted(self, x: torch.Tensor, minexp_word: torch.Tensor, maxprec: int = 64, index_stride: int = 0,
                      slot=None):
        """`encode` under expert(1, 16658, maxprec, minexp) with minexp read on the device from minexp_word (a
        fit_device record) when the kernels run (codec.encode_fitted_device): -> (words, bits, index). Output buffers
        cached per slot like the encoders', apart from theirs."""
        from . import codec
        x = x.reshape(-1)
        key = (slot, x.numel(), x.dtype, x.device, int(maxprec), index_stride, "fitted")
        enc = self._cached(key, lambda: codec.Encoder((x.numel(),), x.dtype, codec.fitted_params(maxprec, 0),
                                                      x.device, index_stride))
        e = codec._encode_fitted_into(enc, x if x.is_contiguous() else x.contiguous(), minexp_word)
        return e.words, e.bits_dev, e.index

    def encode_residual_fitted(self, x: torch.Tensor, err: torch.Tensor, minexp_word: torch.Tensor, maxprec: int = 64,
                               index_stride: int = 0, slot=None):
        """`encode_residual` under the set minexp_word stands for, read on the device
        (codec.encode_residual_fitted_device): -> (words, bits, index), `err` updated in place. Output buffers cached
        per slot like `encode_fitted`'s, apart from theirs."""
        from . import codec
        x = x.reshape(-1)
        key = (slot, x.numel(), x.dtype, x.device, int(maxprec), index_stride, "fitted", "residual")
        enc = self._cached(key, lambda: codec.Encoder((x.numel(),), torch.float32, codec.fitted_params(maxprec, 0),
                                                      x.device, index_stride))
        e = codec._encode_residual_fitted_into(enc, x if x.is_contiguous() else x.contiguous(), err, minexp_word)
        return e.words, e.bits_dev, e.index

    def roundtrip_fitted(self, x: torch.Tensor, minexp_word: torch.Tensor, maxprec: int = 64, out=None):
        """`roundtrip` under the set minexp_word stands for, read on the device (codec.roundtrip_fitted): nothing
        cached, nothing allocated when `out` is given (out=x: in place)."""
        from . import codec
        return codec.roundtrip_fitted(x, minexp_word, maxprec, out=out)

    def encode_per_tensor(self, x: torch.Tensor, counts, bits_per_value: float, maxprec: int = 64,
                          index_stride: int = 0, slot=None):
        """The bucket x (contiguous 1-D, its tensors `counts` values each, in order) encoded with a bit budget per
        tensor, fitted on the device (codec.PerTensorFittedEncoder: per-tensor tables, batch fit, segmented encode; no
        host read): -> (words, bits, index, fits), fits the int64[S, 2] gcow_fit records a receiver decodes under.
        Cached per (slot, counts, dtype, device, budget, maxprec, index stride) like the encoders."""
        from . import codec
        counts = tuple(int(c) for c in counts)
        key = (slot, counts, x.dtype, x.device, float(bits_per_value), int(maxprec), index_stride, "per_tensor")
        enc = self._cached(key, lambda: codec.PerTensorFittedEncoder(bits_per_value, maxprec))
        e, fits = enc(x, counts, index_stride)
        return e.words, e.bits_dev, e.index, fits

    def encode_residual_per_tensor(self, x: torch.Tensor, err: torch.Tensor, counts, bits_per_value: float,
                                   maxprec: int = 64, index_stride: int = 0, slot=None):
        """`encode_per_tensor` with error feedback (codec.PerTensorFittedResidualEncoder: the per-tensor tables of
        y = x + err, batch fit, segmented residual encode; no host read): -> (words, bits, index, fits), `err`
        (fp32, parallel to x) updated in place with each tensor's y - decode(y) under its own fit. Cached per slot like
        `encode_per_tensor`, in buffers apart from that method's."""
        from . import codec
        counts = tuple(int(c) for c in counts)
        key = (slot, counts, x.dtype, x.device, float(bits_per_value), int(maxprec), index_stride, "per_tensor",
               "residual")
        enc = self._cached(key, lambda: codec.PerTensorFittedResidualEncoder(bits_per_value, maxprec))
        e, fits = enc(x, err, counts, index_stride)
        return e.words, e.bits_dev, e.index, fits

    def encode_relative(self, x: torch.Tensor, counts, rel_bits: int, maxprec: int = 64, index_stride: int = 0,
                        slot=None):
        """The bucket x (contiguous 1-D, its tensors `counts` values each, in order) encoded under a tolerance of
        2^-rel_bits of each tensor's own largest magnitude (codec.PerTensorRelativeEncoder: the words pass, then the
        segmented encode; no host read): -> (words, bits, index, minexp_words), minexp_words the int32[S] words a
        receiver decodes under (decode_mean_per_tensor takes them as `fits`). Cached per (slot, counts, dtype, device,
        rel_bits, maxprec, index stride) like the encoders."""
        from . import codec
        counts = tuple(int(c) for c in counts)
        key = (slot, counts, x.dtype, x.device, int(rel_bits), int(maxprec), index_stride, "relative_wire")
        enc = self._cached(key, lambda: codec.PerTensorRelativeEncoder(rel_bits, maxprec))
        e, words = enc(x, counts, index_stride)
        return e.words, e.bits_dev, e.index, words

    def encode_residual_relative(self, x: torch.Tensor, err: torch.Tensor, counts, rel_bits: int, maxprec: int = 64,
                                 index_stride: int = 0, slot=None):
        """`encode_relative` with error feedback (codec.PerTensorRelativeResidualEncoder: the words of y = x + err,
        then the segmented residual encode under them; no host read): -> (words, bits, index, minexp_words), `err`
        (fp32, parallel to x) updated in place with each tensor's y - decode(y) under its own word. Cached per slot
        like `encode_relative`, in buffers apart from that method's."""
        from . import codec
        counts = tuple(int(c) for c in counts)
        key = (slot, counts, x.dtype, x.device, int(rel_bits), int(maxprec), index_stride, "relative_wire", "residual")
        enc = self._cached(key, lambda: codec.PerTensorRelativeResidualEncoder(rel_bits, maxprec))
        e, words = enc(x, err, counts, index_stride)
        return e.words, e.bits_dev, e.index, words

    def decode_mean_per_tensor(self, streams, stream_words: int, nstreams: int, counts, fits, maxprec: int = 64,
                               index=None, index_words: int = 0, index_stride: int = 16, out=None, slot=None):
        """The mean of nstreams segmented streams of one shape, each tensor under its stream's own fit
        (codec.decode_mean_segmented): fits is one set (int64[S, 2] records or int32[S] words) or one per stream
        (int64[W, S, 2] / int32[W, S]). The plan is cached per (slot, counts, dtype, device)."""
        from . import codec
        counts = tuple(int(c) for c in counts)
        dtype = out.dtype if out is not None else torch.float32
        key = (slot, counts, dtype, streams.device, "segment_plan")
        plan = self._cached(key, lambda: codec.SegmentPlan(counts, dtype, streams.device))
        return codec.decode_mean_segmented(streams, stream_words, nstreams, counts, fits, maxprec, index, index_words,
                                           index_stride, dtype, out, plan=plan)

    def pack_index16(self, index8, n: int, params):
        from . import codec
        return codec.pack_index16(index8, n, params)

    def decode_mean(self, streams, stream_words: int, nstreams: int, n: int, params, index=None,
                    index_words: int = 0, index_stride: int = 0, out=None):
        from . import codec
        return codec.decode_mean(streams, stream_words, nstreams, n, params, index, index_words, index_stride, out)


_DEVICE = None


def device_codec() -> DeviceCodec:
    global _DEVICE
    if _DEVICE is None:
        _DEVICE = DeviceCodec()
    return _DEVICE


def shard_bounds(nvals: int, world: int, rank: int, block: int = 4, align_blocks: int = 16):
    """Contiguous block-aligned shard [lo, hi) of a 1-D bucket of nvals values for `rank`. align_blocks = 16 makes
    every full shard end on a 64-bit stream boundary at any rate with 4 * rate integral. Small buckets leave the last
    ranks an empty shard (lo == hi == nvals); they still take part in every collective."""
    nblocks = (nvals + block - 1) // block
    per = (nblocks + world - 1) // world
    per = (per + align_blocks - 1) // align_blocks * align_blocks
    lo_b = min(per * rank, nblocks)
    hi_b = min(lo_b + per, nblocks)
    return min(lo_b * block, nvals), min(hi_b * block, nvals)


def is_nccl(group=None) -> bool:
    return dist.get_backend(group) == "nccl"


def allgather_into(out: torch.Tensor, local: torch.Tensor, group=None):
    """out = concat over ranks of `local` (equal sizes): one all_gather_into_tensor on RCCL, a list all_gather on
    gloo."""
    if is_nccl(group):
        dist.all_gather_into_tensor(out, local, group=group)
    else:
        world = dist.get_world_size(group)
        dist.all_gather(list(out.chunk(world)), local, group=group)
    return out


def allgather_into_async(out: torch.Tensor, local: torch.Tensor, group=None) -> torch.futures.Future:
    """allgather_into with async_op=True: -> the collective's Future (RCCL: completed once enqueued, its waiters
    synchronise on the collective's stream; gloo: completed when the data has arrived)."""
    if is_nccl(group):
        work = dist.all_gather_into_tensor(out, local, group=group, async_op=True)
    else:
        world = dist.get_world_size(group)
        work = dist.all_gather(list(out.chunk(world)), local, group=group, async_op=True)
    return work.get_future()


def allgather_fixed(words: torch.Tensor, nblocks: int, maxbits: int, group=None) -> torch.Tensor:
    """All-gather equal-size fixed-rate shard streams (each shard nblocks blocks of maxbits bits)."""
    if (nblocks * maxbits) % 64:
        raise GcowError("fixed-rate shard must end on a 64-bit boundary (shard blocks * maxbits % 64 == 0)")
    nw = nblocks * maxbits // 64
    local = words[:nw].contiguous()
    world = dist.get_world_size(group)
    out = torch.empty(world * nw, dtype=torch.int64, device=local.device)
    allgather_into(out, local, group)
    return out


def gather_lengths(bits, device, group=None):
    """All-gather one unflushed bit count per rank (an int or an int64[1] tensor): -> (device tensor, host list)."""
    world = dist.get_world_size(group)
    mine = bits.reshape(1).to(device=device, dtype=torch.int64) if isinstance(bits, torch.Tensor) else \
        torch.tensor([int(bits)], dtype=torch.int64, device=device)
    lens = torch.empty(world, dtype=torch.int64, device=device)
    allgather_into(lens, mine, group)
    return lens, [int(v) for v in lens.tolist()]  # the one host read: it sizes the padded buffers


def allgather_padded(words: torch.Tensor, nw: int, maxw: int, group=None, pad: int = 0) -> torch.Tensor:
    """All-gather each rank's first nw words padded with zeros to maxw: -> world * maxw (+ pad zero) words."""
    world = dist.get_world_size(group)
    local = torch.zeros(maxw, dtype=torch.int64, device=words.device)
    if nw:
        local[:nw] = words[:nw]
    out = torch.zeros(world * maxw + pad, dtype=torch.int64, device=words.device)
    allgather_into(out[: world * maxw], local, group)
    return out


def allgather_variable(words: torch.Tensor, bits, group=None, codec=None):
    """All-gather variable-rate shard streams and stitch them into one stream. `bits`: this rank's unflushed bit
    count (int or int64[1] tensor on words' device). Returns (words, total_bits)."""
    codec = codec or device_codec()
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    lens, lens_h = gather_lengths(bits, words.device, group)
    maxw = max(1, max((b + 63) // 64 for b in lens_h))
    gathered = allgather_padded(words, (lens_h[rank] + 63) // 64, maxw, group)
    total = sum(lens_h)
    out = torch.empty(max((total + 63) // 64, 1), dtype=torch.int64, device=words.device)
    codec.stitch_shards(out, gathered, maxw, lens, world)
    return out[: (total + 63) // 64], total


def encode_allgather(bucket: torch.Tensor, params, group=None, codec=None):
    """Encode this rank's contiguous shard of a 1-D bucket (replicated on every rank: the C4 layout) and rebuild the
    full stream on every rank. Returns (words, total_bits). A rank whose shard is empty (small buckets) joins the
    exchange with zero bits instead of encoding."""
    codec = codec or device_codec()
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    bounds = [shard_bounds(bucket.numel(), world, r) for r in range(world)]
    lo, hi = bounds[rank]
    fixed = params.minbits == params.maxbits
    if hi > lo:
        words, bits, _ = codec.encode(bucket[lo:hi], params)
    else:
        words, bits = torch.zeros(1, dtype=torch.int64, device=bucket.device), 0
    sizes = {b - a for a, b in bounds}
    nb = (hi - lo + 3) // 4
    if fixed and len(sizes) == 1 and (hi - lo) % 4 == 0 and (nb * params.maxbits) % 64 == 0:
        out = allgather_fixed(words, nb, params.maxbits, group)
        return out, world * nb * params.maxbits
    if fixed:  # ragged shards: the bit counts are known on the host
        bits = nb * params.maxbits
    return allgather_variable(words, bits, group, codec)


# ---------------------------------------------------------------------------------------------- sharded receive
# The receive side of the compressed DDP exchange without decoding every rank's whole stream on every rank: rank r
# owns one block-aligned shard of the bucket. Every rank cuts its own stream at the shard boundaries (fixed rate: at
# b * maxbits; variable rate: at the block index), sends piece r to rank r (one all-to-all), rank r decodes and
# averages the W pieces of its shard (gcow_decode_mean_device on W "streams" of one shard -- the same per-value
# arithmetic, in the same rank order, as decoding the whole streams), and one all-gather of the mean shards rebuilds
# the bucket on every rank. Per rank, against all-gathering the streams and decoding them all: (W - 1) / W of ONE
# stream received instead of W - 1 streams, 1 / W of the decode work, plus the all-gather of the mean (fp32 / bf16).
SHARD_ALIGN_BLOCKS = 64  # shard starts on 64-block multiples: a whole 16-block index chunk, and 64 maxbits % 64 == 0


def shard_plan(nvals: int, world: int):
    """Block-aligned shards [lo, hi) (values) of a 1-D bucket for every rank, and the values in a full shard."""
    bounds = [shard_bounds(nvals, world, r, align_blocks=SHARD_ALIGN_BLOCKS) for r in range(world)]
    per = max(hi - lo for lo, hi in bounds)
    return bounds, per


def alltoall_into(out: torch.Tensor, inp: torch.Tensor, group=None):
    """Equal-split all-to-all: chunk r of `inp` to rank r, chunk s of `out` from rank s."""
    dist.all_to_all_single(out, inp, group=group)
    return out


def shard_pieces_fixed(words: torch.Tensor, nvals: int, maxbits: int, group=None):
    """Fixed rate: this rank's stream cut at the shard boundaries and exchanged. Returns (pieces, piece_words, lo,
    hi): pieces holds rank s's piece of this rank's shard at s * piece_words (+ 2 zero words), [lo, hi) the shard."""
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    bounds, _ = shard_plan(nvals, world)
    nb = (nvals + 3) // 4
    # piece r = the words holding shard r's blocks: from the word its first block starts in (a 64-block multiple of
    # maxbits bits is whole words) to the word its last bit falls in -- a partial last block and a shard whose bits
    # are not a multiple of 64 (the last shard, or a one-shard bucket) end inside a word that must travel too
    spans = [((lo // 4) * maxbits // 64, (min((hi + 3) // 4, nb) * maxbits + 63) // 64) if hi > lo else (0, 0)
             for lo, hi in bounds]
    pw = max(1, max(w1 - w0 for w0, w1 in spans))
    send = torch.zeros(world * pw, dtype=torch.int64, device=words.device)
    for r, (w0, w1) in enumerate(spans):
        if w1 > w0:
            send[r * pw:r * pw + (w1 - w0)] = words[w0:w1]
    pieces = torch.zeros(world * pw + 2, dtype=torch.int64, device=words.device)
    alltoall_into(pieces[: world * pw], send, group)
    lo, hi = bounds[rank]
    return pieces, pw, lo, hi


def shard_pieces_variable(words: torch.Tensor, bits, index: torch.Tensor, nvals: int, index_stride: int = 16,
                          group=None):
    """Variable rate (block index every `index_stride` blocks): this rank's stream cut at the shard boundaries (the
    bit where each shard's first block starts, from the index), every piece starting at the stream word that holds
    its first bit, and its index entries rebased to that word. One all-gather of every rank's W + 1 cut positions
    (the host read that sizes the padded pieces), then two all-to-alls (words, index). Returns (pieces, piece_words,
    pidx, pidx_words, lo, hi): rank s's piece of this rank's shard at s * piece_words (+ 2 zero words) with its index
    at s * pidx_words."""
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    bounds, per = shard_plan(nvals, world)
    dev = words.device
    nb = (nvals + 3) // 4
    if index_stride not in (8, 16):  # the block-index spacings gcow_decode_mean_device takes
        raise GcowError("shard_pieces_variable: index_stride must be 8 or 16, got %r" % (index_stride,))
    starts = [lo // 4 // index_stride for lo, _ in bounds]  # index chunk of each shard's first block
    bits_t = bits.reshape(1).to(device=dev, dtype=torch.int64) if isinstance(bits, torch.Tensor) else \
        torch.tensor([int(bits)], dtype=torch.int64, device=dev)
    cut = torch.empty(world + 1, dtype=torch.int64, device=dev)
    # an empty shard (lo = hi = nvals) starts at the stream's end; nvals need not be a block multiple, so the test is
    # on the shard, not on lo's block (a bucket with a partial last block and empty shards lost its last piece)
    for r, (lo, hi) in enumerate(bounds):
        if hi > lo:
            cut[r:r + 1] = index[starts[r]:starts[r] + 1]
        else:
            cut[r:r + 1] = bits_t
    cut[world:] = bits_t
    allcuts = torch.empty(world * (world + 1), dtype=torch.int64, device=dev)
    allgather_into(allcuts, cut, group)
    C_h = [int(v) for v in allcuts.tolist()]  # the one host read: sizes the padded pieces
    def span(c0, c1):
        return (c0 >> 6, (c1 + 63) >> 6 if c1 > c0 else c0 >> 6)
    pw = 1
    for s in range(world):
        cs = C_h[s * (world + 1):(s + 1) * (world + 1)]
        for r in range(world):
            a, b = span(cs[r], cs[r + 1])
            pw = max(pw, b - a)
    mine = C_h[rank * (world + 1):(rank + 1) * (world + 1)]
    nchunk = [(min((hi + 3) // 4, nb) - lo // 4 + index_stride - 1) // index_stride if hi > lo else 0
              for lo, hi in bounds]
    iw = max(1, max(nchunk))
    send = torch.zeros(world * pw, dtype=torch.int64, device=dev)
    isend = torch.zeros(world * iw, dtype=torch.int64, device=dev)
    for r in range(world):
        a, b = span(mine[r], mine[r + 1])
        if b > a:
            send[r * pw:r * pw + (b - a)] = words[a:b]
        if nchunk[r]:
            isend[r * iw:r * iw + nchunk[r]] = index[starts[r]:starts[r] + nchunk[r]] - 64 * a
    pieces = torch.zeros(world * pw + 2, dtype=torch.int64, device=dev)
    alltoall_into(pieces[: world * pw], send, group)
    pidx = torch.empty(world * iw, dtype=torch.int64, device=dev)
    alltoall_into(pidx, isend, group)
    lo, hi = bounds[rank]
    return pieces, pw, pidx, iw, lo, hi


MEAN_INDEX_STRIDE = 16  # block index spacing of a variable-rate mean shard's stream (allgather_mean_streams)


def mean_stream_plan(nvals: int, world: int, maxbits: int):
    """Fixed rate: the words every rank contributes to allgather_mean_streams -- a full shard's stream (a 64-block
    multiple: whole words), or the whole bucket's flushed stream when it is shorter than one full shard."""
    nb = (nvals + 3) // 4
    per_b = ((nb + world - 1) // world + SHARD_ALIGN_BLOCKS - 1) // SHARD_ALIGN_BLOCKS * SHARD_ALIGN_BLOCKS
    return (min(per_b, nb) * maxbits + 63) // 64


def allgather_mean_streams(flat: torch.Tensor, words, bits, index, nvals: int, params, group=None, codec=None):
    """The sharded exchange's second stage with the mean compressed: every rank contributes the stream of its mean
    shard (`words`, `bits`, and at variable rate `index` every MEAN_INDEX_STRIDE blocks, as `encode` returns them for
    the shard's values; ignored on a rank whose shard is empty), and `flat` (the bucket, n values, any dtype) receives
    the decode of every shard's stream -- the owner's own included, so every rank ends with the same bits.
    Fixed rate: each stream zero-padded to mean_stream_plan words, one all-gather; the gathered buffer is the
    fixed-rate stream of the whole mean bucket and one decode of n values writes every shard. Variable rate:
    gather_lengths (the one host read), allgather_padded of the streams (padded to an even word count: every shard's
    stream starts 16-byte aligned), one all-gather of the indexes padded to a full shard's entry count, then one
    decode per non-empty shard. A bf16 bucket receives the fp32 decode rounded to nearest even; other dtypes and
    non-contiguous buckets go through an fp32 temporary. Ranks with empty shards join every collective with zero
    words."""
    codec = codec or device_codec()
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    bounds, _ = shard_plan(nvals, world)
    lo, hi = bounds[rank]
    dev = flat.device
    direct = flat.dtype in (torch.float32, torch.bfloat16) and flat.is_contiguous()
    out = flat if direct else torch.empty(nvals, dtype=torch.float32, device=dev)
    nb = (nvals + 3) // 4
    if params.minbits == params.maxbits:
        pw = mean_stream_plan(nvals, world, params.maxbits)
        local = torch.zeros(max(pw, 1), dtype=torch.int64, device=dev)
        nw = ((hi - lo + 3) // 4 * params.maxbits + 63) // 64
        if nw:
            local[:nw] = words[:nw]
        gathered = torch.zeros(world * local.numel() + 2, dtype=torch.int64, device=dev)  # + the decoders' slack
        allgather_into(gathered[: world * local.numel()], local, group)
        if nvals:
            codec.decode(gathered, nvals, params, out=out)
    else:
        lens, lens_h = gather_lengths(bits if hi > lo else 0, dev, group)
        maxw = max(2, (max((b + 63) // 64 for b in lens_h) + 1) // 2 * 2)
        mine = words if hi > lo else torch.zeros(1, dtype=torch.int64, device=dev)
        gathered = allgather_padded(mine, (lens_h[rank] + 63) // 64, maxw, group, pad=2)
        per_b = max((b - a + 3) // 4 for a, b in bounds)
        ni = max(1, (min(per_b, nb) + MEAN_INDEX_STRIDE - 1) // MEAN_INDEX_STRIDE)
        nchunk = [((b - a + 3) // 4 + MEAN_INDEX_STRIDE - 1) // MEAN_INDEX_STRIDE for a, b in bounds]
        imine = torch.zeros(ni, dtype=torch.int64, device=dev)
        if nchunk[rank]:
            imine[: nchunk[rank]] = index[: nchunk[rank]]
        idx = torch.empty(world * ni, dtype=torch.int64, device=dev)
        allgather_into(idx, imine, group)
        for r, (a, b) in enumerate(bounds):
            if b > a:
                codec.decode(gathered[r * maxw:(r + 1) * maxw + 2], b - a, params, index=idx[r * ni:r * ni + nchunk[r]],
                             index_stride=MEAN_INDEX_STRIDE, out=out[a:b])
    if not direct:
        flat.copy_(out.to(flat.dtype))
    return flat


def allgather_shards(flat: torch.Tensor, shard: torch.Tensor, nvals: int, group=None):
    """Every rank's decoded shard (shard_plan bounds; `shard` = this rank's values) gathered into `flat` (n values,
    the bucket, any dtype)."""
    world = dist.get_world_size(group)
    _, per = shard_plan(nvals, world)
    mine = torch.zeros(per, dtype=flat.dtype, device=flat.device)
    mine[: shard.numel()] = shard
    if flat.is_contiguous() and flat.numel() == world * per:
        allgather_into(flat, mine, group)  # straight into the bucket
    else:
        full = torch.empty(world * per, dtype=flat.dtype, device=flat.device)
        allgather_into(full, mine, group)
        flat.copy_(full[: flat.numel()])
    return flat
