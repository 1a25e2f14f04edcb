"""compressed_sharded_hook with `compress_mean` on the CPU: the hook runs exactly as written over gloo with the
oracle-backed codec of tests/mean_codec.py injected. Every rank's bucket must equal, bit for bit, the model's
decode(encode(mean shard)) of every shard (the mean = the fp32 sum, in rank order, of the oracle's per-rank decodes,
divided by the world size), and the second stage's collectives must carry int64 stream words of exactly the planned
count -- never the fp32 mean."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist

from test_dist_cpu import _Bucket, _init, _run

SIZES = [10, 29, 255, 3 * 256 + 5, 2 * 256]  # ragged shards, empty shards, a partial last block
MODES = ["rate16", "rate8", "acc1e-3"]


def _modes():
    from gcow_amd import codec
    return {"rate16": codec.rate(16, 1), "rate8": codec.rate(8, 1), "acc1e-3": codec.accuracy(1e-3)}


def _grad(step, rank, n):
    from oracle import oracle as O
    return O.gen_normal(n, 1e-3, 5000 + 64 * step + rank, True)


def _bounds(n, world):
    from gcow_amd import dist as gdist
    return gdist.shard_plan(n, world)[0]


def _first_stage_mean(O, grads, errs, op):
    """The mean the first stage forms: with errs (a list, updated in place) the per-rank error feedback model."""
    from mean_codec import mean_of
    from residual_model import model_step
    decs = []
    for r, g in enumerate(grads):
        if errs is None:
            decs.append(O.decompress(O.compress(g, op)[0], g.shape, op))
        else:
            _, _, _, d, errs[r] = model_step(g, errs[r], op)
            decs.append(d)
    return mean_of(decs)


def _expected_second_stage(O, m, n, world, mp):
    """-> (bucket every rank must hold, per-shard stream bit counts)."""
    want = np.zeros(n, np.float32)
    bits = []
    for lo, hi in _bounds(n, world):
        if hi > lo:
            w, b = O.compress(m[lo:hi], mp)
            want[lo:hi] = O.decompress(w, (hi - lo,), mp)
            bits.append(b)
        else:
            bits.append(0)
    return want, bits


def _planned_gathers(n, world, p, bits):
    """numel of each rank's contribution to the second stage's all-gathers, derived here from the shard layout (a
    full shard is a 64-block multiple) and the model's stream lengths, not from the code under test."""
    nb = (n + 3) // 4
    per_b = ((nb + world - 1) // world + 63) // 64 * 64
    if p.minbits == p.maxbits:
        return [(min(per_b, nb) * p.maxbits + 63) // 64]
    maxw = max(2, (max((b + 63) // 64 for b in bits) + 1) // 2 * 2)  # even: shard streams start 16-byte aligned
    return [1, maxw, max(1, (min(per_b, nb) + 15) // 16)]  # the lengths, the streams, the indexes every 16 blocks


class _GatherLog:
    """Wraps gcow_amd.dist.allgather_into: records (dtype, numel) of every contribution."""

    def __init__(self, gdist):
        self.calls = []
        self.inner = gdist.allgather_into

    def __call__(self, out, local, group=None):
        self.calls.append((local.dtype, int(local.numel())))
        return self.inner(out, local, group)


def _check_case(O, ddp, gdist, state, log, rank, world, n, case):
    """One hook call on a fresh bucket index; returns an error string or None."""
    p = state.params
    op = O.expert(*p.tuple())
    grads = [_grad(0, r, n) for r in range(world)]
    m = _first_stage_mean(O, grads, None, op)
    want, bits = _expected_second_stage(O, m, n, world, op)
    del log.calls[:]
    nrec = len(state.codec.records)
    g = torch.from_numpy(grads[rank].copy())
    out = ddp.compressed_sharded_hook(state, _Bucket(g, case)).wait()
    out = out[0] if isinstance(out, (list, tuple)) else out
    if not np.array_equal(out.numpy().view(np.uint32), want.view(np.uint32)):
        return "n=%d: bucket != decode(encode(mean shard)) of the model" % n
    if world > 1 and n > 64 and np.array_equal(want.view(np.uint32), m.view(np.uint32)):  # world 1: idempotent
        return "n=%d: the coded mean equals the mean: the test shows nothing" % n
    if any(dt != torch.int64 for dt, _ in log.calls):
        return "n=%d: a non-int64 tensor was all-gathered: %r" % (n, log.calls)
    plan = _planned_gathers(n, world, p, bits)
    if [k for _, k in log.calls[-len(plan):]] != plan:
        return "n=%d: second-stage all-gathers %r, planned %r" % (n, log.calls, plan)
    recs = state.codec.records[nrec:]
    decs = [r for r in recs if r[0] == "decode"]
    lo, hi = _bounds(n, world)[rank]
    if p.minbits == p.maxbits:
        if [(r[1], r[2], r[3]) for r in decs] != [(world * plan[0] + 2, torch.int64, n)]:
            return "n=%d: fixed rate decodes the gathered stream once: %r" % (n, decs)
    else:
        sizes = [b - a for a, b in _bounds(n, world) if b > a]
        if [r[3] for r in decs] != sizes or any(r[2] != torch.int64 for r in decs):
            return "n=%d: one decode per non-empty shard: %r" % (n, decs)
    owner = [r for r in recs if r[0] == "decode_mean_encode"]
    if len(owner) != (1 if hi > lo else 0):
        return "n=%d: decode_mean_encode calls %r for shard [%d, %d)" % (n, owner, lo, hi)
    if any(r[0] == "decode_mean" and r[2].size != hi - lo for r in recs):
        return "n=%d: decode_mean of something other than this rank's shard" % n
    return None


def _run_cases(rank, world, codec_cls="OracleMeanCodec"):
    import mean_codec
    from gcow_amd import ddp
    from gcow_amd import dist as gdist
    from oracle import oracle as O
    log = _GatherLog(gdist)
    gdist.allgather_into = log
    try:
        case = 0
        for mode in MODES:
            state = ddp.make_hook_state(hook=ddp.compressed_sharded_hook, params=_modes()[mode],
                                        codec=getattr(mean_codec, codec_cls)(), compress_mean=True)
            for n in SIZES:
                bad = _check_case(O, ddp, gdist, state, log, rank, world, n, case)
                case += 1
                if bad:
                    return "%s world %d rank %d %s" % (mode, world, rank, bad)
    finally:
        gdist.allgather_into = log.inner
    return None


def _hook_worker(rank, world, port, q):
    _init(rank, world, port)
    try:
        bad = _run_cases(rank, world)
        q.put((rank, True if bad is None else bad))
    except Exception as ex:  # pragma: no cover - reported through the queue
        q.put((rank, repr(ex)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_compress_mean_hook_gloo(world):
    """Every size and mode in one set of processes (the cases are tiny; starting the ranks is what takes time)."""
    _run(_hook_worker, world)


@pytest.fixture
def gloo_world1():
    tests = os.path.dirname(os.path.abspath(__file__))
    if tests not in sys.path:
        sys.path.insert(0, tests)
    dist.init_process_group("gloo", store=dist.HashStore(), rank=0, world_size=1)
    yield
    dist.destroy_process_group()


def test_compress_mean_hook_world1(orc, gloo_world1):
    assert _run_cases(0, 1) is None


# ---------------------------------------------------------------------------------------------- error feedback
def _ef_worker(rank, world, port, q):
    _init(rank, world, port)
    try:
        from gcow_amd import ddp
        from mean_codec import OracleMeanCodec
        from oracle import oracle as O
        from residual_model import model_step
        n = 3 * 256 + 5
        bounds = _bounds(n, world)
        lo, hi = bounds[rank]
        bad = None
        for mode in ("rate16", "acc1e-3"):
            p = _modes()[mode]
            op = O.expert(*p.tuple())
            state = ddp.make_hook_state(hook=ddp.compressed_sharded_hook, params=p, codec=OracleMeanCodec(),
                                        compress_mean=True, error_feedback=True)
            errs = [None] * world                 # first stage: every rank's carried error of its bucket
            e2 = [None] * world                   # second stage: every owner's carried error of its mean shard
            sum_hat = np.zeros(hi - lo, np.float32)   # of the hook's outputs on this rank's shard
            sum_model = np.zeros(hi - lo, np.float32)  # the same sums over the model's decodes
            sum_m = np.zeros(hi - lo, np.float64)
            ymax = 0.0
            for step in range(2):
                grads = [_grad(step, r, n) for r in range(world)]
                m = _first_stage_mean(O, grads, errs, op)
                want = np.zeros(n, np.float32)
                for r, (a, b) in enumerate(bounds):
                    y, _, _, d, e2[r] = model_step(m[a:b], e2[r], op)
                    want[a:b] = d
                    if r == rank:
                        ymax = max(ymax, float(np.abs(y).max()))
                out = ddp.compressed_sharded_hook(state, _Bucket(torch.from_numpy(grads[rank].copy()), 0)).wait()
                out = (out[0] if isinstance(out, (list, tuple)) else out).numpy()
                if not np.array_equal(out.view(np.uint32), want.view(np.uint32)):
                    bad = bad or "%s step %d: bucket != the model's" % (mode, step)
                got1 = state.error_buffer(0, torch.from_numpy(grads[rank])).numpy()
                got2 = state.mean_error_buffer(0, hi - lo, torch.device("cpu")).numpy()
                if not np.array_equal(got1.view(np.uint32), errs[rank].view(np.uint32)):
                    bad = bad or "%s step %d: the bucket's carried error != the model's" % (mode, step)
                if not np.array_equal(got2.view(np.uint32), e2[rank].view(np.uint32)):
                    bad = bad or "%s step %d: the mean shard's carried error != the model's" % (mode, step)
                sum_hat = sum_hat + out[lo:hi]
                sum_model = sum_model + want[lo:hi]
                sum_m += m[lo:hi]
            if not np.any(e2[rank]):
                bad = bad or "%s: the model's second error is all zero: the test shows nothing" % mode
            if set(k for k in state._errors) != {0, (0, "mean", hi - lo)}:
                bad = bad or "%s: error buffers %r" % (mode, list(state._errors))
            # telescoping on the owner's shard, e_0 = 0: sum_t yhat_t = sum_t m_t - e_2. The hook's side and the
            # model's side agree in their fp32 bit patterns (the model reproduces every rounding); against the exact
            # sums the identity holds up to the two fp32 roundings per step (y = fl(m + e), r = fl(y - yhat), each
            # within 2^-24 relative of values bounded by max|y|), as in test_residual_cpu.test_model_identity
            if not np.array_equal(sum_hat.view(np.uint32), sum_model.view(np.uint32)):
                bad = bad or "%s: sum of the sent shards != the model's" % mode
            lhs = sum_model.astype(np.float64)
            rhs = sum_m - e2[rank].astype(np.float64)
            if np.abs(lhs - rhs).max() > 3 * 2.0 ** -23 * ymax:  # 2 steps, and the fp32 sum of the two yhat
                bad = bad or "%s: telescoping identity off by %g" % (mode, np.abs(lhs - rhs).max())
            state.reset_error_feedback()
            if state._errors:
                bad = bad or "reset_error_feedback left %r" % list(state._errors)
        q.put((rank, True if bad is None else bad))
    except Exception as ex:  # pragma: no cover - reported through the queue
        q.put((rank, repr(ex)))
    finally:
        dist.destroy_process_group()


def test_compress_mean_error_feedback_two_steps():
    _run(_ef_worker, 2)


# ---------------------------------------------------------------------------------------------- other checks
def test_codec_without_decode_mean_encode_gives_the_same_bucket(orc, gloo_world1):
    from mean_codec import OracleComposedCodec
    assert not hasattr(OracleComposedCodec(), "decode_mean_encode")
    from gcow_amd import ddp
    outs = {}
    for cls in ("OracleMeanCodec", "OracleComposedCodec"):
        import mean_codec
        for ef in (False, True):
            state = ddp.make_hook_state(hook=ddp.compressed_sharded_hook, params=_modes()["rate8"],
                                        codec=getattr(mean_codec, cls)(), compress_mean=True, error_feedback=ef)
            for step in range(2):
                g = torch.from_numpy(_grad(step, 0, 3 * 256 + 5).copy())
                out = ddp.compressed_sharded_hook(state, _Bucket(g, 0)).wait()
                outs[cls, ef, step] = (out[0] if isinstance(out, (list, tuple)) else out).numpy().copy()
            names = [r[0] for r in state.codec.records]
            assert ("decode_mean_encode" in names) == (cls == "OracleMeanCodec")
    for ef in (False, True):
        for step in range(2):
            a, b = outs["OracleMeanCodec", ef, step], outs["OracleComposedCodec", ef, step]
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert not np.array_equal(outs["OracleMeanCodec", True, 1], outs["OracleMeanCodec", False, 1])


def test_mean_params_select_the_second_stage_set(orc, gloo_world1):
    from gcow_amd import ddp
    from mean_codec import OracleMeanCodec
    p, mp = _modes()["rate16"], _modes()["rate8"]
    state = ddp.make_hook_state(hook=ddp.compressed_sharded_hook, params=p, mean_params=mp, codec=OracleMeanCodec(),
                                compress_mean=True)
    a = _grad(0, 0, 2 * 256)
    out = ddp.compressed_sharded_hook(state, _Bucket(torch.from_numpy(a.copy()), 0)).wait()
    op, omp = orc.expert(*p.tuple()), orc.expert(*mp.tuple())
    m = _first_stage_mean(orc, [a], None, op)
    want = orc.decompress(orc.compress(m, omp)[0], m.shape, omp)
    assert np.array_equal(out.numpy().view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("hook", ["roundtrip_hook", "compressed_allgather_hook"])
def test_other_hooks_refuse_compress_mean(hook):
    from gcow_amd import ddp
    state = ddp.GcowHookState(compress_mean=True)
    with pytest.raises(ValueError, match="compress_mean"):
        getattr(ddp, hook)(state, _Bucket(torch.zeros(16), 0))


def test_default_state_leaves_the_mean_uncompressed(orc, gloo_world1):
    from gcow_amd import ddp
    from mean_codec import OracleMeanCodec
    state = ddp.make_hook_state(hook=ddp.compressed_sharded_hook, codec=OracleMeanCodec())
    assert state.compress_mean is False and state.mean_params is None
    a = _grad(0, 0, 3 * 256 + 5)
    out = ddp.compressed_sharded_hook(state, _Bucket(torch.from_numpy(a.copy()), 0)).wait()
    op = orc.expert(*state.params.tuple())
    dec = orc.decompress(orc.compress(a, op)[0], a.shape, op)
    assert np.array_equal(out.numpy().view(np.uint32), ((np.zeros_like(dec) + dec) / np.float32(1)).view(np.uint32))
    names = [r[0] for r in state.codec.records]
    assert "decode_mean_encode" not in names and "decode" not in names  # the parent's exchange, unchanged


@pytest.mark.parametrize("nstreams", [1, 2, 3])
def test_gpu_case_inputs_reach_the_rare_lanes(orc, nstreams):
    """The oracle pipeline alone reproduces what the inputs of tests/test_gpu_mean_encode.py are built for: received
    words and coded words that the pair decoder's fast path hands to the generic decoder (tests/test_dec_pair_fastpath
    's model of it), a mean that overflows to Inf from two streams on (the coder's special lane, a zeroed residual),
    and subnormal residuals."""
    from test_dec_pair_fastpath import fast_pair
    from test_gpu_mean_encode import CHUNK, _case
    n = 12 * CHUNK + 5
    c = _case(n, nstreams, "rate16")
    received = c["streams"][: nstreams * c["sw"]]
    assert sum(1 for v in received.tolist() if fast_pair(int(v), True)[0]) >= 100 * nstreams
    w, _, e1 = c["steps"][0]
    assert sum(1 for v in w.tolist() if fast_pair(int(v), True)[0]) >= 100
    bad = ~np.isfinite(c["m"])
    assert not np.any(e1[bad]) and np.all(np.isfinite(e1))
    if nstreams > 1:  # one stream's decode is finite everywhere: nothing overflows
        assert bad.sum() >= 4 and np.any(np.isposinf(c["m"]))
    assert np.any((np.abs(e1) < np.finfo(np.float32).tiny) & (e1 != 0))
