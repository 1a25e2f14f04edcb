"""GcowHookState.target_bits (accuracy mode under a bit budget) on gloo process groups on the CPU, worlds 2 and 3.

The hooks run as written, with their codec calls injected: tests/oracle_codec.OracleCodec plus a rate_table made of
288 oracle encodes. Three steps on per-rank buckets of 1027 fp32 values (one seed per rank and step), both wire hooks:
every rank codes under the same set in every step; step 1 under state.params; step t + 1 under the fit of the sum over
ranks of step t's oracle tables against world budgets; and after each step the bucket is the mean of the oracle round
trips under that step's set. roundtrip_hook: the bucket is the oracle round trip under the fit of the reduced bucket's
table, whose stream is within the budget. The ValueError cases, and target_bits=None never asking for a table."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

from test_dist_cpu import _Bucket, _init, _run  # noqa: E402

N = 1027
TARGET = 6.0
BUDGET = int(TARGET * N)
MAXPREC = 24


def _codec_class():
    from oracle_codec import OracleCodec, _np_values

    import rate_table_inputs as RT

    class RateCodec(OracleCodec):
        """OracleCodec + rate_table through the oracle; `seen` keeps the parameter set of every encode."""

        def __init__(self, refuse=False):
            super().__init__()
            self.seen, self.tables, self.refuse = [], 0, refuse

        def encode(self, x, params, index_stride=0, slot=None):
            self.seen.append(params.tuple())
            return super().encode(x, params, index_stride, slot)

        def rate_table(self, x, maxprec=64, slot=None):
            if self.refuse:
                raise AssertionError("rate_table called without target_bits")
            self.tables += 1
            return torch.from_numpy(RT.oracle_table(_np_values(x), maxprec).copy())

    return RateCodec


def _grads(world, step):
    from oracle import oracle as O
    return [O.gen_normal(N, 1e-3, 5000 + 16 * r + step, False) for r in range(world)]


def _mean_of_roundtrips(grads, op):
    from oracle import oracle as O
    acc = np.zeros(N, np.float32)
    for a in grads:
        acc = acc + O.decompress(O.compress(a, op)[0], a.shape, op)
    return acc / np.float32(len(grads))


def _wire_worker(rank, world, port, q, hook_name):
    _init(rank, world, port)
    try:
        import rate_table_inputs as RT
        from gcow_amd import codec, ddp
        from oracle import oracle as O
        p0 = codec.expert(1, 16658, MAXPREC, -14)
        cdc = _codec_class()()
        hook = getattr(ddp, hook_name)
        state = ddp.make_hook_state(hook=hook, params=p0, codec=cdc, target_bits=TARGET)
        want_p = p0.tuple()
        for step in range(3):
            grads = _grads(world, step)
            g = torch.from_numpy(grads[rank].copy())
            hook(state, _Bucket(g, 0)).wait()
            used = cdc.seen[-1]
            everyone = [None] * world
            dist.all_gather_object(everyone, used)
            assert all(u == used for u in everyone), (step, everyone)  # the same set on every rank
            assert used == want_p, (step, used, want_p)                # state.params, then the lagged fit
            want = _mean_of_roundtrips(grads, O.expert(*used))
            assert np.array_equal(g.numpy().view(np.uint32), want.view(np.uint32)), step
            total = sum(RT.oracle_table(a, MAXPREC) for a in grads)
            me, bits = RT.fit(total, world * BUDGET)
            assert bits <= world * BUDGET
            want_p = (1, 16658, MAXPREC, me)
        assert cdc.tables == 3 and len(cdc.seen) == 3
        # reset_error_feedback keeps the fit, reset_rate_fit drops it
        state.reset_error_feedback()
        assert state.step_params(0, N).tuple() == want_p
        state.reset_rate_fit()
        assert state.step_params(0, N).tuple() == p0.tuple()
        q.put((rank, True))
    except Exception as ex:  # pragma: no cover - reported through the queue
        q.put((rank, repr(ex)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("hook_name", ["compressed_allgather_hook", "compressed_sharded_hook"])
@pytest.mark.parametrize("world", [2, 3])
def test_wire_hooks_track_the_budget(orc, world, hook_name):
    _run(_wire_worker, world, hook_name)


def _roundtrip_worker(rank, world, port, q):
    _init(rank, world, port)
    try:
        import rate_table_inputs as RT
        from gcow_amd import codec, ddp
        from oracle import oracle as O
        p0 = codec.expert(1, 16658, MAXPREC, -14)
        cdc = _codec_class()()
        state = ddp.make_hook_state(hook=ddp.roundtrip_hook, params=p0, codec=cdc, target_bits=TARGET)
        grads = _grads(world, 0)
        g = torch.from_numpy(grads[rank].copy())
        ddp.roundtrip_hook(state, _Bucket(g, 0)).wait()
        mean = grads[0] / np.float32(world)
        for a in grads[1:]:
            mean = mean + a / np.float32(world)  # world 2: exact in any order
        me, bits = RT.fit(RT.oracle_table(mean, MAXPREC), BUDGET)
        op = O.expert(1, 16658, MAXPREC, me)
        w, got_bits = O.compress(mean, op)
        assert got_bits == bits and bits <= BUDGET
        assert me == RT.MINEXP_LO or RT.oracle_bits(mean, MAXPREC, me - 1) > BUDGET
        assert cdc.seen == [(1, 16658, MAXPREC, me)] and state._fits[0] == (N, me)
        want = O.decompress(w, (N,), op)
        assert np.array_equal(g.numpy().view(np.uint32), want.view(np.uint32))
        q.put((rank, True))
    except Exception as ex:  # pragma: no cover
        q.put((rank, repr(ex)))
    finally:
        dist.destroy_process_group()


def test_roundtrip_hook_bounds_the_budget(orc):
    _run(_roundtrip_worker, 2)


def _unset_worker(rank, world, port, q):
    _init(rank, world, port)
    try:
        from gcow_amd import codec, ddp
        from oracle import oracle as O
        p0 = codec.expert(1, 16658, MAXPREC, -14)
        grads = _grads(world, 0)
        for name in ("compressed_allgather_hook", "compressed_sharded_hook", "roundtrip_hook"):
            cdc = _codec_class()(refuse=True)
            hook = getattr(ddp, name)
            state = ddp.make_hook_state(hook=hook, params=p0, codec=cdc)
            for _ in range(2):
                g = torch.from_numpy(grads[rank].copy())
                hook(state, _Bucket(g, 0)).wait()
            assert all(s == p0.tuple() for s in cdc.seen) and cdc.tables == 0 and not state._fits
            if name != "roundtrip_hook":
                want = _mean_of_roundtrips(grads, O.expert(*p0.tuple()))
                assert np.array_equal(g.numpy().view(np.uint32), want.view(np.uint32))
        q.put((rank, True))
    except Exception as ex:  # pragma: no cover
        q.put((rank, repr(ex)))
    finally:
        dist.destroy_process_group()


def test_unset_target_never_asks_for_a_table(orc):
    _run(_unset_worker, 2)


@pytest.mark.parametrize("hook_name", ["compressed_allgather_hook", "compressed_sharded_hook", "roundtrip_hook"])
def test_target_bits_value_errors(hook_name):
    from gcow_amd import codec, ddp
    hook = getattr(ddp, hook_name)
    b = _Bucket(torch.zeros(N), 0)
    for bad in (codec.rate(16, 1), codec.rate(8, 1), codec.expert(1, 100, 64, -30), codec.expert(8, 512, 32, -1074)):
        with pytest.raises(ValueError, match="target_bits"):  # raised before any collective: no process group here
            hook(ddp.GcowHookState(params=bad, target_bits=4.0), b)
    with pytest.raises(ValueError, match="relative_bits"):
        hook(ddp.GcowHookState(params=codec.accuracy(1e-3), target_bits=4.0, relative_bits=8), b)
