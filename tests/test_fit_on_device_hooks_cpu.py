"""GcowHookState.fit_on_device (the fit of the step that is encoded, on the device) on gloo process groups on the CPU,
worlds 2 and 3, with the harness of tests/test_rate_fit_hooks_cpu.py: its buckets, budget and oracle-backed codec, here
with fit_device, encode_fitted and roundtrip_fitted added through the oracle and the numpy model of the fit kernel
(tests/fit_device_inputs.py).

compressed_allgather_hook, three steps: in every step all ranks code under the same set; that set is the fit of THIS
step's summed oracle tables against world budgets (step 1 included); the bucket ends as the mean of the oracle round
trips under it; the ranks' stream lengths total at most world * BUDGET; the state keeps the record and no host fit.
With fit_on_device unset the same worker sees the lagged control of the parent hook. roundtrip_hook: the oracle round
trip under the fit of the reduced bucket, no host fit kept. The ValueError combinations."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

import test_rate_fit_hooks_cpu as H  # noqa: E402
from test_dist_cpu import _Bucket, _init, _run  # noqa: E402

N, TARGET, BUDGET, MAXPREC = H.N, H.TARGET, H.BUDGET, H.MAXPREC


def _fit_codec_class():
    import fit_device_inputs as FI
    from gcow_amd import codec

    class FitCodec(H._codec_class()):
        """The harness's codec + the three device-fit calls; `fits` keeps every record fit_device wrote."""

        def __init__(self, refuse=False):
            super().__init__(refuse)
            self.fits = []

        def fit_device(self, table, budget_bits, slot=None):
            rec = FI.model_fit(table.numpy().view(np.uint64), budget_bits)
            self.fits.append(rec)
            return torch.from_numpy(FI.pack_record(*rec).copy())

        def _params(self, minexp_word, maxprec):
            return codec.fitted_params(maxprec, FI.clamp(codec.read_fit(minexp_word)[0]))

        def encode_fitted(self, x, minexp_word, maxprec=64, index_stride=0, slot=None):
            return self.encode(x, self._params(minexp_word, maxprec), index_stride, slot)

        def roundtrip_fitted(self, x, minexp_word, maxprec=64, out=None):
            p = self._params(minexp_word, maxprec)
            words, _, _ = self.encode(x, p)
            return self.decode(words, x.numel(), p, out=out)

    return FitCodec


def _allgather_worker(rank, world, port, q, fod):
    _init(rank, world, port)
    try:
        import rate_table_inputs as RT
        from gcow_amd import codec, ddp
        from oracle import oracle as O
        p0 = codec.expert(1, 16658, MAXPREC, -14)
        cdc = _fit_codec_class()()
        hook = ddp.compressed_allgather_hook
        state = ddp.make_hook_state(hook=hook, params=p0, codec=cdc, target_bits=TARGET, fit_on_device=fod)
        lagged = p0.tuple()
        for step in range(3):
            grads = H._grads(world, step)
            total = sum(RT.oracle_table(a, MAXPREC) for a in grads)
            me, bits = RT.fit(total, world * BUDGET)
            assert bits <= world * BUDGET
            own = (1, 16658, MAXPREC, me)  # the fit of this step's own tables
            g = torch.from_numpy(grads[rank].copy())
            hook(state, _Bucket(g, 0)).wait()
            used = cdc.seen[-1]
            everyone = [None] * world
            dist.all_gather_object(everyone, used)
            assert all(u == used for u in everyone), (step, everyone)  # the same set on every rank
            assert used == (own if fod else lagged), (step, used, own, lagged)
            want = H._mean_of_roundtrips(grads, O.expert(*used))
            assert np.array_equal(g.numpy().view(np.uint32), want.view(np.uint32)), step
            sent = sum(RT.oracle_bits(a, MAXPREC, used[3]) for a in grads)  # the W streams of this step
            if fod:
                assert sent == bits and sent <= world * BUDGET, (step, sent)
                assert codec.read_fit(state.fit_record(0)) == (me, 0, bits) and cdc.fits[-1] == (me, 0, bits)
                assert not state._fits
            lagged = own
        assert cdc.tables == 3 and len(cdc.seen) == 3 and len(cdc.fits) == (3 if fod else 0)
        if fod:
            state.reset_rate_fit()
            assert state.fit_record(0) is None
        else:
            assert state.fit_record(0) is None and state.step_params(0, N).tuple() == lagged
        q.put((rank, True))
    except Exception as ex:  # pragma: no cover - reported through the queue
        q.put((rank, repr(ex)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_allgather_hook_fits_the_step_it_encodes(orc, world):
    _run(_allgather_worker, world, True)


def test_unset_keeps_the_lagged_control(orc):
    _run(_allgather_worker, 2, False)


def _coarsest_worker(rank, world, port, q):
    """A budget below one bit per block: status 1, the coarsest set, on every rank."""
    _init(rank, world, port)
    try:
        from gcow_amd import codec, ddp
        from oracle import oracle as O
        p0 = codec.expert(1, 16658, MAXPREC, -14)
        cdc = _fit_codec_class()()
        hook = ddp.compressed_allgather_hook
        state = ddp.make_hook_state(hook=hook, params=p0, codec=cdc, target_bits=0.1, fit_on_device=True)
        grads = H._grads(world, 0)
        g = torch.from_numpy(grads[rank].copy())
        hook(state, _Bucket(g, 0)).wait()
        assert cdc.seen == [(1, 16658, MAXPREC, 133)]
        assert codec.read_fit(state.fit_record(0)) == (133, 1, world * ((N + 3) // 4))
        want = H._mean_of_roundtrips(grads, O.expert(1, 16658, MAXPREC, 133))
        assert np.array_equal(g.numpy().view(np.uint32), want.view(np.uint32))
        q.put((rank, True))
    except Exception as ex:  # pragma: no cover
        q.put((rank, repr(ex)))
    finally:
        dist.destroy_process_group()


def test_budget_below_one_bit_per_block(orc):
    _run(_coarsest_worker, 2)


def _roundtrip_worker(rank, world, port, q):
    _init(rank, world, port)
    try:
        import rate_table_inputs as RT
        from gcow_amd import codec, ddp
        from oracle import oracle as O
        p0 = codec.expert(1, 16658, MAXPREC, -14)
        cdc = _fit_codec_class()()
        state = ddp.make_hook_state(hook=ddp.roundtrip_hook, params=p0, codec=cdc, target_bits=TARGET,
                                    fit_on_device=True)
        grads = H._grads(world, 0)
        g = torch.from_numpy(grads[rank].copy())
        ddp.roundtrip_hook(state, _Bucket(g, 0)).wait()
        mean = grads[0] / np.float32(world)
        for a in grads[1:]:
            mean = mean + a / np.float32(world)  # world 2: exact in any order
        me, bits = RT.fit(RT.oracle_table(mean, MAXPREC), BUDGET)
        op = O.expert(1, 16658, MAXPREC, me)
        w, got_bits = O.compress(mean, op)
        assert got_bits == bits and bits <= BUDGET
        assert cdc.seen == [(1, 16658, MAXPREC, me)] and not state._fits
        assert codec.read_fit(state.fit_record(0)) == (me, 0, bits)
        want = O.decompress(w, (N,), op)
        assert np.array_equal(g.numpy().view(np.uint32), want.view(np.uint32))
        q.put((rank, True))
    except Exception as ex:  # pragma: no cover
        q.put((rank, repr(ex)))
    finally:
        dist.destroy_process_group()


def test_roundtrip_hook_fits_on_the_device(orc):
    _run(_roundtrip_worker, 2)


def test_fit_on_device_value_errors(orc):
    """Raised before any collective: no process group here."""
    from gcow_amd import codec, ddp
    from oracle_codec import OracleCodec
    acc = codec.accuracy(1e-3)
    b = _Bucket(torch.zeros(N), 0)
    full = _fit_codec_class()()
    S = ddp.GcowHookState
    with pytest.raises(ValueError, match="compressed_sharded_hook"):
        ddp.compressed_sharded_hook(S(params=acc, codec=full, target_bits=4.0, fit_on_device=True, sharded=True), b)
    with pytest.raises(ValueError, match="error_feedback"):
        ddp.compressed_allgather_hook(S(params=acc, codec=full, target_bits=4.0, fit_on_device=True,
                                        error_feedback=True), b)
    with pytest.raises(ValueError, match="compress_mean"):
        ddp.compressed_sharded_hook(S(params=acc, codec=full, target_bits=4.0, fit_on_device=True, sharded=True,
                                      compress_mean=True), b)
    for hook in (ddp.roundtrip_hook, ddp.compressed_allgather_hook):
        with pytest.raises(ValueError, match="target_bits"):  # the flag alone
            hook(S(params=acc, codec=full, fit_on_device=True), b)
        with pytest.raises(ValueError, match="fit_device"):  # a codec without the methods
            hook(S(params=acc, codec=H._codec_class()(), target_bits=4.0, fit_on_device=True), b)
        with pytest.raises(ValueError, match="rate_table"):
            hook(S(params=acc, codec=OracleCodec(), target_bits=4.0, fit_on_device=True), b)
