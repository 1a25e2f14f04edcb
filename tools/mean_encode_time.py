#!/usr/bin/env python3
"""The sharded hook's second stage on one shard: W received fixed-rate pieces into the stream of their mean. The
fused call (codec.ReduceEncoder -> gcow_decode_mean_encode_device) against the composition a caller writes without it
-- codec.decode_mean into an fp32 temporary, then codec.Encoder or, with error feedback, codec.ResidualEncoder -- every
buffer preallocated, one process. The composition is timed before and after the fused form; each leg by the bench's
driver protocol (5 untimed + 20 timed launches, mean HIP-event time: "cold") and in steady state (after 0.25 s of
back-to-back launches, 50 launches). Both forms must leave the same stream and the same err (checked before timing).
Default: the 256 Mi-value bucket's shard at W = 8 (32 Mi values, 8 pieces) and W = 2 (128 Mi values, 2 pieces),
rates 16 and 8, with and without the residual: one JSON line per config.
usage: mean_encode_time.py [--world W --rate R [--residual]] [--bucket-log2n 28] [--lib libgcow_NAME.so]"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gcow_amd import _ffi, codec  # noqa: E402

if "--lib" in sys.argv:  # an A/B build (tools/build_variant.sh)
    _ffi.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def timed(fn, warm, steps, st):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    ev[0].record(st)
    for i in range(steps):
        fn()
        ev[i + 1].record(st)
    torch.cuda.synchronize()
    per = [ev[i].elapsed_time(ev[i + 1]) for i in range(steps)]
    return sum(per) / len(per)


def leg(fn, st):
    cold = timed(fn, 5, 20, st)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.25:
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
    return {"cold_ms": round(cold, 4), "steady_ms": round(timed(fn, 0, 50, st), 4)}


def run(bucket, world, rate, residual):
    n = bucket // world
    p = codec.rate(rate, 1)
    st = torch.cuda.current_stream()
    sw = n // 4 * int(p.maxbits) // 64
    pieces = torch.zeros(world * sw + 2, dtype=torch.int64, device="cuda")
    x = torch.empty(n, dtype=torch.float32, device="cuda")
    enc = codec.Encoder((n,), torch.float32, p)
    for r in range(world):
        codec.fill_normal(x, 1e-3, seed=0x67636F77 + r, inject=True)
        pieces[r * sw:(r + 1) * sw] = enc(x, st).words[:sw]
    del x
    fused_enc = codec.ReduceEncoder(n, p, world, residual=residual)
    m = torch.empty(n, dtype=torch.float32, device="cuda")
    inner = codec.ResidualEncoder(n, torch.float32, p) if residual else enc
    err0 = err = None
    if residual:
        err0 = torch.zeros(n, dtype=torch.float32, device="cuda")
        fused_enc(pieces, sw, err=err0, stream=st)  # a real residual to carry
        err = err0.clone()

    def fused():
        fused_enc(pieces, sw, err=err, stream=st)

    def composed():
        codec.decode_mean(pieces, sw, world, n, p, out=m, stream=st)
        if residual:
            inner(m, err, st)
        else:
            inner(m, st)

    # same result from the same state
    fused()
    torch.cuda.synchronize()
    a_words = fused_enc.words[:sw].clone()
    a_err = err.clone() if residual else None
    if residual:
        err.copy_(err0)
    composed()
    torch.cuda.synchronize()
    same = bool(torch.equal(a_words, inner.words[:sw]) and
                (not residual or torch.equal(a_err.view(torch.int32), err.view(torch.int32))))
    del a_words, a_err
    res = {"shard_values": n, "world": world, "rate": rate, "residual": residual, "same_result": same,
           "path": fused_enc.path, "workspace_bytes": fused_enc.ws_bytes}
    # the first leg of a config would otherwise carry the clock ramp after the setup's idle time into its "cold" mean
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.25:
        composed()
        torch.cuda.synchronize()
    res["composed_before"] = leg(composed, st)
    res["fused"] = leg(fused, st)
    res["composed_after"] = leg(composed, st)
    for k in ("cold_ms", "steady_ms"):
        c = [res["composed_before"][k], res["composed_after"][k]]
        res["composed_spread_" + k] = round(abs(c[0] - c[1]), 4)
        res["fused_gain_" + k] = round(min(c) - res["fused"][k], 4)  # against the faster composed run
    # HBM bytes per block the fused call has to move at least: W words read, one written, and the two e rows
    bpb = (world + 1) * int(p.maxbits) // 8 + (32 if residual else 0)
    res["fused_steady_GBps"] = round(n // 4 * bpb / res["fused"]["steady_ms"] / 1e6, 1)
    print(json.dumps(res), flush=True)


bucket = 1 << arg("--bucket-log2n", 28)
if "--world" in sys.argv:
    run(bucket, arg("--world", 8), arg("--rate", 16.0), "--residual" in sys.argv)
else:
    for world in (8, 2):
        for rate in (16.0, 8.0):
            for residual in (False, True):
                run(bucket, world, rate, residual)
                torch.cuda.empty_cache()
