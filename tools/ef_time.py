#!/usr/bin/env python3
"""Error feedback on 256 Mi fp32 values at rate 16 (the C2 bucket): the fused call (codec.ResidualEncoder ->
gcow_encode_residual_device) against the composition a caller writes without it -- torch add, codec.encode,
codec.decode, torch subtract and the finite mask, every buffer preallocated -- and, for context, the encoder alone and
gcow_copy_pattern_device (the encoder's access pattern without coding). Each is timed by the bench's driver protocol
(5 untimed + 20 timed launches, mean HIP-event time: "cold") and in steady state (after 0.25 s of back-to-back launches,
50 launches). The two error-feedback forms must leave the same err and stream (checked before timing).
usage: ef_time.py [--rate 16] [--log2n 28]"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gcow_amd import codec  # noqa: E402


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


rate = arg("--rate", 16.0)
n = 1 << arg("--log2n", 28)
p = codec.rate(rate, 1)
st = torch.cuda.current_stream()
x = torch.empty(n, dtype=torch.float32, device="cuda")
codec.fill_normal(x, 1e-3, seed=0x67636F77, inject=True)
err0 = torch.zeros(n, dtype=torch.float32, device="cuda")
fused_enc = codec.ResidualEncoder(n, torch.float32, p)
fused_enc(x, err0)  # a real residual to carry
err = err0.clone()

plain_enc = codec.Encoder((n,), torch.float32, p)
y = torch.empty_like(x)
d = torch.empty_like(x)
copy_out = torch.empty(n // 4 * int(p.maxbits) // 64 + 1, dtype=torch.int64, device="cuda")


def fused():
    fused_enc(x, err, st)


def composed():
    torch.add(x, err, out=y)
    e = plain_enc(y, st)
    codec.decode(e, out=d, stream=st)
    torch.sub(y, d, out=err)
    err.nan_to_num_(nan=0.0, posinf=0.0, neginf=0.0)


def encode_only():
    plain_enc(x, st)


def copy_pattern():
    codec.copy_pattern(x, copy_out, int(p.maxbits), st)


# same result from the same state
err.copy_(err0)
fused()
a_err, a_words = err.clone(), fused_enc.words[: n // 4 * int(p.maxbits) // 64].clone()
err.copy_(err0)
composed()
same = bool(torch.equal(a_err.view(torch.int32), err.view(torch.int32)) and
            torch.equal(a_words, plain_enc.words[: a_words.numel()]))
del a_err, a_words


def timed(fn, warm, steps):
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
    return sum(per) / len(per), sorted(per)[len(per) // 2]


res = {"n": n, "rate": rate, "same_result": same}
for name, fn in (("fused", fused), ("composed", composed), ("encode_only", encode_only), ("copy_pattern", copy_pattern)):
    cold, med = timed(fn, 5, 20)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.25:
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
    steady, _ = timed(fn, 0, 50)
    res[name] = {"cold_ms": round(cold, 4), "cold_median_ms": round(med, 4), "steady_ms": round(steady, 4)}
# HBM bytes per value: fused 4 + 4 + rate / 8 + 4
bpv = 12 + rate / 8
res["fused_steady_GBps"] = round(n * bpv / res["fused"]["steady_ms"] / 1e6, 1)
res["composed_over_fused_cold"] = round(res["composed"]["cold_ms"] / res["fused"]["cold_ms"], 3)
res["composed_over_fused_steady"] = round(res["composed"]["steady_ms"] / res["fused"]["steady_ms"], 3)
print(json.dumps(res), flush=True)
