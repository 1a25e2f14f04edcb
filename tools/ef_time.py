#!/usr/bin/env python3
"""Error feedback on 256 Mi values: the fused call (codec.ResidualEncoder -> gcow_encode_residual_device) against the
composition a caller writes without it -- torch add, codec.encode, codec.decode, torch subtract and the finite mask,
every buffer preallocated -- and, for context, the encoder alone and, at fixed rate, gcow_copy_pattern_device (the
encoder's access pattern without coding; it has no meaning at variable rate). Each is timed by the bench's driver
protocol (5 untimed + 20 timed launches, mean HIP-event time: "cold") and in steady state (after 0.25 s of
back-to-back launches, 50 launches). The two error-feedback forms must leave the same err and stream (checked before
timing). --rate R is the C2 bucket at fixed rate; --accuracy T / --precision P are the variable-rate sets without a
budget (the C5 bucket is --dtype bf16 --accuracy 1e-6), where the plain encoder writes the block index (every 16
blocks) its decoder needs and the fused call writes none.
usage: ef_time.py [--rate 16 | --accuracy T | --precision P] [--dtype fp32|bf16] [--log2n 28] [--lib libgcow_NAME.so]"""
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


n = 1 << arg("--log2n", 28)
dtype = {"fp32": torch.float32, "bf16": torch.bfloat16}[arg("--dtype", "fp32")]
if "--accuracy" in sys.argv:
    mode, p = "accuracy %g" % arg("--accuracy", 1e-3), codec.accuracy(arg("--accuracy", 1e-3))
elif "--precision" in sys.argv:
    mode, p = "precision %d" % arg("--precision", 32), codec.precision(arg("--precision", 32))
else:
    mode, p = "rate %g" % arg("--rate", 16.0), codec.rate(arg("--rate", 16.0), 1)
fixed = codec.is_fixed(p)
st = torch.cuda.current_stream()
xf = torch.empty(n, dtype=torch.float32, device="cuda")
codec.fill_normal(xf, 1e-3, seed=0x67636F77, inject=True)
x = xf if dtype == torch.float32 else xf.to(dtype)
del xf
err0 = torch.zeros(n, dtype=torch.float32, device="cuda")
fused_enc = codec.ResidualEncoder(n, dtype, p)
fused_enc(x, err0)  # a real residual to carry
err = err0.clone()

plain_enc = codec.Encoder((n,), torch.float32, p, index_stride=0 if fixed else 16)
y = torch.empty(n, dtype=torch.float32, device="cuda")
d = torch.empty_like(y)
copy_out = torch.empty(n // 4 * int(p.maxbits) // 64 + 1, dtype=torch.int64, device="cuda") if fixed else None


def fused():
    fused_enc(x, err, st)


def composed():
    torch.add(x, err, out=y)
    e = plain_enc(y, st)
    codec.decode(e, out=d, stream=st)
    torch.sub(y, d, out=err)
    err.nan_to_num_(nan=0.0, posinf=0.0, neginf=0.0)


def encode_only():
    plain_enc(y, st)


def copy_pattern():
    codec.copy_pattern(x, copy_out, int(p.maxbits), st)


# same result from the same state
err.copy_(err0)
fused()
torch.cuda.synchronize()
nwords = (int(fused_enc.bits_dev.item()) + 63) // 64
a_err, a_words, a_bits = err.clone(), fused_enc.words[:nwords].clone(), int(fused_enc.bits_dev.item())
err.copy_(err0)
composed()
torch.cuda.synchronize()
same = bool(torch.equal(a_err.view(torch.int32), err.view(torch.int32)) and
            a_bits == int(plain_enc.bits_dev.item()) and torch.equal(a_words, plain_enc.words[:nwords]))
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


res = {"n": n, "mode": mode, "dtype": arg("--dtype", "fp32"), "same_result": same, "stream_bits_per_value": a_bits / n,
       "path": getattr(fused_enc, "path", None), "workspace_bytes": fused_enc.ws_bytes}
legs = [("fused", fused), ("composed", composed), ("encode_only", encode_only)]
if fixed:
    legs.append(("copy_pattern", copy_pattern))
for name, fn in legs:
    cold, med = timed(fn, 5, 20)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.25:
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
    steady, _ = timed(fn, 0, 50)
    res[name] = {"cold_ms": round(cold, 4), "cold_median_ms": round(med, 4), "steady_ms": round(steady, 4)}
# HBM bytes per value the fused call has to move at least: x and e read, the stream and e' written (the variable-rate
# form reads x and e once more in its count pass)
bpv = x.element_size() + 4 + a_bits / n / 8 + 4
res["fused_steady_GBps"] = round(n * bpv / res["fused"]["steady_ms"] / 1e6, 1)
res["composed_over_fused_cold"] = round(res["composed"]["cold_ms"] / res["fused"]["cold_ms"], 3)
res["composed_over_fused_steady"] = round(res["composed"]["steady_ms"] / res["fused"]["steady_ms"], 3)
print(json.dumps(res), flush=True)
