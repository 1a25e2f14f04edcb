#!/usr/bin/env python3
"""The fused round trip (codec.roundtrip -> gcow_roundtrip_device) against the composition it replaces -- a
preallocated codec.Encoder followed by codec.decode(..., out=), what roundtrip_hook ran before -- on 256 Mi values,
for fp32 at rate 16, rate 8 and accuracy 1e-3 and bf16 at accuracy 1e-6 and 1e-3. Every buffer is preallocated. Per
config the two forms must leave identical outputs (checked before timing); then, alternating in one process, the
composed form, the fused form and the composed form again (its own run-to-run spread) are each timed by the bench's
driver protocol (5 untimed + 20 timed launches, mean HIP-event time: "cold") and in steady state (after 0.25 s of
back-to-back launches, 50 launches). One JSON line per config; the fused call's bytes/s counts input plus output bytes
per value, from the shapes. faster_*: the fused form beats the faster composed run by more than the composed form's
spread.
usage: roundtrip_time.py [--log2n 28] [--only NAME]"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gcow_amd import codec  # noqa: E402
from gcow_amd.ddp import INDEX_STRIDE  # noqa: E402


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


n = 1 << arg("--log2n", 28)
only = arg("--only", "")
st = torch.cuda.current_stream()

CONFIGS = [
    ("fp32_rate16", torch.float32, codec.rate(16, 1)),
    ("fp32_rate8", torch.float32, codec.rate(8, 1)),
    ("fp32_acc1e-3", torch.float32, codec.accuracy(1e-3)),
    ("bf16_acc1e-6", torch.bfloat16, codec.accuracy(1e-6)),
    ("bf16_acc1e-3", torch.bfloat16, codec.accuracy(1e-3)),
]


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
    return sum(per) / len(per)


def cold_and_steady(fn):
    cold = timed(fn, 5, 20)
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.25:
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
    return cold, timed(fn, 0, 50)


x32 = torch.empty(n, dtype=torch.float32, device="cuda")
codec.fill_normal(x32, 1e-3, seed=0x67636F77, inject=True)

for name, dtype, p in CONFIGS:
    if only and name != only:
        continue
    x = x32 if dtype == torch.float32 else x32.to(dtype)
    fixed = codec.is_fixed(p)
    enc = codec.Encoder((n,), dtype, p, index_stride=0 if fixed else INDEX_STRIDE)
    out_f = torch.empty_like(x)
    out_c = torch.empty_like(x)
    bits = None if fixed else torch.zeros(1, dtype=torch.int64, device="cuda")

    def fused():
        codec.roundtrip(x, p, out=out_f, bits=bits, stream=st)

    def composed():
        codec.decode(enc(x, st), out=out_c, stream=st)

    fused()
    composed()
    torch.cuda.synchronize()
    view = torch.int16 if dtype == torch.bfloat16 else torch.int32
    same = bool(torch.equal(out_f.view(view), out_c.view(view)))
    if bits is not None:
        same = same and int(bits.item()) == enc.bits_dev.item()
    res = {"config": name, "n": n, "same_result": same}
    c1 = cold_and_steady(composed)
    f = cold_and_steady(fused)
    c2 = cold_and_steady(composed)
    for k, i in (("cold", 0), ("steady", 1)):
        res["fused_%s_ms" % k] = round(f[i], 4)
        res["composed_%s_ms" % k] = [round(c1[i], 4), round(c2[i], 4)]
        res["composed_over_fused_%s" % k] = round(min(c1[i], c2[i]) / f[i], 3)
        res["faster_%s" % k] = bool(min(c1[i], c2[i]) - f[i] > abs(c1[i] - c2[i]))
    res["fused_bytes_per_value"] = 2 * x.element_size()
    res["fused_steady_GBps"] = round(n * 2 * x.element_size() / f[1] / 1e6, 1)
    print(json.dumps(res), flush=True)
    del enc, out_f, out_c, x
