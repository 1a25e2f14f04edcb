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
usage: roundtrip_time.py [--log2n 28] [--only NAME]

--list: the round trip over a tensor list instead (codec.roundtrip_tensors -> gcow_roundtrip_list_device), on a
ResNet-50-shaped fp32 list made here from the architecture's layer recipe (161 tensors, 25.6 M values, each tensor its
own allocation as .grad tensors are), at rate 16 and accuracy 1e-3. Form A is the flow the list call replaces:
torch.cat into a preallocated flat buffer, codec.roundtrip in place on it, one copy_ per tensor back. Form B is
roundtrip_tensors in place with a kept plan object. Both run on the same tensors; they must leave identical bits and
bit counts (checked first, on clones); then A, B and A again are timed, cold and steady, as above. The list with one
scalar tensor put first -- every later row of the field then lies off 16-byte alignment in its tensor -- is timed too.
single_*: B on one tensor of the same total against plain codec.roundtrip in place on it, the price of the chunk
descriptors. Each line reports the plan's direct / gather chunk counts. not_slower_*: B is not slower than the faster A
run by more than A's own run-to-run spread.
usage: roundtrip_time.py --list [--only NAME]

--relative: the tolerance relative to each tensor (codec.roundtrip_tensors_relative -> gcow_roundtrip_rel_device,
rel_bits 8) next to roundtrip_tensors at accuracy 1e-3, in place on the same ResNet-50-shaped list, fp32 and bf16
(relative_leg's docstring).
usage: roundtrip_time.py --relative [--only NAME]"""
import json
import math
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


def resnet50_shapes():
    """The parameter shapes of ResNet-50 in module order (conv, then its batch norm's weight and bias; the
    downsample path after a stage's first bottleneck; the classifier last)."""
    shapes = [(64, 3, 7, 7), (64,), (64,)]
    inplanes = 64
    for planes, blocks in ((64, 3), (128, 4), (256, 6), (512, 3)):
        for b in range(blocks):
            shapes += [(planes, inplanes, 1, 1), (planes,), (planes,), (planes, planes, 3, 3), (planes,), (planes,),
                       (4 * planes, planes, 1, 1), (4 * planes,), (4 * planes,)]
            if b == 0:
                shapes += [(4 * planes, inplanes, 1, 1), (4 * planes,), (4 * planes,)]
            inplanes = 4 * planes
    return shapes + [(1000, 2048), (1000,)]


def list_leg():
    shapes = resnet50_shapes()
    lists = {"resnet50": shapes, "resnet50_scalar_first": [()] + shapes, "single": [(sum(math.prod(s) for s in shapes),)]}
    configs = [("fp32_rate16", codec.rate(16, 1)), ("fp32_acc1e-3", codec.accuracy(1e-3))]
    for lname, shp in lists.items():
        total = sum(math.prod(s) for s in shp)
        src = torch.empty(total, dtype=torch.float32, device="cuda")
        codec.fill_normal(src, 1e-3, seed=0x67636F77, inject=True)
        offs = [0]
        for s in shp:
            offs.append(offs[-1] + math.prod(s))

        def fresh():
            return [src[offs[i]:offs[i + 1]].clone().view(s) for i, s in enumerate(shp)]

        for cname, p in configs:
            name = "list_%s_%s" % (lname, cname)
            if only and name != only:
                continue
            fixed = codec.is_fixed(p)
            flat = torch.empty(total, dtype=torch.float32, device="cuda")
            bits_a = torch.zeros(1, dtype=torch.int64, device="cuda")
            bits_b = torch.zeros(1, dtype=torch.int64, device="cuda")
            plan = codec.TensorListRoundtrip(p)

            def form_a(ts, views, backs):
                torch.cat(views, out=flat)
                codec.roundtrip(flat, p, out=flat, bits=None if fixed else bits_a, stream=st)
                for t, b in zip(ts, backs):
                    t.copy_(b)

            def bind(ts):
                return ts, [t.view(-1) for t in ts], [flat[offs[i]:offs[i + 1]].view(s) for i, s in enumerate(shp)]

            # the same bits first, on clones
            ta, tb = fresh(), fresh()
            form_a(*bind(ta))
            codec.roundtrip_tensors(tb, p, bits=None if fixed else bits_b, stream=st)
            torch.cuda.synchronize()
            same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(ta, tb))
            if not fixed:
                same = same and int(bits_a.item()) == int(bits_b.item())
            del ta, tb
            ts = fresh()
            bound = bind(ts)

            def a_fn():
                form_a(*bound)

            def b_fn():
                codec.roundtrip_tensors(ts, p, bits=None if fixed else bits_b, stream=st, plan=plan)

            def r_fn():  # single: the contiguous call in place
                codec.roundtrip(ts[0], p, out=ts[0], bits=None if fixed else bits_a, stream=st)

            base = r_fn if lname == "single" else a_fn
            b_fn()
            stats = plan.stats()
            res = {"config": name, "tensors": len(shp), "n": total, "same_result": same,
                   "direct_chunks": int(stats.direct_chunks), "gather_chunks": int(stats.gather_chunks),
                   "gather_share": round(stats.gather_chunks / max(1, stats.direct_chunks + stats.gather_chunks), 4),
                   "row_rule": int(stats.row_rule), "baseline": "roundtrip" if lname == "single" else "cat_roundtrip_copy"}
            a1 = cold_and_steady(base)
            b = cold_and_steady(b_fn)
            a2 = cold_and_steady(base)
            for k, i in (("cold", 0), ("steady", 1)):
                res["list_%s_ms" % k] = round(b[i], 4)
                res["baseline_%s_ms" % k] = [round(a1[i], 4), round(a2[i], 4)]
                res["baseline_over_list_%s" % k] = round(min(a1[i], a2[i]) / b[i], 3)
                res["not_slower_%s" % k] = bool(b[i] - min(a1[i], a2[i]) <= abs(a1[i] - a2[i]))
            res["plan_rebuilds"] = plan.rebuilds
            print(json.dumps(res), flush=True)
            del ts, bound, flat


def relative_leg():
    """roundtrip_tensors_relative (rel_bits 8) next to roundtrip_tensors at accuracy 1e-3, both in place with a kept
    plan on clones of the same ResNet-50-shaped list, fp32 and bf16: absolute, relative, absolute again, cold and
    steady as above. Each tensor of the list is scaled by its own power of two (2^-12 .. 2^0 in module order), the
    spread of magnitudes the relative form is for. The relative call reads every value twice (the maximum pass)."""
    shapes = resnet50_shapes()
    total = sum(math.prod(s) for s in shapes)
    src = torch.empty(total, dtype=torch.float32, device="cuda")
    codec.fill_normal(src, 1e-3, seed=0x67636F77, inject=False)
    offs = [0]
    for s in shapes:
        offs.append(offs[-1] + math.prod(s))
    p = codec.accuracy(1e-3)
    for dname, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        name = "relative_resnet50_%s_k8" % dname
        if only and name != only:
            continue

        def fresh():
            return [(src[offs[i]:offs[i + 1]] * 2.0 ** -(i % 13)).to(dtype).view(s) for i, s in enumerate(shapes)]

        ta, tr = fresh(), fresh()
        bits_a = torch.zeros(1, dtype=torch.int64, device="cuda")
        bits_r = torch.zeros(1, dtype=torch.int64, device="cuda")
        plan_a = codec.TensorListRoundtrip(p)
        plan_r = codec.TensorListRelative(8)

        def a_fn():
            codec.roundtrip_tensors(ta, p, bits=bits_a, stream=st, plan=plan_a)

        def r_fn():
            codec.roundtrip_tensors_relative(tr, 8, bits=bits_r, stream=st, plan=plan_r)

        a_fn()
        r_fn()
        torch.cuda.synchronize()
        sa, sr = plan_a.stats(), plan_r.stats()
        res = {"config": name, "tensors": len(shapes), "n": total,
               "bits_per_value_absolute": round(int(bits_a.item()) / total, 3),
               "bits_per_value_relative": round(int(bits_r.item()) / total, 3),
               "absolute_direct_chunks": int(sa.direct_chunks), "absolute_gather_chunks": int(sa.gather_chunks),
               "relative_direct_chunks": int(sr.direct_chunks), "relative_gather_chunks": int(sr.gather_chunks),
               "relative_total_blocks": int(sr.total_blocks), "relative_plan_bytes": int(sr.used_bytes)}
        a1 = cold_and_steady(a_fn)
        r = cold_and_steady(r_fn)
        a2 = cold_and_steady(a_fn)
        for k, i in (("cold", 0), ("steady", 1)):
            res["relative_%s_ms" % k] = round(r[i], 4)
            res["absolute_%s_ms" % k] = [round(a1[i], 4), round(a2[i], 4)]
            res["relative_over_absolute_%s" % k] = round(r[i] / min(a1[i], a2[i]), 3)
        res["plan_rebuilds"] = [plan_a.rebuilds, plan_r.rebuilds]
        print(json.dumps(res), flush=True)
        del ta, tr


if "--list" in sys.argv:
    list_leg()
    sys.exit(0)
if "--relative" in sys.argv:
    relative_leg()
    sys.exit(0)

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
