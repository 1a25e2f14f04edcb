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
usage: roundtrip_time.py --relative [--only NAME]

--fitted-list: accuracy mode under a bit budget over the same ResNet-50-shaped fp32 list (fitted_list_leg's docstring):
the composed flow torch.cat + rate table + device fit + roundtrip_fitted + one copy_ per tensor against
codec.TensorListFitted, at 8.0 and 2.5 bits per value, with the table pass, the fit and the round trip of both broken
out. Medians over interleaved rounds with their spread.
usage: roundtrip_time.py --fitted-list [--only NAME] [--rounds 9]

--fitted-per-tensor: a bit budget per tensor (codec.TensorListFittedPerTensor) on that list against one budget for the
list, the relative tolerance and the per-tensor loop of single calls (fitted_per_tensor_leg's docstring).
usage: roundtrip_time.py --fitted-per-tensor [--only NAME] [--rounds 9]"""
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


def fitted_list_leg():
    """Form A is the flow the parent offers for a tensor list under a bit budget: torch.cat into a preallocated flat
    buffer, the rate table of it (a kept codec.RateTable), codec.fit_device into a kept record, codec.roundtrip_fitted
    in place on the flat buffer under the record, one copy_ per tensor into the outputs. Form B is a kept
    codec.TensorListFitted called with the same tensors and outputs. Nothing is allocated in either timed call and
    neither reads anything on the host. The inputs are never written (outputs are tensors of their own), so every
    launch of a form does the same work. Checked first: the outputs, the bit count, the table and the fit record of
    the two forms are identical. Then every part -- A, B, and of each its table pass, its fit and its round trip, and
    A's cat and copy-back, and both forms captured into a graph and replayed (which leaves the host out: an eager call
    of either form is bound by its launches and by Python) -- is timed in rounds that take the parts in turn in one
    process: 3 untimed and 20 timed launches per part and round, mean HIP-event time; reported are the median over the
    rounds and [min, max].
    table_within_spread: the two table passes' [min, max] overlap. list_faster: B's maximum is below A's minimum."""
    rounds = arg("--rounds", 9)
    shapes = resnet50_shapes()
    total = sum(math.prod(s) for s in shapes)
    src = torch.empty(total, dtype=torch.float32, device="cuda")
    codec.fill_normal(src, 1e-3, seed=0x67636F77, inject=True)
    offs = [0]
    for s in shapes:
        offs.append(offs[-1] + math.prod(s))
    ts = [src[offs[i]:offs[i + 1]].clone().view(s) for i, s in enumerate(shapes)]
    views = [t.view(-1) for t in ts]
    outs_a = [torch.empty_like(t) for t in ts]
    outs_b = [torch.empty_like(t) for t in ts]
    flat = torch.empty(total, dtype=torch.float32, device="cuda")
    backs = [flat[offs[i]:offs[i + 1]].view(s) for i, s in enumerate(shapes)]
    for bpv in (8.0, 2.5):
        name = "fitted_list_resnet50_fp32_%gbpv" % bpv
        if only and name != only:
            continue
        budget = int(math.floor(bpv * total))
        table_a = codec.RateTable(total, torch.float32)
        fit_a = codec.new_fit_record()
        bits_a = torch.zeros(1, dtype=torch.int64, device="cuda")
        bits_b = torch.zeros(1, dtype=torch.int64, device="cuda")
        plan = codec.TensorListFitted(bpv)

        def a_cat():
            torch.cat(views, out=flat)

        cur = {"st": st}  # the stream the forms launch on: the timing stream, or the capturing one

        def a_table():
            table_a(flat, 64, cur["st"])

        def a_fit():
            codec.fit_device(table_a.table, budget, fit_a, cur["st"])

        def a_rt():
            codec.roundtrip_fitted(flat, fit_a, 64, out=flat, bits=bits_a, stream=cur["st"])

        def a_back():
            for o, b in zip(outs_a, backs):
                o.copy_(b)

        def a_fn():
            a_cat()
            a_table()
            a_fit()
            a_rt()
            a_back()

        def b_fn():
            plan(ts, outs_b, bits_b, cur["st"])

        # B's parts go to the C ABI with the plan as b_fn left it: through the object each would pay again for the
        # comparison of 161 pointers with the plan's key, which b_fn pays once
        def b_table():
            plan._table(st)

        def b_fit():
            codec.fit_device(plan.table, budget, plan.fit, st)

        def b_rt():
            plan.L.gcow_roundtrip_list_fitted_device(plan._h.data_ptr(), plan._d.data_ptr(), plan._used, 64,
                                                     plan.fit.data_ptr(), bits_b.data_ptr(), st.cuda_stream)

        def captured(fn):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                cur["st"] = torch.cuda.current_stream()
                fn()
            cur["st"] = st
            return g.replay

        a_fn()
        b_fn()
        torch.cuda.synchronize()
        same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(outs_a, outs_b))
        same = same and int(bits_a.item()) == int(bits_b.item()) and torch.equal(table_a.table, plan.table)
        same = same and codec.read_fit(fit_a) == codec.read_fit(plan.fit)
        stats = plan.stats()
        me, status, fbits = codec.read_fit(plan.fit)
        res = {"config": name, "tensors": len(shapes), "n": total, "bits_per_value": bpv, "same_result": bool(same),
               "fitted_minexp": me, "fit_status": status, "stream_bits_per_value": round(fbits / total, 3),
               "direct_chunks": int(stats.direct_chunks), "gather_chunks": int(stats.gather_chunks), "rounds": rounds}
        # a_rt alone runs on whatever a_cat left in flat: the round trip of a round trip, the same work per launch
        a_graph, b_graph = captured(a_fn), captured(b_fn)
        a_graph()
        b_graph()
        torch.cuda.synchronize()
        same = same and all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(outs_a, outs_b))
        res["same_result"] = bool(same)
        parts = [("composed", a_fn), ("list", b_fn), ("composed_graph", a_graph), ("list_graph", b_graph),
                 ("composed_cat", a_cat), ("composed_table", a_table),
                 ("list_table", b_table), ("composed_fit", a_fit), ("list_fit", b_fit), ("composed_roundtrip", a_rt),
                 ("list_roundtrip", b_rt), ("composed_copy_back", a_back)]
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.25:
            a_fn()
            b_fn()
            torch.cuda.synchronize()
        got = {k: [] for k, _ in parts}
        for _ in range(rounds):
            for k, fn in parts:
                if k == "composed_roundtrip":
                    a_cat()  # the flat buffer holds the inputs again
                got[k].append(timed(fn, 3, 20))
        for k, v in got.items():
            v.sort()
            res[k + "_ms"] = {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}
        res["composed_over_list"] = round(res["composed_ms"]["median"] / res["list_ms"]["median"], 3)
        res["list_faster"] = bool(res["list_ms"]["max"] < res["composed_ms"]["min"])
        res["composed_over_list_graph"] = round(res["composed_graph_ms"]["median"] / res["list_graph_ms"]["median"], 3)
        res["list_graph_faster"] = bool(res["list_graph_ms"]["max"] < res["composed_graph_ms"]["min"])
        res["table_list_over_composed"] = round(res["list_table_ms"]["median"] / res["composed_table_ms"]["median"], 3)
        res["table_within_spread"] = bool(res["list_table_ms"]["min"] <= res["composed_table_ms"]["max"]
                                          and res["composed_table_ms"]["min"] <= res["list_table_ms"]["max"])
        res["plan_rebuilds"] = plan.rebuilds
        print(json.dumps(res), flush=True)


def fitted_per_tensor_leg():
    """A bit budget per tensor (codec.TensorListFittedPerTensor) on the ResNet-50-shaped fp32 list of fitted_list_leg,
    against the three forms it stands beside: one budget for the list (codec.TensorListFitted), the relative
    tolerance (codec.TensorListRelative, 8 bits) and the loop a caller had to write for a budget per tensor -- per
    tensor a kept codec.RateTable, codec.fit_device into a kept record and codec.roundtrip_fitted. All four write
    outputs of their own from inputs that are never written, allocate nothing in a timed call and read nothing on the
    host. Checked first: the per-tensor form and the loop give the same outputs, records and summed bits. Then the
    four forms, eager and captured into a graph, the two table passes (one table for the list; a table per tensor:
    the same bytes read), the batch fit and the fitted round trip are timed in rounds that take the parts in turn in
    one process, as fitted_list_leg does: 3 untimed and 20 timed launches per part and round, mean HIP-event time;
    reported are the median over the rounds and [min, max]."""
    rounds = arg("--rounds", 9)
    shapes = resnet50_shapes()
    total = sum(math.prod(s) for s in shapes)
    src = torch.empty(total, dtype=torch.float32, device="cuda")
    codec.fill_normal(src, 1e-3, seed=0x67636F77, inject=True)
    offs = [0]
    for s in shapes:
        offs.append(offs[-1] + math.prod(s))
    ts = [src[offs[i]:offs[i + 1]].clone().view(s) for i, s in enumerate(shapes)]
    flats = [t.view(-1) for t in ts]
    outs = {k: [torch.empty_like(t) for t in ts] for k in "pblr"}
    flat_l = [o.view(-1) for o in outs["l"]]
    for bpv in (8.0, 2.5):
        name = "fitted_per_tensor_resnet50_fp32_%gbpv" % bpv
        if only and name != only:
            continue
        bits = {k: torch.zeros(1, dtype=torch.int64, device="cuda") for k in "pbr"}
        plan_p = codec.TensorListFittedPerTensor(bpv)
        plan_b = codec.TensorListFitted(bpv)
        plan_r = codec.TensorListRelative(8)
        tabs = [codec.RateTable(f.numel(), torch.float32) for f in flats]
        recs = torch.zeros((len(ts), codec.FIT_WORDS), dtype=torch.int64, device="cuda")
        bits_l = torch.zeros(len(ts), dtype=torch.int64, device="cuda")
        budgets = [int(math.floor(bpv * f.numel())) for f in flats]
        cur = {"st": st}  # the stream the forms launch on: the timing stream, or the capturing one

        def p_fn():
            plan_p(ts, outs["p"], bits["p"], cur["st"])

        def b_fn():
            plan_b(ts, outs["b"], bits["b"], cur["st"])

        def r_fn():
            plan_r(ts, outs["r"], None, bits["r"], cur["st"])

        def l_fn():
            for i, f in enumerate(flats):
                tabs[i](f, 64, cur["st"])
                codec.fit_device(tabs[i].table, budgets[i], recs[i], cur["st"])
                codec.roundtrip_fitted(f, recs[i], 64, out=flat_l[i], bits=bits_l[i:i + 1], stream=cur["st"])

        # the parts go to the C ABI with the plans as the whole calls left them (fitted_list_leg says why)
        def b_table():
            plan_b._table(st)

        def p_tables():
            plan_p._tables(len(ts), st)

        def p_fit():
            codec.fit_device_batch(plan_p.tables, plan_p.budgets, plan_p.minexp_floor, plan_p.fits, st)

        def p_rt():
            plan_p.L.gcow_roundtrip_rel_fitted_device(plan_p._h.data_ptr(), plan_p._d.data_ptr(), plan_p._used, 64,
                                                      plan_p.fits.data_ptr(), 4, bits["p"].data_ptr(), st.cuda_stream)

        def captured(fn):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                cur["st"] = torch.cuda.current_stream()
                fn()
            cur["st"] = st
            return g.replay

        for fn in (p_fn, b_fn, r_fn, l_fn):
            fn()
        torch.cuda.synchronize()
        # the floor is out of reach for this data, so the loop (which has none) must agree
        same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(outs["p"], outs["l"]))
        same = same and torch.equal(plan_p.fits, recs) and int(bits["p"].item()) == int(bits_l.sum().item())
        same = same and all(torch.equal(plan_p.tables[i], tabs[i].table) for i in range(len(ts)))
        fits = plan_p.fits.cpu()
        mes = sorted(int(w) & 0xFFFFFFFF for w in fits[:, 0].tolist())
        mes = [m - (1 << 32) if m >> 31 else m for m in mes]
        stats = plan_p.stats()
        res = {"config": name, "tensors": len(shapes), "n": total, "bits_per_value": bpv, "same_as_loop": bool(same),
               "fitted_minexp_min": min(mes), "fitted_minexp_max": max(mes),
               "fit_status_1": int(sum((int(w) >> 32) & 1 for w in fits[:, 0].tolist())),
               "stream_bits_per_value": round(int(bits["p"].item()) / total, 3),
               "one_budget_minexp": codec.read_fit(plan_b.fit)[0],
               "direct_chunks": int(stats.direct_chunks), "gather_chunks": int(stats.gather_chunks), "rounds": rounds}
        graphs = {k: captured(fn) for k, fn in (("p", p_fn), ("b", b_fn), ("r", r_fn), ("l", l_fn))}
        for g in graphs.values():
            g()
        torch.cuda.synchronize()
        same = same and all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(outs["p"], outs["l"]))
        res["same_as_loop"] = bool(same)
        parts = [("per_tensor", p_fn), ("one_budget", b_fn), ("relative", r_fn), ("loop", l_fn),
                 ("per_tensor_graph", graphs["p"]), ("one_budget_graph", graphs["b"]), ("relative_graph", graphs["r"]),
                 ("loop_graph", graphs["l"]), ("one_budget_table", b_table), ("per_tensor_tables", p_tables),
                 ("per_tensor_fit", p_fit), ("per_tensor_roundtrip", p_rt)]
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.25:
            p_fn()
            b_fn()
            torch.cuda.synchronize()
        got = {k: [] for k, _ in parts}
        for _ in range(rounds):
            for k, fn in parts:
                got[k].append(timed(fn, 3, 20))
        for k, v in got.items():
            v.sort()
            res[k + "_ms"] = {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}
        res["tables_over_one_table"] = round(res["per_tensor_tables_ms"]["median"] / res["one_budget_table_ms"]["median"], 3)
        res["tables_within_spread"] = bool(res["per_tensor_tables_ms"]["min"] <= res["one_budget_table_ms"]["max"]
                                           and res["one_budget_table_ms"]["min"] <= res["per_tensor_tables_ms"]["max"])
        res["loop_over_per_tensor"] = round(res["loop_ms"]["median"] / res["per_tensor_ms"]["median"], 3)
        res["loop_over_per_tensor_graph"] = round(res["loop_graph_ms"]["median"] / res["per_tensor_graph_ms"]["median"], 3)
        res["per_tensor_over_one_budget_graph"] = round(res["per_tensor_graph_ms"]["median"]
                                                        / res["one_budget_graph_ms"]["median"], 3)
        res["per_tensor_over_relative_graph"] = round(res["per_tensor_graph_ms"]["median"]
                                                      / res["relative_graph_ms"]["median"], 3)
        res["plan_rebuilds"] = plan_p.rebuilds
        print(json.dumps(res), flush=True)


if "--fitted-per-tensor" in sys.argv:
    fitted_per_tensor_leg()
    sys.exit(0)
if "--list" in sys.argv:
    list_leg()
    sys.exit(0)
if "--fitted-list" in sys.argv:
    fitted_list_leg()
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
