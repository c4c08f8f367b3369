#!/usr/bin/env python3
"""The eval forward (model.eval() under torch.no_grad(), the reference's evaluate() / --test_only) of bench.py's models and scenes,
in three forms per configuration, in one process:
  aten   heads.INFER = False: the paths the eval forward took before the inference forms (library GEMMs + ATen BatchNorm)
  eager  heads.INFER = True: one heads launch per stage, the position MLP with its running statistics, GenericMLPs as GEMM + bn_act
  graph  the eager form captured once in a torch.cuda.graph and replayed
Precomputed FPS indices are fed, as bench.py does.  The forms are warmed up, then alternated, each forward timed with HIP events on
the launching stream.  Prints ONE JSON line: per configuration the median / min ms of each form, the speed-up of eager and graph over
aten, and the max relative difference of `outputs` (and of `aux_outputs`) of eager and graph against aten.

  python tools/infer_bench.py [--configs c2,c5] [--iters 20] [--warmup 3] [--forms aten,eager,graph] [--tile 0]

--forms with one form and a small --iters is what a `rocprofv3 --kernel-trace --stats -- python tools/infer_bench.py ...` run wants
(dispatch counts and kernel times of one form)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _tensors(out):
    stages = [("outputs", out["outputs"])] + [(f"aux{i}", o) for i, o in enumerate(out["aux_outputs"])]
    return {f"{s}.{k}": v for s, o in stages for k, v in o.items() if torch.is_tensor(v) and v.is_floating_point()}


def _max_rel(a, b, prefix):
    worst = 0.0
    for k, t in a.items():
        if k.startswith(prefix):
            ref = b[k].double()
            worst = max(worst, float((t.double() - ref).abs().max()) / max(float(ref.abs().max()), 1e-30))
    return worst


def run_config(cfg, forms, iters, warmup, dev):
    import bench
    from vdetr_amd import heads as HD
    from vdetr_amd.dist import FlatParams
    model = bench.build_model(cfg, dev)
    # the parameter layout of a training run (an eval pass normally follows optimiser steps of bench.py's trainer)
    FlatParams([p for p in model.parameters() if p.requires_grad], groups=model.flat_param_groups())
    model.eval()
    inp = bench.make_inputs(cfg, dev, 0)
    with torch.no_grad():
        inp["fps_inds"] = model.sample_indices(inp)

    def forward(infer):
        HD.INFER = infer
        with torch.no_grad():
            return model(inp)

    outs, graph = {}, None
    for f in forms:
        for _ in range(warmup):
            o = forward(f != "aten")
        torch.cuda.synchronize()
        if f == "graph":
            graph = torch.cuda.CUDAGraph()
            with torch.no_grad(), torch.cuda.graph(graph):
                HD.INFER = True
                o = model(inp)
            graph.replay()
            torch.cuda.synchronize()
        outs[f] = {k: v.clone() for k, v in _tensors(o).items()} if f != "graph" else _tensors(o)
    times = {f: [] for f in forms}
    stream = torch.cuda.current_stream()
    for _ in range(iters):
        for f in forms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            if f == "graph":
                graph.replay()
            else:
                forward(f != "aten")
            e1.record(stream)
            e1.synchronize()
            times[f].append(e0.elapsed_time(e1))
    HD.INFER = True
    res = {}
    for f in forms:
        t = sorted(times[f])
        res[f] = {"ms_median": round(t[len(t) // 2], 4), "ms_min": round(t[0], 4)}
    if "aten" in forms:
        for f in forms:
            if f != "aten":
                res[f]["speedup_vs_aten"] = round(res["aten"]["ms_median"] / res[f]["ms_median"], 3)
                res[f]["max_rel_diff_outputs"] = _max_rel(outs[f], outs["aten"], "outputs.")
                res[f]["max_rel_diff_aux_outputs"] = _max_rel(outs[f], outs["aten"], "aux")
    if "eager" in forms and "graph" in forms:
        res["graph"]["bit_identical_to_eager"] = all(torch.equal(outs["graph"][k], outs["eager"][k]) for k in outs["eager"])
    npts, bs, npre, nq, nl, *_ = bench.CONFIGS[cfg]
    res["shape"] = {"scenes": bs, "tokens": npre, "queries": nq, "head_stages": len(model.decoder.mlp_heads)}
    del graph, model
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--configs", default="c2,c5")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--forms", default="aten,eager,graph")
    ap.add_argument("--tile", type=int, default=0, help="tokens per workgroup of the heads launch: 16, 32 or 0 (library's choice)")
    a = ap.parse_args()
    from vdetr_amd import heads as HD
    HD.INFER_TILE = a.tile
    dev = torch.device("cuda", 0)
    forms = [f for f in a.forms.split(",") if f]
    assert all(f in ("aten", "eager", "graph") for f in forms), forms
    out = {"bench": "infer", "iters": a.iters, "warmup": a.warmup, "tile": a.tile, "device": torch.cuda.get_device_name(0)}
    for cfg in a.configs.split(","):
        out[cfg] = run_config(cfg, forms, a.iters, a.warmup, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
