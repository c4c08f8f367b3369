#!/usr/bin/env python3
"""Kernel statistics of the eval forward from a rocprofv3 --kernel-trace database (rocpd SQLite, results.db) of
`tools/infer_bench.py --configs c2,c5 --warmup W --iters I --forms <one form>`.

A forward is delimited by its gather_rows_kernel<4> launch (one per forward).  The first W + I forwards are the first
configuration, the rest the second.  Only the spans between two consecutive forwards of the same configuration are counted.
The span of the last forward of a configuration also holds the next configuration's set-up.  Inside a forward, a stage's heads are the
dispatches after the launch that writes the stage's features and before its box decode.  That launch is the FFN launch,
rb_ffn_kernel<-2> for stage 0 and rb_ffn_kernel<4> for the decoder layers, or add_ln_fwd_kernel where the first layer is not fused.

  python tools/infer_profile_summary.py --per-config 6 LABEL=results.db [LABEL=results.db ...]"""
import argparse
import sqlite3
import statistics


def forwards(db, per_config):
    c = sqlite3.connect(db)
    rows = c.execute("select name, start, end, duration, grid_x, grid_y from kernels order by start").fetchall()
    marks = [i for i, r in enumerate(rows) if r[0].startswith("void vdetr::gather_rows_kernel<4>")]
    out = []
    for cfg in range(len(marks) // per_config):
        m = marks[cfg * per_config:(cfg + 1) * per_config]
        out.append([rows[a:b] for a, b in zip(m[:-1], m[1:])])
    return out


def heads_windows(fwd):
    """[(dispatch count, summed kernel us, names)] per stage"""
    res, start = [], None
    for i, r in enumerate(fwd):
        if r[0].startswith("void vdetr::rb_ffn_kernel") or r[0].startswith("void vdetr::add_ln_fwd_kernel"):
            start = i
        elif r[0].startswith("vdetr::box_decode_fwd_kernel") and start is not None:
            win = fwd[start + 1:i]
            res.append((len(win), sum(w[3] for w in win) / 1e3, sorted({w[0].split("(")[0][:60] for w in win})))
            start = None
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--per-config", type=int, default=6, help="forwards per configuration in the run (warmup + iters)")
    ap.add_argument("--configs", default="c2,c5")
    ap.add_argument("dbs", nargs="+", help="LABEL=path of a rocpd results.db")
    a = ap.parse_args()
    names = a.configs.split(",")
    for spec in a.dbs:
        label, path = spec.split("=", 1)
        for cfg, fwds in zip(names, forwards(path, a.per_config)):
            n = [len(f) for f in fwds]
            busy = [sum(r[3] for r in f) / 1e3 for f in fwds]
            stages = [heads_windows(f) for f in fwds]
            print(f"== {label} {cfg}: {len(fwds)} forwards, dispatches per forward {statistics.median(n):.0f} "
                  f"(min {min(n)}, max {max(n)}), summed kernel time per forward {statistics.median(busy):.0f} us")
            ns = len(stages[0])
            for s in range(ns):
                cnt = statistics.median(st[s][0] for st in stages)
                us = statistics.median(st[s][1] for st in stages)
                print(f"   stage {s}: heads {cnt:.0f} dispatches, {us:.1f} us  [{', '.join(stages[-1][s][2])}]")
            print(f"   heads, all {ns} stages: {sum(statistics.median(st[s][0] for st in stages) for s in range(ns)):.0f} dispatches, "
                  f"{sum(statistics.median(st[s][1] for st in stages) for s in range(ns)):.1f} us")


if __name__ == "__main__":
    main()
