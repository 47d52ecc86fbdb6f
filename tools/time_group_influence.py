"""Time fia_group_influence per group, beside the per-query time of fia_query_batch's solve.

Workloads of bench.py at k = 16: ml-1m-ex MF (synth.ML1M) and yelp-ex NCF (synth.YELP), the test
queries in bench.py's (item-major) order.  For a group size m the batch is one group per query,
the first m distinct rows of the query's related list, over the first --max-queries queries
whose related list holds at least 2 m distinct rows (a group removes at most half of it); the
number of such queries is reported.

Per figure: warm-up calls, then --steps calls each timed by its own pair of HIP events on the
stream (torch events) around the call; the median is reported with the minimum and maximum, and
divided by the number of groups.  `group_only` is the call without first_order (no x_q
pre-kernel).  The comparator is the library's `solve` phase (fia_profile_read phase 1) of
fia_query_batch over the same queries, per query.  Prints one JSON line.

    python tools/time_group_influence.py --model MF --steps 30 --warmup 5
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fia-kdd-19_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="MF", choices=["MF", "NCF"])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--max-queries", type=int, default=2048)
    ap.add_argument("--sizes", default="1,16,256")
    args = ap.parse_args()

    import torch
    from influence import _lib, synth

    k = 16
    cfg = synth.ML1M if args.model == "MF" else synth.YELP
    d = synth.make_dataset(cfg, seed=0)
    params = (synth.mf_params if args.model == "MF" else synth.ncf_params)(d["U"], d["I"], k, 0)
    tu, ti, tr = d["train"]
    qu_np, qi_np, _ = d["test"]
    order = np.lexsort((qu_np, qi_np))          # bench.py's (item-major) query order
    qu_np, qi_np = np.ascontiguousarray(qu_np[order]), np.ascontiguousarray(qi_np[order])
    U, I = d["U"], d["I"]
    dev = torch.device("cuda", 0)
    ctx = _lib.Context(0)
    tables = [torch.from_numpy(np.ascontiguousarray(params[n], np.float32)).to(dev) for n in params]
    ctx.set_params(_lib.FIA_MODEL_MF if args.model == "MF" else _lib.FIA_MODEL_NCF, k, U, I, tables, 1e-3, 1e-6)
    t_u, t_i, t_r = (torch.from_numpy(a).to(dev) for a in (tu, ti, tr))
    ctx.build_index(t_u, t_i, t_r, U, I)
    ctx.prepare()
    D = ctx.num_params()

    # related lists of all queries, once (host side: the group members are drawn from them)
    qu_all, qi_all = torch.from_numpy(qu_np).to(dev), torch.from_numpy(qi_np).to(dev)
    off_all, total_all = ctx.count_related(qu_all, qi_all)
    rel_all = torch.empty(max(total_all, 1), dtype=torch.int32, device=dev)
    ctx.related(qu_all, qi_all, off_all, rel_all)
    off_h, rel_h = off_all.cpu().numpy(), rel_all.cpu().numpy()

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize(dev)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
        for a, b in ev:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize(dev)
        ms = sorted(a.elapsed_time(b) for a, b in ev)
        return dict(median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1])

    out = dict(model=args.model, k=k, config=cfg["name"], steps=args.steps, warmup=args.warmup, sizes=[])
    for m in [int(s) for s in args.sizes.split(",")]:
        sel, mem = [], []
        for q in range(qu_np.size):
            rows = np.unique(rel_h[off_h[q]:off_h[q + 1]])      # (sorted: the lowest m train rows)
            if rows.size >= 2 * m:
                sel.append(q)
                mem.append(rows[:m])
                if len(sel) == args.max_queries:
                    break
        G = len(sel)
        if G == 0:
            out["sizes"].append(dict(members=m, groups=0))
            continue
        qu, qi = torch.from_numpy(qu_np[sel]).to(dev), torch.from_numpy(qi_np[sel]).to(dev)
        go = torch.arange(G + 1, dtype=torch.int64, device=dev)
        mo = torch.arange(G + 1, dtype=torch.int64, device=dev) * m
        mr = torch.from_numpy(np.ascontiguousarray(np.concatenate(mem), np.int32)).to(dev)
        grp = torch.empty(G, dtype=torch.float64, device=dev)
        fo = torch.empty(G, dtype=torch.float64, device=dev)
        dth = torch.empty(G * D, dtype=torch.float64, device=dev)
        full = timed(lambda: ctx.group_influence(qu, qi, go, mo, mr, grp, fo, dth))
        only = timed(lambda: ctx.group_influence(qu, qi, go, mo, mr, grp, None, None))
        # the comparator: the solve phase of fia_query_batch over the same queries
        off, total = ctx.count_related(qu, qi)
        x = torch.empty(G * D, dtype=torch.float64, device=dev)
        tp = torch.empty(G, dtype=torch.int64, device=dev)
        tix = torch.empty(G, dtype=torch.int64, device=dev)
        tv = torch.empty(G, dtype=torch.float64, device=dev)
        call = lambda: ctx.query_batch(qu, qi, off, total, None, None, x, 1, tp, tix, tv)
        for _ in range(args.warmup):
            call()
        ctx.set_profiling(True, ["solve"])
        ctx.profile_read()
        for _ in range(args.steps):
            call()
        torch.cuda.synchronize(dev)
        ms, cnt = ctx.profile_read()["solve"]
        ctx.set_profiling(False)
        solve_ms = ms / max(cnt, 1)
        g_h, f_h = grp.cpu().numpy(), fo.cpu().numpy()
        out["sizes"].append(dict(
            members=m, groups=G, call=full, call_group_only=only,
            us_per_group=1e3 * full["median_ms"] / G, us_per_group_group_only=1e3 * only["median_ms"] / G,
            solve_phase_ms=solve_ms, solve_us_per_query=1e3 * solve_ms / G,
            finite=bool(np.isfinite(g_h).all() and np.isfinite(f_h).all()),
            median_abs_group_over_first_order=float(np.median(np.abs(g_h) / np.maximum(np.abs(f_h), 1e-300)))))
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
