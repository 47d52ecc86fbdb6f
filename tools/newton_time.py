"""Time fia_query_batch_newton on a full test batch beside the first-order call and the singleton
route through fia_group_influence.

Workloads: ml-1m-ex MF k=16 and yelp-ex NCF k=16 by default (synth.ML1M / synth.YELP with
synthetic parameters; --sizes DATA:MODEL:K,... for others), the whole test split as one batch.
Paths:

    newton_full  fia_query_batch_newton with rel_idx, newton and K = 64
    newton_topk  fia_query_batch_newton with K = 64 and no per-rating array
    first_order  fia_query_batch on the same batch with rel_idx, influence and K = 64
    group        fia_group_influence, one singleton group per related rating of the first --gq
                 queries (group written); reported as ms per related rating

Every path of every size runs in a child process of its own under `timeout -k 10`; the first one
that fails ends the run.  In a child: warm-up calls, then --steps calls each between its own pair
of events on the stream, the device synchronised before the times are read; the median is
reported with the minimum and maximum.  The newton paths then run --steps more calls with the
library's phase events on (fia_set_profiling) for the split into the chunk scan, the per-query
kernel (phase solve), the scoring kernel (phase score) and the top-K merge; those calls are not
the timed ones.  Writes the table to --out and prints one JSON line.

    python tools/newton_time.py --steps 20 --warmup 3 --out profiles/newton.md
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fia-kdd-19_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

PATHS = ("newton_full", "newton_topk", "first_order", "group")
K_TOP = 64


def worker(args):
    import torch
    from influence import _lib, synth

    model, k = args.model, args.k
    cfg = {"ml-1m-ex": synth.ML1M, "yelp-ex": synth.YELP}[args.data]
    d = synth.make_dataset(cfg, seed=0)
    params = (synth.mf_params if model == "MF" else synth.ncf_params)(d["U"], d["I"], k, 0)
    tu, ti, tr = d["train"]
    U, I = d["U"], d["I"]
    dev = torch.device("cuda", 0)
    ctx = _lib.Context(0)
    tables = [torch.from_numpy(np.ascontiguousarray(params[n], np.float32)).to(dev) for n in params]
    ctx.set_params(_lib.FIA_MODEL_MF if model == "MF" else _lib.FIA_MODEL_NCF, k, U, I, tables, 1e-3, 1e-6)
    t_u, t_i, t_r = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (tu, ti, tr))
    ctx.build_index(t_u, t_i, t_r, U, I)
    ctx.prepare()
    qu_h, qi_h = (np.ascontiguousarray(a, np.int32) for a in d["test"][:2])
    if args.path == "group":
        qu_h, qi_h = qu_h[:args.gq], qi_h[:args.gq]
    qu, qi = torch.from_numpy(qu_h).to(dev), torch.from_numpy(qi_h).to(dev)
    Q = int(qu.numel())
    offsets, total = ctx.count_related(qu, qi)
    f64 = lambda m: torch.empty(max(m, 1), dtype=torch.float64, device=dev)
    i64 = lambda m: torch.empty(max(m, 1), dtype=torch.int64, device=dev)
    i32 = lambda m: torch.empty(max(m, 1), dtype=torch.int32, device=dev)
    tp, tix, tv = i64(Q * K_TOP), i64(Q * K_TOP), f64(Q * K_TOP)
    vals = None
    if args.path == "newton_full":
        rel, vals = i32(total), f64(total)
        call = lambda: ctx.query_batch_newton(qu, qi, offsets, total, rel, vals, K_TOP, tp, tix, tv)
    elif args.path == "newton_topk":
        call = lambda: ctx.query_batch_newton(qu, qi, offsets, total, None, None, K_TOP, tp, tix, tv)
    elif args.path == "first_order":
        rel, vals = i32(total), f64(total)
        call = lambda: ctx.query_batch(qu, qi, offsets, total, rel, vals, None, K_TOP, tp, tix, tv)
    else:
        rel, vals = i32(total), f64(total)
        ctx.related(qu, qi, offsets, rel)
        mo = torch.arange(total + 1, dtype=torch.int64, device=dev)
        call = lambda: ctx.group_influence(qu, qi, offsets, mo, rel, vals, None, None)
    torch.cuda.synchronize(dev)
    for _ in range(args.warmup):
        call()
    torch.cuda.synchronize(dev)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    for a, b in ev:
        a.record()
        call()
        b.record()
    torch.cuda.synchronize(dev)
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    out = dict(data=args.data, model=model, k=k, path=args.path, queries=Q, related=int(total), steps=args.steps,
               warmup=args.warmup, median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1])
    if args.path.startswith("newton"):
        ctx.set_profiling(True, phases=("solve", "score", "topk", "chunks"))
        for _ in range(args.steps):
            call()
        torch.cuda.synchronize(dev)
        ph = ctx.profile_read()
        ctx.set_profiling(False)
        out["phase_ms"] = {p: ph[p][0] / args.steps for p in ("chunks", "solve", "score", "topk")}
    if vals is not None:
        h = vals[:total].cpu().numpy()
        out["finite_fraction"] = float(np.isfinite(h).mean())
    out["top1"] = [int(tix[0].item()), float(tv[0].item())] if args.path != "group" else None
    print(json.dumps(out))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="ml-1m-ex:MF:16,yelp-ex:NCF:16")
    ap.add_argument("--paths", default=",".join(PATHS))
    ap.add_argument("--gq", type=int, default=256, help="queries of the singleton-group path")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "newton.md"))
    ap.add_argument("--label", default="")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--data")
    ap.add_argument("--model")
    ap.add_argument("--k", type=int)
    ap.add_argument("--path")
    args = ap.parse_args()
    if args.worker:
        return worker(args)

    results, failed = [], None
    for size in args.sizes.split(","):
        data, model, k = size.split(":")
        for path in args.paths.split(","):
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--worker",
                   "--data", data, "--model", model, "--k", k, "--path", path, "--gq", str(args.gq), "--steps",
                   str(args.steps), "--warmup", str(args.warmup)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            if r.returncode != 0:
                failed = dict(data=data, model=model, k=int(k), path=path, exit=r.returncode)
                break
            results.append(json.loads(r.stdout.strip().splitlines()[-1]))
        if failed:
            break

    lines = ["# Per-rating Newton influence: fia_query_batch_newton, first order and the singleton route", "",
             "`tools/newton_time.py --sizes %s --gq %d --steps %d --warmup %d`%s on one MI355X; median (min .. max) "
             "of the per-call device time between stream events; top-K with K = %d on the three batch paths." % (
                 args.sizes, args.gq, args.steps, args.warmup, (" (" + args.label + ")") if args.label else "",
                 K_TOP), "",
             "| workload | path | queries | related ratings | ms per call | ns per related rating |",
             "|---|---|---|---|---|---|"]
    for r in results:
        lines.append("| %s %s k=%d | %s | %d | %d | %.3f (%.3f .. %.3f) | %.2f |" % (
            r["data"], r["model"], r["k"], r["path"], r["queries"], r["related"], r["median_ms"], r["min_ms"],
            r["max_ms"], 1e6 * r["median_ms"] / max(r["related"], 1)))
    lines += ["", "Phases of the new call (fia_set_profiling events, mean ms per call over separate calls; `solve` is "
              "the per-query kernel `k_newton_query`, `score` the scoring kernel `k_newton_score`):", "",
              "| workload | path | chunk scan | per-query kernel | scoring kernel | top-K merge |", "|---|---|---|---|---|---|"]
    for r in results:
        if "phase_ms" in r:
            p = r["phase_ms"]
            lines.append("| %s %s k=%d | %s | %.3f | %.3f | %.3f | %.3f |" % (
                r["data"], r["model"], r["k"], r["path"], p["chunks"], p["solve"], p["score"], p["topk"]))
    if failed:
        lines += ["", "The run ended at %s %s k=%d, path %s (exit status %d); nothing after it was started." % (
            failed["data"], failed["model"], failed["k"], failed["path"], failed["exit"])]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(dict(results=results, failed=failed)))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
