"""Time fia_score_candidates_newton beside the first-order candidate call and the per-rating Newton
call on the same work.

Workloads: ml-1m-ex MF k=16 and yelp-ex NCF k=16 by default (synth.ML1M / synth.YELP with synthetic
parameters; --sizes DATA:MODEL:K,... for others), the whole test split as one batch.  The candidates
are each query's own related rows (tu[rel], ti[rel], tr[rel]), so all three calls handle the same
number of ratings of the same entities.  Paths:

    cand_newton       fia_score_candidates_newton with newton_add, no top-K
    cand_newton_topk  the same with K = 64
    first_order       fia_score_candidates (x from fia_query_batch, not timed) with influence, no top-K
    list_newton       fia_query_batch_newton with rel_idx and newton, no top-K: the same number of
                      quadratic forms, e_j and g_j from the per-list-position caches
    list_newton_topk  the same with K = 64

Every path of every size runs in a child process of its own under `timeout -k 10`; the first one
that fails ends the run.  In a child: warm-up calls, then --steps calls each between its own pair
of events on the stream, the device synchronised before the times are read; the median is reported
with the minimum and maximum.  The cand_newton paths then run --steps more calls with the library's
phase events on (fia_set_profiling) for the split into the per-query records (phase solve), the
partition by (query, side) (phase chunks), the scoring (phase score), the `both` solves (phase
prepare) and the top-K (phase topk); those calls are not the timed ones.  Writes the tables to --out
and prints one JSON line.

    python tools/cand_newton_time.py --steps 20 --warmup 3 --out profiles/cand_newton.md
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

PATHS = ("cand_newton", "cand_newton_topk", "first_order", "list_newton", "list_newton_topk")
K_TOP = 64
PHASE_OF = (("records", "solve"), ("partition", "chunks"), ("score", "score"), ("both", "prepare"), ("topk", "topk"))


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
    qu, qi = torch.from_numpy(qu_h).to(dev), torch.from_numpy(qi_h).to(dev)
    Q = int(qu.numel())
    offsets, total = ctx.count_related(qu, qi)
    f64 = lambda m: torch.empty(max(m, 1), dtype=torch.float64, device=dev)
    i64 = lambda m: torch.empty(max(m, 1), dtype=torch.int64, device=dev)
    rel = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    ctx.related(qu, qi, offsets, rel)
    rows = rel[:total].long()
    c_u, c_i, c_r = t_u[rows].contiguous(), t_i[rows].contiguous(), t_r[rows].contiguous()
    both = int(((c_u == qu.repeat_interleave(offsets[1:] - offsets[:-1])) &
                (c_i == qi.repeat_interleave(offsets[1:] - offsets[:-1]))).sum().item())
    vals = f64(total)
    tp, tv = i64(Q * K_TOP), f64(Q * K_TOP)
    if args.path == "cand_newton":
        call = lambda: ctx.score_candidates_newton(qu, qi, offsets, total, c_u, c_i, c_r, vals, 0, None, None)
    elif args.path == "cand_newton_topk":
        call = lambda: ctx.score_candidates_newton(qu, qi, offsets, total, c_u, c_i, c_r, vals, K_TOP, tp, tv)
    elif args.path == "first_order":
        x = f64(Q * ctx.num_params())
        ctx.query_batch(qu, qi, offsets, total, None, None, x, 0, None, None, None)
        call = lambda: ctx.score_candidates(qu, qi, x, offsets, total, c_u, c_i, c_r, vals, 0, None, None)
    elif args.path == "list_newton":
        call = lambda: ctx.query_batch_newton(qu, qi, offsets, total, rel, vals, 0, None, None, None)
    else:
        tix = i64(Q * K_TOP)
        call = lambda: ctx.query_batch_newton(qu, qi, offsets, total, rel, vals, K_TOP, tp, tix, tv)
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
    out = dict(data=args.data, model=model, k=k, path=args.path, queries=Q, candidates=int(total), both=both,
               steps=args.steps, warmup=args.warmup, median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1])
    if args.path.startswith("cand_newton"):
        ctx.set_profiling(True, phases=[p for _, p in PHASE_OF])
        for _ in range(args.steps):
            call()
        torch.cuda.synchronize(dev)
        ph = ctx.profile_read()
        ctx.set_profiling(False)
        out["phase_ms"] = {name: ph[p][0] / args.steps for name, p in PHASE_OF}
    h = vals[:total].cpu().numpy()
    out["finite_fraction"] = float(np.isfinite(h).mean())
    print(json.dumps(out))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="ml-1m-ex:MF:16,yelp-ex:NCF:16")
    ap.add_argument("--paths", default=",".join(PATHS))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cand_newton.md"))
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
                   "--data", data, "--model", model, "--k", k, "--path", path, "--steps", str(args.steps), "--warmup",
                   str(args.warmup)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            if r.returncode != 0:
                failed = dict(data=data, model=model, k=int(k), path=path, exit=r.returncode)
                break
            results.append(json.loads(r.stdout.strip().splitlines()[-1]))
        if failed:
            break

    ns = lambda r: 1e6 * r["median_ms"] / max(r["candidates"], 1)
    lines = ["# Newton-corrected candidates: fia_score_candidates_newton, first order and the list call", "",
             "`tools/cand_newton_time.py --sizes %s --steps %d --warmup %d`%s on one MI355X; median (min .. max) of "
             "the per-call device time between stream events.  The candidates are each query's own related rows, so "
             "every path handles the same ratings; `both` counts the candidates that are their query's own pair "
             "(a full solve each); the last column is the ratio to `list_newton`, for a path with top-K to "
             "`list_newton_topk`." % (args.sizes, args.steps, args.warmup,
                                       (" (" + args.label + ")") if args.label else ""), "",
             "| workload | path | queries | candidates | both | ms per call | ns per candidate | x the list call |",
             "|---|---|---|---|---|---|---|---|"]
    for r in results:
        # (a path with top-K beside the list call with top-K)
        like = "list_newton_topk" if r["path"].endswith("_topk") else "list_newton"
        base = [b for b in results if b["path"] == like and (b["data"], b["model"], b["k"]) ==
                (r["data"], r["model"], r["k"])]
        lines.append("| %s %s k=%d | %s | %d | %d | %d | %.3f (%.3f .. %.3f) | %.2f | %s |" % (
            r["data"], r["model"], r["k"], r["path"], r["queries"], r["candidates"], r["both"], r["median_ms"],
            r["min_ms"], r["max_ms"], ns(r), ("%.2f" % (ns(r) / ns(base[0]))) if base else "-"))
    lines += ["", "Phases of the new call (fia_set_profiling events, mean ms per call over separate calls: the "
              "per-query records `k_newton_query<NewtonAdd>`, the partition -- classification, radix sort, segment "
              "starts --, the scoring `k_cand_newton_score` + `k_cand_newton_neither`, the `both` solves "
              "`k_cand_newton_both`, the top-K selection and merge):", "",
              "| workload | path | records | partition | score | both solves | top-K |", "|---|---|---|---|---|---|---|"]
    for r in results:
        if "phase_ms" in r:
            p = r["phase_ms"]
            lines.append("| %s %s k=%d | %s | %.3f | %.3f | %.3f | %.3f | %.3f |" % (
                r["data"], r["model"], r["k"], r["path"], p["records"], p["partition"], p["score"], p["both"],
                p["topk"]))
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
