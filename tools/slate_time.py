"""Time fia_slate_batch: beside fia_pair_batch at m = 2, beside fia_query_batch at m = 1, and alone at
longer slates.

Workloads: ml-1m-ex MF k=16 and yelp-ex NCF k=16 with m in {2, 1, 10, 64}, and ml-1m-ex MF k=64 and
NCF k=32 (the sizes fia_pair_batch refuses) with m in {2, 10}, by default (synth.ML1M / synth.YELP
with synthetic parameters; --sizes DATA:MODEL:K:M+M+..,... for others), the first --queries test
ratings (u, i).  The slates:
  m = 2   (i, j) with weights (1, -1), j as tools/pair_time.py picks it: fia_pair_batch's system, the
          two calls alternating (only at the sizes where the pair call exists)
  m = 1   (i) with weight 1: fia_query_batch's system, the two calls alternating
  m > 2   the first m items from i + 1 on (modulo the item count) that u has not rated, DCG weights
          1 / log2(rank + 2): a recommended list, block diagonal

Every size runs in a child process of its own under `timeout -k 10`; the first one that fails ends
the run.  In a child, per m: warm-up calls, then --steps rounds, every call between its own pair of
events on the stream, the device synchronised before the times are read; the median is reported
with the minimum and maximum.  Every call writes rel_idx, influence, x and a top-1 (and value /
diff).  Then --steps more rounds with every profiling phase recorded give the per-phase means
(those windows carry the events' own cost).  Writes the table to --out and prints one JSON line;
--render FILE writes the table again from such a line, without a GPU run.

    python tools/slate_time.py --steps 20 --warmup 3 --out profiles/slate.md
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fia-kdd-19_amd"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from pair_time import second_items  # noqa: E402

PAIR_SIZES = {("MF", 8), ("MF", 16), ("MF", 32), ("NCF", 8), ("NCF", 16)}


def unrated_slates(tu, ti, qu, qi, n_items, m):
    """Per query the first m items from i + 1 on (modulo n_items) that the user has not rated."""
    rated = {}
    for u in set(int(a) for a in qu):
        rated[u] = set()
    for a, b in zip(tu, ti):
        if int(a) in rated:
            rated[int(a)].add(int(b))
    out = np.empty((len(qu), m), np.int32)
    for t, (u, i) in enumerate(zip(qu, qi)):
        r, b, got = rated[int(u)], int(i), 0
        for _ in range(n_items):
            b = (b + 1) % n_items
            if b not in r and b != int(i):
                out[t, got] = b
                got += 1
                if got == m:
                    break
        assert got == m, "user %d has fewer than %d unrated items" % (u, m)
    return out


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
    Q = min(args.queries, len(d["test"][0]))
    qu_h, qi_h = (np.ascontiguousarray(a[:Q], np.int32) for a in d["test"][:2])
    qj_h = second_items(np.asarray(d["test"][0]), np.asarray(d["test"][1]), I, Q)
    qu, qi, qj = (torch.from_numpy(a).to(dev) for a in (qu_h, qi_h, qj_h))
    D = ctx.num_params()
    Ds = D // 2
    f64 = lambda n: torch.empty(max(n, 1), dtype=torch.float64, device=dev)
    i64 = lambda n: torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    i32 = lambda n: torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    res = dict(data=args.data, model=model, k=k, queries=Q, steps=args.steps, warmup=args.warmup, runs=[])
    for m in [int(v) for v in args.ms.split("+")]:
        if m == 1:
            items_h, w_h = qi_h.reshape(Q, 1), np.ones((Q, 1))
        elif m == 2:
            items_h, w_h = np.stack([qi_h, qj_h], 1), np.tile([1.0, -1.0], (Q, 1))
        else:
            items_h = unrated_slates(tu, ti, qu_h, qi_h, I, m)
            w_h = np.tile(1.0 / np.log2(np.arange(m) + 2.0), (Q, 1))
        so = torch.from_numpy(np.arange(Q + 1, dtype=np.int64) * m).to(dev)
        it = torch.from_numpy(np.ascontiguousarray(items_h.reshape(-1), np.int32)).to(dev)
        wt = torch.from_numpy(np.ascontiguousarray(w_h.reshape(-1), np.float64)).to(dev)
        s_off, s_total = ctx.count_related_slate(qu, so, it)
        s_buf = (i32(s_total), f64(s_total), f64(Ds * (Q * m + Q)), f64(Q), i64(Q), i64(Q), f64(Q))
        calls = dict(
            slate=lambda: ctx.slate_batch(qu, so, it, wt, s_off, s_total, s_buf[0], s_buf[1], s_buf[2], s_buf[3], 1,
                                          s_buf[4], s_buf[5], s_buf[6]),
            slate_count=lambda: ctx.count_related_slate(qu, so, it, s_off, want_total=False))
        related = dict(slate=int(s_total))
        other = None
        if m == 2 and (model, k) in PAIR_SIZES:
            other = "pair"
            o_off, o_total = ctx.count_related_pair(qu, qi, qj)
            o_buf = (i32(o_total), f64(o_total), f64(Q * 3 * D // 2), f64(Q), i64(Q), i64(Q), f64(Q))
            calls["pair"] = lambda: ctx.pair_batch(qu, qi, qj, o_off, o_total, o_buf[0], o_buf[1], o_buf[2], o_buf[3],
                                                   1, o_buf[4], o_buf[5], o_buf[6])
            calls["pair_count"] = lambda: ctx.count_related_pair(qu, qi, qj, o_off, want_total=False)
        elif m == 1:
            other = "query"
            o_off, o_total = ctx.count_related(qu, qi)
            o_buf = (i32(o_total), f64(o_total), f64(Q * D), i64(Q), i64(Q), f64(Q))
            calls["query"] = lambda: ctx.query_batch(qu, qi, o_off, o_total, o_buf[0], o_buf[1], o_buf[2], 1, o_buf[3],
                                                     o_buf[4], o_buf[5])
            calls["query_count"] = lambda: ctx.count_related(qu, qi, o_off, want_total=False)
        if other:
            related[other] = int(o_total)
        names = ["slate", "slate_count"] + ([other, other + "_count"] if other else [])
        for _ in range(args.warmup):
            for n in names:
                calls[n]()
        torch.cuda.synchronize(dev)
        ev = {n: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                  for _ in range(args.steps)] for n in names}
        for s in range(args.steps):
            for n in names:
                a, b = ev[n][s]
                a.record()
                calls[n]()
                b.record()
        torch.cuda.synchronize(dev)
        run = dict(m=m, other=other, related=related)
        for n in names:
            t = sorted(a.elapsed_time(b) for a, b in ev[n])
            run[n] = dict(median_ms=t[len(t) // 2], min_ms=t[0], max_ms=t[-1])
        # per-phase means, every phase recorded (a window of its own)
        for n in ["slate"] + ([other] if other else []):
            ctx.set_profiling(True)
            ctx.profile_read()
            for _ in range(args.steps):
                calls[n + "_count"]()
                calls[n]()
            ph = ctx.profile_read()
            ctx.set_profiling(False)
            run[n]["phases_ms"] = {p: (ph[p][0] / args.steps) for p in ph}
        got = s_buf[1][:s_total].cpu().numpy()
        run["slate"]["finite_fraction"] = float(np.isfinite(got).mean()) if got.size else 1.0
        run["slate"]["checksum"] = float(np.nansum(got))
        if other:
            run[other]["checksum"] = float(np.nansum(o_buf[1][:o_total].cpu().numpy()))
        res["runs"].append(run)
    print(json.dumps(res))
    ctx.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="ml-1m-ex:MF:16:2+1+10+64,yelp-ex:NCF:16:2+1+10+64,ml-1m-ex:MF:64:2+10,"
                                       "ml-1m-ex:NCF:32:2+10")
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slate.md"))
    ap.add_argument("--label", default="")
    ap.add_argument("--render", default="", help="write the table from the JSON line of an earlier run; no GPU run")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--data")
    ap.add_argument("--model")
    ap.add_argument("--k", type=int)
    ap.add_argument("--ms")
    args = ap.parse_args()
    if args.worker:
        return worker(args)

    results, failed = [], None
    if args.render:
        with open(args.render) as f:
            saved = json.loads(f.read().strip().splitlines()[-1])
        results, failed = saved["results"], saved["failed"]
    for size in ([] if args.render else args.sizes.split(",")):
        data, model, k, ms_ = size.split(":")
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--worker",
               "--data", data, "--model", model, "--k", k, "--ms", ms_, "--queries", str(args.queries),
               "--steps", str(args.steps), "--warmup", str(args.warmup)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            failed = dict(data=data, model=model, k=int(k), exit=r.returncode)
            break
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))

    ms = lambda t: "%.3f (%.3f .. %.3f)" % (t["median_ms"], t["min_ms"], t["max_ms"])
    label = dict(slate="fia_slate_batch", pair="fia_pair_batch", query="fia_query_batch")
    lines = ["# Slate queries: fia_slate_batch beside fia_pair_batch (m = 2) and fia_query_batch (m = 1), and alone", "",
             "`tools/slate_time.py --sizes %s --queries %d --steps %d --warmup %d`%s on one MI355X; median (min .. max) "
             "of the per-call device time between stream events, one process per workload, the calls of a row pair "
             "alternating; rel_idx, influence, x and a top-1 written (and value / diff).  m = 2: (i, j) with weights "
             "(1, -1); m = 1: (i); m > 2: m consecutive items the user has not rated, DCG weights." % (
                 args.sizes, args.queries, args.steps, args.warmup, (" (" + args.label + ")") if args.label else ""),
             "",
             "| workload | m | call | queries | related ratings | ms per call | ns per related rating | count call ms |",
             "|---|---|---|---|---|---|---|---|"]
    for r in results:
        for run in r["runs"]:
            for n in ["slate"] + ([run["other"]] if run["other"] else []):
                lines.append("| %s %s k=%d | %d | %s | %d | %d | %s | %.3f | %s |" % (
                    r["data"], r["model"], r["k"], run["m"], label[n], r["queries"], run["related"][n], ms(run[n]),
                    1e6 * run[n]["median_ms"] / max(run["related"][n], 1), ms(run[n + "_count"])))
    lines += ["", "Ratio of the medians, fia_slate_batch over the call beside it (the same system, the same lists):", "",
              "| workload | m | beside | ms ratio |", "|---|---|---|---|"]
    for r in results:
        for run in r["runs"]:
            if run["other"]:
                lines.append("| %s %s k=%d | %d | %s | %.3f |" % (
                    r["data"], r["model"], r["k"], run["m"], label[run["other"]],
                    run["slate"]["median_ms"] / run[run["other"]]["median_ms"]))
    lines += ["", "Per-phase means (ms per call) from a window of its own with every phase recorded -- the event "
              "pairs add their own cost, so the phases do not sum to the call times above.  chunks = the count and "
              "scan (and, for the slate and pair calls, the related rows); MF k=16 fia_query_batch runs its chunk "
              "scan inside the solve's launch.  score ns = the scoring phase per related rating.", "",
              "| workload | m | call | chunks | solve | score | topk | score ns per related rating |",
              "|---|---|---|---|---|---|---|---|"]
    for r in results:
        for run in r["runs"]:
            for n in ["slate"] + ([run["other"]] if run["other"] else []):
                ph = run[n]["phases_ms"]
                lines.append("| %s %s k=%d | %d | %s | %.4f | %.4f | %.4f | %.4f | %.3f |" % (
                    r["data"], r["model"], r["k"], run["m"], label[n], ph["chunks"], ph["solve"], ph["score"],
                    ph["topk"], 1e6 * ph["score"] / max(run["related"][n], 1)))
    for r in results:
        for run in r["runs"]:
            tail = ""
            if run["other"]:
                tail = " (%s's %.9e)" % (label[run["other"]], run[run["other"]]["checksum"])
            lines += ["", "%s %s k=%d m=%d: finite fraction of the slate influences %.6f, sum %.9e%s." % (
                r["data"], r["model"], r["k"], run["m"], run["slate"]["finite_fraction"], run["slate"]["checksum"], tail)]
    if failed:
        lines += ["", "The run ended at %s %s k=%d (exit status %d); nothing after it was started." % (
            failed["data"], failed["model"], failed["k"], failed["exit"])]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(dict(results=results, failed=failed)))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
