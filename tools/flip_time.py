"""Time fia_pair_flip beside fia_pair_batch on the same pairs.

Workloads: tools/pair_time.py's -- ml-1m-ex MF k=16 and yelp-ex NCF k=16 by default (synth.ML1M /
synth.YELP with synthetic parameters; --sizes DATA:MODEL:K,... for others), the first --queries
test ratings, the second item j of a pair as pair_time.second_items chooses it.  The yardstick is
what the flip sets cost without the call: fia_pair_batch on the same pairs with `influence` and a
top-16 written (rel_idx, x and diff too), from which a host would still have to sort each user's
list.  fia_pair_flip runs with margin NULL, max_set = --max-set and every output written.

Every size runs in a child process of its own under `timeout -k 10`; the first one that fails ends
the run.  In a child: warm-up calls of both, then --steps rounds, each round one fia_pair_flip and
one fia_pair_batch call, every call between its own pair of events on the stream, the device
synchronised before the times are read; the median is reported with the minimum and maximum.  Then
--steps more rounds with every profiling phase recorded give the per-phase means (those windows
carry the events' own cost): for the flip call solve / score / topk are the solves, the selection
and the re-solved sets.  Writes the table to --out and prints one JSON line.

    python tools/flip_time.py --steps 20 --warmup 3 --out profiles/flip.md
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

TOPK = 16
BINS = ((-1, -1), (0, 0), (1, 1), (2, 4), (5, 8), (9, 15), (16, 32), (33, 64))


def worker(args):
    import torch
    from influence import _lib, synth

    model, k, ms = args.model, args.k, args.max_set
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
    D3 = 3 * ctx.num_params() // 2
    f64 = lambda m: torch.empty(max(m, 1), dtype=torch.float64, device=dev)
    i64 = lambda m: torch.empty(max(m, 1), dtype=torch.int64, device=dev)
    i32 = lambda m: torch.empty(max(m, 1), dtype=torch.int32, device=dev)

    p_off, p_total = ctx.count_related_pair(qu, qi, qj)
    p_buf = (i32(p_total), f64(p_total), f64(Q * D3), f64(Q), i64(Q * TOPK), i64(Q * TOPK), f64(Q * TOPK))
    f_buf = dict(set_size=i32(Q), set_row=i32(Q * ms), set_val=f64(Q * ms), first_order=f64(Q), newton=f64(Q),
                 dtheta=f64(Q * D3), diff=f64(Q))
    user_rows = int((np.bincount(np.asarray(tu), minlength=U)[qu_h]).sum())
    calls = dict(
        flip=lambda: ctx.pair_flip(qu, qi, qj, ms, None, **f_buf),
        pair=lambda: ctx.pair_batch(qu, qi, qj, p_off, p_total, p_buf[0], p_buf[1], p_buf[2], p_buf[3], TOPK, p_buf[4],
                                    p_buf[5], p_buf[6]))
    names = ("flip", "pair")
    for _ in range(args.warmup):
        for n in names:
            calls[n]()
    torch.cuda.synchronize(dev)
    ev = {n: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
          for n in names}
    for s in range(args.steps):
        for n in names:
            a, b = ev[n][s]
            a.record()
            calls[n]()
            b.record()
    torch.cuda.synchronize(dev)
    res = dict(data=args.data, model=model, k=k, queries=Q, steps=args.steps, warmup=args.warmup, max_set=ms,
               related=dict(pair=int(p_total), flip=user_rows))
    for n in names:
        t = sorted(a.elapsed_time(b) for a, b in ev[n])
        res[n] = dict(median_ms=t[len(t) // 2], min_ms=t[0], max_ms=t[-1])
    # per-phase means, every phase recorded (a window of its own)
    for n in names:
        ctx.set_profiling(True)
        ctx.profile_read()
        for _ in range(args.steps):
            calls[n]()
        ph = ctx.profile_read()
        ctx.set_profiling(False)
        res[n]["phases_ms"] = {p: (ph[p][0] / args.steps) for p in ph}
    size = f_buf["set_size"][:Q].cpu().numpy()
    diff, first, newton = (f_buf[key][:Q].cpu().numpy() for key in ("diff", "first_order", "newton"))
    ok = size >= 0
    res["flip"].update(
        sizes={"%d..%d" % b if b[0] != b[1] else str(b[0]): int(((size >= b[0]) & (size <= b[1])).sum()) for b in BINS},
        mean_size=float(size[ok].mean()) if ok.any() else 0.0,
        flipped_first_order=int((ok & (diff + first < 0.0)).sum()), flipped_newton=int((ok & (diff + newton < 0.0)).sum()),
        finite_newton=int(np.isfinite(newton[ok]).sum()), checksum=float(np.nansum(first)))
    res["pair"]["checksum"] = float(np.nansum(p_buf[1][:p_total].cpu().numpy()))
    print(json.dumps(res))
    ctx.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="ml-1m-ex:MF:16,yelp-ex:NCF:16")
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-set", type=int, default=16)
    ap.add_argument("--limit", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flip.md"))
    ap.add_argument("--label", default="")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--data")
    ap.add_argument("--model")
    ap.add_argument("--k", type=int)
    args = ap.parse_args()
    if args.worker:
        return worker(args)

    results, failed = [], None
    for size in args.sizes.split(","):
        data, model, k = size.split(":")
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--worker",
               "--data", data, "--model", model, "--k", k, "--queries", str(args.queries), "--steps", str(args.steps),
               "--warmup", str(args.warmup), "--max-set", str(args.max_set)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            failed = dict(data=data, model=model, k=int(k), exit=r.returncode)
            break
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))

    ms = lambda t: "%.3f (%.3f .. %.3f)" % (t["median_ms"], t["min_ms"], t["max_ms"])
    lines = ["# Flip sets: fia_pair_flip beside fia_pair_batch on the same pairs", "",
             "`tools/flip_time.py --sizes %s --queries %d --steps %d --warmup %d --max-set %d`%s on one MI355X; median "
             "(min .. max) of the per-call device time between stream events, one process per workload, the two calls "
             "alternating.  fia_pair_flip: margin NULL, every output written.  fia_pair_batch (the yardstick): rel_idx, "
             "influence, x, diff and a top-%d written; a host-side sort of each user's list would come on top." % (
                 args.sizes, args.queries, args.steps, args.warmup, args.max_set,
                 (" (" + args.label + ")") if args.label else "", TOPK),
             "",
             "| workload | call | queries | ratings scored | ms per call |",
             "|---|---|---|---|---|"]
    for r in results:
        for n, label in (("flip", "fia_pair_flip"), ("pair", "fia_pair_batch")):
            lines.append("| %s %s k=%d | %s | %d | %d | %s |" % (
                r["data"], r["model"], r["k"], label, r["queries"], r["related"][n], ms(r[n])))
    lines += ["", "Ratio of the medians, flip over pair (the flip call scores R_u only and re-solves one system per "
              "non-empty set):", "", "| workload | ms ratio | ratings scored ratio |", "|---|---|---|"]
    for r in results:
        lines.append("| %s %s k=%d | %.3f | %.3f |" % (
            r["data"], r["model"], r["k"], r["flip"]["median_ms"] / r["pair"]["median_ms"],
            r["related"]["flip"] / max(r["related"]["pair"], 1)))
    lines += ["", "Per-phase means (ms per call) from a window of its own with every phase recorded -- the event "
              "pairs add their own cost, so the phases do not sum to the call times above.  fia_pair_flip: solve = "
              "k_pair_solve, score = k_flip_select, topk = k_flip_newton; fia_pair_batch: chunks = the related rows.",
              "", "| workload | call | chunks | solve | score | topk |", "|---|---|---|---|---|---|"]
    for r in results:
        for n, label in (("flip", "fia_pair_flip"), ("pair", "fia_pair_batch")):
            ph = r[n]["phases_ms"]
            lines.append("| %s %s k=%d | %s | %.4f | %.4f | %.4f | %.4f |" % (
                r["data"], r["model"], r["k"], label, ph["chunks"], ph["solve"], ph["score"], ph["topk"]))
    lines += ["", "Set sizes (max_set = %d, margin 0; -1: no set -- n = 0):" % args.max_set, "",
              "| workload | " + " | ".join("%d..%d" % b if b[0] != b[1] else str(b[0]) for b in BINS) +
              " | mean | flipped, first order | flipped, re-solved | finite newton |",
              "|---|" + "---|" * (len(BINS) + 4)]
    for r in results:
        f = r["flip"]
        lines.append("| %s %s k=%d | " % (r["data"], r["model"], r["k"]) + " | ".join(str(v) for v in f["sizes"].values()) +
                     " | %.2f | %d | %d | %d |" % (f["mean_size"], f["flipped_first_order"], f["flipped_newton"],
                                                   f["finite_newton"]))
    for r in results:
        lines += ["", "%s %s k=%d: sum of first_order %.9e, sum of the pair influences %.9e." % (
            r["data"], r["model"], r["k"], r["flip"]["checksum"], r["pair"]["checksum"])]
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
