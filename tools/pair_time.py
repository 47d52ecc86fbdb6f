"""Time fia_pair_batch beside fia_query_batch on the same (u, i).

Workloads: ml-1m-ex MF k=16 and yelp-ex NCF k=16 by default (synth.ML1M / synth.YELP with
synthetic parameters; --sizes DATA:MODEL:K,... for others), the first --queries test ratings.  The
second item j of a pair is the next test item of the same user, or i + 1 modulo the item count
where there is none (or where that item is i itself).  fia_query_batch on the same (u, i) is the
yardstick: two blocks and two lists against three of each.

Every size runs in a child process of its own under `timeout -k 10`; the first one that fails ends
the run.  In a child: warm-up calls of both, then --steps rounds, each round one fia_pair_batch and
one fia_query_batch call, every call between its own pair of events on the stream, the device
synchronised before the times are read; the median is reported with the minimum and maximum.  Both
calls write rel_idx, influence, x and a top-1 (the pair call also diff).  The count calls
(fia_count_related_pair / fia_count_related, no total) are timed the same way.  Then --steps more
rounds with every profiling phase recorded give the per-phase means (those windows carry the
events' own cost).  Writes the table to --out and prints one JSON line.

    python tools/pair_time.py --steps 20 --warmup 3 --out profiles/pair.md
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


def second_items(users, items, n_items, Q):
    """j per test rating t < Q: the item of the next test rating of the same user, else i + 1 mod I."""
    nxt, last = np.full(len(users), -1, np.int64), {}
    for t in range(len(users) - 1, -1, -1):
        nxt[t] = last.get(int(users[t]), -1)
        last[int(users[t])] = t
    j = np.empty(Q, np.int32)
    for t in range(Q):
        cand = int(items[nxt[t]]) if nxt[t] >= 0 else -1
        j[t] = cand if cand >= 0 and cand != int(items[t]) else (int(items[t]) + 1) % n_items
    return j


def compulsory_bytes(model, k):
    """Bytes the scoring pass cannot avoid per related rating: the list entry (other endpoint 4 B,
    rating 4 B), the other endpoint's parameter row (MF: k floats + its bias; NCF: the GMF row of k
    floats and the fp64 layer-1 row of k doubles) and the influence written (8 B).  The query's own
    rows and its record are shared by the whole list."""
    return 4 + 4 + (4 * k + 4 if model == "MF" else 4 * k + 8 * k) + 8


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
    f64 = lambda m: torch.empty(max(m, 1), dtype=torch.float64, device=dev)
    i64 = lambda m: torch.empty(max(m, 1), dtype=torch.int64, device=dev)
    i32 = lambda m: torch.empty(max(m, 1), dtype=torch.int32, device=dev)

    p_off, p_total = ctx.count_related_pair(qu, qi, qj)
    q_off, q_total = ctx.count_related(qu, qi)
    p_buf = (i32(p_total), f64(p_total), f64(Q * 3 * D // 2), f64(Q), i64(Q), i64(Q), f64(Q))
    q_buf = (i32(q_total), f64(q_total), f64(Q * D), i64(Q), i64(Q), f64(Q))
    calls = dict(
        pair=lambda: ctx.pair_batch(qu, qi, qj, p_off, p_total, p_buf[0], p_buf[1], p_buf[2], p_buf[3], 1, p_buf[4],
                                    p_buf[5], p_buf[6]),
        query=lambda: ctx.query_batch(qu, qi, q_off, q_total, q_buf[0], q_buf[1], q_buf[2], 1, q_buf[3], q_buf[4],
                                      q_buf[5]),
        pair_count=lambda: ctx.count_related_pair(qu, qi, qj, p_off, want_total=False),
        query_count=lambda: ctx.count_related(qu, qi, q_off, want_total=False))
    names = ("pair", "query", "pair_count", "query_count")
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
    res = dict(data=args.data, model=model, k=k, queries=Q, steps=args.steps, warmup=args.warmup,
               related=dict(pair=int(p_total), query=int(q_total)), compulsory=compulsory_bytes(model, k))
    for n in names:
        ms = sorted(a.elapsed_time(b) for a, b in ev[n])
        res[n] = dict(median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1])
    # per-phase means, every phase recorded (a window of its own)
    for n in ("pair", "query"):
        ctx.set_profiling(True)
        ctx.profile_read()
        for _ in range(args.steps):
            calls[n + "_count"]()
            calls[n]()
        ph = ctx.profile_read()
        ctx.set_profiling(False)
        res[n]["phases_ms"] = {p: (ph[p][0] / args.steps) for p in ph}
    res["pair"]["finite_fraction"] = float(np.isfinite(p_buf[1][:p_total].cpu().numpy()).mean())
    res["pair"]["checksum"] = float(np.nansum(p_buf[1][:p_total].cpu().numpy()))
    res["query"]["checksum"] = float(np.nansum(q_buf[1][:q_total].cpu().numpy()))
    print(json.dumps(res))
    ctx.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="ml-1m-ex:MF:16,yelp-ex:NCF:16")
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair.md"))
    ap.add_argument("--label", default="")
    ap.add_argument("--score-bytes", default="",
                    help="DATA:MODEL:K=BYTES,...: bytes per related rating of k_pair_score from a counter pass "
                         "run on its own (else the column says not measured)")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--data")
    ap.add_argument("--model")
    ap.add_argument("--k", type=int)
    args = ap.parse_args()
    if args.worker:
        return worker(args)

    measured = dict(kv.split("=") for kv in args.score_bytes.split(",") if kv)
    results, failed = [], None
    for size in args.sizes.split(","):
        data, model, k = size.split(":")
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--worker",
               "--data", data, "--model", model, "--k", k, "--queries", str(args.queries), "--steps", str(args.steps),
               "--warmup", str(args.warmup)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            failed = dict(data=data, model=model, k=int(k), exit=r.returncode)
            break
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))

    ms = lambda t: "%.3f (%.3f .. %.3f)" % (t["median_ms"], t["min_ms"], t["max_ms"])
    lines = ["# Pair queries: fia_pair_batch beside fia_query_batch on the same (u, i)", "",
             "`tools/pair_time.py --sizes %s --queries %d --steps %d --warmup %d`%s on one MI355X; median (min .. max) "
             "of the per-call device time between stream events, one process per workload, the two calls alternating; "
             "rel_idx, influence, x and a top-1 written (the pair call also diff)." % (
                 args.sizes, args.queries, args.steps, args.warmup, (" (" + args.label + ")") if args.label else ""),
             "",
             "| workload | call | queries | related ratings | ms per call | ns per related rating | count call ms |",
             "|---|---|---|---|---|---|---|"]
    for r in results:
        for n, label in (("pair", "fia_pair_batch"), ("query", "fia_query_batch")):
            lines.append("| %s %s k=%d | %s | %d | %d | %s | %.2f | %s |" % (
                r["data"], r["model"], r["k"], label, r["queries"], r["related"][n], ms(r[n]),
                1e6 * r[n]["median_ms"] / max(r["related"][n], 1), ms(r[n + "_count"])))
    lines += ["", "Ratio of the medians, pair over query (the pair call solves three blocks and scores three lists):", "",
              "| workload | ms ratio | related ratings ratio |", "|---|---|---|"]
    for r in results:
        lines.append("| %s %s k=%d | %.3f | %.3f |" % (
            r["data"], r["model"], r["k"], r["pair"]["median_ms"] / r["query"]["median_ms"],
            r["related"]["pair"] / max(r["related"]["query"], 1)))
    lines += ["", "Per-phase means (ms per call) from a window of its own with every phase recorded -- the event "
              "pairs add their own cost, so the phases do not sum to the call times above.  chunks = the count and "
              "scan (and, for the pair call, the related rows); MF k=16 fia_query_batch runs its chunk scan inside "
              "the solve's launch.", "",
              "| workload | call | chunks | solve | score | topk |", "|---|---|---|---|---|---|"]
    for r in results:
        for n, label in (("pair", "fia_pair_batch"), ("query", "fia_query_batch")):
            ph = r[n]["phases_ms"]
            lines.append("| %s %s k=%d | %s | %.4f | %.4f | %.4f | %.4f |" % (
                r["data"], r["model"], r["k"], label, ph["chunks"], ph["solve"], ph["score"], ph["topk"]))
    lines += ["", "k_pair_score, bytes per related rating against the compulsory bytes (list entry, the other "
              "endpoint's parameter row, the influence written):", "",
              "| workload | compulsory B | measured B |", "|---|---|---|"]
    for r in results:
        key = "%s:%s:%d" % (r["data"], r["model"], r["k"])
        lines.append("| %s %s k=%d | %d | %s |" % (r["data"], r["model"], r["k"], r["compulsory"],
                                                    measured.get(key, "not measured")))
    for r in results:
        lines += ["", "%s %s k=%d: finite fraction of the pair influences %.6f, sum %.9e (fia_query_batch's %.9e)." % (
            r["data"], r["model"], r["k"], r["pair"]["finite_fraction"], r["pair"]["checksum"], r["query"]["checksum"])]
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
