"""Time the self-influence scan of every train row: fia_self_influence beside the same scan
written with fia_group_influence (one query and one singleton group per train row).

Workload: ml-1m-ex (synth.ML1M, 975,460 ratings), MF k=16 and NCF k=16 by default, all train rows
(--rows N takes the first N; --sizes MODEL:K,... other sizes with synthetic parameters).  Paths:

    group      fia_group_influence, Q = G = n rows: queries = the rows' pairs, groups {j}; group and
               first_order written, device time of the call only (the index arrays are built before)
    self       fia_self_influence with first_order, newton and error
    self_topk  fia_self_influence with K = 64 and no per-row array (full=False)

Every path of every size runs in a child process of its own under `timeout -k 10`; the first one
that fails ends the run.  In a child: warm-up calls, then --steps calls each between its own pair
of events on the stream, the device synchronised before the times are read; the median is
reported with the minimum and maximum.  Device memory: what the device reports as free before the
first call (after the caller's arrays exist) minus after the last one, i.e. what the context
reserved for the path (row table, scratch), and the bytes of the caller's arrays beside it.
Writes the table to --out and prints one JSON line.

    python tools/self_scan_time.py --steps 10 --warmup 3 --out profiles/self_influence.md
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

PATHS = ("group", "self", "self_topk")


def worker(args):
    import torch
    from influence import _lib, synth

    model, k = args.model, args.k
    d = synth.make_dataset(synth.ML1M, seed=0)
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
    N = int(t_u.numel())
    n = N if args.rows <= 0 else min(args.rows, N)
    f64 = lambda m: torch.empty(m, dtype=torch.float64, device=dev)
    caller = []
    if args.path == "group":
        qu, qi = t_u[:n].contiguous(), t_i[:n].contiguous()
        go = torch.arange(n + 1, dtype=torch.int64, device=dev)
        mo = torch.arange(n + 1, dtype=torch.int64, device=dev)
        mr = torch.arange(n, dtype=torch.int32, device=dev)
        newton, first = f64(n), f64(n)
        caller = [qu, qi, go, mo, mr, newton, first]
        call = lambda: ctx.group_influence(qu, qi, go, mo, mr, newton, first, None)
    else:
        rows = None if n == N else torch.arange(n, dtype=torch.int32, device=dev)
        if args.path == "self":
            first, newton, err = f64(n), f64(n), f64(n)
            caller = [first, newton, err] + ([rows] if rows is not None else [])
            call = lambda: ctx.self_influence(rows, first, newton, err)
        else:
            K = 64
            tp = torch.empty(K, dtype=torch.int64, device=dev)
            tix = torch.empty(K, dtype=torch.int64, device=dev)
            tv = f64(K)
            caller = [tp, tix, tv] + ([rows] if rows is not None else [])
            call = lambda: ctx.self_influence(rows, None, None, None, K, tp, tix, tv)
    torch.cuda.synchronize(dev)
    free0 = torch.cuda.mem_get_info(dev)[0]
    for _ in range(args.warmup):
        call()
    torch.cuda.synchronize(dev)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    for a, b in ev:
        a.record()
        call()
        b.record()
    torch.cuda.synchronize(dev)
    free1 = torch.cuda.mem_get_info(dev)[0]
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    out = dict(model=model, k=k, path=args.path, rows=n, n_train=N, steps=args.steps, warmup=args.warmup,
               median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1],
               context_reserved_bytes=int(free0 - free1),
               caller_bytes=int(sum(t.numel() * t.element_size() for t in caller)))
    if args.path != "self_topk":
        h = newton.cpu().numpy()
        out["finite"] = bool(np.isfinite(h).all())
        out["newton_checksum"] = float(np.abs(h).sum())
    else:
        out["top1"] = [int(tix[0].item()), float(tv[0].item())]
    print(json.dumps(out))
    ctx.close()


def mb(b):
    return "%.1f MB" % (b / 1e6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="MF:16,NCF:16")
    ap.add_argument("--paths", default=",".join(PATHS))
    ap.add_argument("--rows", type=int, default=0, help="first N train rows (0: all)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "self_influence.md"))
    ap.add_argument("--label", default="")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--model")
    ap.add_argument("--k", type=int)
    ap.add_argument("--path")
    args = ap.parse_args()
    if args.worker:
        return worker(args)

    results, failed = [], None
    for size in args.sizes.split(","):
        model, k = size.split(":")
        for path in args.paths.split(","):
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--worker",
                   "--model", model, "--k", k, "--path", path, "--rows", str(args.rows), "--steps", str(args.steps),
                   "--warmup", str(args.warmup)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            if r.returncode != 0:
                failed = dict(model=model, k=int(k), path=path, exit=r.returncode)
                break
            results.append(json.loads(r.stdout.strip().splitlines()[-1]))
        if failed:
            break

    lines = ["# Self-influence scan: fia_self_influence against the group call", "",
             "`tools/self_scan_time.py --sizes %s --rows %d --steps %d --warmup %d`%s on one MI355X; ml-1m-ex, "
             "median (min .. max) of the per-call device time between stream events." % (
                 args.sizes, args.rows, args.steps, args.warmup, (" (" + args.label + ")") if args.label else ""), "",
             "| size | rows | path | ms per call | µs per row | context reserved | caller arrays |",
             "|---|---|---|---|---|---|---|"]
    for r in results:
        lines.append("| %s k=%d | %d | %s | %.2f (%.2f .. %.2f) | %.3f | %s | %s |" % (
            r["model"], r["k"], r["rows"], r["path"], r["median_ms"], r["min_ms"], r["max_ms"],
            1e3 * r["median_ms"] / max(r["rows"], 1), mb(r["context_reserved_bytes"]), mb(r["caller_bytes"])))
    lines += ["", "| size | group / self | group / self_topk | newton checksums equal |", "|---|---|---|---|"]
    ratios = {}
    by = {(r["model"], r["k"], r["path"]): r for r in results}
    for (model, k) in sorted({(r["model"], r["k"]) for r in results}):
        g, s, t = (by.get((model, k, p)) for p in PATHS)
        ratio = lambda a, b: "%.2f" % (a["median_ms"] / b["median_ms"]) if a and b else "-"
        same = "-"
        if g and s:
            same = "yes" if g["newton_checksum"] == s["newton_checksum"] else "no (%.17g / %.17g)" % (
                g["newton_checksum"], s["newton_checksum"])
            ratios["%s%d" % (model, k)] = g["median_ms"] / s["median_ms"]
        lines.append("| %s k=%d | %s | %s | %s |" % (model, k, ratio(g, s), ratio(g, t), same))
    if failed:
        lines += ["", "The run ended at %s k=%d, path %s (exit status %d); nothing after it was started." % (
            failed["model"], failed["k"], failed["path"], failed["exit"])]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(dict(results=results, group_over_self=ratios, failed=failed)))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
