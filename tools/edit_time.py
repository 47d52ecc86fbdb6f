"""Time fia_edit_influence beside fia_group_influence on the same groups.

Workloads: ml-1m-ex MF k=16 and yelp-ex NCF k=16 by default (synth.ML1M / synth.YELP with
synthetic parameters; --sizes DATA:MODEL:K,... for others), the first --queries test ratings, one
group per query unless said otherwise.  Paths (a child process each; the member counts 1 / 16 /
256 of a path run one after another inside its child):

    rem_edit      removal-only groups of m of the query's related rows (fewer where the query has
                  fewer) through fia_edit_influence, edit written
    rem_group     the same groups through fia_group_influence, group written
    add_edit      addition-only groups of m ratings, user side and item side alternating
    replace_edit  one related row removed and the same pair added with another rating
    shared_edit   the first --queries / 8 queries with 8 groups each (2 removals + 2 additions):
                  alternative edit sets against one prediction

Every path of every size runs in a child process of its own under `timeout -k 10`; the first one
that fails ends the run.  In a child: warm-up calls, then --steps calls each between its own pair
of events on the stream, the device synchronised before the times are read; the median is
reported with the minimum and maximum.  Writes the table to --out and prints one JSON line.

    python tools/edit_time.py --steps 20 --warmup 3 --out profiles/edit.md
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

PATHS = ("rem_edit", "rem_group", "add_edit", "replace_edit", "shared_edit")
MEMBERS = (1, 16, 256)


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
    per = 8 if args.path == "shared_edit" else 1
    Q = args.queries // per
    qu_h, qi_h = (np.ascontiguousarray(a[:Q], np.int32) for a in d["test"][:2])
    Q = int(qu_h.size)
    qu, qi = torch.from_numpy(qu_h).to(dev), torch.from_numpy(qi_h).to(dev)
    offsets, total = ctx.count_related(qu, qi)
    rel = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    ctx.related(qu, qi, offsets, rel)
    off_h, rel_h = offsets.cpu().numpy(), rel[:total].cpu().numpy()
    G = Q * per
    rng = np.random.default_rng(5)
    to = lambda a, dt: (torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev) if len(a)
                        else torch.empty(1, dtype=getattr(torch, np.dtype(dt).name), device=dev)[:0])
    go = to(np.arange(Q + 1) * per, np.int64)
    out_v = torch.empty(G, dtype=torch.float64, device=dev)

    def removals(m, shift=0):
        """per group of query q: its related rows [shift, shift + m) (clipped to the list)"""
        lists = [rel_h[min(off_h[q] + shift, off_h[q + 1]):min(off_h[q] + shift + m, off_h[q + 1])]
                 for q in range(Q)]
        return lists

    def additions(m):
        a = np.repeat(qu_h, m).reshape(Q, m).astype(np.int64)
        b = np.repeat(qi_h, m).reshape(Q, m).astype(np.int64)
        side = (np.arange(m) % 2)[None, :].repeat(Q, 0)
        a = np.where(side == 1, rng.integers(0, U, (Q, m)), a)      # item side: another user
        b = np.where(side == 0, rng.integers(0, I, (Q, m)), b)      # user side: another item
        y = rng.random((Q, m)) * 4.0 + 1.0
        return a, b, y

    def pack(rem_lists, add):
        """groups in (query, group) order -> the member arrays of one call"""
        ro = np.concatenate([[0], np.cumsum([len(r) for r in rem_lists])])
        rr = np.concatenate(rem_lists) if len(rem_lists) and ro[-1] else np.zeros(0, np.int32)
        if add is None:
            ao, au, ai, ay = np.zeros(G + 1, np.int64), [], [], []
        else:
            a, b, y = add
            ao = np.arange(G + 1) * a.shape[1]
            au, ai, ay = a.reshape(-1), b.reshape(-1), y.reshape(-1)
        return (to(ro, np.int64), to(rr, np.int32), to(ao, np.int64), to(au, np.int32), to(ai, np.int32),
                to(ay, np.float32), int(ro[-1]), int(ao[-1]))

    cases = []
    if args.path in ("rem_edit", "rem_group"):
        for m in MEMBERS:
            cases.append((m, pack(removals(m), None)))
    elif args.path == "add_edit":
        for m in MEMBERS:
            cases.append((m, pack([np.zeros(0, np.int32)] * G, additions(m))))
    elif args.path == "replace_edit":
        rem = removals(1)
        rows = np.array([r[0] if len(r) else 0 for r in rem], np.int64)
        add = (np.asarray(tu)[rows].reshape(Q, 1).astype(np.int64), np.asarray(ti)[rows].reshape(Q, 1).astype(np.int64),
               np.asarray(tr)[rows].reshape(Q, 1) + 0.5)
        cases.append((1, pack(rem, add)))
    else:
        rem = [r for q_lists in zip(*[removals(2, 2 * j) for j in range(per)]) for r in q_lists]
        a, b, y = additions(2 * per)
        cases.append((2, pack(rem, (a.reshape(G, 2), b.reshape(G, 2), y.reshape(G, 2)))))

    results = []
    for m, (ro, rr, ao, au, ai, ay, n_rem, n_add) in cases:
        if args.path == "rem_group":
            call = lambda: ctx.group_influence(qu, qi, go, ro, rr, out_v, None, None)
        else:
            call = lambda: ctx.edit_influence(qu, qi, go, ro, rr, ao, au, ai, ay, out_v, None, None)
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
        h = out_v.cpu().numpy()
        results.append(dict(data=args.data, model=model, k=k, path=args.path, members=m, queries=Q, groups=G,
                            removals=n_rem, additions=n_add, steps=args.steps, warmup=args.warmup,
                            median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1],
                            finite_fraction=float(np.isfinite(h).mean()), checksum=float(np.nansum(h))))
    print(json.dumps(results))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="ml-1m-ex:MF:16,yelp-ex:NCF:16")
    ap.add_argument("--paths", default=",".join(PATHS))
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit.md"))
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
                   "--data", data, "--model", model, "--k", k, "--path", path, "--queries", str(args.queries),
                   "--steps", str(args.steps), "--warmup", str(args.warmup)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            if r.returncode != 0:
                failed = dict(data=data, model=model, k=int(k), path=path, exit=r.returncode)
                break
            results += json.loads(r.stdout.strip().splitlines()[-1])
        if failed:
            break

    lines = ["# Edit sets: fia_edit_influence beside fia_group_influence", "",
             "`tools/edit_time.py --sizes %s --queries %d --steps %d --warmup %d`%s on one MI355X; median (min .. "
             "max) of the per-call device time between stream events, one process per path; `edit` / `group` "
             "written, no first_order, no dtheta, no top-K." % (
                 args.sizes, args.queries, args.steps, args.warmup, (" (" + args.label + ")") if args.label else ""),
             "",
             "| workload | path | members per group | queries | groups | removals | additions | ms per call | us per group |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        lines.append("| %s %s k=%d | %s | %d | %d | %d | %d | %d | %.3f (%.3f .. %.3f) | %.2f |" % (
            r["data"], r["model"], r["k"], r["path"], r["members"], r["queries"], r["groups"], r["removals"],
            r["additions"], r["median_ms"], r["min_ms"], r["max_ms"], 1e3 * r["median_ms"] / max(r["groups"], 1)))
    key = lambda r: (r["data"], r["model"], r["k"], r["members"])
    grp = {key(r): r for r in results if r["path"] == "rem_group"}
    lines += ["", "Removal-only groups, fia_edit_influence against fia_group_influence on the same groups "
              "(ratio of the medians; the sums of the outputs agree to the digits shown):", "",
              "| workload | members per group | edit ms | group ms | ratio | sum(edit) | sum(group) |", "|---|---|---|---|---|---|---|"]
    for r in results:
        if r["path"] == "rem_edit" and key(r) in grp:
            g = grp[key(r)]
            lines.append("| %s %s k=%d | %d | %.3f | %.3f | %.3f | %.9e | %.9e |" % (
                r["data"], r["model"], r["k"], r["members"], r["median_ms"], g["median_ms"],
                r["median_ms"] / g["median_ms"], r["checksum"], g["checksum"]))
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
