"""Times the BFS parent loop over the positional semirings on R-MAT graphs (GPU box) and writes profiles/r07/bfs_parent.json + .md.

Per scale, on the directed R-MAT graph of synthetic.py (edge factor 16, BOOL iso values) from its heaviest row as the source:
    parent loop   parent[src] = src; q[src] = src; repeat  q(~parent.S, replace) << q.vxm(A, any_secondi);  parent(q.S) << q
                  until q is empty -- GrB_vxm (methods 25 / 26), GrB_Vector_assign, GrB_Vector_nvals through the C ABI
    level loop    the same loop with lor_land over BOOL vectors (the level BFS the benchmark is built around), same build, graph, source
    one step      the step of each loop at a small, a middle and the largest frontier (the frontier and the visited set of that level,
                  saved while the loop ran), under push_mode 0 (pull) and 2 (push)
    host route    A.to_coo() and a numpy BFS that records parents: what a user does without the positional semirings
Loops and steps: median of >= 7 runs after warm-up with min and max beside it, HIP events (GrX_timer_start / GrX_timer_stop) around
the whole loop / the one call; the host route: wall clock, one run.  No ratio is a pass mark: the table records what was measured.

Every scale runs in a process of its own under a time limit; the first failure stops the run.

    python scripts/bench_bfs_parent.py [--scales 20,22] [--runs 7] [--step-timeout 420] [--out profiles/r07]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(ms):
    return {"ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def step(scale, runs):
    import numpy as np

    import graphblas_amd as gb
    from graphblas_amd import _lib, device, synthetic

    gb.init()
    L = _lib.lib
    n = 1 << scale
    ip, col = synthetic.rmat_csr(scale, seed=scale, device="cuda")
    import torch

    A = device.matrix_from_device_csr(ip, col, torch.ones(1, dtype=torch.bool, device="cuda"), n, n, "BOOL", iso=True).dup()
    h_ip = ip.cpu().numpy().astype(np.int64)
    src = int(np.argmax(np.diff(h_ip)))
    nnz = A.nvals
    any_secondi, lor_land = gb.semiring.any_secondi, gb.semiring.lor_land

    def set_push(mode):
        assert L.GrX_option_set(b"push_mode", mode) == 0

    def parent_loop(keep=None):
        parent = gb.Vector.from_coo([src], [src], dtype="INT64", size=n)
        q = gb.Vector.from_coo([src], [src], dtype="INT64", size=n)
        methods = []
        while True:
            if keep is not None:
                keep.append((q.dup(), parent.dup(), q.nvals))
            q(~parent.S, replace=True) << q.vxm(A, any_secondi)
            methods.append(device.last_stats()["method"])
            if q.nvals == 0:
                return parent, methods
            parent(q.S) << q

    def level_loop(keep=None):
        visited = gb.Vector.from_coo([src], [True], dtype="BOOL", size=n)
        q = gb.Vector.from_coo([src], [True], dtype="BOOL", size=n)
        while True:
            if keep is not None:
                keep.append((q.dup(), visited.dup(), q.nvals))
            q(~visited.S, replace=True) << q.vxm(A, lor_land)
            if q.nvals == 0:
                return visited
            visited(q.S) << q

    def timed(fn):
        device.synchronize()
        device.timer_start()
        r = fn()
        return device.timer_stop(), r

    out = {"scale": scale, "runs": runs, "nnz": nnz, "source": src}
    set_push(1)
    pk, lk = [], []
    parent, methods = parent_loop(pk)
    visited = level_loop(lk)
    out["levels"] = len(pk)
    out["reached"] = parent.nvals
    out["same_reached_set"] = bool(np.array_equal(parent.to_coo()[0], visited.to_coo()[0]))
    out["methods_of_the_parent_loop"] = methods
    out["frontier_sizes"] = [k[2] for k in pk]
    for _ in range(2):  # warm-up: code objects, the block cache, the cached transpose
        parent_loop()
        level_loop()
    t_par, t_lev = [], []
    for _ in range(runs):
        t_par.append(timed(parent_loop)[0])
        t_lev.append(timed(level_loop)[0])
    out["parent_loop"], out["level_loop"] = summary(t_par), summary(t_lev)
    out["parent_over_level"] = out["parent_loop"]["ms"] / out["level_loop"]["ms"]

    # one step of each direction at a small, a middle and the largest frontier
    sizes = out["frontier_sizes"]
    largest = int(np.argmax(sizes))
    order = sorted(range(len(sizes)), key=lambda i: sizes[i])
    picks = {"small": 0, "middle": order[len(order) // 2], "largest": largest}
    out["steps"] = []
    for label, lev in picks.items():
        (q_p, par, fsz), (q_l, vis, _) = pk[lev], lk[lev]
        row = {"frontier": label, "level": lev, "entries": fsz}
        for mode, name in ((0, "pull"), (2, "push")):
            set_push(mode)

            def pos_step():
                w = gb.Vector("INT64", size=n)
                w(~par.S, replace=True) << q_p.vxm(A, any_secondi)
                return w

            def lvl_step():
                w = gb.Vector("BOOL", size=n)
                w(~vis.S, replace=True) << q_l.vxm(A, lor_land)
                return w

            for fn, key in ((pos_step, "any_secondi"), (lvl_step, "lor_land")):
                for _ in range(2):
                    fn()
                ts = []
                for _ in range(runs):
                    ms, w = timed(fn)
                    ts.append(ms)
                st = device.last_stats()
                s = summary(ts)
                s.update(method=st["method"], units=st["tiles"], flops=st["flops"], out_nvals=w.nvals)
                row[f"{key}_{name}"] = s
        out["steps"].append(row)
    set_push(1)

    # the host route: to_coo + a numpy BFS that records parents (any parent)
    device.synchronize()
    t0 = time.perf_counter()
    r, c, _ = A.to_coo()
    t_coo = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    cj = np.asarray(c, np.int64)
    hp = np.full(n, -1, np.int64)
    hp[src] = src
    f = np.array([src], np.int64)
    while f.size:
        lens = h_ip[f + 1] - h_ip[f]
        tot = int(lens.sum())
        if tot == 0:
            break
        first = np.repeat(h_ip[f] - (np.cumsum(lens) - lens), lens)
        nb = cj[first + np.arange(tot)]
        who = np.repeat(f, lens)
        new = hp[nb] < 0
        hp[nb[new]] = who[new]
        f = np.unique(nb[new])
    t_bfs = (time.perf_counter() - t0) * 1e3
    out["host_route"] = {"to_coo_ms": t_coo, "numpy_bfs_ms": t_bfs, "same_reached_set": bool(np.array_equal(np.flatnonzero(hp >= 0), parent.to_coo()[0]))}
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", default="20,22")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--step-timeout", type=int, default=420)
    ap.add_argument("--out", default="profiles/r07")
    ap.add_argument("--step", default=None, help="(internal) scale: run one step in this process")
    args = ap.parse_args()
    runs = max(7, args.runs)
    if args.step:
        step(int(args.step), runs)
        return 0
    out_dir = os.path.join(ROOT, args.out)
    os.makedirs(out_dir, exist_ok=True)
    res = {"runs": runs, "steps": []}
    rc = 0
    for scale in [int(s) for s in args.scales.split(",") if s]:
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", str(scale), "--runs", str(runs)]
        p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            print(p.stdout[-4000:])
            print(f"step scale {scale} failed with exit status {p.returncode}: stopping", flush=True)
            res["failed"] = {"scale": scale, "exit": p.returncode}
            rc = 1
            break
        res["steps"].append(json.loads(lines[-1][len("RESULT "):]))
        print(lines[-1], flush=True)
    with open(os.path.join(out_dir, "bfs_parent.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(out_dir, "bfs_parent.md"), "w") as f:
        f.write("# BFS parents over any_secondi on the MI355X (scripts/bench_bfs_parent.py)\n\n")
        f.write(f"Median of {runs} runs after warm-up (min - max in brackets), HIP events around the whole loop / the one call; directed R-MAT, edge "
                "factor 16, iso BOOL values, source = the heaviest row; push_mode 1 for the loops.  The host route (`to_coo`, then a numpy BFS that "
                "records parents) is wall clock, one run.  No ratio is a pass mark.\n\n")
        if not res["steps"]:
            f.write("NOT TIMED YET.\n")
        for s in res["steps"]:
            p, lv, h = s["parent_loop"], s["level_loop"], s["host_route"]
            f.write(f"## scale {s['scale']}: {s['nnz']} entries, {s['levels']} levels, {s['reached']} vertices reached\n\n")
            f.write("| loop | ms |\n|---|---|\n")
            f.write(f"| parent loop (any_secondi) | {p['ms']:.3f} [{p['min_ms']:.3f} - {p['max_ms']:.3f}] |\n")
            f.write(f"| level loop (lor_land) | {lv['ms']:.3f} [{lv['min_ms']:.3f} - {lv['max_ms']:.3f}] |\n")
            f.write(f"| parent / level | {s['parent_over_level']:.2f} |\n")
            f.write(f"| host route: to_coo + numpy BFS | {h['to_coo_ms']:.0f} + {h['numpy_bfs_ms']:.0f} |\n\n")
            f.write(f"Frontier sizes per level: {s['frontier_sizes']}; methods of the parent loop per level (25 pull, 26 push): "
                    f"{s['methods_of_the_parent_loop']}; same reached set as the level loop: {s['same_reached_set']}, as the host route: "
                    f"{h['same_reached_set']}.\n\n")
            f.write("| frontier | level | entries | direction | any_secondi ms | method | units | flops | lor_land ms | method |\n|---|---|---|---|---|---|---|---|---|---|\n")
            for row in s["steps"]:
                for name in ("pull", "push"):
                    a, b = row[f"any_secondi_{name}"], row[f"lor_land_{name}"]
                    f.write(f"| {row['frontier']} | {row['level']} | {row['entries']} | push_mode {0 if name == 'pull' else 2} | "
                            f"{a['ms']:.3f} [{a['min_ms']:.3f} - {a['max_ms']:.3f}] | {a['method']} | {a['units']} | {a['flops']} | "
                            f"{b['ms']:.3f} [{b['min_ms']:.3f} - {b['max_ms']:.3f}] | {b['method']} |\n")
            f.write("\n")
        if "failed" in res:
            f.write(f"\nThe run stopped at scale {res['failed']['scale']} (exit status {res['failed']['exit']}): NOT TIMED YET from there on.\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
