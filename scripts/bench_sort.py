"""Times GxB_Matrix_sort on R-MAT graphs (GPU box) and writes profiles/r07/sort.json + sort.md.

Per scale and value type (FP32, INT64), three operations:
    sort        A.ss.sort()                        both outputs (values and permutation)
    sort_values A.ss.sort(permutation=False)       values only
    largest8    A.ss.compactify("largest", 8)      sort under gt, select col <= 7, resize
each against two things that are not the code under test: ``A.dup()`` of the same matrix, the stream floor (it moves the structure and
the values once), and the route through the host a user takes without the operation: ``to_coo``, ``np.lexsort((value, row))``,
``from_coo``.  Each figure is the median of >= 7 runs after warm-up with min and max beside it (HIP events around the call,
GrX_timer_start / GrX_timer_stop, for the library calls; wall clock for the host route); the routes are timed alternately.
GrX_sort_last -- how many rows took the lane groups, the LDS path and the radix path -- is recorded per matrix.
No speed is promised in advance and no ratio is a pass mark: the table records ms and the ratios to dup() and to the host route.

Every (scale, type) runs in a process of its own under a time limit; the first failure stops the run.

    python scripts/bench_sort.py [--scales 20,22] [--runs 7] [--step-timeout 420] [--out profiles/r07]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ("sort", "sort_values", "largest8")
LABEL = {"sort": "A.ss.sort()", "sort_values": "A.ss.sort(permutation=False)", "largest8": 'A.ss.compactify("largest", 8)'}


def summary(ms):
    return {"ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def step(scale, tname, runs):
    import numpy as np

    import graphblas_amd as gb
    from graphblas_amd import _lib, device, synthetic

    gb.init()
    n = 1 << scale
    ip, col = synthetic.rmat_csr(scale, seed=scale, device="cuda")
    w = synthetic.edge_weights(col, scale)
    A = device.matrix_from_device_csr(ip, col, w if tname == "FP32" else w.long(), n, n, tname).dup()  # (a copy the library owns)
    nnz = A.nvals

    def host_route():
        r, c, x = A.to_coo()
        order = np.lexsort((x, r))  # (stable: ties keep the column order)
        first = np.searchsorted(r, r)
        pos = (np.arange(r.size) - first).astype(np.uint64)
        return gb.Matrix.from_coo(r, pos, x[order], dtype=tname, nrows=n, ncols=n), gb.Matrix.from_coo(r, pos, c[order], dtype="UINT64", nrows=n, ncols=n)

    table = {"sort": lambda: A.ss.sort(), "sort_values": lambda: A.ss.sort(permutation=False), "largest8": lambda: A.ss.compactify("largest", 8)}

    def timed_once(fn):
        device.synchronize()
        device.timer_start()
        r = fn()
        return device.timer_stop(), r

    def wall_once(fn):
        device.synchronize()
        t0 = time.perf_counter()
        r = fn()
        device.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def dup():
        return A.dup()

    out = {"scale": scale, "type": tname, "runs": runs, "nnz": nnz, "cases": {}}
    t_host = []
    for _ in range(2):  # (the host route takes seconds: two runs of it)
        ms, r = wall_once(host_route)
        t_host.append(ms)
    Ch, Ph = r
    C, P = A.ss.sort()
    last = (ctypes.c_int64 * 3)()
    _lib.lib.GrX_sort_last(last)
    out["rows_by_path"] = list(last)
    out["same_result"] = bool(C.isequal(Ch, check_dtype=True) and P.isequal(Ph, check_dtype=True))
    out["host"] = summary(t_host)
    del C, P, Ch, Ph, r
    for name in CASES:
        fn = table[name]
        for f in (fn, dup):  # warm-up: code objects, the block cache
            for _ in range(2):
                r = f()
                del r
        t_new, t_dup = [], []
        for _ in range(runs):
            ms, r = timed_once(fn)
            t_new.append(ms)
            del r
            ms, r = timed_once(dup)
            t_dup.append(ms)
            del r
        s, d = summary(t_new), summary(t_dup)
        s.update(dup=d, ratio_to_dup=s["ms"] / d["ms"], host_over_call=out["host"]["ms"] / s["ms"])
        out["cases"][name] = s
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", default="20,22")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--step-timeout", type=int, default=420)
    ap.add_argument("--out", default="profiles/r07")
    ap.add_argument("--step", default=None, help="(internal) scale:type: run one step in this process")
    args = ap.parse_args()
    runs = max(7, args.runs)
    if args.step:
        scale, tname = args.step.split(":")
        step(int(scale), tname, runs)
        return 0
    out_dir = os.path.join(ROOT, args.out)
    os.makedirs(out_dir, exist_ok=True)
    res = {"runs": runs, "steps": []}
    rc = 0
    for scale, tname in [(int(s), t) for s in args.scales.split(",") if s for t in ("FP32", "INT64")]:
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", f"{scale}:{tname}", "--runs", str(runs)]
        p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            print(p.stdout[-4000:])
            print(f"step scale {scale} {tname} failed with exit status {p.returncode}: stopping", flush=True)
            res["failed"] = {"scale": scale, "type": tname, "exit": p.returncode}
            rc = 1
            break
        res["steps"].append(json.loads(lines[-1][len("RESULT "):]))
        print(lines[-1], flush=True)
    with open(os.path.join(out_dir, "sort.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(out_dir, "sort.md"), "w") as f:
        f.write("# Sort by value on the MI355X (scripts/bench_sort.py)\n\n")
        f.write(f"Median of {runs} runs after warm-up (min - max in brackets); HIP events around the whole call for the sort, for compactify and for "
                "`A.dup()` of the same matrix, wall clock for the `to_coo` -> `np.lexsort` -> `from_coo` route (2 runs); the routes are timed "
                "alternately.  R-MAT, edge factor 16, weights U{1..255} (many ties).  No ratio is a pass mark.\n\n")
        if not res["steps"]:
            f.write("NOT TIMED YET.\n")
        else:
            f.write("| scale | type | entries | rows: lane groups / LDS / radix | operation | ms | dup ms | call / dup | host route ms | host / call | same result as the host route |\n")
            f.write("|---|---|---|---|---|---|---|---|---|---|---|\n")
        for s in res["steps"]:
            for name in CASES:
                x = s["cases"][name]
                y, z = x["dup"], s["host"]
                f.write(f"| {s['scale']} | {s['type']} | {s['nnz']} | {' / '.join(str(v) for v in s['rows_by_path'])} | {LABEL[name]} | "
                        f"{x['ms']:.3f} [{x['min_ms']:.3f} - {x['max_ms']:.3f}] | {y['ms']:.3f} [{y['min_ms']:.3f} - {y['max_ms']:.3f}] | "
                        f"{x['ratio_to_dup']:.2f} | {z['ms']:.1f} [{z['min_ms']:.1f} - {z['max_ms']:.1f}] | {x['host_over_call']:.0f} | {s['same_result']} |\n")
        if "failed" in res:
            f.write(f"\nThe run stopped at scale {res['failed']['scale']} {res['failed']['type']} (exit status {res['failed']['exit']}): NOT TIMED YET from there on.\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
