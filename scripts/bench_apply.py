"""Times GrB_apply on R-MAT graphs (GPU box) and writes profiles/r07/apply.json + apply.md.

Per scale, five cases:
    times FP32   A.apply(times, right=0.85f)    FP32 graph    by value   (method 13)
    times INT64  A.apply(times, right=3)        INT64 graph   by value   (method 13)
    gt -> BOOL   A.apply(gt, right=128f)        FP32 graph    by value   (method 13)
    rowindex     A.apply(rowindex)              FP32 graph    by position (method 14)
    colindex     A.apply(colindex)              FP32 graph    by position (method 14)
each against two things that are not the code under test: ``A.dup()`` of the same matrix, which moves the same structure and value bytes
and is the floor a by-value apply can approach, and the round trip through the host a user takes without apply, ``to_coo`` -> numpy ->
``from_coo``.  Each figure is the median of >= 7 runs after warm-up with min and max beside it (HIP events around the call,
GrX_timer_start / GrX_timer_stop, for apply and dup; wall clock for the host route); the routes are timed alternately.

Moved bytes (algorithmic), m rows, nnz entries, X the operator's type, T the result's: the structure copy reads and writes 8 (m + 1) +
4 nnz each; by value reads sizeof X and writes sizeof T per entry; rowindex reads the 8 (m + 1) row pointers and writes 8 per entry;
colindex reads 4 and writes 8 per entry.  The time is the whole call (``.new()`` included), so bytes / time is an end-to-end rate.
No ratio is a pass mark: the table records ms, bytes / time and the ratio to dup().

Every scale runs in a process of its own under a time limit; the first failure stops the run.

    python scripts/bench_apply.py [--scales 20,22] [--runs 7] [--step-timeout 420] [--out profiles/r07]
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

CASES = ("times_fp32", "times_int64", "gt_bool", "rowindex", "colindex")
LABEL = {"times_fp32": "times, right=0.85 (FP32)", "times_int64": "times, right=3 (INT64)", "gt_bool": "gt, right=128 (FP32 -> BOOL)",
         "rowindex": "rowindex (-> INT64)", "colindex": "colindex (-> INT64)"}


def summary(ms):
    return {"ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def step(scale, runs):
    import numpy as np

    import graphblas_amd as gb
    from graphblas_amd import device, synthetic

    gb.init()
    n = 1 << scale
    ip, col = synthetic.rmat_csr(scale, seed=scale, device="cuda")
    w = synthetic.edge_weights(col, scale)
    A32 = device.matrix_from_device_csr(ip, col, w, n, n, "FP32").dup()  # (copies the library owns)
    A64 = device.matrix_from_device_csr(ip, col, w.long(), n, n, "INT64").dup()
    nnz = A32.nvals
    struct = 2 * (8 * (n + 1) + 4 * nnz)

    def host_route(A, fn, dtype):
        r, c, x = A.to_coo()
        return gb.Matrix.from_coo(r, c, fn(r, c, x), dtype=dtype, nrows=n, ncols=n)

    s85, three, thr = np.float32(0.85), np.int64(3), np.float32(128)
    table = {
        "times_fp32": (A32, lambda: A32.apply(gb.binary.times, right=s85).new(), lambda r, c, x: x * s85, "FP32", struct + 8 * nnz),
        "times_int64": (A64, lambda: A64.apply(gb.binary.times, right=three).new(), lambda r, c, x: x * three, "INT64", struct + 16 * nnz),
        "gt_bool": (A32, lambda: A32.apply(gb.binary.gt, right=thr).new(), lambda r, c, x: x > thr, "BOOL", struct + 5 * nnz),
        "rowindex": (A32, lambda: A32.apply(gb.indexunary.rowindex).new(), lambda r, c, x: r.astype(np.int64), "INT64", struct + 8 * (n + 1) + 8 * nnz),
        "colindex": (A32, lambda: A32.apply(gb.indexunary.colindex).new(), lambda r, c, x: c.astype(np.int64), "INT64", struct + 12 * nnz),
    }

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

    out = {"scale": scale, "runs": runs, "nnz": nnz, "cases": {}}
    for name in CASES:
        A, apply, host_fn, dtype, nbytes = table[name]

        def dup():
            return A.dup()

        def host():
            return host_route(A, host_fn, dtype)

        for fn in (apply, dup):  # warm-up: code objects, the block cache
            for _ in range(2):
                r = fn()
                del r
        t_new, t_dup, t_host = [], [], []
        for k in range(runs):
            ms, r = timed_once(apply)
            t_new.append(ms)
            del r
            ms, r = timed_once(dup)
            t_dup.append(ms)
            del r
            if k < 2:  # (the host route takes seconds: two runs of it)
                ms, r = wall_once(host)
                t_host.append(ms)
                del r
        T = apply()
        st = device.last_stats()
        same = bool(T.isequal(host(), check_dtype=True))
        s = summary(t_new)
        d = summary(t_dup)
        s.update(method=st["method"], units=st["tiles"], launches=st["kernel_launches"], bytes=nbytes, TBps=nbytes / s["ms"] / 1e9, dup=d,
                 ratio_to_dup=s["ms"] / d["ms"], host=summary(t_host), host_runs=len(t_host), same_result=same)
        out["cases"][name] = s
        del T
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
    with open(os.path.join(out_dir, "apply.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(out_dir, "apply.md"), "w") as f:
        f.write("# Matrix apply on the MI355X (scripts/bench_apply.py)\n\n")
        f.write(f"Median of {runs} runs after warm-up (min - max in brackets); HIP events around the whole call (`.new()` included) for apply and "
                "for `A.dup()` of the same matrix, wall clock for the `to_coo` -> numpy -> `from_coo` round trip (2 runs); the routes are timed "
                "alternately.  R-MAT, edge factor 16, weights U{1..255}.  Bytes are algorithmic (see the script); bytes / time is an end-to-end "
                "rate of the call.  No ratio is a pass mark.\n\n")
        if not res["steps"]:
            f.write("NOT TIMED YET.\n")
        else:
            f.write("| scale | entries | case | method | units | launches | apply ms | GB | TB/s | dup ms | apply / dup | host round trip ms | same result |\n")
            f.write("|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for s in res["steps"]:
            for name in CASES:
                x = s["cases"][name]
                y, z = x["dup"], x["host"]
                f.write(f"| {s['scale']} | {s['nnz']} | {LABEL[name]} | {x['method']} | {x['units']} | {x['launches']} | "
                        f"{x['ms']:.3f} [{x['min_ms']:.3f} - {x['max_ms']:.3f}] | {x['bytes'] / 1e9:.3f} | {x['TBps']:.3f} | "
                        f"{y['ms']:.3f} [{y['min_ms']:.3f} - {y['max_ms']:.3f}] | {x['ratio_to_dup']:.2f} | "
                        f"{z['ms']:.1f} [{z['min_ms']:.1f} - {z['max_ms']:.1f}] | {x['same_result']} |\n")
        if "failed" in res:
            f.write(f"\nThe run stopped at scale {res['failed']['scale']} (exit status {res['failed']['exit']}): NOT TIMED YET from there on.\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
