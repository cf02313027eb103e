"""Times GrB_kronecker on pairs of R-MAT graphs (GPU box) and writes profiles/r07/kronecker.json + kronecker.md.

Per pair of scales (10 (x) 10 and 8 (x) 12 by default: about 1.4 * 10^8 entries once the generator has folded duplicates), four cases:
    times FP32   A.kronecker(B, times)    FP32 operands     the value fill            (method 20)
    times INT64  A.kronecker(B, times)    INT64 operands    the value fill            (method 20)
    pair         A.kronecker(B, pair)     FP32 operands     iso: the columns alone    (method 6)
    gt -> BOOL   A.kronecker(B, gt)       FP32 operands     the value fill, 1 byte    (method 20)
each against two things that are not the code under test: ``T.dup()`` of the product itself in the same run -- dup READS and writes the
bytes that kronecker only writes, so a fill slower than the dup of its own result is bound by its index arithmetic or its walk, not by
its stores -- and the round trip through the host a user takes without kronecker: ``to_coo`` of both operands -> the numpy restatement
(rows ``ra * mb + rb``, columns ``ca * nb + cb``, the operator) -> ``from_coo``.  Each figure is the median of >= 7 whole calls after
warm-up with min and max beside it (HIP events around the call, GrX_timer_start / GrX_timer_stop, for kronecker and dup; wall clock for
the host route, which takes a minute: one run, on the FP32 times case only); the routes are timed alternately.

Written bytes (algorithmic): 8 (ma mb + 1) row pointers + nnz(T) (4 + sizeof T); the iso case writes 4 per entry.  The time is the whole
call (``.new()`` included), so bytes / time is an end-to-end rate.  No ratio is a pass mark: the table records ms, bytes / time and the
ratio to dup().

Every pair runs in a process of its own under a time limit; the first failure stops the run.

    python scripts/bench_kronecker.py [--pairs 10x10,8x12] [--runs 7] [--step-timeout 420] [--no-host] [--out profiles/r07]
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

CASES = ("times_fp32", "times_int64", "pair", "gt_bool")
LABEL = {"times_fp32": "times (FP32)", "times_int64": "times (INT64)", "pair": "pair (iso, columns alone)", "gt_bool": "gt (FP32 -> BOOL)"}


def summary(ms):
    return {"ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def step(sa, sb, runs, host_runs):
    import numpy as np

    import graphblas_amd as gb
    from graphblas_amd import device, synthetic

    gb.init()

    def operand(scale, dtype):
        n = 1 << scale
        ip, col = synthetic.rmat_csr(scale, seed=scale, device="cuda")
        w = synthetic.edge_weights(col, scale)
        return device.matrix_from_device_csr(ip, col, w if dtype == "FP32" else w.long(), n, n, dtype).dup()  # (copies the library owns)

    A32, B32, A64, B64 = operand(sa, "FP32"), operand(sb, "FP32"), operand(sa, "INT64"), operand(sb, "INT64")
    rows, nnz = (1 << sa) * (1 << sb), A32.nvals * B32.nvals

    def host_route(A, B, fn, dtype):
        ra, ca, xa = A.to_coo()
        rb, cb, xb = B.to_coo()
        r = (ra[:, None] * B.nrows + rb[None, :]).ravel()
        c = (ca[:, None] * B.ncols + cb[None, :]).ravel()
        return gb.Matrix.from_coo(r, c, fn(xa[:, None], xb[None, :]).ravel(), dtype=dtype, nrows=A.nrows * B.nrows, ncols=A.ncols * B.ncols)

    ptr = 8 * (rows + 1)
    table = {
        "times_fp32": (lambda: A32.kronecker(B32, gb.binary.times).new(), (A32, B32, lambda x, y: x * y, "FP32"), ptr + 8 * nnz),
        "times_int64": (lambda: A64.kronecker(B64, gb.binary.times).new(), None, ptr + 12 * nnz),
        "pair": (lambda: A32.kronecker(B32, gb.binary.pair).new(), None, ptr + 4 * nnz),
        "gt_bool": (lambda: A32.kronecker(B32, gb.binary.gt).new(), None, ptr + 5 * nnz),
    }

    def timed_once(fn):
        device.synchronize()
        device.timer_start()
        r = fn()
        return device.timer_stop(), r

    out = {"scales": [sa, sb], "runs": runs, "nnz": nnz, "nnz_a": A32.nvals, "nnz_b": B32.nvals, "cases": {}}
    for name in CASES:
        kron, host_args, nbytes = table[name]
        T = kron()
        st = device.last_stats()

        def dup():
            return T.dup()

        for fn in (kron, dup):  # warm-up: code objects, the block cache
            for _ in range(2):
                r = fn()
                del r
        t_new, t_dup, t_host = [], [], []
        for _ in range(runs):
            ms, r = timed_once(kron)
            t_new.append(ms)
            del r
            ms, r = timed_once(dup)
            t_dup.append(ms)
            del r
        same = None
        if host_args is not None:
            for _ in range(host_runs):
                device.synchronize()
                t0 = time.perf_counter()
                try:
                    H = host_route(*host_args)
                except MemoryError:  # (the tuples of 3 * 10^8 entries take some 10 GB of host memory: NOT MEASURED where that is not there)
                    break
                device.synchronize()
                t_host.append((time.perf_counter() - t0) * 1e3)
                same = bool(T.isequal(H, check_dtype=True))
                del H
        s = summary(t_new)
        d = summary(t_dup)
        s.update(method=st["method"], units=st["tiles"], launches=st["kernel_launches"], bytes=nbytes, TBps=nbytes / s["ms"] / 1e9, dup=d,
                 ratio_to_dup=s["ms"] / d["ms"], host=summary(t_host) if t_host else None, host_runs=len(t_host), same_result=same)
        out["cases"][name] = s
        print(f"{name}: {s['ms']:.3f} ms, dup {d['ms']:.3f} ms", flush=True)
        del T
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="10x10,8x12")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--step-timeout", type=int, default=420)
    ap.add_argument("--no-host", action="store_true", help="skip the host round trip (written as NOT MEASURED)")
    ap.add_argument("--out", default="profiles/r07")
    ap.add_argument("--step", default=None, help="(internal) a pair of scales: run one step in this process")
    args = ap.parse_args()
    runs = max(7, args.runs)
    host_runs = 0 if args.no_host else 1
    if args.step:
        sa, sb = (int(x) for x in args.step.split("x"))
        step(sa, sb, runs, host_runs)
        return 0
    out_dir = os.path.join(ROOT, args.out)
    os.makedirs(out_dir, exist_ok=True)
    res = {"runs": runs, "steps": []}
    rc = 0
    for pair in [p for p in args.pairs.split(",") if p]:
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", pair, "--runs", str(runs)]
        cmd += ["--no-host"] if args.no_host else []
        p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            print(p.stdout[-4000:])
            print(f"step {pair} failed with exit status {p.returncode}: stopping", flush=True)
            res["failed"] = {"pair": pair, "exit": p.returncode}
            rc = 1
            break
        res["steps"].append(json.loads(lines[-1][len("RESULT "):]))
        print(lines[-1], flush=True)
    with open(os.path.join(out_dir, "kronecker.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(out_dir, "kronecker.md"), "w") as f:
        f.write("# Matrix kronecker on the MI355X (scripts/bench_kronecker.py)\n\n")
        f.write(f"Median of {runs} whole calls after warm-up (min - max in brackets); HIP events around the call (`.new()` included) for kronecker "
                "and for `T.dup()` of the product itself, wall clock for the `to_coo` -> numpy -> `from_coo` round trip (one run, FP32 times "
                "only); the routes are timed alternately.  R-MAT, edge factor 16, weights U{1..255}.  Bytes are the algorithmic WRITTEN bytes "
                "(see the script); bytes / time is an end-to-end rate of the call.  `dup()` reads and writes what kronecker only writes.  No "
                "ratio is a pass mark.\n\n")
        if not res["steps"]:
            f.write("NOT MEASURED.\n")
        else:
            f.write("| scales | entries | case | method | units | launches | kronecker ms | GB written | TB/s | dup ms | kronecker / dup | host round trip ms | same result |\n")
            f.write("|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for s in res["steps"]:
            for name in CASES:
                x = s["cases"][name]
                y, z = x["dup"], x["host"]
                host = f"{z['ms']:.0f}" if z else "NOT MEASURED"
                same = x["same_result"] if x["same_result"] is not None else "NOT MEASURED"
                f.write(f"| {s['scales'][0]} (x) {s['scales'][1]} | {s['nnz']} | {LABEL[name]} | {x['method']} | {x['units']} | {x['launches']} | "
                        f"{x['ms']:.3f} [{x['min_ms']:.3f} - {x['max_ms']:.3f}] | {x['bytes'] / 1e9:.3f} | {x['TBps']:.3f} | "
                        f"{y['ms']:.3f} [{y['min_ms']:.3f} - {y['max_ms']:.3f}] | {x['ratio_to_dup']:.2f} | {host} | {same} |\n")
        if "failed" in res:
            f.write(f"\nThe run stopped at the pair {res['failed']['pair']} (exit status {res['failed']['exit']}): NOT MEASURED from there on.\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
