"""Times GxB_Matrix_eWiseUnion, GrB_Matrix_diag and GxB_Vector_diag on R-MAT graphs (GPU box) and writes profiles/r07/union_diag.json +
union_diag.md.

Per (scale, type):
  * ``A.ewise_union(A.T, minus, 0, 0)`` against ``A.ewise_add(A.T, minus)`` on the same operands, timed alternately: the two make the same
    passes, so the expectation is the same time;
  * ``d.diag()`` (d = the row sums of A) and ``L.diag()`` (L = the Laplacian) against ``dup()`` of their own output; ``d.diag().diag()`` must
    give ``d`` back;
  * the Laplacian ``d.diag().ewise_union(A, minus, 0, 0)`` against the host round trip (``to_coo`` -> numpy -> ``from_coo``), run once.
Each figure is the median of >= 7 whole calls after warm-up with min and max beside it (HIP events on the library's stream:
GrX_timer_start / GrX_timer_stop); the transpose is cached before anything is timed.  Every (scale, type) step runs in a process of its
own under a time limit; the first failure stops the run.

    python scripts/bench_union_diag.py [--scales 20,22] [--types FP32,INT64] [--runs 7] [--step-timeout 420] [--out profiles/r07]
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


def step(scale, tname, runs):
    import numpy as np

    import graphblas_amd as gb
    from graphblas_amd import device, synthetic

    gb.init()
    n = 1 << scale
    ip, col = synthetic.rmat_csr(scale, seed=scale, device="cuda")
    w = synthetic.edge_weights(col, scale)
    A = device.matrix_from_device_csr(ip, col, w, n, n, "FP32").dup(dtype=tname)
    device.cache_transpose(A)
    zero = np.float32(0) if tname == "FP32" else 0  # (a default of the operands' own type: a Python float would make the operator FP64)
    minus = gb.binary.minus

    def timed(fn):
        device.synchronize()
        device.timer_start()
        r = fn()
        return device.timer_stop(), r

    def alternate(f, g):
        for fn in (f, g):
            for _ in range(2):
                r = fn()
                del r
        tf, tg = [], []
        for _ in range(runs):
            ms, r = timed(f)
            tf.append(ms)
            del r
            ms, r = timed(g)
            tg.append(ms)
            del r
        return summary(tf), summary(tg)

    out = {"scale": scale, "type": tname, "runs": runs, "nnz_A": A.nvals}
    out["union"], out["ewise_add"] = alternate(lambda: A.ewise_union(A.T, minus, zero, zero).new(), lambda: A.ewise_add(A.T, minus).new())
    U = A.ewise_union(A.T, minus, zero, zero).new()
    out["union_method"] = device.last_stats()["method"]
    out["nnz_union"] = U.nvals
    out["same_pattern_as_ewise_add"] = bool(U.nvals == A.ewise_add(A.T, minus).new().nvals)
    del U
    d = A.reduce_rowwise().new()
    D = d.diag()
    out["nnz_d"] = d.nvals
    out["vector_diag"], out["dup_of_D"] = alternate(lambda: d.diag(), lambda: D.dup())
    lap = lambda: d.diag().ewise_union(A, minus, zero, zero).new()  # noqa: E731
    L = lap()
    out["nnz_L"] = L.nvals
    v = L.diag()
    out["matrix_diag"], out["dup_of_v"] = alternate(lambda: L.diag(), lambda: v.dup())
    out["diag_round_trip_same"] = bool(D.diag().isequal(d))
    out["laplacian"], _ = alternate(lap, lambda: None)
    t0 = time.perf_counter()
    I, J, X = A.to_coo()
    di, dx = d.to_coo()
    rows, cols, vals = np.concatenate([di, I]), np.concatenate([di, J]), np.concatenate([dx, -X])
    H = gb.Matrix.from_coo(rows, cols, vals, dtype=tname, nrows=n, ncols=n, dup_op=gb.binary.plus)
    out["laplacian_host_ms"] = (time.perf_counter() - t0) * 1e3
    out["laplacian_same"] = bool(H.isequal(L))
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", default="20,22")
    ap.add_argument("--types", default="FP32,INT64")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--step-timeout", type=int, default=420)
    ap.add_argument("--out", default="profiles/r07")
    ap.add_argument("--step", default=None, help="(internal) scale,type: run one step in this process")
    args = ap.parse_args()
    runs = max(7, args.runs)
    if args.step:
        scale, tname = args.step.split(",")
        step(int(scale), tname, runs)
        return 0
    out_dir = os.path.join(ROOT, args.out)
    os.makedirs(out_dir, exist_ok=True)
    res = {"runs": runs, "steps": []}
    rc = 0
    for scale in [int(s) for s in args.scales.split(",") if s]:
        for tname in [t for t in args.types.split(",") if t]:
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", f"{scale},{tname}",
                   "--runs", str(runs)]
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
        if rc:
            break
    with open(os.path.join(out_dir, "union_diag.json"), "w") as f:
        json.dump(res, f, indent=1)

    def cell(x):
        return f"{x['ms']:.3f} [{x['min_ms']:.3f} - {x['max_ms']:.3f}]"

    with open(os.path.join(out_dir, "union_diag.md"), "w") as f:
        f.write("# eWiseUnion and diag on the MI355X (scripts/bench_union_diag.py)\n\n")
        f.write(f"Median of {runs} whole calls after warm-up (min - max in brackets), HIP events around the call (`.new()` included); the transpose "
                "cached before timing; R-MAT, edge factor 16, weights U{1..255}; one run.\n\n")
        f.write("| scale | type | entries A | A.ewise_union(A.T, minus, 0, 0) ms | A.ewise_add(A.T, minus) ms | union / add | entries T |\n|---|---|---|---|---|---|---|\n")
        for s in res["steps"]:
            f.write(f"| {s['scale']} | {s['type']} | {s['nnz_A']} | {cell(s['union'])} | {cell(s['ewise_add'])} | "
                    f"{s['union']['ms'] / s['ewise_add']['ms']:.2f} | {s['nnz_union']} |\n")
        f.write("\n| scale | type | d.diag() ms | dup() of its output ms | L.diag() ms | dup() of its output ms | round trip equal |\n|---|---|---|---|---|---|---|\n")
        for s in res["steps"]:
            f.write(f"| {s['scale']} | {s['type']} | {cell(s['vector_diag'])} | {cell(s['dup_of_D'])} | {cell(s['matrix_diag'])} | {cell(s['dup_of_v'])} | "
                    f"{s['diag_round_trip_same']} |\n")
        f.write("\n| scale | type | d.diag().ewise_union(A, minus, 0, 0) ms | host round trip ms (once) | same result |\n|---|---|---|---|---|\n")
        for s in res["steps"]:
            f.write(f"| {s['scale']} | {s['type']} | {cell(s['laplacian'])} | {s['laplacian_host_ms']:.1f} | {s['laplacian_same']} |\n")
        if "failed" in res:
            f.write(f"\nThe run stopped at scale {res['failed']['scale']} {res['failed']['type']} (exit status {res['failed']['exit']}).\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
