"""Times GrB_Matrix_extract on R-MAT graphs (GPU box) and writes profiles/r07/extract.json + extract.md.

Per scale, on an FP32 graph, four cases:
    rows      A[S, :]          1024 random rows                          (method 9)
    block     A[lo:hi, lo:hi]  a quarter of the vertices, contiguous     (method 9)
    sorted    A[V, V]          a sorted random half of the vertices      (methods 10 / 11)
    shuffled  A[V, V]          the same half, shuffled                   (method 12)
each against the two routes the parent commit has: the product with selection matrices on the device, ``P.mxm(A).new().mxm(Q).new()``
with P(i', I[i']) = 1 and Q(J[j'], j') = 1 (built before anything is timed), and the round trip through the host, ``to_coo`` -> numpy ->
``from_coo``.  Each figure is the median of >= 7 runs after warm-up with min and max beside it (HIP events around the call for the two
device routes, GrX_timer_start / GrX_timer_stop; wall clock for the host route); the three routes are timed alternately.

Moved bytes (algorithmic): E = the entries of the selected rows inside [min J, max J] (what the kernel's units cover); the fill reads (4 + sizeof T) E and writes (4 + sizeof T) nnz T; the count
pass of methods 10 - 12 reads the 4 E bytes of columns once more; method 12 moves 2 x 12 nnz T bytes through its sort on top (not counted).
The time is the whole call (``.new()`` included: the copy of the index lists, the scans, the 8-byte reads), so bytes / time is an end-to-end
rate, set beside the 5.5 - 5.7 TB/s of kept-line streams (profiles/r06/line_floor.md).  There is no pass mark: the table says which route won.

Every scale runs in a process of its own under a time limit; the first failure stops the run.

    python scripts/bench_extract.py [--scales 20,22] [--runs 7] [--step-timeout 420] [--out profiles/r07]
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

KEPT_LINE_STREAM_TBS = (5.5, 5.7)  # profiles/r06/line_floor.md
CASES = ("rows", "block", "sorted", "shuffled")
LABEL = {"rows": "A[S, :], 1024 rows", "block": "A[lo:hi, lo:hi], n / 4", "sorted": "A[V, V], sorted half", "shuffled": "A[V, V], shuffled half"}


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
    A = device.matrix_from_device_csr(ip, col, w, n, n, "FP32").dup()  # (a copy the library owns)
    ip_h, col_h = ip.cpu().numpy().astype(np.int64), col.cpu().numpy()
    row_h = np.repeat(np.arange(n), np.diff(ip_h))

    def entries_in_reach(I, J):
        """E of DESIGN.md section 4.7: the entries of the rows of I (no repeats here) whose column lies inside [min J, max J]"""
        picked = np.zeros(n, bool)
        picked[I] = True
        keep = picked[row_h]
        if J is not None:
            keep &= (col_h >= J.min()) & (col_h <= J.max())
        return int(keep.sum())

    rng = np.random.default_rng(scale)
    V = np.sort(rng.choice(n, n // 2, replace=False))
    lists = {"rows": (rng.choice(n, 1024, replace=False), None), "block": (np.arange(n // 4, n // 2), np.arange(n // 4, n // 2)),
             "sorted": (V, V), "shuffled": (rng.permutation(V), rng.permutation(V))}

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

    out = {"scale": scale, "type": "FP32", "runs": runs, "nnz_A": A.nvals, "cases": {}}
    for name in CASES:
        I, J = lists[name]
        ni, nj = I.size, (n if J is None else J.size)
        one = np.ones(max(ni, nj), np.float32)
        P = gb.Matrix.from_coo(np.arange(ni), I, one[:ni], dtype="FP32", nrows=ni, ncols=n)
        Q = None if J is None else gb.Matrix.from_coo(J, np.arange(nj), one[:nj], dtype="FP32", nrows=n, ncols=nj)

        def extract():
            return A[I, slice(None) if J is None else J].new()

        def product():
            R = P.mxm(A, gb.semiring.plus_times).new()
            return R if Q is None else R.mxm(Q, gb.semiring.plus_times).new()

        def host():
            r, c, x = A.to_coo()
            rinv = np.full(n, -1, np.int64)
            rinv[I] = np.arange(ni)
            keep = rinv[r] >= 0
            if J is None:
                return gb.Matrix.from_coo(rinv[r][keep], c[keep], x[keep], dtype="FP32", nrows=ni, ncols=nj)
            cinv = np.full(n, -1, np.int64)
            cinv[J] = np.arange(nj)
            keep &= cinv[c] >= 0
            return gb.Matrix.from_coo(rinv[r][keep], cinv[c][keep], x[keep], dtype="FP32", nrows=ni, ncols=nj)

        for fn in (extract, product):  # warm-up: code objects, the block cache
            for _ in range(2):
                r = fn()
                del r
        t_new, t_prod, t_host = [], [], []
        for k in range(runs):
            ms, r = timed_once(extract)
            t_new.append(ms)
            del r
            ms, r = timed_once(product)
            t_prod.append(ms)
            del r
            if k < 3 or scale <= 20:  # (the host route takes seconds at scale 22: three runs of it)
                ms, r = wall_once(host)
                t_host.append(ms)
                del r
        T = extract()
        st = device.last_stats()
        same = bool(T.isequal(product())) and bool(T.isequal(host()))
        E, nnz_t = entries_in_reach(I, J), T.nvals
        nbytes = 8 * (E + nnz_t) + (4 * E if st["method"] != 9 else 0)
        s = summary(t_new)
        s.update(method=st["method"], units=st["tiles"], launches=st["kernel_launches"], ni=int(ni), nj=int(nj), E=E, nnz_T=nnz_t, bytes=nbytes,
                 TBps=nbytes / s["ms"] / 1e9, product=summary(t_prod), host=summary(t_host), host_runs=len(t_host), same_result=same)
        out["cases"][name] = s
        del T, P, Q
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
    res = {"runs": runs, "kept_line_stream_TBps": KEPT_LINE_STREAM_TBS, "steps": []}
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
    with open(os.path.join(out_dir, "extract.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(out_dir, "extract.md"), "w") as f:
        f.write("# Matrix extract on the MI355X (scripts/bench_extract.py)\n\n")
        f.write(f"Median of {runs} runs after warm-up (min - max in brackets); HIP events around the whole call (`.new()` included) for extract and "
                "for the product with selection matrices, wall clock for the `to_coo` -> numpy -> `from_coo` round trip; the routes are timed "
                "alternately.  R-MAT, edge factor 16, FP32 weights U{1..255}.  Bytes are algorithmic (see the script); bytes / time is an "
                f"end-to-end rate of the call, set beside the {KEPT_LINE_STREAM_TBS[0]}-{KEPT_LINE_STREAM_TBS[1]} TB/s of kept-line streams "
                "(profiles/r06/line_floor.md).  No pass mark: the last column says which route was fastest.\n\n")
        if not res["steps"]:
            f.write("NOT TIMED YET.\n")
        else:
            f.write("| scale | case | method | units | E | entries T | extract ms | GB | TB/s | product ms | host round trip ms | same result | fastest |\n")
            f.write("|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for s in res["steps"]:
            for name in CASES:
                x = s["cases"][name]
                y, z = x["product"], x["host"]
                best = min((x["ms"], "extract"), (y["ms"], "product"), (z["ms"], "host"))[1]
                f.write(f"| {s['scale']} | {LABEL[name]} | {x['method']} | {x['units']} | {x['E']} | {x['nnz_T']} | "
                        f"{x['ms']:.3f} [{x['min_ms']:.3f} - {x['max_ms']:.3f}] | {x['bytes'] / 1e9:.3f} | {x['TBps']:.3f} | "
                        f"{y['ms']:.3f} [{y['min_ms']:.3f} - {y['max_ms']:.3f}] | {z['ms']:.1f} [{z['min_ms']:.1f} - {z['max_ms']:.1f}] ({x['host_runs']} runs) | "
                        f"{x['same_result']} | {best} |\n")
        if "failed" in res:
            f.write(f"\nThe run stopped at scale {res['failed']['scale']} (exit status {res['failed']['exit']}): NOT TIMED YET from there on.\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
