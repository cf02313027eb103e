"""Times Matrix assign on R-MAT graphs (GPU box) and writes profiles/r07/assign.json + assign.md.

Per scale, FP32, with ``B`` extracted beforehand (``B = A[I, J].new()``) and ``C = A.dup()`` made afresh outside the timed region:
    rows            C()[S, :] << B        S = 1024 random rows, ascending                      (method 15)
    block           C()[lo:hi, lo:hi] << B  the middle n / 4 rows and columns                   (method 15)
    half sorted     C()[V, V] << B        V = a random half of the vertices, ascending         (method 16)
    half shuffled   C()[V, V] << B        the same half in random order                        (method 17)
    scalar, mask    C(A.S) << 1           the scalar form under a structural mask              (method 18)
each beside three things that are not the code under test: ``C.dup()`` (the stream yardstick: it moves the matrix once), ``C.ewise_add(S',
second)`` with ``S'`` -- ``B`` at C's coordinates -- placed beforehand (the merge alone), and the route a user takes without assign,
``to_coo`` -> numpy -> ``from_coo`` (wall clock).  Each figure is the median of >= 7 whole calls after warm-up with min and max beside it
(HIP events, GrX_timer_start / GrX_timer_stop); the routes are timed alternately.  No ratio is a pass mark.

Every scale runs in a process of its own under a time limit; the first failure stops the run.

    python scripts/bench_assign.py [--scales 20,22] [--runs 7] [--step-timeout 420] [--out profiles/r07]
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

CASES = ("rows", "block", "half_sorted", "half_shuffled", "scalar_mask")
LABEL = {"rows": "C()[S, :] << B, 1024 rows", "block": "C()[lo:hi, lo:hi] << B, n / 4", "half_sorted": "C()[V, V] << B, sorted half",
         "half_shuffled": "C()[V, V] << B, shuffled half", "scalar_mask": "C(A.S) << 1"}


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
    nnz = A.nvals
    rng = np.random.default_rng(scale)
    S = np.sort(rng.choice(n, 1024, replace=False)).astype(np.uint64)
    lo, hi = 3 * n // 8, 5 * n // 8
    Vs = np.sort(rng.choice(n, n // 2, replace=False)).astype(np.uint64)
    Vr = rng.permutation(Vs)
    everything = np.arange(n, dtype=np.uint64)
    keys = {"rows": (S, slice(None), S, everything), "block": (slice(lo, hi), slice(lo, hi), everything[lo:hi], everything[lo:hi]),
            "half_sorted": (Vs, Vs, Vs, Vs), "half_shuffled": (Vr, Vr, Vr, Vr)}

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
        if name == "scalar_mask":
            B = Sp = None

            def assign(C):
                C(A.S) << 1.0

            def host():
                r, c, x = A.to_coo()
                return gb.Matrix.from_coo(r, c, np.ones_like(x), dtype="FP32", nrows=n, ncols=n)

            Sp = A.apply(gb.binary.times, right=np.float32(0)).new()
            Sp(A.S) << 1.0
        else:
            ik, jk, I, J = keys[name]
            B = A[ik, jk].new()
            Sp = gb.Matrix("FP32", n, n)
            Sp()[ik, jk] << B  # S': B at C's coordinates

            def assign(C, ik=ik, jk=jk, B=B):
                C()[ik, jk] << B

            def host(I=I, J=J, B=B):
                r, c, x = A.to_coo()
                in_i, in_j = np.zeros(n, bool), np.zeros(n, bool)
                in_i[I.astype(np.int64)], in_j[J.astype(np.int64)] = True, True
                keep = ~(in_i[r.astype(np.int64)] & in_j[c.astype(np.int64)])
                br, bc, bx = B.to_coo()
                return gb.Matrix.from_coo(np.concatenate([r[keep], I[br.astype(np.int64)]]), np.concatenate([c[keep], J[bc.astype(np.int64)]]),
                                          np.concatenate([x[keep], bx]), dtype="FP32", nrows=n, ncols=n)

        def merge_alone(C):
            return C.ewise_add(Sp, gb.binary.second).new()

        for _ in range(2):  # warm-up: code objects, the block cache, the cached layouts
            C = A.dup()
            assign(C)
            r = merge_alone(C)
            del r, C
        t_new, t_dup, t_merge, t_host = [], [], [], []
        for k in range(runs):
            C = A.dup()
            ms, _ = timed_once(lambda: assign(C))
            t_new.append(ms)
            del C
            ms, r = timed_once(A.dup)
            t_dup.append(ms)
            ms, r2 = timed_once(lambda: merge_alone(r))
            t_merge.append(ms)
            del r, r2
            if k < 2:  # (the host route takes seconds: two runs of it)
                ms, r = wall_once(host)
                t_host.append(ms)
                del r
        C = A.dup()
        assign(C)
        st = device.last_stats()
        same = bool(C.isequal(host(), check_dtype=True))
        s, d, mg = summary(t_new), summary(t_dup), summary(t_merge)
        s.update(method=st["method"], units=st["tiles"], launches=st["kernel_launches"], placed=0 if B is None else B.nvals, out_nvals=C.nvals, dup=d,
                 merge=mg, ratio_to_dup=s["ms"] / d["ms"], ratio_to_merge=s["ms"] / mg["ms"], host=summary(t_host), host_runs=len(t_host),
                 same_result=same)
        out["cases"][name] = s
        del C, B, Sp
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
    with open(os.path.join(out_dir, "assign.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(out_dir, "assign.md"), "w") as f:
        f.write("# Matrix assign on the MI355X (scripts/bench_assign.py)\n\n")
        f.write(f"Median of {runs} whole calls after warm-up (min - max in brackets); HIP events for assign, for `C.dup()` (the stream yardstick) and "
                "for `C.ewise_add(S', second)` with `S'` placed beforehand (the merge alone); wall clock for the `to_coo` -> numpy -> `from_coo` "
                "round trip (2 runs); the routes are timed alternately.  R-MAT, edge factor 16, FP32 weights U{1..255}; `B` was extracted "
                "beforehand, `C` is a fresh copy for every call.  No ratio is a pass mark.\n\n")
        if not res["steps"]:
            f.write("NOT MEASURED.\n")
        else:
            f.write("| scale | entries | case | method | units | launches | placed entries | assign ms | dup ms | merge alone ms | assign / dup | assign / merge | "
                    "host round trip ms | same result |\n")
            f.write("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for s in res["steps"]:
            for name in CASES:
                x = s["cases"][name]
                d, m, z = x["dup"], x["merge"], x["host"]
                f.write(f"| {s['scale']} | {s['nnz']} | {LABEL[name]} | {x['method']} | {x['units']} | {x['launches']} | {x['placed']} | "
                        f"{x['ms']:.3f} [{x['min_ms']:.3f} - {x['max_ms']:.3f}] | {d['ms']:.3f} [{d['min_ms']:.3f} - {d['max_ms']:.3f}] | "
                        f"{m['ms']:.3f} [{m['min_ms']:.3f} - {m['max_ms']:.3f}] | {x['ratio_to_dup']:.2f} | {x['ratio_to_merge']:.2f} | "
                        f"{z['ms']:.1f} [{z['min_ms']:.1f} - {z['max_ms']:.1f}] | {x['same_result']} |\n")
        if "failed" in res:
            f.write(f"\nThe run stopped at scale {res['failed']['scale']} (exit status {res['failed']['exit']}): NOT MEASURED from there on.\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
