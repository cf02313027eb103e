"""Times GrB_Matrix_eWiseAdd / eWiseMult on R-MAT graphs (GPU box) and writes profiles/r07/ewise.json + ewise.md.

Per (scale, type): A u A' (plus), A n A' (times), A u B for two independent graphs, and the only route the parent commit had to a
union -- ``C = A.dup(); C(binary.plus) << A.T``, GrB_transpose with an accumulator, the three-list write rule.  Each figure is the
median of >= 7 runs after warm-up with min and max beside it (HIP events around the call: GrX_timer_start / GrX_timer_stop on the
library's stream); the transposes are cached before anything is timed.  The new call and the old route are timed alternately.

Moved bytes (algorithmic): read (4 + sizeof T)(nnz A + nnz B) and both row-pointer arrays, twice (count and fill); write
(4 + sizeof T) nnz T and the row pointers -- next to the 5.5-5.7 TB/s of kept-line streams (profiles/r06/line_floor.md).  The time is
the whole call (``.new()`` included: the unit tables, two scans, two 8-byte reads), so bytes / time is an end-to-end rate, not a
kernel's.

Every (scale, type) step runs in a process of its own under a time limit; the first failure stops the run.

    python scripts/bench_ewise.py [--scales 20,22] [--types FP32,INT64] [--runs 7] [--step-timeout 420] [--out profiles/r07]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEPT_LINE_STREAM_TBS = (5.5, 5.7)  # profiles/r06/line_floor.md
VSIZE = {"FP32": 4, "INT64": 8}


def ewise_bytes(nrows, nnz_a, nnz_b, nnz_t, vsize):
    rd = 2 * ((4 + vsize) * (nnz_a + nnz_b) + 2 * (nrows + 1) * 8)
    wr = (4 + vsize) * nnz_t + (nrows + 1) * 8
    return rd + wr


def summary(ms):
    return {"ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def step(scale, tname, runs):
    import graphblas_amd as gb
    from graphblas_amd import device, synthetic

    gb.init()
    n = 1 << scale

    def graph(seed):
        ip, col = synthetic.rmat_csr(scale, seed=seed, device="cuda")
        w = synthetic.edge_weights(col, seed)
        return device.matrix_from_device_csr(ip, col, w, n, n, "FP32").dup(dtype=tname)  # (a copy the library owns, in the type timed)

    A, B = graph(scale), graph(scale + 100)
    device.cache_transpose(A)

    def timed_once(fn):
        device.synchronize()
        device.timer_start()
        r = fn()
        ms = device.timer_stop()
        return ms, r

    def union():
        return A.ewise_add(A.T, gb.binary.plus).new()

    def old_union():
        C = A.dup()
        C(gb.binary.plus) << A.T
        return C

    def inter():
        return A.ewise_mult(A.T, gb.binary.times).new()

    def union_ab():
        return A.ewise_add(B, gb.binary.plus).new()

    out = {"scale": scale, "type": tname, "runs": runs, "nnz_A": A.nvals, "nnz_B": B.nvals}
    for fn in (union, old_union, inter, union_ab):  # warm-up: code objects, the block cache
        for _ in range(2):
            r = fn()
            del r
    # the new call and the route of the parent commit, alternating
    t_new, t_old = [], []
    for _ in range(runs):
        ms, r = timed_once(union)
        t_new.append(ms)
        del r
        ms, r = timed_once(old_union)
        t_old.append(ms)
        del r
    U, V = union(), old_union()
    out["same_result"] = bool(U.isequal(V))
    out["launches"] = device.last_stats()["kernel_launches"]
    nnz_u = U.nvals
    del U, V
    t_int = []
    for _ in range(runs):
        ms, r = timed_once(inter)
        t_int.append(ms)
        nnz_i = r.nvals
        del r
    t_ab = []
    for _ in range(runs):
        ms, r = timed_once(union_ab)
        t_ab.append(ms)
        nnz_ab = r.nvals
        del r
    vs = VSIZE[tname]
    for key, ms, nb, nt in (("union_AAt", t_new, A.nvals, nnz_u), ("inter_AAt", t_int, A.nvals, nnz_i), ("union_AB", t_ab, B.nvals, nnz_ab)):
        s = summary(ms)
        s["nnz_T"] = nt
        s["bytes"] = ewise_bytes(n, A.nvals, nb, nt, vs)
        s["TBps"] = s["bytes"] / s["ms"] / 1e9
        out[key] = s
    out["dup_accum_transpose"] = summary(t_old)
    spread = (max(t_new) - min(t_new)) + (max(t_old) - min(t_old))
    out["new_not_slower"] = bool(out["union_AAt"]["ms"] <= out["dup_accum_transpose"]["ms"] + spread)
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
    res = {"runs": runs, "kept_line_stream_TBps": KEPT_LINE_STREAM_TBS, "steps": []}
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
            with open(os.path.join(out_dir, "ewise.json"), "w") as f:
                json.dump(res, f, indent=1)
        if rc:
            break
    with open(os.path.join(out_dir, "ewise.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(out_dir, "ewise.md"), "w") as f:
        f.write("# Matrix eWiseAdd / eWiseMult on the MI355X (scripts/bench_ewise.py)\n\n")
        f.write(f"Median of {runs} runs after warm-up (min - max in brackets), HIP events around the whole call (`.new()` included); transposes cached "
                "before timing; R-MAT, edge factor 16, weights U{1..255}.  Bytes are algorithmic (see the script); bytes / time is an end-to-end rate "
                f"of the call, set beside the {KEPT_LINE_STREAM_TBS[0]}-{KEPT_LINE_STREAM_TBS[1]} TB/s of kept-line streams (profiles/r06/line_floor.md).\n\n")
        f.write("| scale | type | call | entries A | entries T | ms | GB | TB/s |\n|---|---|---|---|---|---|---|---|\n")
        for s in res["steps"]:
            for key, label in (("union_AAt", "A u A' (plus)"), ("inter_AAt", "A n A' (times)"), ("union_AB", "A u B (plus)")):
                x = s[key]
                f.write(f"| {s['scale']} | {s['type']} | {label} | {s['nnz_A']} | {x['nnz_T']} | {x['ms']:.3f} [{x['min_ms']:.3f} - {x['max_ms']:.3f}] | "
                        f"{x['bytes'] / 1e9:.3f} | {x['TBps']:.2f} |\n")
        f.write("\n## Against the route of the parent commit to a union: `C = A.dup(); C(binary.plus) << A.T`\n\n")
        f.write("(GrB_transpose with an accumulator: a copy of A, then the three-list write rule.  Timed alternately with the new call.)\n\n")
        f.write("| scale | type | ewise_add ms | dup + accumulate ms | same result | new not slower beyond both spreads |\n|---|---|---|---|---|---|\n")
        for s in res["steps"]:
            x, y = s["union_AAt"], s["dup_accum_transpose"]
            f.write(f"| {s['scale']} | {s['type']} | {x['ms']:.3f} [{x['min_ms']:.3f} - {x['max_ms']:.3f}] | {y['ms']:.3f} [{y['min_ms']:.3f} - {y['max_ms']:.3f}] | "
                    f"{s['same_result']} | {s['new_not_slower']} |\n")
        if "failed" in res:
            f.write(f"\nThe run stopped at scale {res['failed']['scale']} {res['failed']['type']} (exit status {res['failed']['exit']}).\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
