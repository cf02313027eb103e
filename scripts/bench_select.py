"""Times GrB_select on R-MAT graphs (GPU box) and writes profiles/r07/select.json + select.md.

Per line: median milliseconds of >= 11 runs after warm-up (HIP events around the C call: GrX_timer_start / GrX_timer_stop on the
library's stream), the algorithmic bytes -- read nnz * 4 columns (+ nnz * sizeof T for the value operators) + row pointers, write
kept * (4 + sizeof T) + row pointers + the keep words twice -- and their fraction of the 8 TB/s peak, as bench.py computes roofline.frac.

Two comparisons:
  * the path a user had before select existed, with the same result: C<L.S> = A through GrB_transpose (T0) with a prebuilt structural
    mask L (the wavefront-merge write rule), and the to_coo -> numpy -> from_coo round trip as the naive baseline;
  * the memory system: moved bytes / time next to the 5.5-5.7 TB/s of kept-line streams (profiles/r06/skip_rates.jsonl).

    python scripts/bench_select.py [--scales 20,22] [--tri-scales 16,18,20] [--runs 11] [--out profiles/r07]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import graphblas_amd as gb  # noqa: E402
from graphblas_amd import device, synthetic  # noqa: E402

HBM_PEAK_GBS = 8000.0  # (bench.py)
KEPT_LINE_STREAM_TBS = (5.5, 5.7)  # profiles/r06/skip_rates.jsonl


def timed(fn, runs, warmup=3):
    for _ in range(warmup):
        r = fn()
        del r
    ms = []
    for _ in range(runs):
        device.synchronize()
        device.timer_start()
        r = fn()
        ms.append(device.timer_stop())
        del r
    return ms


def spread(ms):
    """median and the run-to-run spread (half the distance between the 1st and 3rd quartile) of a sample"""
    q = statistics.quantiles(ms, n=4)
    return statistics.median(ms), (q[2] - q[0]) / 2


def select_bytes(nrows, nnz, kept, vsize, reads_values, flag_pass=True):
    rd = nnz * 4 + (nnz * vsize if reads_values else 0) + (nrows + 1) * 8
    wr = kept * (4 + vsize) + (nrows + 1) * 8
    keep_words = 2 * (-(-nnz // 64)) * 8 if flag_pass else 0  # written by the flag pass, read by the fill pass
    return rd + wr + keep_words


def symmetric_pattern(scale):
    """The R-MAT graph symmetrised (self-loops kept), as device CSR"""
    n = 1 << scale
    ip, col = synthetic.rmat_csr(scale, device="cuda")
    row = torch.repeat_interleave(torch.arange(n, device="cuda"), ip[1:] - ip[:-1])
    key = torch.unique(torch.cat([row * n + col.long(), col.long() * n + row]))
    r = torch.div(key, n, rounding_mode="floor")
    c = (key - r * n).to(torch.int32)
    p = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    p[1:] = torch.cumsum(torch.bincount(r, minlength=n), 0)
    return n, p, c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", default="20,22")
    ap.add_argument("--tri-scales", default="16,18,20")
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--out", default="profiles/r07")
    args = ap.parse_args()
    runs = max(11, args.runs)
    os.makedirs(args.out, exist_ok=True)
    gb.init()
    res = {"runs": runs, "hbm_peak_GBps": HBM_PEAK_GBS, "kept_line_stream_TBps": KEPT_LINE_STREAM_TBS, "select": [], "compare": [], "triangles": []}

    def flush():
        with open(os.path.join(args.out, "select.json"), "w") as f:
            json.dump(res, f, indent=1)

    for scale in [int(s) for s in args.scales.split(",") if s]:
        n = 1 << scale
        ip, col = synthetic.rmat_csr(scale, device="cuda")
        w = synthetic.edge_weights(col, scale)
        nnz = int(col.numel())
        A = device.matrix_from_device_csr(ip, col, w, n, n, "FP32")
        med_w = float(torch.median(w).item())
        for name, op, thunk, reads in (("tril", "tril", -1, False), ("offdiag", "offdiag", 0, False), ("valuege", "valuege", med_w, True),
                                       ("rowle", "rowle", n // 2 - 1, False)):
            ms = timed(lambda: A.select(op, thunk).new(), runs)
            kept = A.select(op, thunk).new().nvals
            med, sp = spread(ms)
            nbytes = select_bytes(n, nnz, kept, 4, reads, flag_pass=name != "rowle")
            line = {"scale": scale, "op": name, "thunk": thunk, "nnz": nnz, "kept": kept, "ms": med, "spread_ms": sp, "min_ms": min(ms),
                    "bytes": nbytes, "GBps": nbytes / med / 1e6, "frac": nbytes / med / 1e6 / HBM_PEAK_GBS}
            res["select"].append(line)
            print(json.dumps(line), flush=True)
            flush()
        # the path of the parent commit with the same result: C<L.S> = A through GrB_transpose (T0), L prebuilt
        L = A.select("tril", -1).new()

        def masked_copy():
            C = gb.Matrix("FP32", n, n)
            C(L.S) << A
            return C

        ms_t = timed(masked_copy, runs)
        ms_s = timed(lambda: A.select("tril", -1).new(), runs)
        same = masked_copy().isequal(L)
        (mt, st), (msel, ssel) = spread(ms_t), spread(ms_s)
        cmp_line = {"scale": scale, "transpose_masked_ms": mt, "transpose_masked_spread_ms": st, "select_tril_ms": msel, "select_tril_spread_ms": ssel,
                    "same_result": bool(same), "select_not_slower": bool(msel <= mt + st + ssel)}
        if scale <= 20:  # the naive baseline: through host memory, a sort and a dedupe
            t0 = time.perf_counter()
            r, c, x = A.to_coo()
            k = c < r
            N = gb.Matrix.from_coo(r[k], c[k], x[k], dtype="FP32", nrows=n, ncols=n)
            device.synchronize()
            cmp_line["coo_round_trip_ms"] = (time.perf_counter() - t0) * 1e3
            cmp_line["coo_same_result"] = bool(N.isequal(L))
            del N
        res["compare"].append(cmp_line)
        print(json.dumps(cmp_line), flush=True)
        flush()
        del A, L, ip, col, w
        device.trim_memory()

    for scale in [int(s) for s in args.tri_scales.split(",") if s]:
        n, p, c = symmetric_pattern(scale)
        one = torch.ones(1, dtype=torch.int64, device="cuda")
        S0 = device.matrix_from_device_csr(p, c, one, n, n, "INT64", iso=True)

        def make_l():
            return S0.select("offdiag").new().select("tril", -1).new()

        ms_sel = timed(make_l, runs)
        L = make_l()

        def product():
            C = gb.Matrix("INT64", n, n)
            C(L.S) << L.mxm(L.T, gb.semiring.plus_pair)
            return C

        ms_mxm = timed(product, runs, warmup=2)
        C = product()
        ms_red = timed(lambda: C.reduce_scalar("plus").new(), runs)
        line = {"scale": scale, "entries_L": L.nvals, "triangles": int(C.reduce_scalar("plus").new().value), "select_ms": spread(ms_sel)[0],
                "product_ms": spread(ms_mxm)[0], "reduce_ms": spread(ms_red)[0]}
        res["triangles"].append(line)
        print(json.dumps(line), flush=True)
        flush()
        del S0, L, C
        device.trim_memory()

    with open(os.path.join(args.out, "select.md"), "w") as f:
        f.write("# GrB_select on the MI355X (scripts/bench_select.py)\n\n")
        f.write(f"Median of {runs} runs after warm-up, HIP events around the call (`.new()` included: the output object, the kernels, one 8-byte "
                "read of the kept count).  R-MAT, FP32 weights U{1..255}.  Bytes are algorithmic (see the script).\n\n")
        f.write("| scale | operator | entries | kept | ms | spread | GB | GB/s | of 8 TB/s |\n|---|---|---|---|---|---|---|---|---|\n")
        for x in res["select"]:
            f.write(f"| {x['scale']} | {x['op']} ({x['thunk']}) | {x['nnz']} | {x['kept']} | {x['ms']:.3f} | {x['spread_ms']:.3f} | {x['bytes'] / 1e9:.3f} | "
                    f"{x['GBps']:.0f} | {x['frac']:.3f} |\n")
        f.write(f"\nKept-line streams on this chip: {KEPT_LINE_STREAM_TBS[0]}-{KEPT_LINE_STREAM_TBS[1]} TB/s (profiles/r06/skip_rates.jsonl).\n\n")
        f.write("## Against the path of the parent commit: `C<L.S> = A` through GrB_transpose (T0), L prebuilt\n\n")
        f.write("| scale | transpose + mask ms | spread | select tril ms | spread | same result | select not slower | to_coo -> numpy -> from_coo ms |\n|---|---|---|---|---|---|---|---|\n")
        for x in res["compare"]:
            coo = f"{x['coo_round_trip_ms']:.0f}" if "coo_round_trip_ms" in x else "not run"
            f.write(f"| {x['scale']} | {x['transpose_masked_ms']:.3f} | {x['transpose_masked_spread_ms']:.3f} | {x['select_tril_ms']:.3f} | "
                    f"{x['select_tril_spread_ms']:.3f} | {x['same_result']} | {x['select_not_slower']} | {coo} |\n")
        f.write("\n## Triangle counting: select (offdiag, tril), masked plus_pair product, reduce\n\n")
        f.write("| scale | entries of L | triangles | select ms | product ms | reduce ms |\n|---|---|---|---|---|---|\n")
        for x in res["triangles"]:
            f.write(f"| {x['scale']} | {x['entries_L']} | {x['triangles']} | {x['select_ms']:.3f} | {x['product_ms']:.3f} | {x['reduce_ms']:.3f} |\n")
    flush()


if __name__ == "__main__":
    main()
