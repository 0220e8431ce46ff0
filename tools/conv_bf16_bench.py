#!/usr/bin/env python
"""Speed of the opt-in bf16-input mode of the tactile convolutions (offline_train.model.conv_bf16_inputs) on the student
update: tools/bench_student.py with the mode off and on as ALTERNATING pairs, each run a fresh process against the same
build, at the configs[2] size (2048 envs x 32, tactile + lin) and at the single-rank share of configs[3] (512 envs x 32,
tactile + pcl + lin).  Every pair, the medians and the per-class figures of the igi_prof_* hook go to one JSON record
stamped with the hash of the library's sources.

    python tools/conv_bf16_bench.py --pairs 3 --out profiles/conv_bf16_student.json
    python tools/conv_bf16_bench.py --trace DIR/..._kernel_stats.csv [--trace-on ...] --out ...   # add rocprofv3 tables

The per-kernel table of a ``rocprofv3 --kernel-trace --stats`` run (one run per setting, of its own: tracing perturbs the
step time) is merged in with --trace-off / --trace-on.
"""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"configs[2]: tactile + lin, 2048 envs x 32": ["--config", "3", "--envs", "2048"],
         "configs[3] share: tactile + pcl + lin, 512 envs x 32": ["--config", "4", "--envs", "512"]}


def one(args, on):
    cmd = [sys.executable, os.path.join(ROOT, "tools", "bench_student.py")] + args + (["--conv-bf16"] if on else [])
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed ({r.returncode}): {r.stderr[-2000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def conv_rows(rec):
    return [k for k in rec.get("native_kernels", []) if "gemm_dma_conv_bf16_kernel<" in k["name"] or
            any(t in k["name"] for t in (",1,2,256>", ",6,2,256>", ",4,2,256>", ",5,2,256>", ",5,2,192>", ",3,2,256>"))]


def trace_table(path):
    """rows of a rocprofv3 --stats kernel_stats.csv whose kernel is one of the GEMM tiles: name, calls, average ns"""
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName") or ""
            if "gemm_dma" not in name:
                continue
            rows.append({"name": name.replace("igi::", "").replace("void ", "").split("(")[0].replace(" ", ""),
                         "calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 1),
                         "total_ms": round(float(r["TotalDurationNs"]) / 1e6, 2)})
    return sorted(rows, key=lambda r: -r["total_ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_bf16_student.json"))
    ap.add_argument("--trace-off", help="kernel_stats.csv of a rocprofv3 --kernel-trace --stats run with the mode off")
    ap.add_argument("--trace-on", help="the same with --conv-bf16")
    ap.add_argument("--merge", action="store_true", help="only add the trace tables to an existing record")
    args = ap.parse_args()
    import __graft_entry__ as ge
    rec = json.load(open(args.out)) if args.merge else {
        "what": "student update (ExtrinsicAdapt.update) with the tactile convolutions' bf16-input mode off / on: "
                "tools/bench_student.py, fresh process per run, alternating off / on pairs against one build",
        "build": ge.library_hash(), "sizes": {}}
    if not args.merge:
        for label, a in SIZES.items():
            pairs = []
            for _ in range(args.pairs):
                off, on = one(a, False), one(a, True)
                pairs.append({"off_ms_per_step": off["ms_per_optimizer_step"], "on_ms_per_step": on["ms_per_optimizer_step"],
                              "off_ms_per_update": off["ms_per_update"], "on_ms_per_update": on["ms_per_update"]})
                print(label, pairs[-1], flush=True)
            m_off = statistics.median(p["off_ms_per_update"] for p in pairs)
            m_on = statistics.median(p["on_ms_per_update"] for p in pairs)
            rec["sizes"][label] = {"pairs": pairs, "median_off_ms_per_update": m_off, "median_on_ms_per_update": m_on,
                                   "speedup": round(m_off / m_on, 3), "workload": off["workload"],
                                   "conv_classes_off": conv_rows(off), "conv_classes_on": conv_rows(on)}
    if args.trace_off:
        rec["rocprofv3_kernel_stats_off"] = trace_table(args.trace_off)
    if args.trace_on:
        rec["rocprofv3_kernel_stats_on"] = trace_table(args.trace_on)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
