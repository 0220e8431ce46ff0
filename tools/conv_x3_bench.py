#!/usr/bin/env python
"""Speed of the opt-in split-bf16 mode of the tactile convolutions (offline_train.model.conv_bf16x3) on the student
update, by the method of tools/conv_bf16_bench.py: tools/bench_student.py in a fresh process per run, ALTERNATING rounds
in the order off -> x3 -> bf16 (the one-plane mode, offline_train.model.conv_bf16_inputs), at the configs[2] size (2048
envs x 32, tactile + lin) and at the single-rank share of configs[3] (512 envs x 32, tactile + pcl + lin); per setting the
median (min .. max) over the rounds, and the per-class figures of the igi_prof_* hook.

    python tools/conv_x3_bench.py --rounds 3 --out profiles/conv_x3_student.json
    python tools/conv_x3_bench.py --rounds 3 --control /path/to/parent/checkout ...   # mode off against another build
    python tools/conv_x3_bench.py --merge --trace-off DIR/..._kernel_stats.csv --trace-x3 ...   # add rocprofv3 tables

--control names a built checkout of the parent commit: each round then also runs ITS tools/bench_student.py with the mode
off, one worker per build and round; the two "off" columns must not separate, or the x3 / off ratio means nothing.
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
MODES = {"off": [], "x3": ["--conv-x3"], "bf16": ["--conv-bf16"]}


def one(root, args):
    cmd = [sys.executable, os.path.join(root, "tools", "bench_student.py")] + args
    env = dict(os.environ, PYTHONPATH=root)
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed ({r.returncode}): {r.stderr[-2000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def conv_rows(rec):
    return [k for k in rec.get("native_kernels", []) if "gemm_dma_conv_" in k["name"] or
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


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="*", default=[0, 1], help="indices into the two sizes")
    ap.add_argument("--control", help="a built checkout of the parent commit: mode off from that build, every round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_x3_student.json"))
    ap.add_argument("--trace-off", help="kernel_stats.csv of a rocprofv3 --kernel-trace --stats run with the mode off")
    ap.add_argument("--trace-x3", help="the same with --conv-x3")
    ap.add_argument("--merge", action="store_true", help="only add the trace tables to an existing record")
    args = ap.parse_args()
    import __graft_entry__ as ge
    rec = json.load(open(args.out)) if args.merge else {
        "what": "student update (ExtrinsicAdapt.update) with the tactile convolutions in fp32 (off), split-bf16 (x3: "
                "offline_train.model.conv_bf16x3) and bf16-input (bf16: conv_bf16_inputs) arithmetic: "
                "tools/bench_student.py, fresh process per run, alternating rounds off -> x3 -> bf16 against one build"
                + ("; control = mode off from a build of the parent commit, same rounds" if args.control else ""),
        "split": "per consuming lane, in the k-loop (the only variant built)",
        "build": ge.library_hash(), "sizes": {}}
    if not args.merge:
        for i, (label, a) in enumerate(SIZES.items()):
            if i not in args.sizes:
                continue
            rounds, last = [], {}
            for _ in range(args.rounds):
                row = {}
                for mode, flag in MODES.items():
                    last[mode] = one(ROOT, a + flag)
                    row[mode + "_ms_per_step"] = last[mode]["ms_per_optimizer_step"]
                    row[mode + "_ms_per_update"] = last[mode]["ms_per_update"]
                if args.control:
                    c = one(os.path.abspath(args.control), a)
                    row["control_off_ms_per_step"], row["control_off_ms_per_update"] = \
                        c["ms_per_optimizer_step"], c["ms_per_update"]
                rounds.append(row)
                print(label, row, flush=True)
            cols = sorted({k for r in rounds for k in r})
            summary = {k: spread([r[k] for r in rounds]) for k in cols}
            rec["sizes"][label] = {
                "rounds": rounds, "summary": summary, "workload": last["off"]["workload"],
                "x3_over_off_median": round(summary["x3_ms_per_update"]["median"] / summary["off_ms_per_update"]["median"], 3),
                "x3_faster_than_off_in_every_round": all(r["x3_ms_per_update"] < r["off_ms_per_update"] for r in rounds),
                "conv_classes": {m: conv_rows(last[m]) for m in MODES}}
    if args.trace_off:
        rec["rocprofv3_kernel_stats_off"] = trace_table(args.trace_off)
    if args.trace_x3:
        rec["rocprofv3_kernel_stats_x3"] = trace_table(args.trace_x3)
    if "rocprofv3_kernel_stats_x3" not in rec:
        rec["rocprofv3_kernel_stats"] = "not measured"
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
