#!/usr/bin/env python
"""What the GPU does at the boundary between two gn_estimate calls of the headline configuration (two sub-batch streams, deferred certificate).

    python tools/call_boundary.py --run --certify-eps EPS --out profiles/<tag>_call_boundary.json       # trace + summary
    python tools/call_boundary.py --trace <dir or *_kernel_trace.csv> [--steps 5] [--groups 2]          # summary of an existing trace
    python tools/call_boundary.py --ab <parent's libgisnav_amd.so> [--runs 3] --out ...                 # plain bench.py runs, parent / new alternating

--run starts `rocprofv3 --kernel-trace` (no counters, nothing else traced) over `bench.py --steps 5 --warmup 2 --certify-eps EPS` as a child process and
summarises its kernel trace.  EPS is the `profile_eps_arg` of a plain bench.py line (no calibration pass and no self-check launches among the steps).

From the start / end timestamps of the last `steps` calls, per step:
  no_big_kernel_us   time during which no k_attn_pw / k_ffn128 / k_qkv dispatch is running
  only_pnp_us        time during which k_pnp_* dispatches are the only ones running
  next_start_after_other_pnp_us
                     for every group g and call n + 1: start of the group's first kernel (k_extent) minus the end of the OTHER group's k_pnp_refine of
                     call n.  >= 0 in every call means the group never started before the other group's PnP was over (it waited for it, or for
                     something later); a negative value is a start while that PnP was still running or queued.
and the PnP kernels' own durations.  A dispatch "runs" from Start_Timestamp to End_Timestamp of the trace; the window is first kernel start of the first
of the `steps` calls to the last end of a library kernel.
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = ("k_attn_pw", "k_ffn128", "k_qkv")


def short(name: str) -> str:
    """'void gn::(anonymous namespace)::k_ffn128<0, true, ...>(gn::FfnArgs)' -> 'k_ffn128'; other kernels keep their name."""
    i = name.find("::k_")
    if i < 0:
        return name
    j = i + 2
    k = j
    while k < len(name) and (name[k].isalnum() or name[k] == "_"):
        k += 1
    return name[j:k]


def union(iv):
    """Sorted, merged copy of a list of (start, end)."""
    out = []
    for s, e in sorted(iv):
        if out and s <= out[-1][1]:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([s, e])
    return out


def length(iv) -> int:
    return sum(e - s for s, e in iv)


def subtract(a, b):
    """a minus b, both merged interval lists."""
    out, j = [], 0
    for s, e in a:
        cur = s
        while j < len(b) and b[j][1] <= cur:
            j += 1
        k = j
        while k < len(b) and b[k][0] < e:
            if b[k][0] > cur:
                out.append([cur, b[k][0]])
            cur = max(cur, b[k][1])
            k += 1
        if cur < e:
            out.append([cur, e])
    return out


def clip(iv, lo, hi):
    return [[max(s, lo), min(e, hi)] for s, e in iv if min(e, hi) > max(s, lo)]


def find_trace(path: str) -> str:
    if os.path.isfile(path):
        return path
    hits = sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True))
    if not hits:
        raise SystemExit(f"no *kernel_trace.csv under {path}")
    return hits[0]


def summarise(trace_csv: str, steps: int, groups: int) -> dict:
    rows = []
    with open(trace_csv, newline="") as f:
        for r in csv.DictReader(f):
            rows.append({"name": short(r["Kernel_Name"]), "s": int(r["Start_Timestamp"]), "e": int(r["End_Timestamp"]),
                         "stream": r.get("Stream_Id") or "0", "queue": r.get("Queue_Id") or "0", "lib": "::k_" in r["Kernel_Name"]})
    if len({r["stream"] for r in rows if r["lib"]}) < groups:      # (no stream column, or one value throughout: the hardware queue tells the groups apart)
        for r in rows:
            r["stream"] = r["queue"]
    rows.sort(key=lambda r: r["s"])
    ext = [r for r in rows if r["name"] == "k_extent"]
    if len(ext) < steps * groups:
        raise SystemExit(f"trace holds {len(ext)} k_extent dispatches, fewer than steps x groups = {steps * groups}")
    ext = ext[-steps * groups:]
    t0 = ext[0]["s"]
    t1 = max(r["e"] for r in rows if r["lib"] and r["s"] >= t0)
    win = [r for r in rows if r["e"] > t0 and r["s"] < t1]
    big = clip(union([(r["s"], r["e"]) for r in win if r["name"] in BIG]), t0, t1)
    pnp = clip(union([(r["s"], r["e"]) for r in win if r["name"].startswith("k_pnp")]), t0, t1)
    rest = clip(union([(r["s"], r["e"]) for r in win if not r["name"].startswith("k_pnp")]), t0, t1)
    no_big = (t1 - t0) - length(big)
    only_pnp = length(subtract(pnp, rest))
    # group of a dispatch: the stream of the group's k_extent launches; the PnP kernels may run on a stream of their own, in the order the groups enqueue them
    gstreams = []
    for r in ext:
        if r["stream"] not in gstreams:
            gstreams.append(r["stream"])
    by_stream = len(gstreams) == groups
    first = {}      # (call, group) -> start of the group's first kernel
    seen = {}
    for i, r in enumerate(ext):
        g = gstreams.index(r["stream"]) if by_stream else i % groups
        first[(seen.get(g, 0), g)] = r["s"]
        seen[g] = seen.get(g, 0) + 1
    refine = [r for r in rows if r["name"] == "k_pnp_refine" and r["s"] >= t0]
    ref_end, seen = {}, {}
    for i, r in enumerate(refine):
        g = gstreams.index(r["stream"]) if (by_stream and r["stream"] in gstreams) else i % groups
        ref_end[(seen.get(g, 0), g)] = r["e"]
        seen[g] = seen.get(g, 0) + 1
    gaps = {}
    for g in range(groups):
        for o in range(groups):
            if o == g:
                continue
            vals = [round((first[(n + 1, g)] - ref_end[(n, o)]) / 1e3, 1) for n in range(steps - 1) if (n + 1, g) in first and (n, o) in ref_end]
            gaps[f"group{g}_after_group{o}_pnp"] = vals
    dur = {}
    for k in ("k_pnp_hyp", "k_pnp_refine"):
        d = [(r["e"] - r["s"]) / 1e3 for r in win if r["name"] == k and r["s"] >= t0]
        dur[k] = {"dispatches_per_step": round(len(d) / steps, 2), "avg_us": round(sum(d) / max(len(d), 1), 1), "max_us": round(max(d or [0.0]), 1)}
    head = {}
    for k in ("k_prep", "k_split_hm16", "k_rot_table", "k_extent"):
        d = [(r["e"] - r["s"]) / 1e3 for r in win if r["name"] == k and r["s"] >= t0]
        head[k] = {"dispatches_per_step": round(len(d) / steps, 2), "avg_us": round(sum(d) / max(len(d), 1), 1)}
    allgaps = [v for vals in gaps.values() for v in vals]
    return {"trace": "rocprofv3 --kernel-trace, no counters", "steps": steps, "groups": groups, "group_streams_told_apart": by_stream,
            "window_us_per_step": round((t1 - t0) / 1e3 / steps, 1),
            "no_big_kernel_us_per_step": round(no_big / 1e3 / steps, 1),
            "only_pnp_us_per_step": round(only_pnp / 1e3 / steps, 1),
            "next_start_after_other_pnp_us": gaps,
            "next_start_after_other_pnp_min_us": min(allgaps) if allgaps else None,
            "calls_that_started_before_other_pnp_ended": sum(1 for v in allgaps if v < 0),
            "pnp_kernels": dur, "head_kernels": head}


def lib_env(lib: str) -> dict:
    """Environment of a child that loads another build of the library (an A/B against the parent commit's): _lib.load() takes it as it is."""
    env = dict(os.environ)
    if lib:
        env["GISNAV_AMD_LIB"] = os.path.abspath(lib)
        env["GISNAV_AMD_ALLOW_STALE"] = "1"
    return env


def bench_ab(parent_lib: str, runs: int) -> dict:
    """Plain `python bench.py`, `runs` times each with the parent's library and with the tree's, alternating, one process at a time."""
    vals = {"parent": [], "new": []}
    for _ in range(runs):
        for who, lib in (("parent", parent_lib), ("new", "")):
            r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")], env=lib_env(lib), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                               text=True, timeout=280)
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-2000:])
                raise SystemExit(f"bench.py ({who}) failed (rc {r.returncode})")
            line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
            vals[who].append(line["value"])
            print(who, line["value"], line.get("unit", ""), file=sys.stderr, flush=True)
    med = {k: sorted(v)[len(v) // 2] for k, v in vals.items()}
    spread = max(vals["parent"]) - min(vals["parent"])
    return {"bench": "python bench.py, alternating parent / new, one lease", "pairs_per_s": vals, "median": med,
            "parent_spread": round(spread, 2), "median_gain": round(med["new"] / med["parent"], 4),
            "every_new_run_faster_than_every_parent_run": min(vals["new"]) > max(vals["parent"]),
            "medians_apart_by_more_than_twice_the_parent_spread": med["new"] - med["parent"] > 2 * spread}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--run", action="store_true", help="trace bench.py under rocprofv3 first")
    ap.add_argument("--trace", default="", help="existing trace: a *_kernel_trace.csv or a directory that holds one")
    ap.add_argument("--certify-eps", default="", help="profile_eps_arg of a plain bench.py line (with --run)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--groups", type=int, default=2)
    ap.add_argument("--lib", default="", help="with --run: trace another build of the library (the parent commit's) instead of the tree's")
    ap.add_argument("--ab", default="", help="instead of a trace: A/B of plain bench.py runs against this build of the library (the parent commit's)")
    ap.add_argument("--runs", type=int, default=3, help="with --ab: runs of each build")
    ap.add_argument("--tag", default="", help="label written into the summary")
    ap.add_argument("--out", default="", help="write the summary here as well as to stdout")
    ap.add_argument("--keep-trace", default="", help="with --run: copy the kernel trace CSV here")
    args = ap.parse_args()
    work = None
    if args.ab:
        text = json.dumps(bench_ab(args.ab, args.runs), indent=1)
        print(text)
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return
    if args.run:
        exe = shutil.which("rocprofv3")
        if not exe:
            raise SystemExit("rocprofv3 not on PATH")
        if not args.certify_eps:
            raise SystemExit("--run needs --certify-eps (profile_eps_arg of a plain bench.py run)")
        work = tempfile.mkdtemp(prefix="call_boundary_")
        cmd = [exe, "--kernel-trace", "--output-format", "csv", "-d", work, "--", sys.executable, os.path.join(ROOT, "bench.py"),
               "--steps", str(args.steps), "--warmup", str(args.warmup), "--substreams", str(args.groups), "--certify-eps", args.certify_eps]
        r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=280, env=lib_env(args.lib))
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-2000:])
            raise SystemExit(f"rocprofv3 pass failed (rc {r.returncode})")
        args.trace = work
    if not args.trace:
        raise SystemExit("give --run or --trace")
    if args.keep_trace:
        shutil.copyfile(find_trace(args.trace), args.keep_trace)
    res = summarise(find_trace(args.trace), args.steps, args.groups)
    if args.tag:
        res = {"tag": args.tag, **res}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if work:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
