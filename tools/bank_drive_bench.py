"""Sustained-drive benchmark of the resonator bank: `objects` x 256 modes at 48 kHz, 512-frame blocks, fp32, every object carrying D
force rows in every block -- as D drives (Scene.render_driven), or as D impacts in flight (the only way a tree without drives can do
the same arithmetic: long force pulses, no click), for D = 1, 2, 4, 8.  128 objects: 8 impacts on each is the impact cap (1024).

    python tools/bank_drive_bench.py --kind drives --rows 4            one measurement, one JSON line
    python tools/bank_drive_bench.py --kind impacts --rows 4 [--tree T]   the same rows as impacts, on this tree or on a built checkout T
    python tools/bank_drive_bench.py --against T [--runs 3]            the whole comparison with a built checkout T of the parent commit,
                                                                      interleaved, every run a fresh process -> profiles/bank_drives.json

The comparison also runs the unchanged tools/bank_bench.py of both trees (all_live.ms_per_block).  The resonator kernel's time per block is
the library's kernel-class timer; its issue-bound fraction is derived as tools/bank_bench.py derives it, at 11 + 2 D flop per mode-sample."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR, BLOCK, POINTS, MODES = 48000.0, 512, 4, 256
FP32_VECTOR_PEAK_TFLOPS = 157.3


def measure(tree, kind, rows, objects, blocks, renderers):
    sys.path.insert(0, tree)
    from mesheditor_amd import bank as hipbank
    from tools import bank_bench
    sc = bank_bench.build(objects, MODES, renderers)
    out = np.zeros(BLOCK, np.float32)
    n_rows = objects * rows
    if kind == "impacts":
        # pulses that outlast the run, started a ring-full (256 events) per block; no click (its filter runs all the same)
        step = np.float32(1.0 / (BLOCK * (blocks + 64)))
        queued = 0
        while queued < n_rows:
            for q in range(queued, min(n_rows, queued + 256)):
                o, i = divmod(q, rows)
                assert sc.L.mhx_enqueue(sc.h, hipbank.Event(0, o, i % POINTS, 1.0, 0.5, 0.125 * i, step, 1.0, 0.0, 0.0, 0.0, 0.0))
            queued = min(n_rows, queued + 256)
            sc.render(out)
        assert sc.active_impacts == n_rows, sc.active_impacts

        def block():
            sc.render(out)
    else:
        drives = (hipbank.Drive * n_rows)(*[hipbank.Drive(q // rows, (q % rows) % POINTS, 1.0, 0.5, 0.125 * (q % rows)) for q in range(n_rows)])
        signals = (0.01 * np.random.default_rng(1).standard_normal((n_rows, BLOCK))).astype(np.float32)

        def block():
            sc.render_driven(out, drives, signals)
    for _ in range(8):
        block()
    sc.time_kernels(True)
    times, peak = [], 0.0
    for _ in range(blocks):
        out[:] = 0
        t0 = time.perf_counter()
        block()
        times.append(time.perf_counter() - t0)
        peak = max(peak, float(np.abs(out).max()))
    k = sc.kernel_stats(2)
    sc.time_kernels(False)
    tuned, live, ring = sc.object_state()
    assert np.isfinite(peak) and peak > 0 and (ring == 1).all() and int(live.sum()) == objects * MODES
    if kind == "impacts":
        assert sc.active_impacts == n_rows
    sc.close()
    t = np.array(times)
    kernel_us = 1e3 * k["total_ms"] / max(1, k["launches"])
    flops = (11.0 + 2.0 * rows) * objects * MODES * BLOCK  # per block
    achieved = flops / (kernel_us * 1e-6) / 1e12 if kernel_us > 0 else 0.0
    return {"kind": kind, "rows_per_object": rows, "objects": objects, "modes_per_object": MODES, "blocks": blocks, "ms_per_block": 1e3 * float(t.mean()),
            "ms_per_block_median": 1e3 * float(np.median(t)), "ms_per_block_p99": 1e3 * float(np.quantile(t, 0.99)), "kernel_us_per_block": kernel_us,
            "roofline_bank": {"bound": "fp32 issue", "achieved": achieved, "peak": FP32_VECTOR_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": achieved / FP32_VECTOR_PEAK_TFLOPS,
                              "flop_per_mode_sample": 11 + 2 * rows}}


def child(args, limit=300):
    """One measurement in a fresh process under a time limit; anything but a clean exit ends the comparison."""
    p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable] + args, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit("a measurement ended with status %d: %s" % (p.returncode, " ".join(args)))
    return json.loads(p.stdout.strip().splitlines()[-1])


def compare(parent, runs, objects, blocks, renderers, out_path):
    me = os.path.abspath(__file__)
    common = ["--objects", str(objects), "--blocks", str(blocks), "--renderers", str(renderers)]
    result = {"workload": f"{objects} objects x {MODES} modes @48k, {BLOCK}-frame blocks, fp32, {renderers} renderers, D rows on every object in every block",
              "runs_each": runs, "all_live": {"parent": [], "new": []}, "rows": {}}

    def save():
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)
    q = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", "import torch; p = torch.cuda.get_device_properties(0); print(p.name, p.gcnArchName, '%d CUs' % p.multi_processor_count, '|', torch.version.hip)"], capture_output=True, text=True)
    if q.returncode != 0:
        raise SystemExit("no GPU to measure on: " + q.stderr[-2000:])
    result["device"], result["hip"] = (v.strip() for v in q.stdout.strip().splitlines()[-1].split("|"))
    for _ in range(runs):  # (a) the unchanged all-live benchmark, both trees, interleaved
        for name, tree in (("parent", parent), ("new", HERE)):
            r = child([os.path.join(tree, "tools", "bank_bench.py")], 600)
            result["all_live"][name].append({"ms_per_block": r["all_live"]["ms_per_block"], "kernel_us_per_block": r["all_live"]["kernel_us_per_block"],
                                             "steady_ms_per_block": r["steady_state"]["ms_per_block"]})
            save()
    for rows in (1, 2, 4, 8):  # (b), (c)
        cell = result["rows"][str(rows)] = {"parent_impacts": [], "new_drives": [], "new_impacts": []}
        for _ in range(runs):
            for name, tree, kind in (("parent_impacts", parent, "impacts"), ("new_drives", HERE, "drives"), ("new_impacts", HERE, "impacts")):
                cell[name].append(child([me, "--kind", kind, "--rows", str(rows), "--tree", tree] + common))
                save()
    a = result["all_live"]
    p, n = [r["ms_per_block"] for r in a["parent"]], [r["ms_per_block"] for r in a["new"]]
    result["summary"] = {"all_live_parent_ms": p, "all_live_new_ms": n, "parent_spread_max_over_min": max(p) / min(p), "new_median_over_parent_median": float(np.median(n) / np.median(p)),
                         "rows": {d: {k: float(np.median([r["ms_per_block"] for r in v])) for k, v in c.items()} | {"kernel_us_" + k: float(np.median([r["kernel_us_per_block"] for r in v])) for k, v in c.items()}
                                  for d, c in result["rows"].items()}}
    save()
    print(json.dumps(result["summary"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", choices=["drives", "impacts"], default="drives")
    ap.add_argument("--rows", type=int, default=4)
    ap.add_argument("--objects", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=1000)
    ap.add_argument("--renderers", type=int, default=4)
    ap.add_argument("--tree", default=HERE, help="built checkout whose library is measured (impacts only on one without drives)")
    ap.add_argument("--against", help="built checkout of the parent commit: run the whole comparison")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "bank_drives.json"))
    a = ap.parse_args()
    if a.against:
        compare(os.path.abspath(a.against), a.runs, a.objects, a.blocks, a.renderers, a.out)
    else:
        print(json.dumps(measure(os.path.abspath(a.tree), a.kind, a.rows, a.objects, a.blocks, a.renderers)))


if __name__ == "__main__":
    main()
