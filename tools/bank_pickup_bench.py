"""Pickup benchmark of the resonator bank: `objects` x 256 modes at 48 kHz, 512-frame blocks, fp32, one drive on every object in every
block (every object renders its tuned set), P deflection pickups on every object (Scene.render_read), P = 0, 1, 2, 4, 8.

    python tools/bank_pickup_bench.py --pickups 4                       one measurement, one JSON line
    python tools/bank_pickup_bench.py --pickups 0 --entry driven [--tree T]  the same scene through render_driven, on this tree or on a
                                                                        built checkout T (the parent commit has no render_read)
    python tools/bank_pickup_bench.py --against T [--runs 3]            the whole comparison with a built checkout T of the parent commit,
                                                                        interleaved, every run a fresh process -> profiles/bank_pickups.json

The comparison also runs the unchanged tools/bank_bench.py of both trees (all_live.ms_per_block).  The resonator kernel's time per block is
the library's kernel-class timer; its share of the fp32 issue peak is derived as tools/bank_bench.py derives it, at 11 + 2 (the drive)
+ 4 P flop per mode-sample (a pickup is two multiply-adds per mode and sample)."""
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
PICKUPS = (0, 1, 2, 4, 8)


def measure(tree, entry, pickups, objects, blocks, renderers):
    sys.path.insert(0, tree)
    from mesheditor_amd import bank as hipbank
    from tools import bank_bench
    sc = bank_bench.build(objects, MODES, renderers)
    out = np.zeros(BLOCK, np.float32)
    drives = (hipbank.Drive * objects)(*[hipbank.Drive(o, o % POINTS, 1.0, 0.5, 0.125) for o in range(objects)])
    signals = (0.01 * np.random.default_rng(1).standard_normal((objects, BLOCK))).astype(np.float32)
    loudest = [0.0]
    if entry == "read":
        n = objects * pickups
        probes = (hipbank.Pickup * max(n, 1))(*[hipbank.Pickup.of(q // pickups, ((q % pickups) % POINTS, (q + 1) % POINTS, (q + 2) % POINTS), (0.5, 0.25, 0.25),
                                                                 (0.25, -1.0, 0.5), 1.0, (q % pickups) % 3) for q in range(n)])
        probes = probes if n else []

        def block():
            reads, flags = sc.render_read(out, drives, signals, probes)
            if n:
                assert flags.all()
                loudest[0] = max(loudest[0], float(np.abs(reads).max()))
    else:
        assert pickups == 0

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
    assert pickups == 0 or (np.isfinite(loudest[0]) and loudest[0] > 0)
    sc.close()
    t = np.array(times)
    kernel_us = 1e3 * k["total_ms"] / max(1, k["launches"])
    flop = 11 + 2 + 4 * pickups
    achieved = flop * objects * MODES * BLOCK / (kernel_us * 1e-6) / 1e12 if kernel_us > 0 else 0.0
    return {"entry": entry, "pickups_per_object": pickups, "objects": objects, "modes_per_object": MODES, "blocks": blocks, "ms_per_block": 1e3 * float(t.mean()),
            "ms_per_block_median": 1e3 * float(np.median(t)), "ms_per_block_p99": 1e3 * float(np.quantile(t, 0.99)), "kernel_us_per_block": kernel_us,
            "roofline_bank": {"bound": "fp32 issue", "achieved": achieved, "peak": FP32_VECTOR_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": achieved / FP32_VECTOR_PEAK_TFLOPS,
                              "flop_per_mode_sample": flop}}


def child(args, limit=300):
    """One measurement in a fresh process under a time limit; anything but a clean exit ends the comparison."""
    p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable] + args, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit("a measurement ended with status %d: %s" % (p.returncode, " ".join(args)))
    return json.loads(p.stdout.strip().splitlines()[-1])


def compare(parent, runs, objects, blocks, renderers, out_path, all_live):
    me = os.path.abspath(__file__)
    common = ["--objects", str(objects), "--blocks", str(blocks), "--renderers", str(renderers)]
    result = {"workload": f"{objects} objects x {MODES} modes @48k, {BLOCK}-frame blocks, fp32, {renderers} renderers, one drive and P pickups on every object in every block",
              "runs_each": runs, "all_live": {"parent": [], "new": []}, "p0": {"parent_driven": [], "new_read": []}, "pickups": {}}

    def save():
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)
    q = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", "import torch; p = torch.cuda.get_device_properties(0); print(p.name, p.gcnArchName, '%d CUs' % p.multi_processor_count, '|', torch.version.hip)"], capture_output=True, text=True)
    if q.returncode != 0:
        raise SystemExit("no GPU to measure on: " + q.stderr[-2000:])
    result["device"], result["hip"] = (v.strip() for v in q.stdout.strip().splitlines()[-1].split("|"))
    for _ in range(runs if all_live else 0):  # (b) the unchanged all-live benchmark, both trees, interleaved
        for name, tree in (("parent", parent), ("new", HERE)):
            r = child([os.path.join(tree, "tools", "bank_bench.py")], 600)
            result["all_live"][name].append({"ms_per_block": r["all_live"]["ms_per_block"], "kernel_us_per_block": r["all_live"]["kernel_us_per_block"],
                                             "steady_ms_per_block": r["steady_state"]["ms_per_block"]})
            save()
    for _ in range(runs):  # (a) no pickups: the parent's render_driven against render_read, interleaved
        result["p0"]["parent_driven"].append(child([me, "--entry", "driven", "--pickups", "0", "--tree", parent] + common))
        result["p0"]["new_read"].append(child([me, "--entry", "read", "--pickups", "0"] + common))
        save()
    for _ in range(runs):
        for p in PICKUPS[1:]:
            result["pickups"].setdefault(str(p), []).append(child([me, "--entry", "read", "--pickups", str(p)] + common))
            save()

    def med(rows, key):
        return float(np.median([r[key] for r in rows])) if rows else None
    a, p0 = result["all_live"], result["p0"]
    spread = lambda rows, key: (max(r[key] for r in rows) / min(r[key] for r in rows)) if rows else None
    base_ms, base_us = med(p0["new_read"], "ms_per_block"), med(p0["new_read"], "kernel_us_per_block")
    result["summary"] = {
        "all_live_parent_ms": [r["ms_per_block"] for r in a["parent"]], "all_live_new_ms": [r["ms_per_block"] for r in a["new"]],
        "all_live_parent_spread_max_over_min": spread(a["parent"], "ms_per_block"),
        "all_live_new_median_over_parent_median": (med(a["new"], "ms_per_block") / med(a["parent"], "ms_per_block")) if a["parent"] else None,
        "p0_parent_driven_ms": [r["ms_per_block"] for r in p0["parent_driven"]], "p0_new_read_ms": [r["ms_per_block"] for r in p0["new_read"]],
        "p0_parent_spread_max_over_min": spread(p0["parent_driven"], "ms_per_block"), "p0_new_median_over_parent_median": base_ms / med(p0["parent_driven"], "ms_per_block"),
        "p0_kernel_us": {"parent_driven": med(p0["parent_driven"], "kernel_us_per_block"), "new_read": base_us},
        "pickups": {p: {"ms_per_block": med(rows, "ms_per_block"), "kernel_us_per_block": med(rows, "kernel_us_per_block"),
                        "ms_per_pickup_and_object": (med(rows, "ms_per_block") - base_ms) / (int(p) * objects), "kernel_us_per_pickup": (med(rows, "kernel_us_per_block") - base_us) / int(p),
                        "frac_of_fp32_issue_peak": med([r["roofline_bank"] for r in rows], "frac")} for p, rows in result["pickups"].items()}}
    save()
    print(json.dumps(result["summary"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entry", choices=["read", "driven"], default="read")
    ap.add_argument("--pickups", type=int, default=4)
    ap.add_argument("--objects", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=1000)
    ap.add_argument("--renderers", type=int, default=4)
    ap.add_argument("--tree", default=HERE, help="built checkout whose library is measured (render_driven only on one without pickups)")
    ap.add_argument("--against", help="built checkout of the parent commit: run the whole comparison")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-all-live", action="store_true", help="skip tools/bank_bench.py of both trees")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "bank_pickups.json"))
    a = ap.parse_args()
    if a.against:
        compare(os.path.abspath(a.against), a.runs, a.objects, a.blocks, a.renderers, a.out, not a.no_all_live)
    else:
        print(json.dumps(measure(os.path.abspath(a.tree), a.entry, a.pickups, a.objects, a.blocks, a.renderers)))


if __name__ == "__main__":
    main()
