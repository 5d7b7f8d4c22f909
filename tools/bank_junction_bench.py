"""Junction benchmark of the resonator bank: `objects` x 256 modes at 48 kHz, 512-frame blocks, fp32, one drive on every object in every
block (every object renders its tuned set), J contact junctions (Scene.render_coupled), J = 0, 1, 16, 64, one- and two-sided, K C = 10,
the exciter dipping in and out of the surface.

    python tools/bank_junction_bench.py --junctions 16 --sides 2             one measurement, one JSON line
    python tools/bank_junction_bench.py --entry replay --junctions 16 --sides 2 --forces F [--tree T]
                                                                             the same scene through render_driven with the force rows
                                                                             saved in F (by a --save-forces run) replayed as drives: the
                                                                             open-loop cost of the same excitation, on this tree or on a
                                                                             built checkout T (the parent commit has no render_coupled)
    python tools/bank_junction_bench.py --against T [--runs 3]               the whole comparison with a built checkout T of the parent
                                                                             commit, interleaved, every run a fresh process
                                                                             -> profiles/bank_junctions.json

    python tools/bank_junction_bench.py --law hertz --junctions 16            the same with Hertz junctions (f = K delta^1.5, K chosen so that
                                                                             K C sqrt(x0) = 10 at the approach's peak x0)
    python tools/bank_junction_bench.py --law damped --junctions 16           the same with contact damping (MH_JUNCTION_DAMPED, l x0 = 1 at the approach's
                                                                             peak x0, the carry passed from block to block); hertz-damped: on the Hertz law
    python tools/bank_junction_bench.py --damped-against T [--runs 3]        the all-linear and all-Hertz undamped calls of a built checkout T of the parent
                                                                             commit and of this tree (J = 1, 16, 64, one- and two-sided), interleaved in fresh
                                                                             processes, and this tree's damped calls beside them -> profiles/bank_damped.json
    python tools/bank_junction_bench.py --laws-against T [--runs 3]          the all-linear calls of a built checkout T of the parent commit and
                                                                             of this tree, and this tree's Hertz calls, J = 1, 16, 64, interleaved,
                                                                             every run a fresh process -> profiles/bank_hertz.json

    python tools/bank_junction_bench.py --members 3 --junctions 48            16 groups of three junctions (MH_JUNCTION_SHARED): exciter junctions at
                                                                             three points of each of 16 objects, solved together per frame;
                                                                             with --ungrouped the same 48 junctions on 48 objects of their own
                                                                             (no flag: the coupled kernel, the like-for-like the parent renders)
    python tools/bank_junction_bench.py --groups --against T [--runs 3]      the unchanged paths -- J = 0 and the all-linear ungrouped calls J = 1, 16,
                                                                             64 of a built checkout T of the parent commit and of this tree, and
                                                                             tools/bank_bench.py of both, interleaved, every run a fresh process --
                                                                             and this tree's groups, G = 1, 16, 64 of n = 2, 3, 4, beside the same
                                                                             junctions ungrouped (256 objects) -> profiles/bank_groups.json

    python tools/bank_junction_bench.py --pickups 4 --junctions 16 --sides 2   the call through Scene.render_observed with 4 pickups (advances 0, 1, 2 in
                                                                             turn) on every junction object; --pickups 0: the same entry without them
    python tools/bank_junction_bench.py --observed-against T [--runs 3]      this tree's render_observed with P = 0, 1, 2, 4, 8 pickups on every junction
                                                                             object (16 and 64 junctions, one- and two-sided; 16 and 64 groups of 3), and the
                                                                             unchanged paths -- render_coupled, render_damped and tools/bank_bench.py -- of a
                                                                             built checkout T of the parent commit and of this tree, interleaved in fresh
                                                                             processes -> profiles/bank_observed.json
    python tools/bank_junction_bench.py --friction --law hertz --junctions 16   one measurement: lone junctions with Coulomb friction through Scene.render_friction
    python tools/bank_junction_bench.py --friction --against T               this tree's frictional junctions beside the same junctions without the flag, and the
                                                                             unchanged calls of T and of this tree -> profiles/bank_friction.json

(The coupled kernel and the group kernel are timed under one kernel class, 6: a block that holds lone junctions AND groups makes two
launches of it, and `coupled_kernel_us_per_block`, the class total over its launch count, is then per launch.  No mode here mixes the two.
With --pickups P > 0 the pickup rows' kernel, k_bank_observe_rows, is a second launch of the class: `junction_kernels_us_per_block`, the
class total over the blocks, is the junction kernel and that kernel together.)

The comparison also runs the unchanged tools/bank_bench.py of both trees (all_live.ms_per_block).  Kernel times per block are the
library's kernel-class timers: class 2 the resonator kernel of the objects off the junctions, class 6 the coupled kernel.  The coupled
kernel is one workgroup per junction running a serial chain per frame; `coupled_cycles_per_frame` is its time over the block's frames at
the 2.4 GHz engine clock."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR, BLOCK, POINTS, MODES = 48000.0, 512, 4, 256
ENGINE_MHZ = 2400.0
JUNCTIONS = (0, 1, 16, 64)
NORMAL = (0.25, -1.0, 0.5)


def sides_of(j, sides):
    """The objects of junction j: j itself (one-sided), or 2j and 2j + 1."""
    return (j,) if sides == 1 else (2 * j, 2 * j + 1)


def measure(tree, entry, junctions, sides, objects, blocks, renderers, forces_path, save_forces, law="linear", members=0, ungrouped=False, pickups=None, mixed=False, double=False, damped_groups=False,
            friction=False):
    """members >= 2: the junctions are groups of `members` exciter junctions, junction q at point q % members of object q // members with
    the shared flag -- or, ungrouped, of object q without it.  pickups = P (not None): the call goes through Scene.render_observed with P
    pickups on every junction object.  mixed: with members and law = "hertz", the groups' members are Hertz junctions and the call goes through
    Scene.render_mixed (law = "linear": the same groups with linear members through the same entry).  damped_groups: the call goes through
    Scene.render_damped_groups with the carry passed from block to block; law = "hertz-damped": every member a damped Hertz junction
    (l x0 = 1), "hertz": the same groups with plain Hertz members through the same entry.  friction: lone junctions (law "linear" or "hertz") with
    the friction flag through Scene.render_friction -- tangent (1, 0.25, 0) on side a and its opposite on side b, mu = 0.3 (halved until the
    cone condition admits it), kt = K, a travel of twice the free deflection that swings once per block, the anchor passed from block to block."""
    sys.path.insert(0, tree)
    from mesheditor_amd import bank as hipbank
    from tools import bank_bench
    assert junctions * sides <= objects
    if members:
        assert entry == "coupled" and sides == 1 and (law == "linear" or (mixed and law == "hertz") or (damped_groups and law in ("hertz", "hertz-damped"))) and 2 <= members <= POINTS and junctions % members == 0
    where = lambda q: (q, 1) if not members else ((q, q % members) if ungrouped else (q // members, q % members))  # (object, point) of junction q's side a
    sc = bank_bench.build(objects, MODES, renderers) if not double else build_double(hipbank, bank_bench, objects, renderers)  # double: the fp64 bank
    out = np.zeros(BLOCK, sc.dtype)
    drives = [hipbank.Drive(o, o % POINTS, 1.0, 0.5, 0.125) for o in range(objects)]
    signals = (0.01 * np.random.default_rng(1).standard_normal((objects, BLOCK))).astype(np.float32)
    peak_force, kept = [0.0], []
    if entry == "coupled":
        side = lambda o, sign, point=1: hipbank.JunctionSide.of(o, point, (1.0, 0.0, 0.0), tuple(sign * v for v in NORMAL), 2.0)
        flag = {"hertz": True} if law in ("hertz", "hertz-damped") else {}  # (a tree from before the Hertz law takes no such argument)
        damped = law in ("damped", "hertz-damped")
        if damped:
            flag["damped"] = True
        if friction:
            assert not members and law in ("linear", "hertz") and pickups is None
            flag["friction"] = True
        if members and not ungrouped:
            flag = {"shared": True, "hertz": True} if mixed and law == "hertz" else {"shared": True}
            if damped_groups:
                flag = {"shared": True, "hertz": True, "damped": True} if law == "hertz-damped" else {"shared": True, "hertz": True}
        first = lambda j: side(where(j)[0], 1.0, where(j)[1]) if members else side(sides_of(j, sides)[0], 1.0)
        make = lambda k: (hipbank.Junction * max(junctions, 1))(*[hipbank.Junction.of(first(j), side(sides_of(j, sides)[1], -1.0) if sides == 2 else None, k[j], **flag)
                                                                    for j in range(junctions)])
        rows = (hipbank.Drive * objects)(*drives)
        none = np.zeros((junctions, BLOCK), np.float32)
        # the compliances and the size of the free deflection, from two blocks with K = 0
        comp = np.ones(junctions)
        if junctions:
            dead = (hipbank.Friction * junctions)(*[hipbank.Friction.of() for _ in range(junctions)]) if friction else None
            probe = (lambda *a: sc.render_friction(*a, dead, none)) if friction else sc.render_damped_groups if damped_groups else sc.render_mixed if mixed else sc.render_coupled
            _, _, _, comp, status = probe(out, rows, signals, [], make([0.0] * junctions), none)[:5]
            assert (status == 1).all() and (comp > 0).all()
            picks = (hipbank.Pickup * junctions)(*[hipbank.Pickup.of(where(j)[0] if members else sides_of(j, sides)[0], where(j)[1], (1.0, 0.0, 0.0), NORMAL, 2.0, 1) for j in range(junctions)])
            reads, _ = sc.render_read(out, rows, signals, picks)
            free = np.abs(reads).max(axis=1)
            t = np.arange(BLOCK)
            u = np.array([(free[j] * (np.sin(2 * np.pi * t / 256.0 + j) + 0.1)).astype(np.float32) for j in range(junctions)])  # periodic in the block
        # linear: K C = 10; Hertz: K C sqrt(x0) = 10 at the approach's peak x0
        contacts = make([10.0 / (c * (np.sqrt(float(u[j].max())) if "hertz" in law else 1.0)) for j, c in enumerate(comp)]) if junctions else []
        u = u if junctions else none
        damping = [1.0 / (float(u[j].max()) * SR) for j in range(junctions)]  # damped: D in s/m with l x0 = D SR x0 = 1
        carry = [None]
        if friction and junctions:
            stiff = [float(c.stiffness) for c in contacts]
            travel = np.array([(2.0 * free[j] * np.sin(2 * np.pi * t / 512.0 + 0.5 * j)).astype(np.float32) for j in range(junctions)])
            tangent = (1.0, 0.25, 0.0)
            mu, anchor, counts = 0.3, [None], np.zeros(3, np.int64)
            while True:  # the cone condition mu |C_nt| <= C_nn: a refused junction halves mu
                slides = (hipbank.Friction * junctions)(*[hipbank.Friction.of(tangent, tuple(-v for v in tangent) if sides == 2 else (0.0, 0.0, 0.0), mu, stiff[j]) for j in range(junctions)])
                if (sc.render_friction(out, rows, signals, [], contacts, u, slides, travel)[4] == 1).all():
                    break
                mu *= 0.5
                assert mu > 1e-3
        watched = sorted({where(j)[0] for j in range(junctions)} if members else {o for j in range(junctions) for o in sides_of(j, sides)})
        probes = [hipbank.Pickup.of(o, (o + i) % POINTS, (1.0, 0.0, 0.0), NORMAL, 1.0 + 0.5 * i, i % 3) for o in watched for i in range(pickups or 0)]
        probes = (hipbank.Pickup * len(probes))(*probes) if probes else []
        peak_read = [0.0]

        def block():
            if friction and junctions:
                got = sc.render_friction(out, rows, signals, [], contacts, u, slides, travel, None, None, anchor[0])
                forces, status, anchor[0] = got[2], got[4], got[8]
                counts[:] += got[9].sum(axis=0).astype(np.int64)
            elif friction:
                forces, status = sc.render_friction(out, rows, signals, [], contacts, u, [], none)[2:5:2]
            elif damped_groups:
                _, _, forces, _, status, carry[0], unconverged = sc.render_damped_groups(out, rows, signals, [], contacts, u, damping, carry[0])
                assert not unconverged.any()
            elif mixed:
                _, _, forces, _, status, _, unconverged = sc.render_mixed(out, rows, signals, [], contacts, u)
                assert not unconverged.any()
            elif pickups is not None:
                reads, flags, forces, _, status, carry[0] = sc.render_observed(out, rows, signals, probes, contacts, u, damping if damped else None, carry[0])
                assert (flags == 1).all()
                peak_read[0] = max(peak_read[0], float(np.abs(reads).max()) if len(reads) else 0.0)
            elif damped:
                _, _, forces, _, status, carry[0] = sc.render_damped(out, rows, signals, [], contacts, u, damping, carry[0])
            else:
                _, _, forces, _, status = sc.render_coupled(out, rows, signals, [], contacts, u)
            if junctions:
                assert (status == 1).all()
                peak_force[0] = max(peak_force[0], float(np.abs(forces).max()))
                kept[:] = [forces]
    else:
        replayed = np.load(forces_path) if junctions else np.zeros((0, BLOCK), np.float32)
        assert replayed.shape == (junctions, BLOCK)
        for j in range(junctions):
            for i, o in enumerate(sides_of(j, sides)):
                sign = 1.0 if i == 0 else -1.0
                drives.append(hipbank.Drive(o, 1, *(sign * v for v in NORMAL)))
        rows = (hipbank.Drive * len(drives))(*drives)
        signals = np.concatenate([signals] + [replayed[j:j + 1] for j in range(junctions) for _ in range(sides)]).astype(np.float32)

        def block():
            sc.render_driven(out, rows, signals)
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
    kj = sc.kernel_stats(6) if entry == "coupled" else {"launches": 0, "total_ms": 0.0}
    sc.time_kernels(False)
    tuned, live, ring = sc.object_state()
    assert np.isfinite(peak) and peak > 0 and (ring == 1).all() and int(live.sum()) == objects * MODES
    assert entry != "coupled" or junctions == 0 or (np.isfinite(peak_force[0]) and peak_force[0] > 0)
    assert not pickups or not junctions or (np.isfinite(peak_read[0]) and peak_read[0] > 0)
    if save_forces and junctions:
        np.save(save_forces, kept[0].astype(np.float32))
    sc.close()
    t = np.array(times)
    coupled_us = 1e3 * kj["total_ms"] / max(1, kj["launches"])
    more = {"friction_mu": mu, "friction_frames_stick_slip_none": [int(v) for v in counts]} if friction and junctions else {}
    return {**more, "precision": "fp64" if double else "fp32", "entry": "friction" if friction else "damped_groups" if damped_groups else "mixed" if mixed else entry if pickups is None else "observed", "pickups_per_object": pickups, "junction_kernels_us_per_block": 1e3 * kj["total_ms"] / max(1, blocks), "law": law, "junctions": junctions, "sides": sides, "members": members, "grouped": bool(members) and not ungrouped, "objects": objects, "modes_per_object": MODES, "blocks": blocks, "ms_per_block": 1e3 * float(t.mean()),
            "ms_per_block_median": 1e3 * float(np.median(t)), "ms_per_block_p99": 1e3 * float(np.quantile(t, 0.99)), "kernel_us_per_block": 1e3 * k["total_ms"] / max(1, k["launches"]),
            "coupled_kernel_us_per_block": coupled_us, "coupled_us_per_frame": coupled_us / BLOCK, "coupled_cycles_per_frame": coupled_us / BLOCK * ENGINE_MHZ,
            "real_time_ms_per_block": 1e3 * BLOCK / SR}


def build_double(hipbank, bank_bench, objects, renderers):
    """tools/bank_bench.build's scene on the fp64 bank."""
    pos = np.array([[p * 0.01, 0.0, 0.02 if p % 2 else 0.0] for p in range(POINTS)], np.float32)
    idx = np.array([[p, p + 1, p + 2] for p in range(POINTS - 2)], np.uint32).reshape(-1)
    sc = hipbank.Scene(SR, 0, use_double=True)
    sc.set_renderers(renderers)
    for o in range(objects):
        f, t, sh = bank_bench.modes_for(o, MODES)
        slot = sc.add_object(o, sh, pos, idx)
        sc.tune_object(slot, f, t)
        sc.set_gains(slot, 1.0, 1.0)
    sc.install()
    sc.render(np.zeros(BLOCK, sc.dtype))
    return sc


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
    result = {"workload": f"{objects} objects x {MODES} modes @48k, {BLOCK}-frame blocks, fp32, {renderers} renderers, one drive on every object and J junctions (K C = 10) in every block",
              "runs_each": runs, "all_live": {"parent": [], "new": []}, "j0": {"parent_driven": [], "new_coupled": []}, "junctions": {}}

    def save():
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)
    q = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", "import torch; p = torch.cuda.get_device_properties(0); print(p.name, p.gcnArchName, '%d CUs' % p.multi_processor_count, '|', torch.version.hip)"], capture_output=True, text=True)
    if q.returncode != 0:
        raise SystemExit("no GPU to measure on: " + q.stderr[-2000:])
    result["device"], result["hip"] = (v.strip() for v in q.stdout.strip().splitlines()[-1].split("|"))
    for _ in range(runs if all_live else 0):  # the unchanged all-live benchmark, both trees, interleaved
        for name, tree in (("parent", parent), ("new", HERE)):
            r = child([os.path.join(tree, "tools", "bank_bench.py")], 600)
            result["all_live"][name].append({"ms_per_block": r["all_live"]["ms_per_block"], "kernel_us_per_block": r["all_live"]["kernel_us_per_block"],
                                             "steady_ms_per_block": r["steady_state"]["ms_per_block"]})
            save()
    scratch = tempfile.mkdtemp(prefix="junction_forces_")
    for _ in range(runs):
        result["j0"]["parent_driven"].append(child([me, "--entry", "replay", "--junctions", "0", "--tree", parent] + common))
        result["j0"]["new_coupled"].append(child([me, "--entry", "coupled", "--junctions", "0"] + common))
        save()
        for sides in (1, 2):
            for j in JUNCTIONS[1:]:
                forces = os.path.join(scratch, "f_%d_%d.npy" % (j, sides))
                row = result["junctions"].setdefault("%d x %d-sided" % (j, sides), {"coupled": [], "parent_replay": []})
                row["coupled"].append(child([me, "--entry", "coupled", "--junctions", str(j), "--sides", str(sides), "--save-forces", forces] + common))
                row["parent_replay"].append(child([me, "--entry", "replay", "--junctions", str(j), "--sides", str(sides), "--forces", forces, "--tree", parent] + common))
                save()

    def med(rows, key):
        return float(np.median([r[key] for r in rows])) if rows else None
    a, j0 = result["all_live"], result["j0"]
    spread = lambda rows, key: (max(r[key] for r in rows) / min(r[key] for r in rows)) if rows else None
    result["summary"] = {
        "all_live_parent_ms": [r["ms_per_block"] for r in a["parent"]], "all_live_new_ms": [r["ms_per_block"] for r in a["new"]],
        "all_live_parent_spread_max_over_min": spread(a["parent"], "ms_per_block"),
        "all_live_new_median_over_parent_median": (med(a["new"], "ms_per_block") / med(a["parent"], "ms_per_block")) if a["parent"] else None,
        "j0_parent_driven_ms": [r["ms_per_block"] for r in j0["parent_driven"]], "j0_new_coupled_ms": [r["ms_per_block"] for r in j0["new_coupled"]],
        "j0_parent_spread_max_over_min": spread(j0["parent_driven"], "ms_per_block"),
        "j0_new_median_over_parent_median": med(j0["new_coupled"], "ms_per_block") / med(j0["parent_driven"], "ms_per_block"),
        "real_time_ms_per_block": 1e3 * BLOCK / SR,
        "junctions": {name: {"coupled_ms_per_block": med(row["coupled"], "ms_per_block"), "parent_replay_ms_per_block": med(row["parent_replay"], "ms_per_block"),
                             "coupled_kernel_us_per_block": med(row["coupled"], "coupled_kernel_us_per_block"), "main_kernel_us_per_block": med(row["coupled"], "kernel_us_per_block"),
                             "parent_replay_kernel_us_per_block": med(row["parent_replay"], "kernel_us_per_block"),
                             "coupled_cycles_per_frame": med(row["coupled"], "coupled_cycles_per_frame")} for name, row in result["junctions"].items()}}
    save()
    print(json.dumps(result["summary"]))


def compare_laws(parent, runs, objects, blocks, renderers, out_path):
    """The all-linear calls of the parent and of this tree (the same kernels: the new figures have to land within the parent's own spread)
    and this tree's Hertz calls beside them."""
    me = os.path.abspath(__file__)
    common = ["--objects", str(objects), "--blocks", str(blocks), "--renderers", str(renderers)]
    result = {"workload": f"{objects} objects x {MODES} modes @48k, {BLOCK}-frame blocks, fp32, {renderers} renderers, one drive on every object and J junctions in every block "
                          "(linear: K C = 10; Hertz: K C sqrt(x0) = 10)", "runs_each": runs, "junctions": {}}

    def save():
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)
    q = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", "import torch; p = torch.cuda.get_device_properties(0); print(p.name, p.gcnArchName, '%d CUs' % p.multi_processor_count, '|', torch.version.hip)"], capture_output=True, text=True)
    if q.returncode != 0:
        raise SystemExit("no GPU to measure on: " + q.stderr[-2000:])
    result["device"], result["hip"] = (v.strip() for v in q.stdout.strip().splitlines()[-1].split("|"))
    for _ in range(runs):
        for sides in (1, 2):
            for j in JUNCTIONS[1:]:
                row = result["junctions"].setdefault("%d x %d-sided" % (j, sides), {"parent_linear": [], "new_linear": [], "new_hertz": []})
                shape = ["--entry", "coupled", "--junctions", str(j), "--sides", str(sides)] + common
                row["parent_linear"].append(child([me, "--tree", parent, "--law", "linear"] + shape))
                row["new_linear"].append(child([me, "--law", "linear"] + shape))
                row["new_hertz"].append(child([me, "--law", "hertz"] + shape))
                save()
    med = lambda rows, key: float(np.median([r[key] for r in rows]))
    spread = lambda rows, key: max(r[key] for r in rows) / min(r[key] for r in rows)
    result["summary"] = {name: {"parent_linear_ms_per_block": [r["ms_per_block"] for r in row["parent_linear"]], "new_linear_ms_per_block": [r["ms_per_block"] for r in row["new_linear"]],
                                "parent_spread_max_over_min": spread(row["parent_linear"], "ms_per_block"),
                                "new_linear_median_over_parent_median": med(row["new_linear"], "ms_per_block") / med(row["parent_linear"], "ms_per_block"),
                                "hertz_ms_per_block": med(row["new_hertz"], "ms_per_block"), "linear_ms_per_block": med(row["new_linear"], "ms_per_block"),
                                "parent_linear_coupled_cycles_per_frame": med(row["parent_linear"], "coupled_cycles_per_frame"),
                                "linear_coupled_cycles_per_frame": med(row["new_linear"], "coupled_cycles_per_frame"),
                                "hertz_coupled_cycles_per_frame": med(row["new_hertz"], "coupled_cycles_per_frame"),
                                "hertz_over_linear_cycles_per_frame": med(row["new_hertz"], "coupled_cycles_per_frame") / med(row["new_linear"], "coupled_cycles_per_frame")}
                         for name, row in result["junctions"].items()}
    save()
    print(json.dumps(result["summary"]))


def compare_damped(parent, runs, objects, blocks, renderers, out_path):
    """The all-linear and all-Hertz undamped calls of the parent and of this tree (the same kernels: the new figures have to land within the
    parent's own spread) and this tree's damped calls beside them."""
    me = os.path.abspath(__file__)
    common = ["--objects", str(objects), "--blocks", str(blocks), "--renderers", str(renderers)]
    result = {"workload": f"{objects} objects x {MODES} modes @48k, {BLOCK}-frame blocks, fp32, {renderers} renderers, one drive on every object and J junctions in every block "
                          "(linear: K C = 10; Hertz: K C sqrt(x0) = 10; damped: l x0 = 1, the carry passed on)", "runs_each": runs, "junctions": {}}

    def save():
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)
    q = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", "import torch; p = torch.cuda.get_device_properties(0); print(p.name, p.gcnArchName, '%d CUs' % p.multi_processor_count, '|', torch.version.hip)"], capture_output=True, text=True)
    if q.returncode != 0:
        raise SystemExit("no GPU to measure on: " + q.stderr[-2000:])
    result["device"], result["hip"] = (v.strip() for v in q.stdout.strip().splitlines()[-1].split("|"))
    calls = (("parent_linear", parent, "linear"), ("new_linear", None, "linear"), ("parent_hertz", parent, "hertz"), ("new_hertz", None, "hertz"),
             ("new_damped", None, "damped"), ("new_hertz_damped", None, "hertz-damped"))
    for _ in range(runs):
        for sides in (1, 2):
            for j in JUNCTIONS[1:]:
                row = result["junctions"].setdefault("%d x %d-sided" % (j, sides), {name: [] for name, _, _ in calls})
                shape = ["--entry", "coupled", "--junctions", str(j), "--sides", str(sides)] + common
                for name, tree, law in calls:
                    row[name].append(child([me, "--law", law] + (["--tree", tree] if tree else []) + shape))
                save()
    med = lambda rows, key: float(np.median([r[key] for r in rows]))
    spread = lambda rows, key: max(r[key] for r in rows) / min(r[key] for r in rows)
    summary = {}
    for name, row in result["junctions"].items():
        entry = {"real_time_ms_per_block": 1e3 * BLOCK / SR}
        for law in ("linear", "hertz"):
            entry.update({"parent_%s_ms_per_block" % law: [r["ms_per_block"] for r in row["parent_" + law]], "new_%s_ms_per_block" % law: [r["ms_per_block"] for r in row["new_" + law]],
                          "parent_%s_spread_max_over_min" % law: spread(row["parent_" + law], "ms_per_block"),
                          "new_%s_median_over_parent_median" % law: med(row["new_" + law], "ms_per_block") / med(row["parent_" + law], "ms_per_block"),
                          "new_%s_median_inside_parent_range" % law: bool(min(r["ms_per_block"] for r in row["parent_" + law]) <= med(row["new_" + law], "ms_per_block") <= max(r["ms_per_block"] for r in row["parent_" + law])),
                          "new_%s_median_over_parent_slowest" % law: med(row["new_" + law], "ms_per_block") / max(r["ms_per_block"] for r in row["parent_" + law]),
                          "parent_%s_coupled_cycles_per_frame" % law: med(row["parent_" + law], "coupled_cycles_per_frame"),
                          "%s_coupled_cycles_per_frame" % law: med(row["new_" + law], "coupled_cycles_per_frame")})
        for law, base in (("damped", "linear"), ("hertz_damped", "hertz")):
            entry.update({"%s_ms_per_block" % law: med(row["new_" + law], "ms_per_block"), "%s_coupled_cycles_per_frame" % law: med(row["new_" + law], "coupled_cycles_per_frame"),
                          "%s_over_%s_cycles_per_frame" % (law, base): med(row["new_" + law], "coupled_cycles_per_frame") / med(row["new_" + base], "coupled_cycles_per_frame")})
        summary[name] = entry
    result["summary"] = summary
    save()
    print(json.dumps(summary))


def compare_observed(parent, runs, objects, blocks, renderers, out_path, all_live):
    """This tree's render_observed with P pickups on every junction object (one run each), and the unchanged paths of the parent and of this
    tree, `runs` fresh processes each: the new figures may not be slower than the parent's by more than the spread of the parent's own runs."""
    me = os.path.abspath(__file__)
    common = ["--objects", str(objects), "--blocks", str(blocks), "--renderers", str(renderers)]
    result = {"workload": f"{objects} objects x {MODES} modes @48k, {BLOCK}-frame blocks, fp32, {renderers} renderers, one drive on every object and J junctions (K C = 10) in every block; "
                          "observed: through render_observed with P pickups on every junction object", "runs_each": runs, "observed": {}, "unchanged": {}, "all_live": {"parent": [], "new": []}}

    def save():
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)
    q = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", "import torch; p = torch.cuda.get_device_properties(0); print(p.name, p.gcnArchName, '%d CUs' % p.multi_processor_count, '|', torch.version.hip)"], capture_output=True, text=True)
    if q.returncode != 0:
        raise SystemExit("no GPU to measure on: " + q.stderr[-2000:])
    result["device"], result["hip"] = (v.strip() for v in q.stdout.strip().splitlines()[-1].split("|"))
    shapes = [("%d x %d-sided" % (j, sides), ["--junctions", str(j), "--sides", str(sides)]) for sides in (1, 2) for j in (16, 64)]
    shapes += [("%d groups of 3" % g, ["--members", "3", "--junctions", str(3 * g)]) for g in (16, 64)]  # (every member junction counts as one towards the objects' bound)
    for name, shape in shapes:
        for p in (0, 1, 2, 4, 8):
            result["observed"].setdefault(name, {})["P = %d" % p] = child([me, "--pickups", str(p)] + shape + common + (["--objects", str(max(objects, 256))] if "--members" in shape else []))
            save()
    for _ in range(runs):
        for name, law, shape in (("render_coupled, 16 x 1-sided", "linear", ["--junctions", "16"]), ("render_coupled, 64 x 2-sided", "linear", ["--junctions", "64", "--sides", "2"]),
                                 ("render_damped, 16 x 1-sided", "damped", ["--junctions", "16"]), ("render_damped, 64 x 2-sided", "damped", ["--junctions", "64", "--sides", "2"])):
            row = result["unchanged"].setdefault(name, {"parent": [], "new": []})
            row["parent"].append(child([me, "--tree", parent, "--law", law] + shape + common))
            row["new"].append(child([me, "--law", law] + shape + common))
            save()
        for name, tree in (("parent", parent), ("new", HERE)) if all_live else ():
            r = child([os.path.join(tree, "tools", "bank_bench.py")], 600)
            result["all_live"][name].append({"ms_per_block": r["all_live"]["ms_per_block"], "kernel_us_per_block": r["all_live"]["kernel_us_per_block"]})
            save()
    med = lambda rows, key: float(np.median([r[key] for r in rows])) if rows else None
    pair = lambda old, new: {"parent_ms_per_block": [r["ms_per_block"] for r in old], "new_ms_per_block": [r["ms_per_block"] for r in new],
                             "parent_spread_ms": (max(r["ms_per_block"] for r in old) - min(r["ms_per_block"] for r in old)) if old else None,
                             "new_median_minus_parent_median_ms": (med(new, "ms_per_block") - med(old, "ms_per_block")) if old else None,
                             "parent_coupled_kernel_us_per_block": med(old, "coupled_kernel_us_per_block") if old and "coupled_kernel_us_per_block" in old[0] else None,
                             "new_coupled_kernel_us_per_block": med(new, "coupled_kernel_us_per_block") if new and "coupled_kernel_us_per_block" in new[0] else None}
    result["summary"] = {"real_time_ms_per_block": 1e3 * BLOCK / SR,
                         "observed": {name: {p: {"ms_per_block": r["ms_per_block"], "ms_per_block_median": r["ms_per_block_median"], "junction_kernels_us_per_block": r["junction_kernels_us_per_block"],
                                                 "main_kernel_us_per_block": r["kernel_us_per_block"]} for p, r in row.items()} for name, row in result["observed"].items()},
                         "unchanged": {name: pair(row["parent"], row["new"]) for name, row in result["unchanged"].items()},
                         "all_live": pair(result["all_live"]["parent"], result["all_live"]["new"]) if all_live else None}
    save()
    print(json.dumps(result["summary"]))


def compare_groups(parent, runs, objects, blocks, renderers, out_path, all_live):
    """The unchanged paths of the parent and of this tree -- the same kernels: the new figures have to land within the parent's own spread --
    and this tree's groups beside the same junctions ungrouped."""
    me = os.path.abspath(__file__)
    common = ["--objects", str(objects), "--blocks", str(blocks), "--renderers", str(renderers)]
    result = {"workload": f"{objects} objects x {MODES} modes @48k, {BLOCK}-frame blocks, fp32, {renderers} renderers, one drive on every object in every block; J ungrouped one-sided "
                          "junctions, or G groups of n exciter junctions on one object each (K C = 10)", "runs_each": runs, "all_live": {"parent": [], "new": []},
              "j0": {"parent_driven": [], "new_coupled": []}, "ungrouped": {}, "groups": {}}

    def save():
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)
    q = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", "import torch; p = torch.cuda.get_device_properties(0); print(p.name, p.gcnArchName, '%d CUs' % p.multi_processor_count, '|', torch.version.hip)"], capture_output=True, text=True)
    if q.returncode != 0:
        raise SystemExit("no GPU to measure on: " + q.stderr[-2000:])
    result["device"], result["hip"] = (v.strip() for v in q.stdout.strip().splitlines()[-1].split("|"))
    for _ in range(runs):
        for name, tree in (("parent", parent), ("new", HERE)) if all_live else ():
            r = child([os.path.join(tree, "tools", "bank_bench.py")], 600)
            result["all_live"][name].append({"ms_per_block": r["all_live"]["ms_per_block"], "kernel_us_per_block": r["all_live"]["kernel_us_per_block"]})
        result["j0"]["parent_driven"].append(child([me, "--entry", "replay", "--junctions", "0", "--tree", parent] + common))
        result["j0"]["new_coupled"].append(child([me, "--entry", "coupled", "--junctions", "0"] + common))
        for j in JUNCTIONS[1:]:
            row = result["ungrouped"].setdefault("J = %d" % j, {"parent": [], "new": []})
            row["parent"].append(child([me, "--tree", parent, "--junctions", str(j)] + common))
            row["new"].append(child([me, "--junctions", str(j)] + common))
            save()
        for n in (2, 3, 4):
            for g in (1, 16, 64):
                row = result["groups"].setdefault("G = %d, n = %d" % (g, n), {"grouped": [], "ungrouped": []})
                row["grouped"].append(child([me, "--members", str(n), "--junctions", str(g * n)] + common))
                row["ungrouped"].append(child([me, "--members", str(n), "--junctions", str(g * n), "--ungrouped"] + common))
                save()
    med = lambda rows, key: float(np.median([r[key] for r in rows])) if rows else None
    spread = lambda rows, key: (max(r[key] for r in rows) / min(r[key] for r in rows)) if rows else None
    pair = lambda old, new: {"parent_ms_per_block": [r["ms_per_block"] for r in old], "new_ms_per_block": [r["ms_per_block"] for r in new], "parent_spread_max_over_min": spread(old, "ms_per_block"),
                             "new_median_over_parent_median": (med(new, "ms_per_block") / med(old, "ms_per_block")) if old else None,
                             "parent_kernel_us_per_block": med(old, "kernel_us_per_block"), "new_kernel_us_per_block": med(new, "kernel_us_per_block"),
                             "parent_coupled_kernel_us_per_block": med(old, "coupled_kernel_us_per_block"), "new_coupled_kernel_us_per_block": med(new, "coupled_kernel_us_per_block")}
    result["summary"] = {"real_time_ms_per_block": 1e3 * BLOCK / SR, "all_live": pair(result["all_live"]["parent"], result["all_live"]["new"]) if all_live else None,
                         "j0": pair(result["j0"]["parent_driven"], result["j0"]["new_coupled"]), "ungrouped": {name: pair(row["parent"], row["new"]) for name, row in result["ungrouped"].items()},
                         "groups": {name: {"grouped_ms_per_block": med(row["grouped"], "ms_per_block"), "ungrouped_ms_per_block": med(row["ungrouped"], "ms_per_block"),
                                           "grouped_kernel_us_per_block": med(row["grouped"], "coupled_kernel_us_per_block"), "ungrouped_kernel_us_per_block": med(row["ungrouped"], "coupled_kernel_us_per_block"),
                                           "grouped_cycles_per_frame": med(row["grouped"], "coupled_cycles_per_frame"), "ungrouped_cycles_per_frame": med(row["ungrouped"], "coupled_cycles_per_frame")}
                                    for name, row in result["groups"].items()}}
    save()
    print(json.dumps(result["summary"]))


def compare_mixed(parent, runs, objects, blocks, renderers, out_path, all_live):
    """The unchanged calls of the parent and of this tree, interleaved in fresh processes -- J = 0, ungrouped J = 1, 16, 64, linear groups, and
    tools/bank_bench.py all-live: the new figures have to land within the parent's own spread -- and this tree's groups of n = 2, 3, 4 Hertz
    members through Scene.render_mixed beside the same groups with linear members through the same entry."""
    me = os.path.abspath(__file__)
    common = ["--objects", str(objects), "--blocks", str(blocks), "--renderers", str(renderers)]
    result = {"workload": f"{objects} objects x {MODES} modes @48k, {BLOCK}-frame blocks, fp32, {renderers} renderers, one drive on every object in every block; J ungrouped one-sided "
                          "junctions, or G groups of n exciter junctions on one object each (K C = 10; Hertz: K C sqrt(x0) = 10)", "runs_each": runs, "all_live": {"parent": [], "new": []},
              "j0": {"parent": [], "new": []}, "ungrouped": {}, "linear_groups": {}, "mixed": {}, "mixed_fp64": {}}

    def save():
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)
    q = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", "import torch; p = torch.cuda.get_device_properties(0); print(p.name, p.gcnArchName, '%d CUs' % p.multi_processor_count, '|', torch.version.hip)"], capture_output=True, text=True)
    if q.returncode != 0:
        raise SystemExit("no GPU to measure on: " + q.stderr[-2000:])
    result["device"], result["hip"] = (v.strip() for v in q.stdout.strip().splitlines()[-1].split("|"))
    sizes = [(g, n) for n in (2, 3, 4) for g in (1, 16, 64)]
    for _ in range(runs):
        for name, tree in (("parent", parent), ("new", HERE)) if all_live else ():
            r = child([os.path.join(tree, "tools", "bank_bench.py")], 600)
            result["all_live"][name].append({"ms_per_block": r["all_live"]["ms_per_block"], "kernel_us_per_block": r["all_live"]["kernel_us_per_block"]})
        for name, tree in (("parent", parent), ("new", HERE)):  # (the parent's copy of this tool measures the parent's library)
            tool = os.path.join(tree, "tools", "bank_junction_bench.py")
            result["j0"][name].append(child([tool, "--entry", "coupled", "--junctions", "0"] + common))
            for j in JUNCTIONS[1:]:
                result["ungrouped"].setdefault("J = %d" % j, {"parent": [], "new": []})[name].append(child([tool, "--junctions", str(j)] + common))
            for g, n in sizes:
                result["linear_groups"].setdefault("G = %d, n = %d" % (g, n), {"parent": [], "new": []})[name].append(child([tool, "--members", str(n), "--junctions", str(g * n)] + common))
            save()
        for g, n in sizes:
            row = result["mixed"].setdefault("G = %d, n = %d" % (g, n), {"hertz": [], "linear": []})
            row["hertz"].append(child([me, "--mixed", "--law", "hertz", "--members", str(n), "--junctions", str(g * n)] + common))
            row["linear"].append(child([me, "--mixed", "--members", str(n), "--junctions", str(g * n)] + common))
            save()
        for n in (2, 3, 4):  # the fp64 bank: G = 16 only
            row = result["mixed_fp64"].setdefault("G = 16, n = %d" % n, {"hertz": [], "linear": []})
            try:  # (a block beyond real time may run into the child's limit: the fp32 figures are kept)
                row["hertz"].append(child([me, "--mixed", "--double", "--law", "hertz", "--members", str(n), "--junctions", str(16 * n)] + common))
                row["linear"].append(child([me, "--mixed", "--double", "--members", str(n), "--junctions", str(16 * n)] + common))
            except SystemExit as e:
                result.setdefault("mixed_fp64_errors", []).append(str(e)[:400])
            save()
    med = lambda rows, key: float(np.median([r[key] for r in rows])) if rows else None
    spread = lambda rows, key: (max(r[key] for r in rows) / min(r[key] for r in rows)) if rows else None
    pair = lambda old, new: {"parent_ms_per_block": [r["ms_per_block"] for r in old], "new_ms_per_block": [r["ms_per_block"] for r in new], "parent_spread_max_over_min": spread(old, "ms_per_block"),
                             "new_median_over_parent_median": (med(new, "ms_per_block") / med(old, "ms_per_block")) if old else None}
    result["summary"] = {"real_time_ms_per_block": 1e3 * BLOCK / SR, "all_live": pair(result["all_live"]["parent"], result["all_live"]["new"]) if all_live else None,
                         "j0": pair(result["j0"]["parent"], result["j0"]["new"]), "ungrouped": {name: pair(row["parent"], row["new"]) for name, row in result["ungrouped"].items()},
                         "linear_groups": {name: pair(row["parent"], row["new"]) for name, row in result["linear_groups"].items()},
                         "mixed": {name: {"hertz_ms_per_block": med(row["hertz"], "ms_per_block"), "linear_ms_per_block": med(row["linear"], "ms_per_block"),
                                          "hertz_kernel_us_per_block": med(row["hertz"], "coupled_kernel_us_per_block"), "linear_kernel_us_per_block": med(row["linear"], "coupled_kernel_us_per_block"),
                                          "hertz_cycles_per_frame": med(row["hertz"], "coupled_cycles_per_frame"), "linear_cycles_per_frame": med(row["linear"], "coupled_cycles_per_frame"),
                                          "hertz_over_linear_kernel_time": med(row["hertz"], "coupled_kernel_us_per_block") / med(row["linear"], "coupled_kernel_us_per_block")}
                                   for name, row in result["mixed"].items()}}
    result["summary"]["mixed_fp64"] = {name: {"hertz_ms_per_block": med(row["hertz"], "ms_per_block"), "linear_ms_per_block": med(row["linear"], "ms_per_block"),
                                              "hertz_kernel_us_per_block": med(row["hertz"], "coupled_kernel_us_per_block"), "linear_kernel_us_per_block": med(row["linear"], "coupled_kernel_us_per_block"),
                                              "hertz_cycles_per_frame": med(row["hertz"], "coupled_cycles_per_frame"), "linear_cycles_per_frame": med(row["linear"], "coupled_cycles_per_frame")}
                                       for name, row in result["mixed_fp64"].items()}
    save()
    print(json.dumps(result["summary"]))


def compare_damped_groups(parent, runs, objects, blocks, renderers, out_path, all_live):
    """This tree's groups of n = 2, 3, 4 damped Hertz members through Scene.render_damped_groups beside the same groups with plain Hertz
    members through the same entry, fp32 (G = 1, 16, 64) and fp64 (G = 16); then the unchanged calls of the parent and of this tree,
    interleaved in fresh processes -- J = 0, ungrouped J = 1, 16, 64, linear and Hertz groups through render_mixed, and tools/bank_bench.py
    all-live: the new figures have to land within the parent's own spread.  The file is written after every row."""
    me = os.path.abspath(__file__)
    common = ["--objects", str(objects), "--blocks", str(blocks), "--renderers", str(renderers)]
    result = {"workload": f"{objects} objects x {MODES} modes @48k, {BLOCK}-frame blocks, {renderers} renderers, one drive on every object in every block; G groups of n exciter "
                          "junctions on one object each (Hertz: K C sqrt(x0) = 10; damped: l x0 = 1), or J ungrouped one-sided junctions (K C = 10)", "runs_each": runs,
              "damped_groups": {}, "damped_groups_fp64": {}, "all_live": {"parent": [], "new": []}, "j0": {"parent": [], "new": []}, "ungrouped": {}, "linear_groups": {}, "hertz_groups": {}}

    def save():
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)
    q = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", "import torch; p = torch.cuda.get_device_properties(0); print(p.name, p.gcnArchName, '%d CUs' % p.multi_processor_count, '|', torch.version.hip)"], capture_output=True, text=True)
    if q.returncode != 0:
        raise SystemExit("no GPU to measure on: " + q.stderr[-2000:])
    result["device"], result["hip"] = (v.strip() for v in q.stdout.strip().splitlines()[-1].split("|"))
    med = lambda rows, key: float(np.median([r[key] for r in rows])) if rows else None
    spread = lambda rows, key: (max(r[key] for r in rows) / min(r[key] for r in rows)) if rows else None
    pair = lambda old, new: {"parent_ms_per_block": [r["ms_per_block"] for r in old], "new_ms_per_block": [r["ms_per_block"] for r in new], "parent_spread_max_over_min": spread(old, "ms_per_block"),
                             "new_median_over_parent_median": (med(new, "ms_per_block") / med(old, "ms_per_block")) if old and new else None}
    both = lambda row: {"damped_ms_per_block": med(row["damped"], "ms_per_block"), "hertz_ms_per_block": med(row["hertz"], "ms_per_block"),
                        "damped_kernel_us_per_block": med(row["damped"], "coupled_kernel_us_per_block"), "hertz_kernel_us_per_block": med(row["hertz"], "coupled_kernel_us_per_block"),
                        "damped_cycles_per_frame": med(row["damped"], "coupled_cycles_per_frame"), "hertz_cycles_per_frame": med(row["hertz"], "coupled_cycles_per_frame")}

    def summarise():
        result["summary"] = {"real_time_ms_per_block": 1e3 * BLOCK / SR, "damped_groups": {name: both(row) for name, row in result["damped_groups"].items()},
                             "damped_groups_fp64": {name: both(row) for name, row in result["damped_groups_fp64"].items()},
                             "all_live": pair(result["all_live"]["parent"], result["all_live"]["new"]), "j0": pair(result["j0"]["parent"], result["j0"]["new"]),
                             "ungrouped": {name: pair(row["parent"], row["new"]) for name, row in result["ungrouped"].items()},
                             "linear_groups": {name: pair(row["parent"], row["new"]) for name, row in result["linear_groups"].items()},
                             "hertz_groups": {name: pair(row["parent"], row["new"]) for name, row in result["hertz_groups"].items()}}
        save()
    for _ in range(runs):
        for double, key, groups in ((False, "damped_groups", (1, 16, 64)), (True, "damped_groups_fp64", (16,))):
            for n in (2, 3, 4):
                for g in groups:
                    row = result[key].setdefault("G = %d, n = %d" % (g, n), {"damped": [], "hertz": []})
                    extra = ["--double"] if double else []
                    row["damped"].append(child([me, "--damped-groups", "--law", "hertz-damped", "--members", str(n), "--junctions", str(g * n)] + extra + common))
                    row["hertz"].append(child([me, "--damped-groups", "--law", "hertz", "--members", str(n), "--junctions", str(g * n)] + extra + common))
                    summarise()
    for _ in range(runs):
        for name, tree in (("parent", parent), ("new", HERE)):  # (the parent's copy of this tool measures the parent's library)
            tool = os.path.join(tree, "tools", "bank_junction_bench.py")
            result["j0"][name].append(child([tool, "--entry", "coupled", "--junctions", "0"] + common))
            for j in JUNCTIONS[1:]:
                result["ungrouped"].setdefault("J = %d" % j, {"parent": [], "new": []})[name].append(child([tool, "--junctions", str(j)] + common))
            for n in (2, 4):
                result["linear_groups"].setdefault("G = 16, n = %d" % n, {"parent": [], "new": []})[name].append(child([tool, "--mixed", "--members", str(n), "--junctions", str(16 * n)] + common))
                result["hertz_groups"].setdefault("G = 16, n = %d" % n, {"parent": [], "new": []})[name].append(child([tool, "--mixed", "--law", "hertz", "--members", str(n), "--junctions", str(16 * n)] + common))
            summarise()
        for name, tree in (("parent", parent), ("new", HERE)) if all_live else ():
            r = child([os.path.join(tree, "tools", "bank_bench.py")], 600)
            result["all_live"][name].append({"ms_per_block": r["all_live"]["ms_per_block"], "kernel_us_per_block": r["all_live"]["kernel_us_per_block"]})
            summarise()
    print(json.dumps(result["summary"]))


def compare_friction(parent, runs, objects, blocks, renderers, out_path, all_live):
    """This tree's J = 1, 16, 64 lone frictional junctions, linear and Hertz, one- and two-sided (J = 16), through Scene.render_friction beside the
    same junctions without the flag through the same entry, fp32 and fp64 (J = 16); then the unchanged calls of the parent and of this tree,
    interleaved in fresh processes -- J = 0, J = 1, 16, 64 linear and Hertz through render_coupled, and tools/bank_bench.py all-live: the new
    figures have to land within the parent's own spread.  The file is written after every row."""
    me = os.path.abspath(__file__)
    common = ["--objects", str(objects), "--blocks", str(blocks), "--renderers", str(renderers)]
    result = {"workload": f"{objects} objects x {MODES} modes @48k, {BLOCK}-frame blocks, {renderers} renderers, one drive on every object in every block; J lone junctions "
                          "(linear: K C = 10; Hertz: K C sqrt(x0) = 10), with friction: mu = 0.3, kt = K, a travel of twice the free deflection", "runs_each": runs,
              "friction": {}, "friction_fp64": {}, "all_live": {"parent": [], "new": []}, "j0": {"parent": [], "new": []}, "linear": {}, "hertz": {}}

    def save():
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)
    q = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", "import torch; p = torch.cuda.get_device_properties(0); print(p.name, p.gcnArchName, '%d CUs' % p.multi_processor_count, '|', torch.version.hip)"], capture_output=True, text=True)
    if q.returncode != 0:
        raise SystemExit("no GPU to measure on: " + q.stderr[-2000:])
    result["device"], result["hip"] = (v.strip() for v in q.stdout.strip().splitlines()[-1].split("|"))
    med = lambda rows, key: float(np.median([r[key] for r in rows])) if rows else None
    spread = lambda rows, key: (max(r[key] for r in rows) / min(r[key] for r in rows)) if rows else None
    pair = lambda old, new: {"parent_ms_per_block": [r["ms_per_block"] for r in old], "new_ms_per_block": [r["ms_per_block"] for r in new], "parent_spread_max_over_min": spread(old, "ms_per_block"),
                             "new_median_over_parent_median": (med(new, "ms_per_block") / med(old, "ms_per_block")) if old and new else None}
    both = lambda row: {"friction_ms_per_block": med(row["friction"], "ms_per_block"), "plain_ms_per_block": med(row["plain"], "ms_per_block"),
                        "friction_kernel_us_per_block": med(row["friction"], "coupled_kernel_us_per_block"), "plain_kernel_us_per_block": med(row["plain"], "coupled_kernel_us_per_block"),
                        "friction_cycles_per_frame": med(row["friction"], "coupled_cycles_per_frame"), "plain_cycles_per_frame": med(row["plain"], "coupled_cycles_per_frame"),
                        "frames_stick_slip_none": row["friction"][-1].get("friction_frames_stick_slip_none") if row["friction"] else None}

    def summarise():
        result["summary"] = {"real_time_ms_per_block": 1e3 * BLOCK / SR, "friction": {name: both(row) for name, row in result["friction"].items()},
                             "friction_fp64": {name: both(row) for name, row in result["friction_fp64"].items()},
                             "all_live": pair(result["all_live"]["parent"], result["all_live"]["new"]), "j0": pair(result["j0"]["parent"], result["j0"]["new"]),
                             "linear": {name: pair(row["parent"], row["new"]) for name, row in result["linear"].items()},
                             "hertz": {name: pair(row["parent"], row["new"]) for name, row in result["hertz"].items()}}
        save()
    for _ in range(runs):
        for double, key, counts in ((False, "friction", JUNCTIONS[1:]), (True, "friction_fp64", (16,))):
            for law in ("linear", "hertz"):
                for j, sides in [(j, 1) for j in counts] + [(16, 2)]:
                    row = result[key].setdefault("%s, J = %d x %d-sided" % (law, j, sides), {"friction": [], "plain": []})
                    extra = (["--double"] if double else []) + ["--law", law, "--junctions", str(j), "--sides", str(sides)]
                    row["friction"].append(child([me, "--friction"] + extra + common))
                    row["plain"].append(child([me, "--damped-groups"] + extra + common))
                    summarise()
    for _ in range(runs if parent else 0):
        for name, tree in (("parent", parent), ("new", HERE)):  # (the parent's copy of this tool measures the parent's library)
            tool = os.path.join(tree, "tools", "bank_junction_bench.py")
            result["j0"][name].append(child([tool, "--entry", "coupled", "--junctions", "0"] + common))
            for j in JUNCTIONS[1:]:
                result["linear"].setdefault("J = %d" % j, {"parent": [], "new": []})[name].append(child([tool, "--junctions", str(j)] + common))
                result["hertz"].setdefault("J = %d" % j, {"parent": [], "new": []})[name].append(child([tool, "--law", "hertz", "--junctions", str(j)] + common))
            summarise()
        for name, tree in (("parent", parent), ("new", HERE)) if all_live else ():
            r = child([os.path.join(tree, "tools", "bank_bench.py")], 600)
            result["all_live"][name].append({"ms_per_block": r["all_live"]["ms_per_block"], "kernel_us_per_block": r["all_live"]["kernel_us_per_block"]})
            summarise()
    print(json.dumps(result["summary"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entry", choices=["coupled", "replay"], default="coupled")
    ap.add_argument("--junctions", type=int, default=16)
    ap.add_argument("--sides", type=int, choices=[1, 2], default=1)
    ap.add_argument("--objects", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=1000)
    ap.add_argument("--renderers", type=int, default=4)
    ap.add_argument("--tree", default=HERE, help="built checkout whose library is measured (replay only on one without junctions)")
    ap.add_argument("--forces", help="replay: the force rows a --save-forces run wrote")
    ap.add_argument("--save-forces", help="coupled: write the last block's force rows here (.npy)")
    ap.add_argument("--law", choices=["linear", "hertz", "damped", "hertz-damped"], default="linear", help="coupled: the junctions' law")
    ap.add_argument("--damped-against", help="built checkout of the parent commit: its undamped linear and Hertz calls, this tree's, and this tree's damped calls -> profiles/bank_damped.json")
    ap.add_argument("--laws-against", help="built checkout of the parent commit: its all-linear calls, this tree's, and this tree's Hertz calls -> profiles/bank_hertz.json")
    ap.add_argument("--against", help="built checkout of the parent commit: run the whole comparison")
    ap.add_argument("--members", type=int, default=0, help="coupled: the junctions are groups of this many exciter junctions on one object each (2 ... 4)")
    ap.add_argument("--ungrouped", action="store_true", help="with --members: the same junctions on objects of their own, without the shared flag")
    ap.add_argument("--groups", action="store_true", help="with --against: the unchanged paths of both trees and this tree's groups -> profiles/bank_groups.json")
    ap.add_argument("--pickups", type=int, default=None, help="coupled: through Scene.render_observed with this many pickups on every junction object (0 ... 8)")
    ap.add_argument("--observed-against", help="built checkout of the parent commit: this tree's render_observed with P pickups per junction object, and the unchanged paths of both trees -> profiles/bank_observed.json")
    ap.add_argument("--mixed", action="store_true", help="with --members: through Scene.render_mixed (--law hertz: Hertz members); with --against: the unchanged calls of both trees and this tree's groups with Hertz members -> profiles/bank_mixed.json")
    ap.add_argument("--double", action="store_true", help="the fp64 bank (with --mixed or --damped-groups)")
    ap.add_argument("--damped-groups", action="store_true", help="with --members: through Scene.render_damped_groups (--law hertz-damped: damped Hertz members; --law hertz: plain ones); with --against: this tree's groups with damped members and the unchanged calls of both trees -> profiles/bank_damped_groups.json")
    ap.add_argument("--friction", action="store_true", help="lone junctions with Coulomb friction through Scene.render_friction (--law linear or hertz); with --against: this tree's frictional junctions beside the same junctions without the flag, and the unchanged calls of both trees -> profiles/bank_friction.json")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-all-live", action="store_true", help="skip tools/bank_bench.py of both trees")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "bank_junctions.json"))
    a = ap.parse_args()
    if a.observed_against:
        out = a.out if a.out != ap.get_default("out") else os.path.join(HERE, "profiles", "bank_observed.json")
        compare_observed(os.path.abspath(a.observed_against), a.runs, a.objects, a.blocks, a.renderers, out, not a.no_all_live)
    elif a.damped_against:
        out = a.out if a.out != ap.get_default("out") else os.path.join(HERE, "profiles", "bank_damped.json")
        compare_damped(os.path.abspath(a.damped_against), a.runs, a.objects, a.blocks, a.renderers, out)
    elif a.laws_against:
        out = a.out if a.out != ap.get_default("out") else os.path.join(HERE, "profiles", "bank_hertz.json")
        compare_laws(os.path.abspath(a.laws_against), a.runs, a.objects, a.blocks, a.renderers, out)
    elif a.against and a.friction:
        out = a.out if a.out != ap.get_default("out") else os.path.join(HERE, "profiles", "bank_friction.json")
        compare_friction(os.path.abspath(a.against), a.runs, a.objects if a.objects != ap.get_default("objects") else 256, a.blocks, a.renderers, out, not a.no_all_live)
    elif a.against and a.damped_groups:
        out = a.out if a.out != ap.get_default("out") else os.path.join(HERE, "profiles", "bank_damped_groups.json")
        compare_damped_groups(os.path.abspath(a.against), a.runs, a.objects if a.objects != ap.get_default("objects") else 256, a.blocks, a.renderers, out, not a.no_all_live)
    elif a.against and a.mixed:
        out = a.out if a.out != ap.get_default("out") else os.path.join(HERE, "profiles", "bank_mixed.json")
        compare_mixed(os.path.abspath(a.against), a.runs, a.objects if a.objects != ap.get_default("objects") else 256, a.blocks, a.renderers, out, not a.no_all_live)
    elif a.against and a.groups:
        out = a.out if a.out != ap.get_default("out") else os.path.join(HERE, "profiles", "bank_groups.json")
        compare_groups(os.path.abspath(a.against), a.runs, a.objects if a.objects != ap.get_default("objects") else 256, a.blocks, a.renderers, out, not a.no_all_live)
    elif a.against:
        compare(os.path.abspath(a.against), a.runs, a.objects, a.blocks, a.renderers, a.out, not a.no_all_live)
    else:
        print(json.dumps(measure(os.path.abspath(a.tree), a.entry, a.junctions, a.sides, a.objects, a.blocks, a.renderers, a.forces, a.save_forces, a.law, a.members, a.ungrouped, a.pickups, a.mixed, a.double, a.damped_groups, a.friction)))


if __name__ == "__main__":
    main()
