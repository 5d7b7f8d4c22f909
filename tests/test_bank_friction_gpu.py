"""GPU tests of the Coulomb friction of the contact junctions (Junction.of(..., friction=True) + Friction -> Scene.render_friction ->
RenderModalFriction -> mh_bank_render_friction -> k_bank_modes_coupled_friction; contract: include/modalhip.h, "Friction").

Scene: objects of 32, 130 and 256 modes (one, two and two waves), rung up by noise drives for two blocks; a two-sided frictional junction
between the first two (side a at a blend of three points, tb = -ta) and a one-sided one on the third; 3 blocks of 512 or of 333 frames
with the anchor passed on; fp32 and fp64, 1 and 4 renderers, linear and Hertz.  u is a slow sine of the size of the free deflection, w a
slower sine plus a ramp, sized on the host (_plan) so that each of O, S, P, M holds at least 5 % of the frames at either junction.

6.  No flagged junction: render_friction is render_damped_groups in everything returned.
7.  Dead friction (kt = 0; mu = 0; zero tangents) is the same call with the flag cleared, bit for bit.
8.  Replay: f_n and f_t as two drives per side on a twin scene give the same block, states and object_state().
9.  The law where it is solved, with advance-1 pickups along n and along t at the sides.
10. Rows, samples, anchors and the four compliances against the longdouble restatement.
11. Bit-exactness: one block against two halves, the anchor dropped, bystanders and renderer counts, other junctions beside a frictional one.
12. The third count.
Left-out kinds through the entries: the last test."""
import numpy as np
import pytest

from tests import drive_harness as dh
from tests import friction_harness as fh
from tests import pickup_harness as ph
from tests import test_bank_junctions_gpu as junctions_suite

pytestmark = pytest.mark.gpu

PRECISIONS = pytest.mark.parametrize("use_double", [False, True], ids=["fp32", "fp64"])
RENDERERS = pytest.mark.parametrize("renderers", [1, 4])
LAWS = pytest.mark.parametrize("hertz", [False, True], ids=["linear", "hertz"])
FRAMES = pytest.mark.parametrize("frames", [512, 333])
BOUND = junctions_suite.BOUND  # x the working-precision restatement's own deviation
MODES, T60, BLOCKS, RING_UP = [32, 130, 256], junctions_suite.REST_T60, 3, 2
_signal, _drive_args, _states, _same = junctions_suite._signal, junctions_suite._drive_args, junctions_suite._states, junctions_suite._same
L = np.longdouble
SIDES = [(fh.side(0, (3, 0, 1), (0.5, 0.25, 0.25), (1.0, 0.5, -0.25), 1.5), fh.side(1, 2, direction=(-1.0, -0.5, 0.25), coupling=1.5)), (fh.side(2, 1, direction=(0.25, -1.0, 0.5), coupling=2.0), None)]
SINGLE = [(fh.side(0, 3, direction=(1.0, 0.5, -0.25), coupling=1.5), fh.side(1, 2, direction=(-1.0, -0.5, 0.25), coupling=1.5)), SIDES[1]]  # single-point sides: what a drive can replay
TANGENTS = [((0.5, -1.0, 0.0), (-0.5, 1.0, 0.0)), ((1.0, 0.25, 0.0), (0.0, 0.0, 0.0))]  # (n . t = 0 on every side)


def _specs(numbers, hertz, sides=SIDES, friction=(True, True), tangents=TANGENTS):
    """The two junctions with (K, mu, kt) per junction."""
    return [fh.spec(a, b, k, hertz, ta, tb, mu, kt, on) for (a, b), (ta, tb), (k, mu, kt), on in zip(sides, tangents, numbers, friction)]


def _ring_rows(frames, b, objects):
    return [(o,) + dh.row_direction(o) + (_signal("noise", o, RING_UP * frames)[b * frames:(b + 1) * frames],) for o in range(objects)]


def _ring_up(sc, rest, frames, objects=len(MODES)):
    """Noise drives on every object for two blocks (render_driven; the same on the restatements, which hold the first three objects): what
    the junctions then act on."""
    for b in range(RING_UP):
        if sc is not None:
            sc.render_driven(np.zeros(frames, sc.dtype), *_drive_args(_ring_rows(frames, b, objects), frames))
        for r in rest:
            r.render_friction(_ring_rows(frames, b, len(MODES)), [], np.zeros((0, frames), np.float32), np.zeros((0, frames), np.float32), frames)


_PLANS = {}
U_RAISE, W_SWING, W_PERIOD, W_DRIFT = 0.5, 2.0, 230.0, 700.0  # of _plan's signals


def _sweep_rows(rows_on, frames, blk):
    """The drives beside the junctions: a swept sine on every object of rows_on."""
    return [(o,) + dh.row_direction(o + 5) + (_signal("sweep", o, BLOCKS * frames)[blk * frames:(blk + 1) * frames],) for o in rows_on]


def _plan(scene, use_double, hertz, frames, sides=SIDES, rows_on=()):
    """The run's numbers, sized on the host from the bank's columns by a float64 restatement (once per setting; the scene is only read):
    the free deflections r_n and r_t are the rms, along n and along t at each junction, of the run without contact (with its drives);
    per junction K with K C_nn = 3 (Hertz: K C_nn sqrt(x0) = 3 at the approach's peak x0), kt with kt C_tt = 3, mu = 0.5 or, where the cone
    condition asks for less, 0.8 C_nn / |C_nt|; u = 3 r_n (sin(2 pi s / (400 + 90 j)) + 0.5) with r_n the free deflection's rms along n; and
    w = 2 m (sin(2 pi s / (230 + 60 j)) + s / 700) with m = max(r_t, s0), r_t the free deflection's rms along t and s0 = mu f0 / kt the stick
    spring's stretch at the cone's edge under f0 = N(x0, C_nn): the travel swings through several stretches and drifts.  Returns (numbers, u, w)."""
    rows_on = tuple(o for o in rows_on if o < len(MODES))
    key = (use_double, hertz, frames, id(sides), rows_on)
    if key not in _PLANS:
        bank_dtype = np.float64 if use_double else np.float32
        scout = fh.Restatement(scene, MODES, np.float64, bank_dtype)
        scout.z = [(np.zeros(n), np.zeros(n)) for n in MODES]
        _ring_up(None, [scout], frames)
        free = _specs([(0.0, 0.0, 0.0)] * 2, hertz, sides)
        n = BLOCKS * frames
        along_n, along_t = [], []
        for blk in range(BLOCKS):
            trace = {}
            scout.render_friction(_sweep_rows(rows_on, frames, blk), free, np.zeros((2, frames), np.float32), np.zeros((2, frames), np.float32), frames, None, trace)
            along_n.append(trace["read1_n"]), along_t.append(trace["read1_t"])
        r_n, r_t = np.sqrt((np.concatenate(along_n, axis=1) ** 2).mean(axis=1)), np.sqrt((np.concatenate(along_t, axis=1) ** 2).mean(axis=1))
        t = np.arange(n)
        numbers, u, w = [], [], []
        for j, s in enumerate(free):
            c_nn, c_nt, c_tn, c_tt = (float(v) for v in scout.four_compliances(s))
            x0 = 3.0 * r_n[j] * 1.1
            k = 3.0 / (c_nn * (np.sqrt(x0) if hertz else 1.0))
            kt = 3.0 / c_tt
            mu = min(0.5, 0.8 * c_nn / abs(c_nt))
            f0 = float(fh.normal_force(x0, c_nn, k, np.float64, hertz))
            m = max(r_t[j], mu * f0 / kt)
            numbers.append((k, mu, kt))
            u.append((3.0 * r_n[j] * (np.sin(2 * np.pi * t / (400.0 + 90 * j)) + U_RAISE)).astype(np.float32))
            w.append((W_SWING * m * (np.sin(2 * np.pi * t / (W_PERIOD + 60 * j)) + t / W_DRIFT)).astype(np.float32))
        _PLANS[key] = (numbers, np.array(u), np.array(w))
    return _PLANS[key]


BYSTANDERS = [64, 64, 64, 40]  # objects 3 .. 6 of the locality test: a linear, a Hertz and a damped junction on the first three, a drive and a pickup on the last


def _bystander_junctions():
    from mesheditor_amd import bank as hipbank
    sd = lambda o: fh.side(o, 1, direction=(0.25, -1.0, 0.5), coupling=2.0)
    return [hipbank.Junction.of(sd(3), None, 1.0), hipbank.Junction.of(sd(4), None, 1e3, hertz=True), hipbank.Junction.of(sd(5), None, 1.0, damped=True)]


def _render(sc, out, rows, specs, u, w, anchor=None, pickups=(), bystanders=False):
    """One block through Scene.render_friction: (f_n, f_t, C, status, anchor, counts, reads) of the specs' junctions.  bystanders: three
    junctions of the other kinds follow them in the call (a constant approach of 2e-6, the size of the surfaces' motion), with a damping of 1e-3 s/m."""
    from mesheditor_amd import bank as hipbank
    junctions, slides = fh.records(specs)
    n, damping = len(specs), None
    if bystanders:
        extra = _bystander_junctions()
        junctions = (hipbank.Junction * (n + 3))(*(list(junctions)[:n] + extra))
        slides = (hipbank.Friction * (n + 3))(*(list(slides)[:n] + [hipbank.Friction.of()] * 3))
        zeros = np.zeros((3, len(out)), np.float32)
        u, w, damping = np.concatenate([u, zeros + np.float32(2e-6)]), np.concatenate([w, zeros]), np.full(n + 3, 1e-3, np.float32)
        anchor = None if anchor is None else list(anchor) + [np.nan] * 3
    got = sc.render_friction(out, *_drive_args(rows, len(out)), ph.records(list(pickups)), junctions, u, slides, w, damping, None, anchor)
    reads, flags, f_n, comp, status, carry, unconverged, f_t, anchor, counts = got
    assert (flags == 1).all() and np.isnan(carry[:n]).all() and (unconverged == 0).all()
    if bystanders:
        assert (status[n:] == 1).all() and np.abs(f_n[n:]).max(axis=1).min() > 0 and (f_t[n:] == 0).all() and np.isnan(anchor[n:]).all() and (counts[n:] == 0).all()
    return f_n[:n], f_t[:n], comp[:n], status[:n], anchor[:n], counts[:n], reads


def _run(use_double, renderers, hertz, frames, numbers=None, friction=(True, True), tangents=TANGENTS, travel=None, sides=SIDES, blocks=BLOCKS, split=False, keep_anchor=True, rows_on=(),
         pickups=(), restate=(), bystanders=False):
    """The scene's run on the device: ring-up, then `blocks` blocks with the anchor passed on (split: every block as two halves).  numbers:
    (K, mu, kt) per junction (None: the plan's).  rows_on: objects that carry a sweep drive beside the junctions.  restate: formats of
    restatements run alongside.  bystanders: four more objects (BYSTANDERS) with junctions of the other kinds, a drive and a pickup.
    Returns a dict of per-block lists; "states": the state columns of the first three objects."""
    sc, _ = dh.device_scene(MODES + (BYSTANDERS if bystanders else []), T60, renderers, use_double)
    plan_numbers, u, w = _plan(sc, use_double, hertz, frames, sides, rows_on)
    specs = _specs(numbers or plan_numbers, hertz, sides, friction, tangents)
    if travel is not None:
        w = travel
    rest = [fh.Restatement(sc, MODES, T, sc.dtype) for T in restate]
    _ring_up(sc, rest, frames, len(MODES) + (len(BYSTANDERS) if bystanders else 0))
    if bystanders:
        rows_on = tuple(rows_on) + (6,)
        pickups = list(pickups) + [ph.spec(6, 2, direction=(1.0, 0.0, 0.5))]
    res = {"f_n": [], "f_t": [], "C": [], "status": [], "anchor": [], "counts": [], "reads": [], "out": [], "object_state": [], "rest": [[] for _ in rest], "specs": specs, "u": u, "w": w}
    anchor, rest_anchor = None, [None for _ in rest]
    for blk in range(blocks):
        rows = _sweep_rows(rows_on, frames, blk)
        pieces = [(0, frames // 2), (frames // 2, frames)] if split else [(0, frames)]
        parts = []
        for lo, hi in pieces:
            sl = slice(blk * frames + lo, blk * frames + hi)
            out = np.zeros(hi - lo, sc.dtype)
            part_rows = [(o, p, d, f[lo:hi]) for (o, p, d, f) in rows]
            f_n, f_t, comp, status, anchor_out, counts, reads = _render(sc, out, part_rows, specs, u[:, sl], w[:, sl], anchor if keep_anchor else None, pickups, bystanders)
            anchor = anchor_out
            parts.append((f_n, f_t, comp, status, anchor_out, counts, reads, out))
        res["f_n"].append(np.concatenate([p[0] for p in parts], axis=1)), res["f_t"].append(np.concatenate([p[1] for p in parts], axis=1))
        res["C"].append(parts[-1][2]), res["status"].append(parts[-1][3]), res["anchor"].append(parts[-1][4]), res["counts"].append(sum(p[5].astype(np.int64) for p in parts))
        res["reads"].append(np.concatenate([p[6] for p in parts], axis=1)), res["out"].append(np.concatenate([p[7] for p in parts]))
        res["object_state"].append([a.copy() for a in sc.object_state()])
        sl = slice(blk * frames, (blk + 1) * frames)
        for i, r in enumerate(rest):
            trace = {}
            got = r.render_friction(rows, specs, u[:, sl], w[:, sl], frames, rest_anchor[i] if keep_anchor else None, trace)
            rest_anchor[i] = got[5]
            res["rest"][i].append(got + (trace,))
    res["states"] = [col[:sum(MODES)] for col in _states(sc)]
    res["object_state"] = [[a[:len(MODES)] for a in blk] for blk in res["object_state"]]
    sc.close()
    return res


def _all_equal(a, b, keys=("f_n", "f_t", "C", "status", "anchor", "counts", "out")):
    for key in keys:
        for blk, (x, y) in enumerate(zip(a[key], b[key])):
            assert np.array_equal(x, y, equal_nan=True), (key, blk)
    assert _same(a["states"], b["states"])
    for x, y in zip(a["object_state"], b["object_state"]):
        assert _same(x, y)


# ---- 6. no flagged junction ----
@PRECISIONS
@RENDERERS
@LAWS
def test_without_a_flagged_junction_it_is_render_damped_groups(use_double, renderers, hertz):
    """The run with both flags cleared against the same blocks through Scene.render_damped_groups: everything both return is array_equal,
    the tangent rows and the counts are zero and the anchors NaN."""
    frames = 333
    got = _run(use_double, renderers, hertz, frames, friction=(False, False), rows_on=(0,))
    assert all((s == 1).all() for s in got["status"]) and all((f == 0).all() for f in got["f_t"]) and all(np.isnan(a).all() for a in got["anchor"]) and all((c == 0).all() for c in got["counts"])
    assert all(np.abs(f).max(axis=1).min() > 0 for f in got["f_n"])
    sc, _ = dh.device_scene(MODES, T60, renderers, use_double)
    _ring_up(sc, [], frames)
    junctions, _ = fh.records(got["specs"])
    for blk in range(BLOCKS):
        sl = slice(blk * frames, (blk + 1) * frames)
        rows = _sweep_rows((0,), frames, blk)
        out = np.zeros(frames, sc.dtype)
        reads, flags, forces, comp, status, carry, unconverged = sc.render_damped_groups(out, *_drive_args(rows, frames), [], junctions, got["u"][:, sl])
        assert np.array_equal(forces, got["f_n"][blk]) and np.array_equal(comp, got["C"][blk]) and np.array_equal(status, got["status"][blk]) and np.array_equal(out, got["out"][blk])
        assert np.isnan(carry).all() and (unconverged == 0).all()
        assert _same(sc.object_state(), got["object_state"][blk])
    assert _same(_states(sc), got["states"])
    sc.close()


# ---- 7. dead friction ----
@PRECISIONS
@RENDERERS
@LAWS
@FRAMES
def test_dead_friction_is_the_call_with_the_flag_cleared(use_double, renderers, hertz, frames):
    """kt = 0, mu = 0 and zero tangents: `out`, the states, object_state(), f_n and C are array_equal to the same call with the flag cleared;
    f_t is 0 for kt = 0 and for mu = 0, and with zero tangents under a travel of 0 (under the scene's travel it is the rigid slider's
    force, inside the cone, and moves nothing: a_t = 0)."""
    sc, _ = dh.device_scene(MODES, T60, 1, use_double)
    numbers, _, w = _plan(sc, use_double, hertz, frames, rows_on=(0,))
    sc.close()
    plain = _run(use_double, renderers, hertz, frames, friction=(False, False), rows_on=(0,))
    none = [((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))] * 2
    variants = {"kt = 0": dict(numbers=[(k, mu, 0.0) for k, mu, kt in numbers]), "mu = 0": dict(numbers=[(k, 0.0, kt) for k, mu, kt in numbers]), "zero tangents": dict(tangents=none),
                "zero tangents, no travel": dict(tangents=none, travel=np.zeros_like(w))}
    for name, how in variants.items():
        got = _run(use_double, renderers, hertz, frames, rows_on=(0,), **how)
        assert all((s == 1).all() for s in got["status"]), name
        _all_equal(got, plain, keys=("f_n", "C", "status", "out"))
        assert all(np.isfinite(a).all() for a in got["anchor"]), name
        if name != "zero tangents":
            assert all((f == 0).all() for f in got["f_t"]), name
        else:
            mu = np.array([n[1] for n in numbers], np.float32).astype(got["f_n"][0].dtype)[:, None]
            outside = sum(int((np.abs(t) > mu * f).sum()) for t, f in zip(got["f_t"], got["f_n"]))
            assert outside <= sum(int(c[:, 2].sum()) for c in got["counts"]) and any((f != 0).any() for f in got["f_t"]), name


# ---- 8, 9. replay, and the law where it is solved ----
def _branches(f_n, f_t, mu):
    """The branch of every frame from the rows the entry returns: open where f_n = 0, slipping where f_t = +- mu f_n to the bit (what a
    slipping frame stores), sticking otherwise."""
    cone = mu * f_n
    return np.where(f_n == 0, fh.O, np.where(f_t == cone, fh.P, np.where(f_t == -cone, fh.M, fh.S)))


@RENDERERS
@LAWS
@FRAMES
def test_the_rows_replayed_as_drives_give_the_run_and_meet_the_law(renderers, hertz, frames):
    """fp32 (a replayed row has to fit a drive's float signal), single-point sides, objects with no other row.  Scene A carries the two
    frictional junctions and advance-1 pickups along n and along t at every side, which this entry reads; scene B the returned rows as
    two drives per side, along n with f_n and along t with f_t: out, every state and object_state() are array_equal block after block.
    With y = u - sum read1_n and e = w - sum read1_t from scene A's pickups, in longdouble: f_n against K phi(y); on sticking frames f_t
    against kt (e - q) with q followed on the host through the branches (a slipping frame leaves q = e - f_t / kt, an open one q = e); on
    slipping frames |f_t| against mu f_n.  Largest deviation over the row's peak, device against the float32 restatement of the same run
    (its own read1 rows): bound 4 x."""
    T = np.float32
    pickups = []
    for (a, b), (ta, tb) in zip(SINGLE, TANGENTS):
        for sd, t in ((a, ta), (b, tb)):
            if sd is not None:
                pickups += [sd + (1,), fh.tangent_side(sd, t) + (1,)]
    got = _run(False, renderers, hertz, frames, sides=SINGLE, pickups=pickups, restate=(T,))
    specs = got["specs"]
    twin, _ = dh.device_scene(MODES, T60, renderers, False)
    _ring_up(twin, [], frames)
    device, yardstick = {"normal": 0.0, "stick": 0.0, "slip": 0.0}, {"normal": 0.0, "stick": 0.0, "slip": 0.0}
    q_dev, q_rest = [None, None], [None, None]
    for blk in range(BLOCKS):
        replay = []
        for j, s in enumerate(specs):
            replay += [(o, p, d, (got["f_n"], got["f_t"])[which][blk][j]) for (o, p, d, which) in fh.replay_drives(s)]
        out = np.zeros(frames, T)
        twin.render_driven(out, *_drive_args(replay, frames))
        assert np.array_equal(out, got["out"][blk]), blk
        assert _same(twin.object_state(), got["object_state"][blk]), blk
        sl = slice(blk * frames, (blk + 1) * frames)
        reads = got["reads"][blk].astype(L)
        rest = got["rest"][0][blk]
        sums = {"device": ([reads[0] + reads[2], reads[4]], [reads[1] + reads[3], reads[5]]), "rest": (list(rest[7]["read1_n"].astype(L)), list(rest[7]["read1_t"].astype(L)))}
        for j, s in enumerate(specs):
            k, mu, kt = L(np.float32(s[2])), L(np.float32(s[5][2])), L(np.float32(s[5][3]))
            for name, f_n, f_t, fig, q_of in (("device", got["f_n"][blk][j], got["f_t"][blk][j], device, q_dev), ("rest", rest[1][j], rest[2][j], yardstick, q_rest)):
                y, e = got["u"][j, sl].astype(L) - sums[name][0][j], got["w"][j, sl].astype(L) - sums[name][1][j]
                law_n = k * np.maximum(y, 0) ** (L(1.5) if hertz else L(1))
                br = _branches(f_n, f_t, T(np.float32(s[5][2])))
                peak_n, peak_t = L(np.abs(f_n).max()), L(np.abs(f_t).max())
                assert peak_n > 0 and peak_t > 0
                fig["normal"] = max(fig["normal"], float(np.abs(f_n.astype(L) - law_n).max() / peak_n))
                q = q_of[j]
                for t in range(frames):
                    if q is None:
                        q = e[t] - (L(f_t[t]) / kt if br[t] == fh.S else 0)  # no history: the first frame's anchor is x_t, which no pickup reads; a sticking first frame gives it by its force
                    if br[t] == fh.S:
                        fig["stick"] = max(fig["stick"], float(abs(L(f_t[t]) - kt * (e[t] - q)) / peak_t))
                    elif br[t] == fh.O:
                        q = e[t]
                    else:
                        fig["slip"] = max(fig["slip"], float(abs(abs(L(f_t[t])) - mu * L(f_n[t])) / peak_t))
                        q = e[t] - L(f_t[t]) / kt
                q_of[j] = q
    assert _same(_states(twin), got["states"])
    twin.close()
    print("the law on the device, %s, %d renderers, %d frames: " % ("hertz" if hertz else "linear", renderers, frames) +
          ", ".join("%s device %.3e / float32 restatement %.3e" % (k, device[k], yardstick[k]) for k in device))
    for key in device:
        assert device[key] <= BOUND * yardstick[key] or (key == "slip" and device[key] <= 2 * float(np.finfo(T).eps)), (key, device[key], yardstick[key])


# ---- 10, 12. against longdouble; the branches and the third count ----
@PRECISIONS
@RENDERERS
@LAWS
@FRAMES
def test_rows_samples_anchors_and_compliances_match_a_longdouble_restatement(use_double, renderers, hertz, frames):
    """Rows f_n and f_t, the block's samples, the anchors (times kt, over the f_t row's peak) and the four compliances (C_nn from the
    entry; all four from the restatements, the device's C_nn standing for the kernel's order) against the longdouble restatement: device
    deviation against the working-precision restatement's own, bound 4 x.  In the longdouble run each of O, S, P, M holds at least 5 % of
    the frames at either junction, and the device's counts say the same (O, S and P + M; the sign of f_t on slipping frames splits P from
    M).  The third count: 0 in fp64; in fp32 at most the count of the float32 restatement plus the device's own frames whose branch differs
    from the longdouble run's.

    Measured on an MI355X: see DESIGN.md section 3j (this test prints them)."""
    T = np.float64 if use_double else np.float32
    got = _run(use_double, renderers, hertz, frames, rows_on=(0, 1, 2), restate=(L, T))
    exact, working = got["rest"]
    eps = float(np.finfo(T).eps)
    fig = {k: [0.0, 0.0] for k in ("f_n", "f_t", "out", "anchor", "C")}
    total = BLOCKS * frames
    for blk in range(BLOCKS):
        assert list(got["status"][blk]) == [1, 1]
        for key, i in (("f_n", 1), ("f_t", 2)):
            fig[key][0], fig[key][1] = max(fig[key][0], fh.jh.row_figure(got[key][blk], exact[blk][i])), max(fig[key][1], fh.jh.row_figure(working[blk][i], exact[blk][i]))
        fig["out"][0], fig["out"][1] = max(fig["out"][0], fh.jh.row_figure(got["out"][blk][None, :], exact[blk][0][None, :])), max(fig["out"][1], fh.jh.row_figure(working[blk][0][None, :], exact[blk][0][None, :]))
        kt = np.array([L(np.float32(s[5][3])) for s in got["specs"]])
        peak = np.abs(exact[blk][2]).max(axis=1)
        fig["anchor"][0] = max(fig["anchor"][0], float((np.abs(got["anchor"][blk].astype(L) - exact[blk][5]) * kt / peak).max()))
        fig["anchor"][1] = max(fig["anchor"][1], float((np.abs(working[blk][5].astype(L) - exact[blk][5]) * kt / peak).max()))
        c_exact = np.array([[L(v) for v in four] for four in exact[blk][7]["compliances"]])
        c_work = np.array([[L(v) for v in four] for four in working[blk][7]["compliances"]])
        fig["C"][0] = max(fig["C"][0], float(np.abs((got["C"][blk].astype(L) - c_exact[:, 0]) / c_exact[:, 0]).max()))
        fig["C"][1] = max(fig["C"][1], float(np.abs((c_work - c_exact) / c_exact).max()))
    print("%s, %s, %d renderers, %d frames: " % ("fp64" if use_double else "fp32", "hertz" if hertz else "linear", renderers, frames) +
          ", ".join("%s device %.3e / restatement %.3e (%.2f x)" % (k, v[0], v[1], v[0] / v[1] if v[1] else float("inf")) for k, v in fig.items()))
    exact_branch = np.concatenate([b[7]["branch"] for b in exact], axis=1)
    work_none = sum(int(b[6][:, 2].sum()) for b in working)
    dev_none = sum(int(c[:, 2].sum()) for c in got["counts"])
    differ = 0
    for j, s in enumerate(got["specs"]):
        shares = [float((exact_branch[j] == b).mean()) for b in (fh.O, fh.S, fh.P, fh.M)]
        f_n, f_t = np.concatenate([f[j] for f in got["f_n"]]), np.concatenate([f[j] for f in got["f_t"]])
        dev_branch = _branches(f_n, f_t, T(np.float32(s[5][2])))
        counts = sum(c[j] for c in got["counts"])
        dev_shares = [1 - (counts[0] + counts[1]) / total, counts[0] / total, float(((dev_branch != fh.O) & (dev_branch != fh.S) & (f_t > 0)).sum()) / total,
                      float(((dev_branch != fh.O) & (dev_branch != fh.S) & (f_t < 0)).sum()) / total]
        print("  junction %d: shares of O, S, P, M: longdouble %s, device %s" % (j, ["%.3f" % v for v in shares], ["%.3f" % v for v in dev_shares]))
        assert min(shares) >= 0.05 and min(dev_shares) >= 0.05, (j, shares, dev_shares)
        assert int((f_n == 0).sum()) == total - counts[0] - counts[1], j  # the counts and the rows agree on the open frames
        differ += int((dev_branch != exact_branch[j]).sum())
    print("  frames without a consistent candidate: device %d, %s restatement %d; frames whose branch differs from the longdouble run's: %d" % (dev_none, T.__name__, work_none, differ))
    if use_double:
        assert dev_none == 0
    else:
        assert dev_none <= work_none + differ, (dev_none, work_none, differ)
    for key, (device, yardstick) in fig.items():
        assert 0 < yardstick < 1e7 * eps, (key, yardstick)
        assert device <= BOUND * yardstick, (key, device, yardstick)


# ---- 11. bit-exactness ----
@PRECISIONS
@LAWS
def test_a_block_is_its_two_halves_and_the_anchor_matters(use_double, hertz):
    """One block against two halves with the anchor passed on: bit-equal in everything.  With the anchor dropped at every block's start
    the f_t rows move by far more than the bound of the test against longdouble allows: the deviation from the run that keeps it, over the
    row's peak, is above 4 x that run's working-precision yardstick (printed: how many times)."""
    T = np.float64 if use_double else np.float32
    whole = _run(use_double, 1, hertz, 512, rows_on=(0,), restate=(L, T))
    halves = _run(use_double, 1, hertz, 512, rows_on=(0,), split=True)
    _all_equal(whole, halves)
    dropped = _run(use_double, 1, hertz, 512, rows_on=(0,), keep_anchor=False)
    exact, working = whole["rest"]
    yard = max(fh.jh.row_figure(working[blk][2], exact[blk][2]) for blk in range(BLOCKS))
    moved = max(fh.jh.row_figure(dropped["f_t"][blk], whole["f_t"][blk]) for blk in range(1, BLOCKS))
    print("%s %s: without the anchor the f_t rows move by %.3e of their peak, %.1f x the bound (%.3e)" % (T.__name__, "hertz" if hertz else "linear", moved, moved / (BOUND * yard), BOUND * yard))
    assert yard > 0 and moved > BOUND * yard


@PRECISIONS
@LAWS
def test_a_frictional_junction_is_local_and_deterministic(use_double, hertz):
    """A second run is the same bits.  With bystander junctions of every other kind on further objects, drives and pickups on other objects
    and another renderer count, the frictional junction's rows, anchor, counts and its objects' states are the same bits."""
    frames = 333
    first, second = _run(use_double, 1, hertz, frames, rows_on=(0,)), _run(use_double, 1, hertz, frames, rows_on=(0,))
    _all_equal(first, second)
    other = _run(use_double, 4, hertz, frames, rows_on=(0,))
    _all_equal(first, other, keys=("f_n", "f_t", "C", "status", "anchor", "counts"))
    assert _same(first["states"], other["states"])
    beside = _run(use_double, 4, hertz, frames, rows_on=(0,), bystanders=True)
    _all_equal(first, beside, keys=("f_n", "f_t", "C", "status", "anchor", "counts"))
    assert _same(first["states"], beside["states"])


def bh_rate():
    from tests import bank_harness as bh
    return float(bh.SAMPLE_RATE)


@PRECISIONS
def test_an_unflagged_hertz_and_a_damped_junction_keep_their_bits_beside_a_frictional_one(use_double):
    """Junction 0 (objects 0 and 1) a Hertz junction, then a damped one, through render_friction: its force row, C, status, carry and its
    objects' states with the frictional junction 1 (object 2) in the call are array_equal to those of the call without it."""
    from mesheditor_amd import bank as hipbank
    frames = 333
    for kind in ("hertz", "damped"):
        runs = []
        for with_friction in (True, False):
            sc, _ = dh.device_scene(MODES, T60, 1, use_double)
            numbers, u, w = _plan(sc, use_double, False, frames)
            k_hertz = _plan(sc, use_double, True, frames)[0][0][0]
            _ring_up(sc, [], frames)
            other = hipbank.Junction.of(SIDES[0][0], SIDES[0][1], k_hertz if kind == "hertz" else numbers[0][0], hertz=(kind == "hertz"), damped=(kind == "damped"))
            mine, slide = fh.records([_specs(numbers, False)[1]])
            nj = 2 if with_friction else 1
            junctions = (hipbank.Junction * 2)(other, mine[0]) if with_friction else (hipbank.Junction * 1)(other)
            slides = (hipbank.Friction * 2)(hipbank.Friction.of(), slide[0]) if with_friction else (hipbank.Friction * 1)(hipbank.Friction.of())
            blocks, anchor, carry = [], None, None
            for blk in range(BLOCKS):
                sl = slice(blk * frames, (blk + 1) * frames)
                damping = np.full(nj, 50.0 / bh_rate(), np.float32)
                got = sc.render_friction(np.zeros(frames, sc.dtype), [], np.zeros((0, frames), np.float32), [], junctions, u[:nj, sl], slides, w[:nj, sl], damping, carry, anchor)
                carry, anchor = got[5], got[8]
                assert (got[4] == 1).all(), (kind, with_friction, got[4])
                assert np.abs(got[2][0]).max() > 0 and (not with_friction or np.abs(got[7][1]).max() > 0)
                blocks.append((got[2][0].copy(), got[3][0], got[4][0], got[5][0]))
            runs.append((blocks, _states(sc)))
            sc.close()
        end = int(np.cumsum([0] + MODES)[2])
        for blk in range(BLOCKS):
            for a, b in zip(runs[0][0][blk], runs[1][0][blk]):
                assert np.array_equal(a, b, equal_nan=True), (kind, blk)
        assert np.array_equal(runs[0][1][0][:end], runs[1][1][0][:end]) and np.array_equal(runs[0][1][1][:end], runs[1][1][1][:end]), kind


# ---- left out through the entries ----
@PRECISIONS
def test_what_the_entries_leave_out_is_the_call_without_it(use_double):
    """The flag together with bilateral, damped or shared; a tangent component, mu or kt that is not finite; mu < 0, kt < 0: status 0, zero
    rows, C = 0, a NaN anchor, zero counts, and `out` and the states of the call without the junction.  The older entries ignore the bit:
    render_damped_groups with the flag set is the call with it cleared."""
    from mesheditor_amd import bank as hipbank
    frames = 333
    sc, _ = dh.device_scene(MODES, T60, 1, use_double)
    numbers, u, w = _plan(sc, use_double, False, frames)
    ref, _ = dh.device_scene(MODES, T60, 1, use_double)
    _ring_up(sc, [], frames)
    _ring_up(ref, [], frames)
    (a, b), (ta, tb), (k, mu, kt) = SIDES[0], TANGENTS[0], numbers[0]
    good = hipbank.Friction.of(ta, tb, mu, kt)
    kinds = [(hipbank.Junction.of(a, b, k, friction=True, **{extra: True}), good) for extra in ("bilateral", "damped", "shared")]
    for bad in (np.inf, np.nan, -0.25):
        kinds += [(hipbank.Junction.of(a, b, k, friction=True), hipbank.Friction.of(ta, tb, bad, kt)), (hipbank.Junction.of(a, b, k, friction=True), hipbank.Friction.of(ta, tb, mu, bad))]
    for bad in (np.inf, np.nan):
        kinds += [(hipbank.Junction.of(a, b, k, friction=True), hipbank.Friction.of((ta[0], bad, ta[2]), tb, mu, kt)), (hipbank.Junction.of(a, b, k, friction=True), hipbank.Friction.of(ta, (bad, tb[1], tb[2]), mu, kt))]
    for i, (junction, slide) in enumerate(kinds):
        out, plain = np.zeros(frames, sc.dtype), np.zeros(frames, sc.dtype)
        got = sc.render_friction(out, [], np.zeros((0, frames), np.float32), [], [junction], u[:1, :frames], [slide], w[:1, :frames], np.zeros(1, np.float32), None, [0.125])
        ref.render_driven(plain, [], np.zeros((0, frames), np.float32))
        assert got[4][0] == 0 and got[3][0] == 0 and (got[2] == 0).all() and (got[7] == 0).all() and np.isnan(got[8][0]) and (got[9] == 0).all(), i
        assert np.array_equal(out, plain) and _same(_states(sc), _states(ref)) and _same(sc.object_state(), ref.object_state()), i
    flagged, cleared = hipbank.Junction.of(a, b, k, friction=True), hipbank.Junction.of(a, b, k)
    out, plain = np.zeros(frames, sc.dtype), np.zeros(frames, sc.dtype)
    one = sc.render_damped_groups(out, [], np.zeros((0, frames), np.float32), [], [flagged], u[:1, :frames])
    two = ref.render_damped_groups(plain, [], np.zeros((0, frames), np.float32), [], [cleared], u[:1, :frames])
    assert one[4][0] == 1 and np.abs(one[2]).max() > 0
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(one, two)) and np.array_equal(out, plain) and _same(_states(sc), _states(ref))
    sc.close()
    ref.close()
