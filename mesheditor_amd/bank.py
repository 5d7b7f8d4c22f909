"""Python binding of libmodalhost.so: the C++ mirror of the reference's modal bank API (AddModalObject,
TuneModalObject, InstallModalBank, EnqueueModalEvent, RenderModal, ...) running on the MI355X through libmodalhip.
Used by the tests and the bank benchmark; no CPU fallback."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "libmodalhost.so")
_LIB = None

COLUMNS = ["CoeffRe", "CoeffIm", "StateRe", "StateIm", "RadiationGain", "RadiationArea", "DeflectionGain", "OutPhaseIm", "OutPhaseRe",
           "QuadCompliance", "QuadDriveScale", "ShapeX", "ShapeY", "ShapeZ", "OutGain", "ListenerGain", "RadiantRadius", "DeflectionScale"]


class Event(C.Structure):  # ModalEvent, src/audio/ModalAudio.h:28-37
    _fields_ = [("kind", C.c_uint32), ("object", C.c_uint32), ("ex_pos", C.c_uint32), ("jx", C.c_float), ("jy", C.c_float), ("jz", C.c_float),
                ("pulse_step", C.c_float), ("pulse_gamma", C.c_float), ("accel_amp", C.c_float), ("click_b0", C.c_float), ("click_a1", C.c_float),
                ("click_a2", C.c_float)]


class Drive(C.Structure):  # ModalDrive, modal/bank.hpp (mh_drive of modalhip.h field for field)
    _fields_ = [("object", C.c_uint32), ("ex_pos", C.c_uint32), ("jx", C.c_float), ("jy", C.c_float), ("jz", C.c_float)]


class Pickup(C.Structure):  # ModalPickup, modal/bank.hpp (mh_pickup of modalhip.h field for field; `scale` is the caller's coupling here)
    _fields_ = [("object", C.c_uint32), ("points", C.c_uint32 * 3), ("weights", C.c_float * 3), ("nx", C.c_float), ("ny", C.c_float), ("nz", C.c_float),
                ("scale", C.c_float), ("advance", C.c_uint32)]

    @classmethod
    def of(cls, obj, points, weights, direction, coupling=1.0, advance=0):
        """points: one excitation position or three; weights: the blend of the three ((1, 0, 0) for one point)."""
        pts = (points,) * 3 if np.isscalar(points) else tuple(points)
        return cls(obj, (C.c_uint32 * 3)(*pts), (C.c_float * 3)(*weights), direction[0], direction[1], direction[2], coupling, advance)


class JunctionSide(C.Structure):  # ModalJunctionSide, modal/bank.hpp (mh_junction_side of modalhip.h field for field; `scale` is the caller's coupling here)
    _fields_ = [("object", C.c_uint32), ("points", C.c_uint32 * 3), ("weights", C.c_float * 3), ("nx", C.c_float), ("ny", C.c_float), ("nz", C.c_float),
                ("scale", C.c_float)]

    @classmethod
    def of(cls, obj, points, weights, direction, coupling=1.0):
        """points: one excitation position or three; weights: the blend of the three ((1, 0, 0) for one point)."""
        pts = (points,) * 3 if np.isscalar(points) else tuple(points)
        return cls(obj, (C.c_uint32 * 3)(*pts), (C.c_float * 3)(*weights), direction[0], direction[1], direction[2], coupling)


NO_OBJECT, JUNCTION_BILATERAL, JUNCTION_HERTZ, JUNCTION_SHARED = 0xffffffff, 1, 2, 4  # NoModalObject, ModalJunctionBilateral, ModalJunctionHertz, ModalJunctionShared
JUNCTION_DAMPED = 8  # ModalJunctionDamped
JUNCTION_FRICTION = 16  # ModalJunctionFriction


class Friction(C.Structure):  # ModalFriction, modal/bank.hpp (mh_friction of modalhip.h field for field)
    _fields_ = [("ta", C.c_float * 3), ("tb", C.c_float * 3), ("mu", C.c_float), ("stiffness", C.c_float)]

    @classmethod
    def of(cls, ta=(0.0, 0.0, 0.0), tb=(0.0, 0.0, 0.0), mu=0.0, stiffness=0.0):
        """ta, tb: the tangent of side a and of side b (a two-sided junction passes tb = -ta); mu: the Coulomb coefficient; stiffness: the
        stick spring kt of the contact patch in N/m."""
        return cls((C.c_float * 3)(*ta), (C.c_float * 3)(*tb), mu, stiffness)


class Junction(C.Structure):  # ModalJunction, modal/bank.hpp (mh_junction of modalhip.h field for field)
    _fields_ = [("a", JunctionSide), ("b", JunctionSide), ("stiffness", C.c_float), ("flags", C.c_uint32)]

    @classmethod
    def of(cls, a, b=None, stiffness=0.0, bilateral=False, hertz=False, shared=False, damped=False, friction=False):
        """a, b: JunctionSide records or the arguments of JunctionSide.of as tuples; b = None: one-sided (an exciter the caller moves).
        hertz: f = K delta^1.5 with `stiffness` in N/m^1.5 instead of the linear spring (unilateral only: with bilateral it is left out).
        shared: the junction may name an object that an earlier kept junction with shared=True names; up to four linear junctions that
        share objects in this way are one group, solved together in every frame (modalhip.h, MH_JUNCTION_SHARED).
        damped: Hunt-Crossley contact damping on the linear or the Hertz law (Scene.render_damped only; unilateral, and alone on its objects:
        with bilateral, or where it would share an object, it is left out).
        friction: Coulomb friction with stiction beside the normal law (Scene.render_friction only, which takes a Friction record and a travel
        row per junction; unilateral, undamped and without shared: otherwise it is left out)."""
        side = lambda v: v if isinstance(v, JunctionSide) else JunctionSide.of(*v)
        none = JunctionSide(NO_OBJECT, (C.c_uint32 * 3)(0, 0, 0), (C.c_float * 3)(1, 0, 0), 0.0, 0.0, 0.0, 1.0)
        return cls(side(a), side(b) if b is not None else none, stiffness, (JUNCTION_BILATERAL if bilateral else 0) | (JUNCTION_HERTZ if hertz else 0) | (JUNCTION_SHARED if shared else 0) |
                   (JUNCTION_DAMPED if damped else 0) | (JUNCTION_FRICTION if friction else 0))


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(SO_PATH):
        raise RuntimeError(f"{SO_PATH} is missing: run __graft_entry__.build() -- there is no CPU fallback")
    from . import _lib as core
    core.lib()  # libmodalhip first (dependency, also checks its exports)
    L = C.CDLL(SO_PATH)
    vp, u32, i32, f32, f64 = C.c_void_p, C.c_uint32, C.c_int, C.c_float, C.c_double
    sig = {
        "mhx_last_error": (C.c_char_p, []), "mhx_scene_create": (vp, [f32, i32]), "mhx_scene_create_f64": (vp, [f32, i32]), "mhx_scene_destroy": (None, [vp]),
        "mhx_add_object": (u32, [vp, u32, u32, u32, vp, vp, u32, vp]), "mhx_tune_object": (None, [vp, i32, u32, u32, vp, vp, f32]),
        "mhx_set_shapes": (i32, [vp, i32, u32, u32, u32, vp]), "mhx_set_gains": (None, [vp, i32, u32, f32, f32]), "mhx_install": (i32, [vp]),
        "mhx_set_renderers": (None, [vp, u32]), "mhx_set_click_gain": (None, [vp, f32]), "mhx_set_max_impacts": (None, [vp, u32]),
        "mhx_enqueue": (i32, [vp, C.POINTER(Event)]), "mhx_render": (i32, [vp, vp, u32]), "mhx_render_driven": (i32, [vp, vp, u32, u32, vp, vp]),
        "mhx_render_read": (i32, [vp, vp, u32, u32, vp, vp, u32, vp, vp, vp]), "mhx_num_objects": (u32, [vp]),
        "mhx_render_coupled": (i32, [vp, vp, u32, u32, vp, vp, u32, vp, vp, vp, u32, vp, vp, vp, vp, vp]),
        "mhx_render_damped": (i32, [vp, vp, u32, u32, vp, vp, u32, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp]),
        "mhx_render_observed": (i32, [vp, vp, u32, u32, vp, vp, u32, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp]),
        "mhx_render_mixed": (i32, [vp, vp, u32, u32, vp, vp, u32, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp]),
        "mhx_render_damped_groups": (i32, [vp, vp, u32, u32, vp, vp, u32, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp]),
        "mhx_render_friction": (i32, [vp, vp, u32, u32, vp, vp, u32, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "mhx_active_impacts": (u32, [vp]), "mhx_modal_energy": (f64, [vp]), "mhx_render_share": (f32, [vp]), "mhx_find_object": (i32, [vp, u32]),
        "mhx_time_kernels": (i32, [vp, i32]), "mhx_kernel_class_stats": (i32, [vp, i32, C.POINTER(C.c_uint64), C.POINTER(f64), C.POINTER(f64)]),
        "mhx_column": (u32, [vp, i32, i32, vp]), "mhx_object_state": (None, [vp, vp, vp, vp]),
        "mhx_recoil_click_filter": (None, [f64, f64, f64, f64, vp]), "mhx_recoil_object_filter": (None, [f64, f64, f64, vp]),
        "mhx_estimate_contact_time": (f64, [f64, vp, vp, vp, f64, vp, f64, f64, vp, f64, f64, f64, f64]),
        "mhx_striker_mass": (f64, [f64, f32, f32]), "mhx_inverse_inertia_tensor": (None, [vp, vp, vp]),
        "mhx_saturation_penetration": (f64, [f64, f64]), "mhx_punch_stiffness": (f64, [f64, f64]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    _LIB = L
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class Scene:
    """ModalAudio + the bank under construction, as the reference's test harness drives them (tests/ModalBench.h:47-81)."""

    def __init__(self, sample_rate=48000.0, device=0, use_double=False):
        """use_double: the fp64 bank (ModalBank64 / ModalAudio64) -- columns, impacts and output samples in double."""
        self.L = lib()
        self.dtype = np.float64 if use_double else np.float32
        self.h = (self.L.mhx_scene_create_f64 if use_double else self.L.mhx_scene_create)(sample_rate, device)

    def close(self):
        if self.h:
            self.L.mhx_scene_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_object(self, entity, shapes, positions, indices):
        sh, pos, idx = np.ascontiguousarray(shapes, np.float32), np.ascontiguousarray(positions, np.float32), np.ascontiguousarray(indices, np.uint32)
        return self.L.mhx_add_object(self.h, entity, sh.shape[1], sh.shape[0], _p(sh), _p(pos), len(idx), _p(idx))

    def tune_object(self, obj, freqs, t60s, radius_scale=1.0, live=False):
        f, t = np.ascontiguousarray(freqs, np.float32), np.ascontiguousarray(t60s, np.float32)
        self.L.mhx_tune_object(self.h, int(live), obj, min(len(f), len(t)), _p(f), _p(t), radius_scale)

    def set_shapes(self, obj, shapes, live=True):
        sh = np.ascontiguousarray(shapes, np.float32)
        return bool(self.L.mhx_set_shapes(self.h, int(live), obj, sh.shape[1], sh.shape[0], _p(sh)))

    def set_gains(self, obj, out_gain, listener_gain=1.0, live=False):
        self.L.mhx_set_gains(self.h, int(live), obj, out_gain, listener_gain)

    def install(self):
        if self.L.mhx_install(self.h):
            raise RuntimeError(self.L.mhx_last_error().decode())

    def set_renderers(self, n):
        self.L.mhx_set_renderers(self.h, n)

    def set_click_gain(self, g):
        self.L.mhx_set_click_gain(self.h, g)

    def enqueue(self, ev):
        e = Event(*[getattr(ev, n) for n, _ in Event._fields_])
        return bool(self.L.mhx_enqueue(self.h, C.byref(e)))

    def render(self, out):
        assert out.dtype == self.dtype and out.flags["C_CONTIGUOUS"]
        if self.L.mhx_render(self.h, _p(out), len(out)):
            raise RuntimeError(self.L.mhx_last_error().decode())

    def render_driven(self, out, drives, signals):
        """RenderModalDriven: one block with sustained force drives.  drives: a ctypes array of Drive (passed on as it is), or a
        sequence of Drive records or (object, ex_pos, jx, jy, jz) tuples; signals: float32 [len(drives)][len(out)], one force sample per
        drive and frame."""
        assert out.dtype == self.dtype and out.flags["C_CONTIGUOUS"]
        rows = drives if isinstance(drives, C.Array) else (Drive * max(len(drives), 1))(*[v if isinstance(v, Drive) else Drive(*v) for v in drives])
        sig = np.ascontiguousarray(signals, np.float32).reshape(len(drives), len(out))
        if self.L.mhx_render_driven(self.h, _p(out), len(out), len(drives), C.cast(rows, C.c_void_p), _p(sig)):
            raise RuntimeError(self.L.mhx_last_error().decode())

    def _render(self, entry, out, drives, signals, pickups, junctions=None, approach=None, damping=None, carry=None, counted=False, friction=None, travel=None, anchor=None):
        """One block through `entry` of the C wrapper, with what the entry takes beyond render_read's arguments: junctions and approach
        (render_coupled), damping and carry (render_damped), counted (render_mixed), friction, travel and anchor (render_friction).  Returns
        the tuple of the widest of them the entry reaches: (reads, read_flags, forces, compliances, statuses, carry, unconverged, tangent,
        anchor, friction_counts)."""
        assert out.dtype == self.dtype and out.flags["C_CONTIGUOUS"]
        frames = len(out)
        rows = drives if isinstance(drives, C.Array) else (Drive * max(len(drives), 1))(*[v if isinstance(v, Drive) else Drive(*v) for v in drives])
        sig = np.ascontiguousarray(signals, np.float32).reshape(len(drives), frames)
        probes = pickups if isinstance(pickups, C.Array) else (Pickup * max(len(pickups), 1))(*pickups)
        reads, flags = np.zeros((len(pickups), frames), self.dtype), np.zeros(len(pickups), np.uint8)
        args, result = [len(drives), C.cast(rows, C.c_void_p), _p(sig), len(pickups), C.cast(probes, C.c_void_p), _p(reads), _p(flags)], (reads, flags)
        if junctions is not None:
            n = len(junctions)
            contacts = junctions if isinstance(junctions, C.Array) else (Junction * max(n, 1))(*junctions)
            u = np.ascontiguousarray(approach, np.float32).reshape(n, frames)
            forces, compliances, statuses = np.zeros((n, frames), self.dtype), np.zeros(n), np.zeros(n, np.uint8)
            args += [n, C.cast(contacts, C.c_void_p), _p(u), _p(forces), _p(compliances), _p(statuses)]
            result += (forces, compliances, statuses)
        if damping is not None:
            rates = np.ascontiguousarray(damping, np.float32).reshape(n)
            state = np.full(n, np.nan, self.dtype) if carry is None else np.array(carry, self.dtype).reshape(n)
            args += [_p(rates), _p(state)]
            result += (state,)
        if counted:
            counts = np.zeros(n, np.uint32)
            args += [_p(counts)]
            result += (counts,)
        if friction is not None:
            slides = friction if isinstance(friction, C.Array) else (Friction * max(n, 1))(*friction)
            w = np.ascontiguousarray(travel, np.float32).reshape(n, frames)
            tangent, stands, taken = np.zeros((n, frames), self.dtype), np.full(n, np.nan, self.dtype) if anchor is None else np.array(anchor, self.dtype).reshape(n), np.zeros((n, 3), np.uint32)
            args += [C.cast(slides, C.c_void_p), _p(w), _p(tangent), _p(stands), _p(taken)]
            result += (tangent, stands, taken)
        if entry(self.h, _p(out), frames, *args):
            raise RuntimeError(self.L.mhx_last_error().decode())
        return result

    def render_read(self, out, drives, signals, pickups):
        """RenderModalRead: render_driven plus deflection pickups (a ctypes array or a sequence of Pickup records).  Returns (reads,
        read_flags): reads[q] is pickup q's row of len(out) values in the scene's precision, read_flags[q] is 1 when it was read and 0
        when it was left out (its row is zeros then)."""
        return self._render(self.L.mhx_render_read, out, drives, signals, pickups)

    def render_coupled(self, out, drives, signals, pickups, junctions, approach):
        """RenderModalCoupled: render_read plus contact junctions (a ctypes array or a sequence of Junction records) and their approach
        signals, float32 [len(junctions)][len(out)].  Returns (reads, read_flags, forces, compliances, statuses): forces[j] is junction
        j's contact force row in the scene's precision, compliances[j] its compliance C, statuses[j] 0 = left out (a zero row), 1 =
        solved, 2 = refused (1 + K C not a finite number above 0: a zero row)."""
        return self._render(self.L.mhx_render_coupled, out, drives, signals, pickups, junctions, approach)

    def render_observed(self, out, drives, signals, pickups, junctions, approach, damping=None, carry=None):
        """RenderModalObserved: render_damped that also reads the pickups on objects of kept junctions (render_coupled and render_damped leave
        those out).  damping=None: zeros (no junction with damped=True is expected).  Returns render_damped's tuple."""
        rates = np.zeros(len(junctions), np.float32) if damping is None else damping
        return self._render(self.L.mhx_render_observed, out, drives, signals, pickups, junctions, approach, rates, carry)

    def render_mixed(self, out, drives, signals, pickups, junctions, approach, damping=None, carry=None):
        """RenderModalMixed: render_observed in which a junction with shared=True and hertz=True may be a member of a group (the older entries
        leave it out).  Returns render_observed's tuple plus `unconverged`: per junction, for a member of a group with a Hertz member, the
        frames of the block in which the group's residual test failed (0 on valid input); 0 for every other junction."""
        rates = np.zeros(len(junctions), np.float32) if damping is None else damping
        return self._render(self.L.mhx_render_mixed, out, drives, signals, pickups, junctions, approach, rates, carry, counted=True)

    def render_damped_groups(self, out, drives, signals, pickups, junctions, approach, damping=None, carry=None):
        """RenderModalDampedGroups: render_mixed in which a junction with shared=True and damped=True, linear or Hertz, may be a member of a
        group as well (the older entries leave it out).  Returns render_mixed's tuple: the carry holds, for a damped member of a solved
        group, the compression its last frame's solve left (pass it to the next block), and `unconverged` counts the members of a group
        with a Hertz or a damped member."""
        rates = np.zeros(len(junctions), np.float32) if damping is None else damping
        return self._render(self.L.mhx_render_damped_groups, out, drives, signals, pickups, junctions, approach, rates, carry, counted=True)

    def render_friction(self, out, drives, signals, pickups, junctions, approach, friction, travel, damping=None, carry=None, anchor=None):
        """RenderModalFriction: render_damped_groups in which a lone junction with friction=True also solves a tangential force per frame --
        stick inside the Coulomb cone, slide at its edge (modalhip.h, "Friction").  friction: one Friction record per junction (a ctypes
        array or a sequence) and travel: float32 [len(junctions)][len(out)], the rigid tangential offset of the two surfaces, both read for
        flagged junctions only; anchor: one value per junction in the scene's precision -- where the slider stood after the previous block,
        as this call returned it then; None or a value that is not finite: no history.  Returns render_damped_groups' tuple plus (tangent,
        anchor, counts): tangent[j] is junction j's row of f_t, anchor the new anchors (NaN for every junction that is not a solved
        frictional one), counts[j] the frames taken on stick, on slip, and those without a consistent candidate."""
        rates = np.zeros(len(junctions), np.float32) if damping is None else damping
        return self._render(self.L.mhx_render_friction, out, drives, signals, pickups, junctions, approach, rates, carry, counted=True, friction=friction, travel=travel, anchor=anchor)

    def render_damped(self, out, drives, signals, pickups, junctions, approach, damping, carry=None, entry=None):
        """RenderModalDamped: render_coupled with contact damping.  damping: one D in s/m per junction (float32; read for junctions with
        damped=True, l = D * sample rate per frame); carry: one value per junction in the scene's precision -- the compression the last
        frame of the previous block left, as this call returned it then; None or a value that is not finite: no history.  Returns
        render_coupled's tuple plus the new carry (NaN for every junction that is not a solved damped one)."""
        return self._render(entry or self.L.mhx_render_damped, out, drives, signals, pickups, junctions, approach, damping, carry)

    def time_kernels(self, enable=True):
        """HIP-event timing of the bank's kernels on its device context (measurement aid)."""
        if self.L.mhx_time_kernels(self.h, int(enable)):
            raise RuntimeError(self.L.mhx_last_error().decode())

    def kernel_stats(self, kernel_class=2):
        """{"launches", "total_ms", "work"} of a kernel class since time_kernels(True); class 2 = the resonator kernel, work in flops."""
        n, ms, work = C.c_uint64(0), C.c_double(0), C.c_double(0)
        if self.L.mhx_kernel_class_stats(self.h, kernel_class, C.byref(n), C.byref(ms), C.byref(work)):
            raise RuntimeError(self.L.mhx_last_error().decode())
        return {"launches": n.value, "total_ms": ms.value, "work": work.value}

    def column(self, name, live=True):
        which = COLUMNS.index(name)
        n = self.L.mhx_column(self.h, int(live), which, None)
        out = np.zeros(n)
        self.L.mhx_column(self.h, int(live), which, _p(out))
        return out

    def object_state(self):
        n = self.L.mhx_num_objects(self.h)
        tuned, live, ring = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
        self.L.mhx_object_state(self.h, _p(tuned), _p(live), _p(ring))
        return tuned, live, ring

    @property
    def active_impacts(self):
        return self.L.mhx_active_impacts(self.h)

    @property
    def modal_energy(self):
        return self.L.mhx_modal_energy(self.h)

    @property
    def render_share(self):
        return self.L.mhx_render_share(self.h)
