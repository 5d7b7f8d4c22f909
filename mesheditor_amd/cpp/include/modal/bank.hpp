// Modal synthesis bank behind the reference's API surface (src/audio/ModalAudio.h): ModalEvent, ModalBank (public
// struct-of-arrays columns callers write directly), ModalAudio, and the free functions AddModalObject /
// TuneModalObject / InstallModalBank / SetModalObjectShapes / FindModalObject / EnqueueModalEvent / RenderModal,
// plus the recoil-filter helpers (ModalAudio.h:58-99).
//
// The host bank is the source of truth.  InstallModalBank mirrors it into HBM; RenderModal runs each block on the
// MI355X (mh_bank_render) with one device synchronisation per block.  There is no CPU render path.
//
// Two precisions share one implementation: ModalBank / ModalAudio are the reference's fp32 layout; ModalBank64 /
// ModalAudio64 keep every column, the impact list and the output in double (BASELINE north star: "resonator output
// sample-exact at fp64").  Declarations below follow the reference's names field for field -- that is the contract.
#pragma once
#include "types.hpp"

#include <entt/entity/fwd.hpp>

#include <array>
#include <atomic>
#include <memory>
#include <numbers>
#include <optional>
#include <span>

struct mh_bank;
struct mh_context;

enum class ModalEventKind : uint32_t { Impact, Silence };

// ModalAudio.h:28-37.  Event fields stay float in both precisions (they are produced by float strike code).
struct ModalEvent {
    ModalEventKind Kind{ModalEventKind::Impact};
    uint32_t Object{0}, ExPos{0};
    float Jx{0}, Jy{0}, Jz{0};
    float PulseStep{0}, PulseGamma{0}, AccelAmp{0};
    float ClickB0{0}, ClickA1{0}, ClickA2{0};
};

// Not in the reference's ModalAudio.h: a sustained force drive, the bank-side primitive under the drive rows of the reference's
// surface renderer (src/audio/surface/).  The caller supplies the force signal itself, `frame_count` samples per drive and block
// (RenderModalDriven); the bank applies it at ExPos along (Jx, Jy, Jz) with the gain an impact has there.  No pulse, no click, no
// state between blocks: a drive lasts as long as the caller keeps passing it.  Fields are float like ModalEvent's.
struct ModalDrive {
    uint32_t Object{0}, ExPos{0};
    float Jx{0}, Jy{0}, Jz{0};
};

// Not in the reference's ModalAudio.h: a deflection pickup, the bank-side primitive under the feedback reads of the reference's surface
// renderer (ReadDeflection / ReadRow over ModeReadGains, src/audio/surface/).  A read-only probe: per frame, the object's modal
// displacement along (Nx, Ny, Nz) at the blend Weights of the excitation positions Points ({1, 0, 0} = Points[0] alone), taken from the
// resonator state after that frame's step and advanced freely by Advance samples (0, 1 or 2).  Coupling is the caller's factor; the
// render multiplies it by the object's DeflectionScale.  Passed with a render call (RenderModalRead); it excites and changes nothing.
struct ModalPickup {
    uint32_t Object{0};
    uint32_t Points[3]{0, 0, 0};
    float Weights[3]{1, 0, 0};
    float Nx{0}, Ny{0}, Nz{0};
    float Coupling{1};
    uint32_t Advance{0};
};

// Not in the reference's ModalAudio.h: a contact junction, the bank-side primitive under the per-sample contact solve of the reference's
// surface renderer (SolveChannelStep, src/audio/surface/) with a linear law.  A unilateral -- Flags bit 0: bilateral -- linear spring of
// stiffness Stiffness between a contact point on object A.Object and either a second object (B) or an exciter the caller moves
// (B.Object = NoModalObject), solved implicitly once per frame inside the render call (RenderModalCoupled; the contract, its five steps
// and the returned force rows: include/modalhip.h, mh_junction).  A side is a pickup's contact point and a drive's direction in one record:
// (Nx, Ny, Nz) is the direction in which the junction pushes that side; Coupling is the caller's factor, which the render multiplies by
// the object's DeflectionScale.  Passed with the block it acts in; no state between blocks but a damped junction's carry (below).
// Flags bit 1, ModalJunctionHertz: the Hertzian law f = K delta^(3/2) of ContactModel (modal/contact.hpp) instead of the linear spring,
// with Stiffness = K in N/m^1.5 (ContactStiffness(inv_modulus, curvature) = (4/3) E* sqrt(R) gives it), solved implicitly per frame by the
// fixed Newton iteration of modalhip.h.  Unilateral only: a junction with both bits set is left out.
// Flags bit 2, ModalJunctionShared: the junction may name an object that an earlier kept junction with the same bit names.  The kept
// junctions that share objects in this way -- up to MH_JUNCTION_GROUP of them, linear, their distinct objects within one workgroup's
// waves -- are a group and are solved together per frame (modalhip.h, "Groups"); on a junction that shares nothing the bit changes nothing.
// Flags bit 3, ModalJunctionDamped (RenderModalDamped only; RenderModalCoupled ignores it): Hunt-Crossley contact damping on the linear or
// the Hertz law, f = K phi(y) max(1 + l (y - y_p), 0) with y_p the previous frame's compression, solved implicitly per frame by the fixed
// trees of modalhip.h ("Contact damping").  Unilateral only, and alone on its objects: with ModalJunctionBilateral, or where it would
// share an object with another junction, it is left out.
constexpr uint32_t NoModalObject{0xffffffffu};
constexpr uint32_t ModalJunctionBilateral{1};
constexpr uint32_t ModalJunctionHertz{2};
constexpr uint32_t ModalJunctionShared{4};
constexpr uint32_t ModalJunctionDamped{8};
// Flags bit 4, ModalJunctionFriction (RenderModalFriction only; every older entry ignores it): Coulomb friction with stiction on a lone
// junction -- one slider behind one stick spring beside the normal law, solved in the same frame (modalhip.h, "Friction").  Unilateral,
// undamped and alone on its objects: with ModalJunctionBilateral, ModalJunctionDamped or ModalJunctionShared it is left out.
constexpr uint32_t ModalJunctionFriction{16};
struct ModalJunctionSide {
    uint32_t Object{NoModalObject};
    uint32_t Points[3]{0, 0, 0};
    float Weights[3]{1, 0, 0};
    float Nx{0}, Ny{0}, Nz{0};
    float Coupling{1};
};
struct ModalJunction {
    ModalJunctionSide A, B;
    float Stiffness{0};
    uint32_t Flags{0};
};
// What a junction with ModalJunctionFriction carries beside its record (mh_friction of modalhip.h field for field): a tangent per side -- a
// positive tangential force pushes side A along Ta and side B along Tb, so a two-sided caller passes Tb = -Ta --, the Coulomb coefficient
// and the stick stiffness of the contact patch in N/m (TangentialStiffness of modal/contact.hpp gives it).
struct ModalFriction {
    float Ta[3]{0, 0, 0}, Tb[3]{0, 0, 0};
    float Mu{0};
    float Stiffness{0};
};

constexpr float AirDensity{1.204f}, SpeedOfSound{343.f}, ListenerDistance{1.f};
constexpr float Ln1000 = 3 * std::numbers::ln10_v<float>;

// ---- recoil radiator filters (ModalAudio.h:58-99): bilinear transforms evaluated in double, stored as float ----
struct RecoilPoles {
    double A0{0};
    float A1{0}, A2{0};
};
RecoilPoles RecoilDenominator(double wc, double kk, double beta);
struct RecoilFilter {
    float RadB0{0}, AirB0{0}, AirB1{0}, AirB2{0}, A1{0}, A2{0};
};
RecoilFilter RecoilObjectFilter(double radius, double volume, double sample_rate);
struct ClickFilter {
    float B0{0}, A1{0}, A2{0};
};
ClickFilter RecoilClickFilter(double radius, double volume, double mass, double sample_rate);

// Not in the reference: the half-open range of per-mode (or shape) entries written since the device mirror last saw
// them.  Writers widen it from any thread; the render claims it at block start and uploads exactly that range.
class ModalEditSpan {
public:
    ModalEditSpan() = default;
    ModalEditSpan(const ModalEditSpan &o) { *this = o; }
    ModalEditSpan &operator=(const ModalEditSpan &o) {
        First.store(o.First.load(std::memory_order_relaxed), std::memory_order_relaxed);
        End.store(o.End.load(std::memory_order_relaxed), std::memory_order_relaxed);
        return *this;
    }
    void Mark(uint32_t first, uint32_t end) {
        uint32_t seen = First.load(std::memory_order_relaxed);
        while (first < seen && !First.compare_exchange_weak(seen, first, std::memory_order_relaxed)) {}
        seen = End.load(std::memory_order_relaxed);
        while (end > seen && !End.compare_exchange_weak(seen, end, std::memory_order_release)) {}
    }
    // Claims the pending range; false when nothing was marked.
    bool Take(uint32_t &first, uint32_t &end) {
        end = End.exchange(0, std::memory_order_acquire);
        first = First.exchange(UINT32_MAX, std::memory_order_relaxed);
        return first < end;
    }

private:
    std::atomic<uint32_t> First{UINT32_MAX}, End{0};
};

// ModalAudio.h:103-166, columns in `Real`.
template<typename Real> struct ModalBankColumns {
    using Scalar = Real;
    // per mode
    std::vector<Real> CoeffRe, CoeffIm, StateRe, StateIm, RadiationGain, RadiationArea, DeflectionGain, OutPhaseIm, OutPhaseRe, QuadCompliance, QuadDriveScale;
    // per (object, sample position, mode): ShapeOffset[o] + p * ModeCount[o] + k
    std::vector<Real> ShapeX, ShapeY, ShapeZ;
    // per object
    std::vector<entt::entity> Entities;
    std::vector<uint32_t> ModeOffset, ModeCount, ShapeOffset, TunedModeCount, LiveModeCount;
    std::vector<Real> OutGain, ListenerGain, RadiantRadius, DeflectionScale;
    std::vector<uint8_t> Ringing;
    std::vector<Real> RigidInvMass;
    std::vector<vec3> RigidVel;
    std::vector<Real> RadiatorB0, AirB0, AirB1, AirB2, RecoilA1, RecoilA2, RadiatorZ1, RadiatorZ2, AirZ1, AirZ2;
    struct ActiveImpact {
        uint32_t Object, ExPos, SamplesLeft;
        Real Jx, Jy, Jz, PhaseRe, PhaseIm, RotRe, RotIm, Gamma, AccelAmp, ClickB0, ClickA1, ClickA2, ClickZ1, ClickZ2;
    };
    std::vector<ActiveImpact> Impacts;
    Real SampleRate{48'000};
    ModalEditSpan EditedModes, EditedShapes; // device-mirror bookkeeping (not in the reference)
};
struct ModalBank : ModalBankColumns<float> {};
struct ModalBank64 : ModalBankColumns<double> {};

// Callers that write per-mode or shape columns of a published bank directly tell the mirror which range they touched.
template<typename Real> void MarkModalColumnsEdited(ModalBankColumns<Real> &b, uint32_t first_mode, uint32_t end_mode) { b.EditedModes.Mark(first_mode, end_mode); }
template<typename Real> void MarkModalShapesEdited(ModalBankColumns<Real> &b, uint32_t first, uint32_t end) { b.EditedShapes.Mark(first, end); }

constexpr uint32_t Lanes{8};

// The reference's pool of render threads is a renderer COUNT here: it fixes the deterministic deal of objects to
// renderers and with it the summation order of the mix; the rendering itself happens on the device.
struct ModalRenderPool {
    void SetSize(uint32_t count);
    void SetWorkgroup(void *) {}
    uint32_t Size() const { return Active; }

private:
    uint32_t Active{1};
};

struct ModalDeviceMirror; // opaque: device context, device bank, per-block staging

// ModalAudio.h:255-291 over a bank type.
template<typename Bank> struct ModalAudioCore {
    using BankType = Bank;
    using Scalar = typename Bank::Scalar;
    ModalAudioCore();
    ~ModalAudioCore();
    ModalAudioCore(const ModalAudioCore &) = delete;
    ModalAudioCore &operator=(const ModalAudioCore &) = delete;

    std::unique_ptr<Bank> Live;
    std::atomic<Bank *> Published;
    std::atomic<uint64_t> ReaderSeq{0};
    std::atomic<float> ClickGain{1};
    std::atomic<uint32_t> MaxImpacts{1024}, ActiveImpacts{0}, ActiveVoices{0};
    std::atomic<double> ModalEnergy{0}, PeakModalEnergy{0};
    std::atomic<float> RenderSeconds{0}, RenderShare{0}, PeakRenderShare{0};
    uint64_t EventsDropped{0};
    static constexpr uint32_t EventCapacity{256};
    std::array<ModalEvent, EventCapacity> Events;
    std::atomic<uint32_t> EventWrite{0}, EventRead{0};
    std::atomic<bool> FlushEvents{false};
    ModalRenderPool RenderPool;
    int Device{0}; // HIP device the bank lives on
    std::unique_ptr<ModalDeviceMirror> Dev;
};
struct ModalAudio : ModalAudioCore<ModalBank> {};
struct ModalAudio64 : ModalAudioCore<ModalBank64> {};

inline ModalBank &LiveBank(ModalAudio &m) { return *m.Live; }
inline ModalBank64 &LiveBank(ModalAudio64 &m) { return *m.Live; }

// ModalAudio.h:294-315, once per precision.
uint32_t AddModalObject(ModalBank &, entt::entity, const ModalModes &);
uint32_t AddModalObject(ModalBank64 &, entt::entity, const ModalModes &);
void InstallModalBank(ModalAudio &, ModalBank &next);
void InstallModalBank(ModalAudio64 &, ModalBank64 &next);
void TuneModalObject(ModalBank &, uint32_t object, std::span<const float> freqs, std::span<const float> t60s, float radius_scale = 1.f);
void TuneModalObject(ModalBank64 &, uint32_t object, std::span<const float> freqs, std::span<const float> t60s, float radius_scale = 1.f);
bool SetModalObjectShapes(ModalBank &, uint32_t object, const ModalModes &);
bool SetModalObjectShapes(ModalBank64 &, uint32_t object, const ModalModes &);
std::optional<uint32_t> FindModalObject(const ModalBank &, entt::entity);
std::optional<uint32_t> FindModalObject(const ModalBank64 &, entt::entity);
void EnqueueModalEvent(ModalAudio &, const ModalEvent &);
void EnqueueModalEvent(ModalAudio64 &, const ModalEvent &);
// Adds frame_count mono samples into `out`.  Events take effect at the start of the block.
void RenderModal(ModalAudio &, float *out, uint32_t frame_count);
void RenderModal(ModalAudio64 &, double *out, uint32_t frame_count);
// Not in the reference: RenderModal with sustained drives.  `signals` holds drives.size() rows of frame_count force samples, in the
// drives' order.  Per sample a mode's excitation is the running sum over its object's impacts (impact-list order, as RenderModal),
// then over its drives in the order given here.  A sample that is not finite counts as 0.  An object with a drive is excited for the
// block like one with an impact in flight: it rings, is dealt at and renders its tuned mode count, is not silenced, and leaves the
// block with LiveModeCount = TunedModeCount.  A drive addressed to an object the bank does not have, to one without modes, or to an
// excitation position its shape columns do not cover is dropped, as such an impact is.  Without drives this is RenderModal.
void RenderModalDriven(ModalAudio &, std::span<const ModalDrive> drives, const float *signals, float *out, uint32_t frame_count);
void RenderModalDriven(ModalAudio64 &, std::span<const ModalDrive> drives, const float *signals, double *out, uint32_t frame_count);
// Not in the reference: RenderModalDriven with pickups.  `reads` receives pickups.size() rows of frame_count values (written, not added
// to), `read_flags` (nullable) one byte per pickup: 1 = read, 0 = left out (row of zeros) -- an object the bank does not have or without
// modes, a point its shape columns do not cover, a weight, direction component or coupling that is not finite, Advance > 2, or more than
// MH_PICKUPS_PER_OBJECT (modalhip.h) pickups on the object before it.  A pickup on an object at rest reads zeros and counts as read.
// Pickups observe: `out`, the bank and every decision of the block are those of RenderModalDriven.  Without pickups this is it.
void RenderModalRead(ModalAudio &, std::span<const ModalDrive> drives, const float *signals, std::span<const ModalPickup> pickups, float *reads, float *out,
                     uint32_t frame_count, uint8_t *read_flags = nullptr);
void RenderModalRead(ModalAudio64 &, std::span<const ModalDrive> drives, const float *signals, std::span<const ModalPickup> pickups, double *reads, double *out,
                     uint32_t frame_count, uint8_t *read_flags = nullptr);
// Not in the reference: RenderModalRead with contact junctions.  `approach` holds junctions.size() rows of frame_count samples (the rigid
// indentation the caller's physics imposes; a sample that is not finite counts as 0), `forces` receives as many rows of the contact force
// (written, not added to), `compliances` (nullable) the compliance C of each junction and `statuses` (nullable) one byte each: 0 = left
// out (row of zeros), 1 = solved, 2 = refused (1 + K C is not a finite number above 0 -- Hertz: C < 0, or C or K C not finite --: no
// force, the objects render as with K = 0).  An object on a side of a junction that is not left out is excited for the block like one with
// a drive: it rings, is dealt at and renders its tuned mode count, is not silenced, and leaves the block with LiveModeCount =
// TunedModeCount.  Left out, and exciting nothing: a side naming no object of the bank (B.Object = NoModalObject is the one-sided
// junction, not that), an object without modes or without tuned modes, a point its shape columns do not cover, a weight, direction
// component, coupling or stiffness that is not finite, a negative stiffness, ModalJunctionHertz together with ModalJunctionBilateral, both
// sides the same object, an object already on a side of an earlier junction of the call that was kept (one junction per object, unless
// both junctions carry ModalJunctionShared), and sides that together take more than MH_JUNCTION_MODES / 128 waves of 128 tuned modes
// (modalhip.h).  Junctions with ModalJunctionShared that share objects form a group, which is solved together in every frame: every
// member's force meets its law at the next frame's displacement at once.  Left out among those, in call order: the junction that would
// be a group's fifth (MH_JUNCTION_GROUP is 4), the one with which the group's distinct objects would take more than
// MH_JUNCTION_MODES / 128 waves, a Hertz junction that would join another junction, and any junction that would join a Hertz one.  The
// decision is taken here and again by the device entry, from one definition (modalhip_groups.hpp); every kept junction counts as an
// excitation of its objects.  A pickup on an object that is on a kept junction's side is left out in this version (RenderModalObserved
// below reads it).  Without junctions this is RenderModalRead.
void RenderModalCoupled(ModalAudio &, std::span<const ModalDrive> drives, const float *signals, std::span<const ModalPickup> pickups, float *reads,
                        std::span<const ModalJunction> junctions, const float *approach, float *forces, float *out, uint32_t frame_count, uint8_t *read_flags = nullptr,
                        double *compliances = nullptr, uint8_t *statuses = nullptr);
void RenderModalCoupled(ModalAudio64 &, std::span<const ModalDrive> drives, const float *signals, std::span<const ModalPickup> pickups, double *reads,
                        std::span<const ModalJunction> junctions, const float *approach, double *forces, double *out, uint32_t frame_count, uint8_t *read_flags = nullptr,
                        double *compliances = nullptr, uint8_t *statuses = nullptr);
// Not in the reference: RenderModalCoupled with contact damping (ModalJunctionDamped).  `damping` holds one D in s/m per junction (read for
// flagged junctions only; ContactDamping(restitution, approach speed) of modal/contact.hpp gives it), which the render turns into the
// per-frame l = float(D) * float(SampleRate), rounded once in float.  `carry` holds one value per junction in the bank's precision, in and
// out: the compression the last frame's solve left.  A value that is not finite on entry means "no history" (the first frame is solved
// without damping and starts it); on return a damped junction that was solved has its carry, every other junction a quiet NaN; with
// frame_count = 0 it comes back unchanged.  Hand it to the next block's call as it is.  Left out beyond RenderModalCoupled's kinds: a
// damped junction whose D * SampleRate is not finite or is below 0, ModalJunctionDamped with ModalJunctionBilateral, a damped junction that
// would join a group, and a junction that would join a damped one.  Refused (status 2): a damped junction when C < 0, or C, K C or K C l is
// not finite.  Without a flagged junction this is RenderModalCoupled, plus NaN carries.
void RenderModalDamped(ModalAudio &, std::span<const ModalDrive> drives, const float *signals, std::span<const ModalPickup> pickups, float *reads,
                       std::span<const ModalJunction> junctions, const float *approach, std::span<const float> damping, std::span<float> carry, float *forces, float *out,
                       uint32_t frame_count, uint8_t *read_flags = nullptr, double *compliances = nullptr, uint8_t *statuses = nullptr);
void RenderModalDamped(ModalAudio64 &, std::span<const ModalDrive> drives, const float *signals, std::span<const ModalPickup> pickups, double *reads,
                       std::span<const ModalJunction> junctions, const float *approach, std::span<const float> damping, std::span<double> carry, double *forces, double *out,
                       uint32_t frame_count, uint8_t *read_flags = nullptr, double *compliances = nullptr, uint8_t *statuses = nullptr);
// Not in the reference: RenderModalDamped that also reads the pickups on junction objects.  A pickup on an object that is on a side of a kept
// junction (status 1 or 2; a lone linear, Hertz or damped junction, or a member of a group) is read like any other: frame s of its row is the
// sum over the object's rendered modes of g_im Im z[s] + g_re Re z[s], with the pickup's gains of RenderModalRead (Advance 0, 1 or 2) and z[s]
// the state after the frame's contact force was applied -- the state the frame's output is formed from.  The advance is free: no contact
// force acts in the look-ahead.  So Advance-1 pickups at a junction's own sides (same points, weights, direction and coupling) sum to
// d + C f[s], and approach[s] minus that sum is the compression of frame s + 1, the quantity every law is implicit in; for a damped junction
// the last frame's value is the returned carry, up to rounding.  The summation order is RenderModalRead's, so a row depends on its object's
// state trajectory and its own record only.  Pickups only observe: with them removed, `out`, the bank, the forces, compliances, statuses and
// carries are the same bits.  A refused junction's objects render as with K = 0 and are read.  Every other pickup, every left-out kind and
// everything else is RenderModalDamped's; the older entries above keep leaving such pickups out.
void RenderModalObserved(ModalAudio &, std::span<const ModalDrive> drives, const float *signals, std::span<const ModalPickup> pickups, float *reads,
                         std::span<const ModalJunction> junctions, const float *approach, std::span<const float> damping, std::span<float> carry, float *forces, float *out,
                         uint32_t frame_count, uint8_t *read_flags = nullptr, double *compliances = nullptr, uint8_t *statuses = nullptr);
void RenderModalObserved(ModalAudio64 &, std::span<const ModalDrive> drives, const float *signals, std::span<const ModalPickup> pickups, double *reads,
                         std::span<const ModalJunction> junctions, const float *approach, std::span<const float> damping, std::span<double> carry, double *forces, double *out,
                         uint32_t frame_count, uint8_t *read_flags = nullptr, double *compliances = nullptr, uint8_t *statuses = nullptr);
// Hertz junctions in groups (modalhip.h, mh_bank_render_mixed): RenderModalObserved -- its parameters in its order, then
// `unconverged`, one count per junction -- except that a kept junction with ModalJunctionShared | ModalJunctionHertz may be a member of a
// group, beside linear unilateral, bilateral and other Hertz members.  Such a group's step 4 is the header's step 4m: y = x - C f(y) with
// every member's own law, by a fixed tree (each member alone, one Gauss-Seidel sweep, ten Newton steps, the last one from a residual
// summed in twice the working precision).  unconverged[j]: for a member
// of a group with a Hertz member, the frames of the block in which the group's final residual test failed -- 0 on valid input --; 0 for
// every other junction.  Still left out: Hertz with bilateral, a damped junction in a group, a fifth member, a ninth wave, a flagged
// junction on an unflagged junction's object.  A group without a Hertz member, every other junction and every older entry are what they were.
void RenderModalMixed(ModalAudio &, std::span<const ModalDrive> drives, const float *signals, std::span<const ModalPickup> pickups, float *reads,
                      std::span<const ModalJunction> junctions, const float *approach, std::span<const float> damping, std::span<float> carry, float *forces, float *out,
                      uint32_t frame_count, std::span<uint32_t> unconverged, uint8_t *read_flags = nullptr, double *compliances = nullptr, uint8_t *statuses = nullptr);
void RenderModalMixed(ModalAudio64 &, std::span<const ModalDrive> drives, const float *signals, std::span<const ModalPickup> pickups, double *reads,
                      std::span<const ModalJunction> junctions, const float *approach, std::span<const float> damping, std::span<double> carry, double *forces, double *out,
                      uint32_t frame_count, std::span<uint32_t> unconverged, uint8_t *read_flags = nullptr, double *compliances = nullptr, uint8_t *statuses = nullptr);
// Damped junctions in groups (modalhip.h, mh_bank_render_damped_groups): RenderModalMixed -- its parameters in its
// order -- except that a kept junction with ModalJunctionShared | ModalJunctionDamped, linear or Hertz, may be a member of a group as well,
// beside linear unilateral, bilateral, Hertz and other damped members.  Such a group's step 4 is the header's step 4g: step 4m's tree with
// f = K phi(y) max(1 + l (y - y_p), 0) on the damped members.  carry: one value per junction, in and out, with RenderModalDamped's meaning
// (not finite: no history; a quiet NaN comes back for every junction that is not a solved damped one); unconverged[j] counts the frames of
// a member of a group with a Hertz or a damped member that failed the residual test.  Still left out: damped or Hertz with bilateral, a
// damping that is not a finite number from 0 up, a fifth member, a ninth wave, a flagged junction on an unflagged junction's object.
// Every other junction, every other group and every older entry are what they were.
void RenderModalDampedGroups(ModalAudio &, std::span<const ModalDrive> drives, const float *signals, std::span<const ModalPickup> pickups, float *reads,
                             std::span<const ModalJunction> junctions, const float *approach, std::span<const float> damping, std::span<float> carry, float *forces, float *out,
                             uint32_t frame_count, std::span<uint32_t> unconverged, uint8_t *read_flags = nullptr, double *compliances = nullptr, uint8_t *statuses = nullptr);
void RenderModalDampedGroups(ModalAudio64 &, std::span<const ModalDrive> drives, const float *signals, std::span<const ModalPickup> pickups, double *reads,
                             std::span<const ModalJunction> junctions, const float *approach, std::span<const float> damping, std::span<double> carry, double *forces, double *out,
                             uint32_t frame_count, std::span<uint32_t> unconverged, uint8_t *read_flags = nullptr, double *compliances = nullptr, uint8_t *statuses = nullptr);
// Friction (modalhip.h, mh_bank_render_friction): RenderModalDampedGroups -- its parameters in its order up to
// `unconverged` -- followed by what the tangential channel takes and returns.  A kept lone junction with ModalJunctionFriction also solves,
// in every frame, a tangential force f_t: stick inside the Coulomb cone (f_t = kt (e - q), the slider q stays), slide at its edge
// (|f_t| = Mu f_n, the slider follows).  friction: one record per junction and travel: one row of frame_count samples per junction (the
// rigid tangential offset of the two surfaces, a position; a sample that is not finite counts as 0), both read for flagged junctions only.
// tangents receives one row of f_t per junction (written).  anchor: one value per junction in the bank's precision, in and out: where the
// slider stands.  A value that is not finite on entry means "no history" (frame 0 takes it from the contact itself); on return a solved
// frictional junction has its anchor, every other junction a quiet NaN; with frame_count = 0 it comes back unchanged.  friction_counts: three
// per junction -- the frames taken on stick, on slip, and those on which rounding left no candidate consistent (small on valid input).
// Left out beyond RenderModalDampedGroups' kinds: the flag with ModalJunctionBilateral, ModalJunctionDamped or ModalJunctionShared; a
// tangent component, Mu or Stiffness that is not finite; Mu < 0 or Stiffness < 0.  Refused (status 2) beyond the normal law's conditions:
// the cone condition Mu |C_nt| <= C_nn fails, or a compliance is not finite.  Stiffness = 0, Mu = 0 or zero tangents leave the normal force,
// `out` and the bank as without the flag.  Without a flagged junction this is RenderModalDampedGroups.
void RenderModalFriction(ModalAudio &, std::span<const ModalDrive> drives, const float *signals, std::span<const ModalPickup> pickups, float *reads,
                         std::span<const ModalJunction> junctions, const float *approach, std::span<const float> damping, std::span<float> carry, float *forces, float *out,
                         uint32_t frame_count, std::span<uint32_t> unconverged, std::span<const ModalFriction> friction, const float *travel, float *tangents,
                         std::span<float> anchor, std::span<uint32_t> friction_counts, uint8_t *read_flags = nullptr, double *compliances = nullptr, uint8_t *statuses = nullptr);
void RenderModalFriction(ModalAudio64 &, std::span<const ModalDrive> drives, const float *signals, std::span<const ModalPickup> pickups, double *reads,
                         std::span<const ModalJunction> junctions, const float *approach, std::span<const float> damping, std::span<double> carry, double *forces, double *out,
                         uint32_t frame_count, std::span<uint32_t> unconverged, std::span<const ModalFriction> friction, const float *travel, double *tangents,
                         std::span<double> anchor, std::span<uint32_t> friction_counts, uint8_t *read_flags = nullptr, double *compliances = nullptr, uint8_t *statuses = nullptr);
// Not in the reference: the libmodalhip context the bank's device mirror lives on (created on demand), for callers that
// time its kernels (mh_context_time_kernels / mh_context_kernel_class_stats).
mh_context *ModalDeviceContext(ModalAudio &);
mh_context *ModalDeviceContext(ModalAudio64 &);
// Not in the reference: copies the device-resident StateRe / StateIm back into the host bank for inspection.
void SyncModalState(ModalAudio &);
void SyncModalState(ModalAudio64 &);
