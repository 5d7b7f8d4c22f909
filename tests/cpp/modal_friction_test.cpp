// Coulomb friction through the mirrored API (ModalJunctionFriction / ModalFriction / RenderModalFriction, modal/bank.hpp;
// TangentialStiffness, modal/contact.hpp), included the way a caller of the reference includes the bank (<audio/ModalAudio.h>): the record is
// mh_friction field for field; a frictional junction stays inside its cone, sticks and slips under a travel that swings, and hands its
// anchor from block to block; with a stick stiffness of 0 the normal force, the block and the bank are those of the unflagged junction
// through RenderModalDampedGroups; friction together with bilateral, damped or shared is left out.  The cases whose names begin with host_
// need no GPU (`--host` runs them alone).  Compiles and links without a GPU.
#include "harness.hpp"

#include <audio/ContactModel.h>
#include <audio/ModalAudio.h>
#include <modalhip.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <limits>
#include <span>

static_assert(ModalJunctionFriction == 16u && MH_JUNCTION_FRICTION == 16u, "the flag bit of modalhip.h (MH_JUNCTION_FRICTION)");
static_assert(sizeof(mh_friction) == 32 && sizeof(ModalFriction) == sizeof(mh_friction), "the record of modalhip.h (mh_friction): 32 bytes");
static_assert(offsetof(ModalFriction, Ta) == offsetof(mh_friction, ta) && offsetof(ModalFriction, Tb) == offsetof(mh_friction, tb) && offsetof(ModalFriction, Mu) == offsetof(mh_friction, mu) &&
                  offsetof(ModalFriction, Stiffness) == offsetof(mh_friction, stiffness),
              "ModalFriction is mh_friction field for field");
static_assert(sizeof(mh_junction) == sizeof(ModalJunction), "no change to the junction's record");

namespace {
constexpr float kRate = 48'000.f;
constexpr uint32_t kBlock = 512, kPoints = 4, kModes = 130, kRingUp = 3, kCoupled = 3;

// The synthetic body of the render tests (tests/cpp/modal_junction_test.cpp).
ModalModes LadderModes(uint32_t n_modes, float slowest) {
    ModalModes body;
    body.Freqs.resize(n_modes);
    body.T60s.resize(n_modes);
    for (uint32_t k = 0; k < n_modes; ++k) {
        body.Freqs[k] = 40.f * float(k + 1) * 1.031f;
        body.T60s[k] = slowest / float(k + 1);
    }
    for (uint32_t p = 0; p < kPoints; ++p) {
        body.Positions.push_back({float(p) * 0.01f, 0.f, (p & 1u) ? 0.02f : 0.f});
        if (p >= 2) body.Indices.insert(body.Indices.end(), {p - 2, p - 1, p});
        auto &row = body.Shapes.emplace_back(n_modes);
        for (uint32_t k = 0; k < n_modes; ++k) {
            const float phase = float(k + 1) * 0.37f + float(p);
            row[k] = vec3{std::sin(phase), std::cos(phase * 1.7f), std::sin(phase * 2.3f)} * 0.01f;
        }
    }
    return body;
}

constexpr uint32_t kPoint = 1;
constexpr float kNormal[3] = {0.25f, -1.f, 0.5f}, kTangent[3] = {1.f, 0.25f, 0.f}, kCoupling = 2.f; // (n . t = 0)

// tests/cpp/modal_hertz_test.cpp's rig: two bodies, body 0 rung up by a drive for kRingUp blocks and then left to itself.
struct Rig {
    ModalAudio Engine;
    Rig() {
        const ModalModes body = LadderModes(kModes, 0.3f);
        ModalBank building;
        building.SampleRate = kRate;
        for (uint32_t i = 0; i < 2; ++i) {
            const uint32_t slot = AddModalObject(building, entt::entity{i}, body);
            TuneModalObject(building, slot, body.Freqs, body.T60s);
            building.OutGain[slot] = 1;
        }
        InstallModalBank(Engine, building);
        const std::vector<ModalDrive> drives{{0, 2, 0.5f, -0.25f, 1.f}};
        std::vector<float> force(size_t(kRingUp) * kBlock), out(kBlock);
        for (size_t s = 0; s < force.size(); ++s) force[s] = std::sin(float(s) * 0.013f);
        for (uint32_t i = 0; i < kRingUp; ++i) RenderModalRead(Engine, drives, force.data() + size_t(i) * kBlock, {}, static_cast<float *>(nullptr), out.data(), kBlock);
    }
};

// The largest free deflection at the junction's point along its normal over one block (an advance-1 pickup, no contact): the scale of
// the approach and travel signals.
float FreeReach(Rig &rig) {
    ModalPickup p;
    p.Object = 0, p.Points[0] = p.Points[1] = p.Points[2] = kPoint, p.Nx = kNormal[0], p.Ny = kNormal[1], p.Nz = kNormal[2], p.Coupling = kCoupling, p.Advance = 1;
    const std::vector<ModalPickup> pickups{p};
    std::vector<float> reads(kBlock), out(kBlock, 0.f);
    RenderModalRead(rig.Engine, {}, static_cast<const float *>(nullptr), pickups, reads.data(), out.data(), kBlock);
    float x0 = 0;
    for (float v : reads) x0 = std::max(x0, std::fabs(v));
    return x0;
}

ModalJunction Contact(float stiffness, uint32_t flags) {
    ModalJunction j;
    j.A.Object = 0, j.A.Points[0] = j.A.Points[1] = j.A.Points[2] = kPoint, j.A.Nx = kNormal[0], j.A.Ny = kNormal[1], j.A.Nz = kNormal[2], j.A.Coupling = kCoupling;
    j.Stiffness = stiffness, j.Flags = flags;
    return j;
}
ModalFriction Slider(float mu, float stiffness) {
    ModalFriction f;
    std::copy(kTangent, kTangent + 3, f.Ta);
    f.Mu = mu, f.Stiffness = stiffness;
    return f;
}

struct Block {
    std::vector<float> Forces, Tangents, Out;
    double Compliance{0};
    uint8_t Status{0};
    uint32_t Counts[3]{0, 0, 0};
};
Block RunFriction(Rig &rig, const ModalJunction &junction, const ModalFriction &friction, const float *approach, const float *travel, float &anchor, uint32_t frames = kBlock) {
    Block r;
    r.Forces.assign(kBlock, 0.f), r.Tangents.assign(kBlock, 0.f), r.Out.assign(kBlock, 0.f);
    float damping = 0, carry = std::numeric_limits<float>::quiet_NaN();
    uint32_t unconverged = 0;
    RenderModalFriction(rig.Engine, {}, static_cast<const float *>(nullptr), {}, static_cast<float *>(nullptr), std::span<const ModalJunction>(&junction, 1), approach,
                        std::span<const float>(&damping, 1), std::span<float>(&carry, 1), r.Forces.data(), r.Out.data(), frames, std::span<uint32_t>(&unconverged, 1),
                        std::span<const ModalFriction>(&friction, 1), travel, r.Tangents.data(), std::span<float>(&anchor, 1), std::span<uint32_t>(r.Counts, 3), nullptr, &r.Compliance, &r.Status);
    return r;
}
Block RunPlain(Rig &rig, const ModalJunction &junction, const float *approach) {
    Block r;
    r.Forces.assign(kBlock, 0.f), r.Out.assign(kBlock, 0.f);
    float damping = 0, carry = std::numeric_limits<float>::quiet_NaN();
    uint32_t unconverged = 0;
    RenderModalDampedGroups(rig.Engine, {}, static_cast<const float *>(nullptr), {}, static_cast<float *>(nullptr), std::span<const ModalJunction>(&junction, 1), approach,
                            std::span<const float>(&damping, 1), std::span<float>(&carry, 1), r.Forces.data(), r.Out.data(), kBlock, std::span<uint32_t>(&unconverged, 1), nullptr, &r.Compliance,
                            &r.Status);
    return r;
}
bool SameBank(ModalAudio &a, ModalAudio &b) {
    SyncModalState(a);
    SyncModalState(b);
    return LiveBank(a).StateRe == LiveBank(b).StateRe && LiveBank(a).StateIm == LiveBank(b).StateIm;
}
constexpr float kNoHistory = std::numeric_limits<float>::quiet_NaN();
} // namespace

CASE(host_the_stick_stiffness_helper_is_mindlins_relation) {
    EXPECT(TangentialStiffness(2.0e9, 1.0e-3) == 8.0 * 2.0e9 * 1.0e-3);
    EXPECT(TangentialStiffness(0.0, 1.0e-3) == 0.0 && TangentialStiffness(2.0e9, 0.0) == 0.0);
}

CASE(host_the_record_starts_dead) {
    const ModalFriction f;
    EXPECT(f.Mu == 0 && f.Stiffness == 0 && f.Ta[0] == 0 && f.Ta[1] == 0 && f.Ta[2] == 0 && f.Tb[0] == 0 && f.Tb[1] == 0 && f.Tb[2] == 0);
}

CASE(a_frictional_contact_stays_in_its_cone_sticks_and_slips) {
    Rig scout;
    const std::vector<float> still(kBlock, 0.f);
    float none = kNoHistory;
    const Block probe = RunFriction(scout, Contact(0.f, ModalJunctionFriction), Slider(0.f, 0.f), still.data(), still.data(), none);
    EXPECT(probe.Status == 1 && probe.Compliance > 0 && std::isfinite(none));
    Rig reach;
    const float stiffness = float(3.0 / probe.Compliance), mu = 0.4f, x0 = FreeReach(reach); // K C = 3
    EXPECT(x0 > 0);
    const ModalJunction junction = Contact(stiffness, ModalJunctionFriction);
    const ModalFriction slider = Slider(mu, stiffness); // kt = K
    Rig a;
    std::vector<float> approach(kBlock), travel(kBlock);
    float anchor = kNoHistory;
    uint32_t stick = 0, slip = 0, open = 0, unsolved = 0, outside = 0;
    for (uint32_t i = 0; i < kCoupled; ++i) {
        for (uint32_t s = 0; s < kBlock; ++s) {
            const float t = float(i * kBlock + s);
            approach[s] = x0 * (std::sin(t * 0.016f) + 0.4f);
            travel[s] = 2.f * x0 * std::sin(t * 0.005f);
        }
        const Block got = RunFriction(a, junction, slider, approach.data(), travel.data(), anchor);
        EXPECT(got.Status == 1 && std::isfinite(anchor));
        stick += got.Counts[0], slip += got.Counts[1], unsolved += got.Counts[2], open += kBlock - got.Counts[0] - got.Counts[1];
        for (uint32_t s = 0; s < kBlock; ++s) {
            EXPECT(got.Forces[s] >= 0 && std::isfinite(got.Forces[s]) && std::isfinite(got.Tangents[s]));
            // inside the cone or on its edge (a slipping frame's f_t is mu f_n rounded once; a sticking one's is below it), except where
            // rounding left no candidate consistent
            outside += std::fabs(got.Tangents[s]) > mu * got.Forces[s];
            if (got.Forces[s] == 0) EXPECT(got.Tangents[s] == 0); // an open contact carries no shear
        }
    }
    const uint32_t frames = kCoupled * kBlock;
    EXPECT_NOTE(stick > frames / 20 && slip > frames / 20 && open > frames / 20, std::to_string(stick) + " " + std::to_string(slip) + " " + std::to_string(open));
    EXPECT_NOTE(unsolved <= frames / 100 && outside <= unsolved, std::to_string(unsolved) + " " + std::to_string(outside));
}

CASE(a_dead_slider_leaves_the_unflagged_junction_and_no_frames_leave_the_anchor) {
    Rig with, without, scout;
    const std::vector<float> still(kBlock, 0.f);
    float none = kNoHistory;
    const Block probe = RunFriction(scout, Contact(0.f, 0), Slider(0.f, 0.f), still.data(), still.data(), none);
    EXPECT(probe.Status == 1 && probe.Compliance > 0 && std::isnan(none)); // an unflagged junction has no anchor
    const float stiffness = float(3.0 / probe.Compliance);
    std::vector<float> approach(kBlock), travel(kBlock);
    Rig reach;
    const float x0 = FreeReach(reach);
    for (uint32_t s = 0; s < kBlock; ++s) approach[s] = x0 * (std::sin(float(s) * 0.016f) + 0.4f), travel[s] = 2.f * x0 * std::sin(float(s) * 0.005f);
    float anchor = 0.125f;
    const Block nothing = RunFriction(with, Contact(stiffness, ModalJunctionFriction), Slider(0.4f, 0.f), approach.data(), travel.data(), anchor, 0);
    EXPECT(anchor == 0.125f && nothing.Status == 0); // no frames: nothing is touched
    anchor = kNoHistory;
    const Block got = RunFriction(with, Contact(stiffness, ModalJunctionFriction), Slider(0.4f, 0.f), approach.data(), travel.data(), anchor); // kt = 0
    const Block plain = RunPlain(without, Contact(stiffness, 0), approach.data());
    EXPECT(got.Status == 1 && plain.Status == 1 && got.Compliance == plain.Compliance && std::isfinite(anchor));
    EXPECT(got.Forces == plain.Forces && got.Out == plain.Out);
    EXPECT(std::all_of(got.Tangents.begin(), got.Tangents.end(), [](float v) { return v == 0; }));
    EXPECT(SameBank(with.Engine, without.Engine));
}

CASE(friction_with_bilateral_damped_or_shared_is_left_out) {
    Rig with, without;
    std::vector<float> approach(kBlock, 1e-5f), travel(kBlock, 1e-5f);
    for (const uint32_t extra : {ModalJunctionBilateral, ModalJunctionDamped, ModalJunctionShared}) {
        float anchor = 0.125f;
        const Block got = RunFriction(with, Contact(1e6f, ModalJunctionFriction | extra), Slider(0.4f, 1e6f), approach.data(), travel.data(), anchor);
        EXPECT_NOTE(got.Status == 0 && got.Compliance == 0 && std::isnan(anchor), std::to_string(extra));
        EXPECT(std::all_of(got.Forces.begin(), got.Forces.end(), [](float v) { return v == 0; }) && std::all_of(got.Tangents.begin(), got.Tangents.end(), [](float v) { return v == 0; }));
        std::vector<float> plain(kBlock, 0.f);
        RenderModalRead(without.Engine, {}, static_cast<const float *>(nullptr), {}, static_cast<float *>(nullptr), plain.data(), kBlock);
        EXPECT(plain == got.Out);
    }
    for (const float bad : {-0.1f, std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN()}) { // a mu or kt that is no finite number from 0 up
        for (const bool on_mu : {true, false}) {
            float anchor = 0.125f;
            const Block got = RunFriction(with, Contact(1e6f, ModalJunctionFriction), on_mu ? Slider(bad, 1e6f) : Slider(0.4f, bad), approach.data(), travel.data(), anchor);
            EXPECT_NOTE(got.Status == 0 && std::isnan(anchor), std::to_string(bad));
            std::vector<float> plain(kBlock, 0.f);
            RenderModalRead(without.Engine, {}, static_cast<const float *>(nullptr), {}, static_cast<float *>(nullptr), plain.data(), kBlock);
            EXPECT(plain == got.Out);
        }
    }
    EXPECT(SameBank(with.Engine, without.Engine));
}

int main(int argc, char **argv) {
    if (argc > 1 && std::strcmp(argv[1], "--host") == 0) std::erase_if(check::cases(), [](const check::Case &c) { return c.name.rfind("host_", 0) != 0; });
    return check::run_all();
}
