// Damped junctions in groups through the mirrored API (RenderModalDampedGroups, modal/bank.hpp), included the way a caller of the reference
// includes the bank (<audio/ModalAudio.h>): a damped member of a group, linear or Hertz, is solved through RenderModalDampedGroups and left
// out through RenderModalMixed; without a damped junction in a group the entry is RenderModalMixed, bit for bit, carries and counts
// included.  The cases whose names begin with host_ need no GPU (`--host` runs them alone).  Compiles and links without a GPU.
#include "harness.hpp"

#include <audio/ModalAudio.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <span>
#include <stdexcept>
#include <type_traits>

namespace {
// RenderModalDampedGroups takes RenderModalMixed's parameters in its order and nothing more, in both precisions.
using MixedF = void (*)(ModalAudio &, std::span<const ModalDrive>, const float *, std::span<const ModalPickup>, float *, std::span<const ModalJunction>, const float *,
                        std::span<const float>, std::span<float>, float *, float *, uint32_t, std::span<uint32_t>, uint8_t *, double *, uint8_t *);
using MixedD = void (*)(ModalAudio64 &, std::span<const ModalDrive>, const float *, std::span<const ModalPickup>, double *, std::span<const ModalJunction>, const float *,
                        std::span<const float>, std::span<double>, double *, double *, uint32_t, std::span<uint32_t>, uint8_t *, double *, uint8_t *);
[[maybe_unused]] constexpr MixedF kMixedF = &RenderModalMixed;
[[maybe_unused]] constexpr MixedD kMixedD = &RenderModalMixed;
[[maybe_unused]] constexpr MixedF kDampedGroupsF = &RenderModalDampedGroups;
[[maybe_unused]] constexpr MixedD kDampedGroupsD = &RenderModalDampedGroups;

constexpr float kRate = 48'000.f;
constexpr uint32_t kBlock = 512, kPoints = 4, kModes = 130, kRingUp = 3, kBlocks = 3;

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

std::vector<float> Scrape(uint32_t blocks, uint32_t seed) {
    std::vector<float> f(size_t(blocks) * kBlock);
    uint32_t lcg = seed;
    for (size_t s = 0; s < f.size(); ++s) {
        lcg = lcg * 1664525u + 1013904223u;
        f[s] = 0.6f * std::sin(float(s) * 0.013f) + 0.4f * (float(lcg >> 8) / float(1u << 24) - 0.5f);
    }
    return f;
}

constexpr float kNormal[3] = {0.25f, -1.f, 0.5f};

// Three bodies (130, 130 and 37 modes), every one rung up by a drive for kRingUp blocks.
struct Rig {
    ModalAudio Engine;
    Rig() {
        ModalBank building;
        building.SampleRate = kRate;
        for (uint32_t i = 0; i < 3; ++i) {
            const ModalModes body = LadderModes(i == 2 ? 37 : kModes, 0.3f);
            const uint32_t slot = AddModalObject(building, entt::entity{i}, body);
            TuneModalObject(building, slot, body.Freqs, body.T60s);
            building.OutGain[slot] = 1;
        }
        InstallModalBank(Engine, building);
        const std::vector<ModalDrive> drives{{0, 2, 0.5f, -0.25f, 1.f}, {1, 1, 1.f, 0.5f, 0.f}, {2, 3, 0.f, 1.f, 0.5f}};
        std::vector<float> force;
        for (uint32_t d = 0; d < 3; ++d) {
            const std::vector<float> one = Scrape(kRingUp, 4321u + d);
            force.insert(force.end(), one.begin(), one.end());
        }
        std::vector<float> out(kBlock), block(3 * kBlock);
        for (uint32_t i = 0; i < kRingUp; ++i) {
            for (uint32_t d = 0; d < 3; ++d) std::copy_n(force.begin() + size_t(d) * kRingUp * kBlock + size_t(i) * kBlock, kBlock, block.begin() + size_t(d) * kBlock);
            RenderModalRead(Engine, drives, block.data(), {}, static_cast<float *>(nullptr), out.data(), kBlock);
        }
    }
};

ModalJunctionSide Side(uint32_t object, uint32_t point, float sign, float coupling) {
    ModalJunctionSide s;
    s.Object = object, s.Points[0] = s.Points[1] = s.Points[2] = point;
    s.Nx = sign * kNormal[0], s.Ny = sign * kNormal[1], s.Nz = sign * kNormal[2], s.Coupling = coupling;
    return s;
}
ModalJunction Contact(const ModalJunctionSide &a, float stiffness, uint32_t flags) {
    ModalJunction j;
    j.A = a, j.Stiffness = stiffness, j.Flags = flags;
    return j;
}
ModalJunction Contact(const ModalJunctionSide &a, const ModalJunctionSide &b, float stiffness, uint32_t flags) {
    ModalJunction j = Contact(a, stiffness, flags);
    j.B = b;
    return j;
}
ModalPickup Probe(uint32_t object, uint32_t point, uint32_t advance, float coupling = 1.f) {
    ModalPickup p;
    p.Object = object, p.Points[0] = p.Points[1] = p.Points[2] = point, p.Nx = kNormal[0], p.Ny = kNormal[1], p.Nz = kNormal[2], p.Coupling = coupling, p.Advance = advance;
    return p;
}

struct Block {
    std::vector<float> Out, Reads, Forces, Carry;
    std::vector<uint8_t> Flags, Status;
    std::vector<double> Compliance;
    std::vector<uint32_t> Counts;
};
// One block through RenderModalDampedGroups (damped_groups) or RenderModalMixed; carry: what the block before returned (empty: no history).
Block Run(bool damped_groups, ModalAudio &engine, std::span<const ModalPickup> pickups, std::span<const ModalJunction> junctions, const float *approach, float damping,
          const std::vector<float> &carry = {}) {
    Block r;
    r.Out.assign(kBlock, 0.f), r.Reads.assign(pickups.size() * kBlock, 0.f), r.Forces.assign(junctions.size() * kBlock, 0.f);
    r.Flags.assign(pickups.size(), 0), r.Status.assign(junctions.size(), 0), r.Compliance.assign(junctions.size(), 0.0);
    r.Carry = carry.empty() ? std::vector<float>(junctions.size(), std::numeric_limits<float>::quiet_NaN()) : carry;
    r.Counts.assign(junctions.size(), 7u);
    const std::vector<float> rates(junctions.size(), damping);
    (damped_groups ? kDampedGroupsF : kMixedF)(engine, {}, nullptr, pickups, r.Reads.data(), junctions, approach, rates, std::span<float>(r.Carry), r.Forces.data(), r.Out.data(), kBlock,
                                               r.Counts, r.Flags.data(), r.Compliance.data(), r.Status.data());
    return r;
}
bool SameBits(const std::vector<float> &a, const std::vector<float> &b) { return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0); }
bool SameBank(ModalAudio &a, ModalAudio &b) {
    SyncModalState(a);
    SyncModalState(b);
    return LiveBank(a).StateRe == LiveBank(b).StateRe && LiveBank(a).StateIm == LiveBank(b).StateIm;
}
constexpr float kReach = 1e-5f;
constexpr float kDamping = 1.f / kReach / kRate; // D in s/m with l = D * sample rate = 1 / kReach per frame

// The hub (object 1) with a two-sided junction to object 0, one to object 2 and an exciter; K from the compliances a K = 0 block returns.
// laws: the flags each member gets beside ModalJunctionShared.
std::vector<ModalJunction> Star(ModalAudio &scout, const uint32_t (&laws)[3]) {
    std::vector<ModalJunction> star{Contact(Side(1, 1, 1.f, 1.5f), Side(0, 2, -1.f, 1.5f), 0.f, ModalJunctionShared), Contact(Side(1, 2, 1.f, 2.f), Side(2, 0, -1.f, 2.f), 0.f, ModalJunctionShared),
                                    Contact(Side(1, 3, 1.f, 1.f), 0.f, ModalJunctionShared)};
    const std::vector<float> still(3 * kBlock, 0.f);
    const Block free = Run(false, scout, {}, star, still.data(), 0.f);
    for (size_t j = 0; j < star.size(); ++j) {
        star[j].Stiffness = float(3.0 / free.Compliance[j]) / ((laws[j] & ModalJunctionHertz) ? std::sqrt(kReach) : 1.f);
        star[j].Flags |= laws[j];
    }
    return star;
}
std::vector<float> Approach(uint32_t block) {
    std::vector<float> u(3 * kBlock);
    for (uint32_t j = 0; j < 3; ++j)
        for (uint32_t s = 0; s < kBlock; ++s) u[j * kBlock + s] = kReach * (std::sin(float(block * kBlock + s) * 0.016f - 0.9f * float(j)) + 0.1f);
    return u;
}
} // namespace

CASE(host_a_damping_a_carry_and_a_count_per_junction_are_required) {
    ModalAudio engine; // (never rendered: the argument check comes first)
    const ModalJunction junction = Contact(Side(0, 1, 1.f, 2.f), 1.f, ModalJunctionShared | ModalJunctionDamped);
    std::vector<float> approach(kBlock, 0.f), forces(kBlock), out(kBlock), carry(1, 0.f);
    std::vector<uint32_t> counts(1, 0u);
    const float damping = 0.f;
    int threw = 0;
    try {
        RenderModalDampedGroups(engine, {}, static_cast<const float *>(nullptr), {}, static_cast<float *>(nullptr), std::span<const ModalJunction>(&junction, 1), approach.data(),
                                std::span<const float>(&damping, 1), std::span<float>(carry), forces.data(), out.data(), kBlock, {});
    } catch (const std::invalid_argument &) { ++threw; }
    try {
        RenderModalDampedGroups(engine, {}, static_cast<const float *>(nullptr), {}, static_cast<float *>(nullptr), std::span<const ModalJunction>(&junction, 1), approach.data(),
                                std::span<const float>(&damping, 1), std::span<float>(), forces.data(), out.data(), kBlock, counts);
    } catch (const std::invalid_argument &) { ++threw; }
    try {
        RenderModalDampedGroups(engine, {}, static_cast<const float *>(nullptr), {}, static_cast<float *>(nullptr), std::span<const ModalJunction>(&junction, 1), approach.data(),
                                std::span<const float>(), std::span<float>(carry), forces.data(), out.data(), kBlock, counts);
    } catch (const std::invalid_argument &) { ++threw; }
    EXPECT(threw == 3);
}

CASE(a_damped_member_of_a_group_is_solved_by_the_damped_groups_render_alone) {
    Rig a, b, scout;
    // member 0: damped and linear; member 1: damped and Hertz; member 2: a plain Hertz junction
    const std::vector<ModalJunction> star = Star(scout.Engine, {ModalJunctionDamped, ModalJunctionDamped | ModalJunctionHertz, ModalJunctionHertz});
    size_t pressed = 0;
    std::vector<float> carry, old_carry;
    for (uint32_t i = 0; i < kBlocks; ++i) {
        const std::vector<float> u = Approach(i);
        const Block got = Run(true, a.Engine, {}, star, u.data(), kDamping, carry);
        const Block old = Run(false, b.Engine, {}, star, u.data(), kDamping, old_carry);
        carry = got.Carry, old_carry = old.Carry;
        EXPECT(got.Status == std::vector<uint8_t>({1, 1, 1}) && old.Status == std::vector<uint8_t>({1, 0, 0}));
        EXPECT(got.Counts == std::vector<uint32_t>({0, 0, 0}));
        EXPECT(std::isfinite(got.Carry[0]) && std::isfinite(got.Carry[1]) && std::isnan(got.Carry[2]));
        EXPECT(std::isfinite(old.Carry[0]) && std::isnan(old.Carry[1]) && std::isnan(old.Carry[2])); // (there member 0 is a lone damped junction)
        EXPECT(std::all_of(got.Forces.begin(), got.Forces.end(), [](float f) { return std::isfinite(f) && f >= 0; }));
        EXPECT(std::all_of(old.Forces.begin() + kBlock, old.Forces.end(), [](float f) { return f == 0; }));
        for (uint32_t j = 1; j < 3; ++j) pressed += std::any_of(got.Forces.begin() + j * kBlock, got.Forces.begin() + (j + 1) * kBlock, [](float f) { return f > 0; });
    }
    EXPECT_NOTE(pressed > 0, std::to_string(pressed)); // the members the older entry leaves out did push
}

CASE(without_a_damped_junction_in_a_group_it_is_the_mixed_render) {
    Rig a, b, scout;
    // a Hertz group of two on objects 0 and 1, and a lone damped junction on object 2
    std::vector<ModalJunction> junctions = Star(scout.Engine, {ModalJunctionHertz, 0, ModalJunctionHertz});
    junctions[1] = Contact(Side(2, 0, 1.f, 2.f), junctions[1].Stiffness, ModalJunctionShared | ModalJunctionDamped);
    const std::vector<ModalPickup> pickups{Probe(0, 2, 1, 1.5f), Probe(1, 1, 1, 1.5f), Probe(2, 3, 0)};
    std::vector<float> carry, want_carry;
    for (uint32_t i = 0; i < kBlocks; ++i) {
        const std::vector<float> u = Approach(i);
        const Block got = Run(true, a.Engine, pickups, junctions, u.data(), kDamping, carry);
        const Block want = Run(false, b.Engine, pickups, junctions, u.data(), kDamping, want_carry);
        carry = got.Carry, want_carry = want.Carry;
        EXPECT(want.Status == std::vector<uint8_t>({1, 1, 1}) && got.Status == want.Status && got.Flags == want.Flags && got.Compliance == want.Compliance);
        EXPECT(SameBits(got.Out, want.Out) && SameBits(got.Reads, want.Reads) && SameBits(got.Forces, want.Forces) && SameBits(got.Carry, want.Carry));
        EXPECT(std::isfinite(got.Carry[1]) && std::isnan(got.Carry[0]) && std::isnan(got.Carry[2]));
        EXPECT(got.Counts == std::vector<uint32_t>({0, 0, 0}) && want.Counts == got.Counts);
        EXPECT(SameBank(a.Engine, b.Engine));
    }
}

int main(int argc, char **argv) {
    if (argc > 1 && std::strcmp(argv[1], "--host") == 0) std::erase_if(check::cases(), [](const check::Case &c) { return c.name.rfind("host_", 0) != 0; });
    return check::run_all();
}
