// Pickups on junction objects through the mirrored API (RenderModalObserved, modal/bank.hpp), included the way a caller of the reference
// includes the bank (<audio/ModalAudio.h>): without a pickup on a junction object it is RenderModalDamped, bit for bit; and the pickups on
// the objects of dead junctions -- K = 0 under a lively approach, a stiff spring whose exciter is far away, a lone junction and a group of
// two -- read what RenderModalRead reads on a twin bank with zero-signal drives in the junctions' place.  The cases whose names begin with
// host_ need no GPU (`--host` runs them alone).  Compiles and links without a GPU.
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
// RenderModalObserved takes RenderModalDamped's parameters, in both precisions.
using DampedF = void (*)(ModalAudio &, std::span<const ModalDrive>, const float *, std::span<const ModalPickup>, float *, std::span<const ModalJunction>, const float *,
                         std::span<const float>, std::span<float>, float *, float *, uint32_t, uint8_t *, double *, uint8_t *);
using DampedD = void (*)(ModalAudio64 &, std::span<const ModalDrive>, const float *, std::span<const ModalPickup>, double *, std::span<const ModalJunction>, const float *,
                         std::span<const float>, std::span<double>, double *, double *, uint32_t, uint8_t *, double *, uint8_t *);
static_assert(std::is_same_v<decltype(static_cast<DampedF>(&RenderModalObserved)), decltype(static_cast<DampedF>(&RenderModalDamped))>);
static_assert(std::is_same_v<decltype(static_cast<DampedD>(&RenderModalObserved)), decltype(static_cast<DampedD>(&RenderModalDamped))>);

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
};
template<typename Entry>
Block Run(Entry entry, ModalAudio &engine, std::span<const ModalDrive> drives, const float *signals, std::span<const ModalPickup> pickups, std::span<const ModalJunction> junctions,
          const float *approach, std::span<const float> damping, std::vector<float> carry) {
    Block r;
    r.Out.assign(kBlock, 0.f), r.Reads.assign(pickups.size() * kBlock, 0.f), r.Forces.assign(junctions.size() * kBlock, 0.f);
    r.Flags.assign(pickups.size(), 0), r.Status.assign(junctions.size(), 0), r.Compliance.assign(junctions.size(), 0.0), r.Carry = std::move(carry);
    entry(engine, drives, signals, pickups, r.Reads.data(), junctions, approach, damping, std::span<float>(r.Carry), r.Forces.data(), r.Out.data(), kBlock, r.Flags.data(),
          r.Compliance.data(), r.Status.data());
    return r;
}
bool SameBits(const std::vector<float> &a, const std::vector<float> &b) { return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0); }
bool SameBank(ModalAudio &a, ModalAudio &b) {
    SyncModalState(a);
    SyncModalState(b);
    return LiveBank(a).StateRe == LiveBank(b).StateRe && LiveBank(a).StateIm == LiveBank(b).StateIm;
}
constexpr float kNoHistory = std::numeric_limits<float>::quiet_NaN();
} // namespace

CASE(host_a_damping_and_a_carry_per_junction_are_required) {
    ModalAudio engine; // (never rendered: the argument check comes first)
    const ModalJunction junction = Contact(Side(0, 1, 1.f, 2.f), 1.f, 0);
    std::vector<float> approach(kBlock, 0.f), forces(kBlock), out(kBlock);
    bool threw = false;
    try {
        RenderModalObserved(engine, {}, static_cast<const float *>(nullptr), {}, static_cast<float *>(nullptr), std::span<const ModalJunction>(&junction, 1), approach.data(), {}, {}, forces.data(),
                            out.data(), kBlock);
    } catch (const std::invalid_argument &) { threw = true; }
    EXPECT(threw);
}

CASE(without_a_pickup_on_a_junction_object_it_is_the_damped_render) {
    // a linear, a Hertz and a damped junction in turn on object 0 (two-sided with object 1 for the linear one); a drive and two pickups on object 2
    Rig a, b, scout;
    EXPECT(SameBank(a.Engine, b.Engine));
    const std::vector<ModalDrive> drives{{2, 1, 1.f, 0.5f, 0.f}};
    const std::vector<float> force = Scrape(kBlocks, 99u);
    const std::vector<ModalPickup> pickups{Probe(2, 0, 0), Probe(2, 3, 2, 1.5f)};
    const std::vector<float> still(kBlock, 0.f);
    const float zero = 0.f;
    const ModalJunction probe = Contact(Side(0, 1, 1.f, 2.f), 0.f, 0);
    const Block free = Run(static_cast<DampedF>(&RenderModalObserved), scout.Engine, {}, nullptr, std::vector<ModalPickup>{Probe(0, 1, 1, 2.f)}, std::span<const ModalJunction>(&probe, 1),
                           still.data(), std::span<const float>(&zero, 1), {kNoHistory});
    EXPECT(free.Status[0] == 1 && free.Compliance[0] > 0 && free.Flags[0] == 1);
    float x0 = 0;
    for (float v : free.Reads) x0 = std::max(x0, std::fabs(v)); // the free deflection at the contact, read through the new entry
    EXPECT(x0 > 0);
    const float k = float(3.0 / free.Compliance[0]);
    const std::vector<ModalJunction> laws{Contact(Side(0, 1, 1.f, 2.f), Side(1, 2, -1.f, 2.f), k, 0), Contact(Side(0, 1, 1.f, 2.f), k / std::sqrt(x0), ModalJunctionHertz),
                                          Contact(Side(0, 1, 1.f, 2.f), k, ModalJunctionDamped)};
    const float damping = 4.f / (x0 * kRate);
    size_t pressed = 0;
    for (const ModalJunction &junction : laws) {
        std::vector<float> carry_a{kNoHistory}, carry_b{kNoHistory};
        for (uint32_t i = 0; i < kBlocks; ++i) {
            std::vector<float> approach(kBlock);
            for (uint32_t s = 0; s < kBlock; ++s) approach[s] = x0 * (std::sin(float(i * kBlock + s) * 0.016f) + 0.1f);
            const Block want = Run(static_cast<DampedF>(&RenderModalDamped), a.Engine, drives, force.data() + size_t(i) * kBlock, pickups, std::span<const ModalJunction>(&junction, 1),
                                   approach.data(), std::span<const float>(&damping, 1), carry_a);
            const Block got = Run(static_cast<DampedF>(&RenderModalObserved), b.Engine, drives, force.data() + size_t(i) * kBlock, pickups, std::span<const ModalJunction>(&junction, 1),
                                  approach.data(), std::span<const float>(&damping, 1), carry_b);
            EXPECT(want.Status[0] == 1 && got.Status == want.Status && got.Flags == want.Flags && got.Compliance == want.Compliance);
            EXPECT(SameBits(got.Out, want.Out) && SameBits(got.Reads, want.Reads) && SameBits(got.Forces, want.Forces) && SameBits(got.Carry, want.Carry));
            EXPECT(SameBank(a.Engine, b.Engine));
            carry_a = want.Carry, carry_b = got.Carry;
            for (float f : want.Forces) pressed += f > 0;
        }
    }
    EXPECT_NOTE(pressed > 3 * kBlocks * kBlock / 20, std::to_string(pressed)); // the junctions did push
}

CASE(dead_junctions_read_what_a_twin_with_zero_drives_reads) {
    // a lone junction on object 2 and a group of two on objects 0 and 1; every object also carries a drive; pickups of all three advances
    const std::vector<ModalDrive> drives{{0, 2, 0.5f, -0.25f, 1.f}, {1, 1, 1.f, 0.5f, 0.f}, {2, 3, 0.f, 1.f, 0.5f}};
    const std::vector<ModalDrive> twin_drives{drives[0], drives[1], drives[2], {2, 1, kNormal[0], kNormal[1], kNormal[2]}, {0, 1, kNormal[0], kNormal[1], kNormal[2]},
                                              {1, 2, -kNormal[0], -kNormal[1], -kNormal[2]}, {1, 3, kNormal[0], kNormal[1], kNormal[2]}};
    const std::vector<ModalPickup> pickups{Probe(0, 1, 1, 2.f), Probe(0, 3, 0), Probe(1, 2, 2), Probe(1, 0, 1, 1.5f), Probe(2, 1, 1), Probe(2, 2, 2), Probe(2, 0, 0, 0.5f)};
    std::vector<float> force;
    for (uint32_t d = 0; d < 3; ++d) {
        const std::vector<float> one = Scrape(1, 77u + d);
        force.insert(force.end(), one.begin(), one.end());
    }
    std::vector<float> twin_force = force;
    twin_force.resize(twin_drives.size() * kBlock, 0.f);
    for (int variant = 0; variant < 2; ++variant) { // 0: K = 0 under a lively approach; 1: a stiff spring, the exciter far away
        Rig a, b;
        const float k = variant == 0 ? 0.f : 1e6f;
        const std::vector<ModalJunction> junctions{Contact(Side(2, 1, 1.f, 2.f), k, 0), Contact(Side(0, 1, 1.f, 1.f), Side(1, 2, -1.f, 1.f), k, ModalJunctionShared),
                                                   Contact(Side(1, 3, 1.f, 1.5f), k, ModalJunctionShared)};
        std::vector<float> approach = Scrape(3, 5u); // [junction][frame]
        for (float &v : approach) v = variant == 0 ? std::fabs(v) : -1e30f;
        const std::vector<float> damping(3, 0.f);
        for (uint32_t i = 0; i < 2; ++i) {
            const Block got = Run(static_cast<DampedF>(&RenderModalObserved), a.Engine, drives, force.data(), pickups, junctions, approach.data(), damping, std::vector<float>(3, kNoHistory));
            std::vector<float> reads(pickups.size() * kBlock), out(kBlock, 0.f);
            std::vector<uint8_t> flags(pickups.size(), 0);
            RenderModalRead(b.Engine, twin_drives, twin_force.data(), pickups, reads.data(), out.data(), kBlock, flags.data());
            EXPECT(std::all_of(got.Status.begin(), got.Status.end(), [](uint8_t s) { return s == 1; }));
            EXPECT(std::all_of(got.Forces.begin(), got.Forces.end(), [](float f) { return f == 0; }));
            EXPECT(std::all_of(got.Flags.begin(), got.Flags.end(), [](uint8_t f) { return f == 1; }) && got.Flags == flags);
            EXPECT(std::any_of(reads.begin(), reads.end(), [](float v) { return v != 0; }));
            EXPECT_NOTE(got.Reads == reads, "variant " + std::to_string(variant) + ", block " + std::to_string(i));
            EXPECT(got.Out == out);
            EXPECT(SameBank(a.Engine, b.Engine));
        }
    }
}

int main(int argc, char **argv) {
    if (argc > 1 && std::strcmp(argv[1], "--host") == 0) std::erase_if(check::cases(), [](const check::Case &c) { return c.name.rfind("host_", 0) != 0; });
    return check::run_all();
}
