// Sustained force drives through the mirrored API (RenderModalDriven, modal/bank.hpp), included the way a caller of the
// reference includes the bank (<audio/ModalAudio.h>): the properties tests/ModalRenderTest.cpp of the reference states
// for strikes -- superposition, renderer-count independence -- restated for drives, in both precisions, plus what is
// particular to a drive: an empty drive list is RenderModal, a drive outside the bank changes nothing, a driven object
// stays excited.  Compiles and links without a GPU; runs on one.
#include "harness.hpp"

#include <audio/ModalAudio.h>

#include <algorithm>
#include <numeric>
#include <span>

namespace {
constexpr float kRate = 48'000.f;
constexpr uint32_t kBlock = 512, kPoints = 4;

// The synthetic body of the render tests: 40 Hz x 1.031 x ordinal, decay times slowest / ordinal, trigonometric shapes
// of amplitude 0.01 on a zig-zag strip of four sample points.
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

// A deterministic force signal: a decaying two-tone scrape, different per `voice`.
std::vector<float> Scrape(uint32_t voice, uint32_t blocks) {
    std::vector<float> f(size_t(blocks) * kBlock);
    uint32_t lcg = 12345u + 977u * voice;
    for (size_t s = 0; s < f.size(); ++s) {
        lcg = lcg * 1664525u + 1013904223u;
        const float noise = float(lcg >> 8) / float(1u << 24) - 0.5f;
        f[s] = (0.6f * std::sin(float(s) * (0.013f + 0.004f * float(voice))) + 0.4f * noise) * std::exp(-float(s) / 3000.f);
    }
    return f;
}

template<typename Audio, typename Bank, typename Sample> struct RigT {
    Audio Engine;
    std::vector<uint32_t> Slots;
    RigT(uint32_t bodies, uint32_t n_modes, float slowest, uint32_t renderers) {
        const ModalModes body = LadderModes(n_modes, slowest);
        Engine.RenderPool.SetSize(renderers);
        Bank building;
        building.SampleRate = kRate;
        for (uint32_t i = 0; i < bodies; ++i) {
            const uint32_t slot = AddModalObject(building, entt::entity{i}, body);
            TuneModalObject(building, slot, body.Freqs, body.T60s);
            building.OutGain[slot] = 1;
            Slots.push_back(slot);
        }
        InstallModalBank(Engine, building);
        std::vector<Sample> first(kBlock, Sample(0));
        RenderModal(Engine, first.data(), kBlock);
    }
    // `blocks` blocks; drive j plays rows[j] (blocks * kBlock samples) from the first block on
    std::vector<Sample> Run(uint32_t blocks, std::span<const ModalDrive> drives, const std::vector<std::vector<float>> &rows) {
        std::vector<Sample> signal(size_t(blocks) * kBlock, Sample(0));
        std::vector<float> block(drives.size() * kBlock);
        for (uint32_t i = 0; i < blocks; ++i) {
            for (size_t j = 0; j < drives.size(); ++j) std::copy_n(rows[j].begin() + size_t(i) * kBlock, kBlock, block.begin() + j * kBlock);
            RenderModalDriven(Engine, drives, block.data(), signal.data() + size_t(i) * kBlock, kBlock);
        }
        return signal;
    }
};
using Rig = RigT<ModalAudio, ModalBank, float>;
using Rig64 = RigT<ModalAudio64, ModalBank64, double>;

template<typename Sample> double Loudest(const std::vector<Sample> &s) {
    return std::accumulate(s.begin(), s.end(), 0.0, [](double m, Sample v) { return std::max(m, std::abs(double(v))); });
}
template<typename Sample> double Gap(const std::vector<Sample> &a, const std::vector<Sample> &b) {
    return std::inner_product(a.begin(), a.end(), b.begin(), 0.0, [](double m, double d) { return std::max(m, d); }, [](Sample x, Sample y) { return std::abs(double(x) - double(y)); });
}

template<typename R, typename Sample> void DrivesSuperpose() {
    const std::vector<ModalDrive> voices{{0, 0, 1.f, 0.5f, 0.f}, {0, 2, -0.3f, 0.f, 0.8f}};
    const std::vector<std::vector<float>> rows{Scrape(0, 8), Scrape(1, 8)};
    const auto heard = [&](std::initializer_list<size_t> which) {
        R rig{1, 64, 0.2f, 1};
        std::vector<ModalDrive> d;
        std::vector<std::vector<float>> r;
        for (const size_t i : which) d.push_back(voices[i]), r.push_back(rows[i]);
        return rig.Run(8, d, r);
    };
    const auto first = heard({0}), second = heard({1}), both = heard({0, 1});
    std::vector<Sample> sum(first.size());
    std::transform(first.begin(), first.end(), second.begin(), sum.begin(), std::plus<Sample>{});
    EXPECT(Loudest(first) > 0 && Loudest(second) > 0);
    EXPECT_NOTE(Gap(both, sum) <= Loudest(both) * 1e-5, std::to_string(Gap(both, sum)));
}
} // namespace

CASE(drives_superpose_linearly) { DrivesSuperpose<Rig, float>(); }
CASE(drives_superpose_linearly_in_double) { DrivesSuperpose<Rig64, double>(); }

CASE(a_drive_does_not_depend_on_the_renderer_count) {
    const auto heard = [](uint32_t renderers) {
        Rig rig{16, 64, 0.2f, renderers};
        std::vector<ModalDrive> d;
        std::vector<std::vector<float>> r;
        for (const uint32_t slot : rig.Slots) d.push_back({slot, slot % kPoints, 1.f, 0.5f, 0.f}), r.push_back(Scrape(slot, 16));
        return rig.Run(16, d, r);
    };
    const auto one = heard(1), four = heard(4);
    EXPECT(Loudest(one) > 0);
    EXPECT(Gap(one, four) < Loudest(one) * 1e-5);
}

CASE(an_empty_drive_list_is_render_modal) {
    const auto heard = [](bool driven_call) {
        Rig rig{2, 64, 0.2f, 1};
        ModalEvent e;
        e.Object = rig.Slots.front(), e.Jx = 1.f, e.Jy = 0.5f, e.PulseStep = 1.f / 300.f, e.PulseGamma = 20.f;
        EnqueueModalEvent(rig.Engine, e);
        std::vector<float> signal(4 * kBlock, 0.f);
        for (uint32_t i = 0; i < 4; ++i) {
            if (driven_call) RenderModalDriven(rig.Engine, {}, nullptr, signal.data() + size_t(i) * kBlock, kBlock);
            else RenderModal(rig.Engine, signal.data() + size_t(i) * kBlock, kBlock);
        }
        return signal;
    };
    const auto plain = heard(false), driven = heard(true);
    EXPECT(Loudest(plain) > 0);
    EXPECT(plain == driven);
}

CASE(a_drive_outside_the_bank_changes_nothing_and_a_driven_object_stays_excited) {
    Rig rig{2, 64, 0.2f, 1};
    const std::vector<ModalDrive> stray{{7, 0, 1.f, 0.f, 0.f}, {0, kPoints, 1.f, 0.f, 0.f}}; // no such object; no such position
    const std::vector<std::vector<float>> rows{Scrape(0, 2), Scrape(1, 2)};
    EXPECT(Loudest(rig.Run(2, stray, rows)) == 0);
    EXPECT(LiveBank(rig.Engine).Ringing[0] == 0 && LiveBank(rig.Engine).Ringing[1] == 0);
    // silence as a drive: nothing to hear, but the object is excited -- ringing, whole tuned set live -- until the drive ends
    const std::vector<ModalDrive> hush{{1, 0, 1.f, 0.f, 0.f}};
    const std::vector<std::vector<float>> zeros{std::vector<float>(4 * kBlock, 0.f)};
    EXPECT(Loudest(rig.Run(4, hush, zeros)) == 0);
    const ModalBank &bank = LiveBank(rig.Engine);
    EXPECT(bank.Ringing[1] == 1 && bank.LiveModeCount[1] == bank.TunedModeCount[1] && bank.Ringing[0] == 0);
    std::vector<float> out(kBlock, 0.f);
    RenderModal(rig.Engine, out.data(), kBlock); // the block after the last driven one: culled and silenced by the usual rule
    EXPECT(bank.Ringing[1] == 0);
}

int main() { return check::run_all(); }
