// The surface-contact model's entry points as the modal core sees them (reference: src/audio/SurfaceContact.h:22-73).
// The model itself (src/audio/surface/, an optional build flag in the reference, off by default) is out of scope; this
// build always links the "absent" implementation (cpp/src/surface_absent.cpp, reference SurfaceContactAbsent.cpp:6-25):
// every hook does nothing and reports nothing, so objects sound by collision alone.  The declarations are the
// reference's, so code that includes <audio/SurfaceContact.h> and calls them compiles and links unchanged.
//
// What the bank does have of it: sustained excitation.  The reference's surface renderer drives an object's modes with per-sample force
// signals through per-mode gain rows; that primitive exists here as ModalDrive / RenderModalDriven (modal/bank.hpp) -- a caller-supplied
// force signal at an excitation position along a direction, for as long as the caller keeps supplying it -- and the read side: the
// renderer's feedback reads (ReadDeflection / ReadRow over ModeReadGains: the object's modal displacement at the contact point along the
// contact normal, the point blended between three excitation positions) exist as ModalPickup / RenderModalRead, one row of reads per
// pickup and block.  The per-sample contact solve (a sample's force depending on the displacement read in the same sample) exists as
// ModalJunction / RenderModalCoupled: one contact per junction between two bank objects or an object and an exciter the caller moves --
// a linear spring, unilateral or bilateral, or (ModalJunctionHertz) the Hertzian law f = K delta^1.5 -- solved implicitly per frame on
// the device (the reference's one-channel SolveChannelStep).  The damping of a contact exists as ModalJunctionDamped / RenderModalDamped:
// the Hunt-Crossley factor max(1 + l (y - y_p), 0) on either law, sized from the pair's restitution by ContactDamping (modal/contact.hpp)
// as the reference's surface renderer sizes its DampingFactor, with one number of state per junction carried from block to block.
// What is still absent is the model on top of them: contact tracking and voices, damping inside a group of contacts that share an
// object, tangential channels, the rigid-body recoil and air-load filters of RenderObjectCoupled, and the roughness / friction signal
// generators.
#pragma once
#include "bank.hpp"

#include <entt/entity/fwd.hpp>

#include <cstdint>
#include <memory>
#include <span>

struct ModalRenderScratch; // a renderer's scratch in the reference; opaque here (the device owns all render scratch)

// Owning handles of the model's two opaque objects (defined by the model, which this build does not have).
struct SurfaceAudioState;
struct SurfaceAudioStateDelete {
    void operator()(SurfaceAudioState *state) const;
};
struct SurfaceRenderScratch;
struct SurfaceRenderScratchDelete {
    void operator()(SurfaceRenderScratch *scratch) const;
};
using SurfaceAudioStatePtr = std::unique_ptr<SurfaceAudioState, SurfaceAudioStateDelete>;
using SurfaceRenderScratchPtr = std::unique_ptr<SurfaceRenderScratch, SurfaceRenderScratchDelete>;

SurfaceAudioStatePtr MakeSurfaceAudioState(); // null without the model

// ---- called from RenderModal (the reference's audio thread)
void SurfaceAdoptVoices(ModalAudio &audio, ModalBank &bank, uint32_t frame_count);
uint32_t SurfaceVoiceCount(const ModalAudio &audio, uint32_t object);
bool SurfaceRenderObject(ModalAudio &audio, ModalRenderScratch &scratch, ModalBank &bank, uint32_t object, std::span<const uint32_t> impacts, float *out,
                         uint32_t frame_count);
void SurfaceSilenceObject(ModalAudio &audio, uint32_t object);
uint32_t SurfaceActiveVoices(const ModalAudio &audio);

// ---- called from the scene update (the reference's main thread)
void SurfaceInstallBank(ModalAudio &audio);
void RegisterSurfaceContactHandlers(entt::registry &registry);
void SurfaceUpdateContacts(entt::registry &registry);
float SurfaceRoughnessOf(const entt::registry &registry, entt::entity node);
entt::entity ContactSurfaceNode(const entt::registry &registry, entt::entity collider, entt::entity body);

// ---- called from the editor's panels
void DrawContactSurfaceControls(entt::registry &registry, entt::entity sound_entity);
void DrawSurfaceSynthControls(entt::registry &registry, entt::entity viewport);
void DrawSurfaceContactDebug(const entt::registry &registry);
