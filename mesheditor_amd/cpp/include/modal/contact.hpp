// Hertz / flat-punch contact-time model with the reference's API (src/audio/ContactModel.h:25-98).  Scalar host code:
// it runs once per strike on the calling thread and produces ModalEvent fields.
#pragma once
#include "types.hpp"

struct ContactDynamics {
    double Mass{0};
    mat3 InverseInertia{};
    std::vector<vec3> ContactArm;
};
struct Striker {
    AcousticMaterial Material{materials::acoustic::Steel};
    float TipRadius{0.01f}, Length{0.19f};
};
struct Impactor {
    AcousticMaterialProperties Material{};
    double Curvature{0}, InvMass{0};
};

double StrikerMass(const Striker &);
Impactor StrikerImpactor(const Striker &);
mat3 InverseInertiaTensor(const MassProperties &);
double ReducedContactMass(const ContactDynamics &, uint32_t excitable_index, vec3 impact_direction, const Impactor &);
double InvEffectiveModulus(const AcousticMaterialProperties &, const AcousticMaterialProperties &);
double CombinedCurvature(double curvature_a, double curvature_b);
double ContactStiffness(double inv_effective_modulus, double combined_curvature);
double ContactPatchRadius(double normal_force, double inv_effective_modulus, double combined_curvature);
double StaticPenetration(double normal_force, double stiffness);
double SaturationPenetration(double combined_curvature, double nominal_area);
double PunchStiffness(double inv_effective_modulus, double nominal_area);
double EstimateContactTime(const ContactDynamics &, uint32_t excitable_index, vec3 impact_direction, double contact_speed,
                           const AcousticMaterialProperties &object_material, double object_curvature, double nominal_area, const Impactor &,
                           double scale_ratio, double combined_roughness = 0);
// Not in the reference's ContactModel.h: the Hunt-Crossley damping D in s/m of a contact pair with restitution e at approach speed v > 0,
// D = 1.5 max(1 - e, 0) / v -- Hunt and Crossley's relation as the reference's surface renderer sizes its damping term (DampingFactor =
// 1.5 (1 - e) ContactDamping, src/audio/surface/SurfaceAudio.cpp).  What RenderModalDamped takes per junction (modal/bank.hpp).
inline double ContactDamping(double restitution, double approach_speed) { return 1.5 * (1.0 - restitution > 0.0 ? 1.0 - restitution : 0.0) / approach_speed; }
// Not in the reference's ContactModel.h: the stick stiffness kt in N/m of a circular contact patch of radius a between bodies with the
// combined shear modulus G* (1 / G* = (2 - nu_1) / G_1 + (2 - nu_2) / G_2), kt = 8 G* a -- Mindlin's tangential compliance of a Hertz
// contact without slip.  What ModalFriction::Stiffness takes (modal/bank.hpp).
inline double TangentialStiffness(double combined_shear_modulus, double patch_radius) { return 8.0 * combined_shear_modulus * patch_radius; }
inline constexpr double MinContactTime = 2e-5, MaxContactTime = 5e-2;
