// The AMBER-style potential, each term stated once: what the energy kernel (tw_energy.hip) and the force, Langevin, trajectory and
// minimiser kernels (tw_md.hip) have in common, and the prototypes of their host entry points (tw_api.hip, tw_mh_step.hip).
//
// OpenMM is a third-party dependency that is not vendored in the reference; the functional forms below restate its published
// Reference-platform algorithms (HarmonicBondForce / ReferenceBondForce, HarmonicAngleForce / AngleBondIxn, PeriodicTorsionForce /
// ProperDihedralBond, NonbondedForce with CutoffNonPeriodic + reaction field / LJCoulombIxn, GBSAOBCForce = OBC + ACE surface term /
// ReferenceObc::computeBornRadii and ::computeBornEnergyForces).  The same maths is restated in plain C in oracle/energy_oracle.c and in
// float64 torch in tests/amber_oracle.py, on purpose independently.
//
// The order of the floating-point operations is behaviour (trajectories and checkpoints are compared bit for bit): a function here
// either returns one term that the caller adds to its own running sum, or adds into that sum through a reference - never a partial
// sum of several terms.  Every function is __forceinline__: the kernels' arithmetic is what it was when the forms stood in line.
#pragma once
#include "tw_common.h"

namespace tw {

#define TW_ONE_4PI_EPS0 138.935456  // OpenMM SimTKOpenMMRealType.h (kJ nm / (mol e^2))

int amber_energy(const tw_forcefield* ff, const float* coords, double* out, double* terms, int64_t n, hipStream_t s);
int amber_energy_forces(const tw_forcefield* ff, const float* coords, double* out_energy, double* out_forces, int64_t n, hipStream_t s);
int langevin_steps(const tw_forcefield* ff, const float* masses, float* coords, float* velocs, int n_steps, double dt,
                   double friction, double kbT, int scheme, unsigned long long seed, long long step0, double* out_energy,
                   int64_t n, hipStream_t s);
int langevin_trajectory(const tw_forcefield* ff, const float* masses, float* coords, float* velocs, double* state64, int n_steps, double dt,
                        double friction, double kbT, int scheme, unsigned long long seed, long long step0, const int* report_steps,
                        int n_frames, float* out_x, float* out_v, float* out_f, double* out_e, int64_t n, bool full_step, hipStream_t s);
int langevin_constrained(const tw_forcefield* ff, const float* masses, float* coords, float* velocs, double* state64, int n_steps, double dt,
                         double friction, double kbT, int scheme, unsigned long long seed, long long step0, const int* report_steps,
                         int n_frames, float* out_x, float* out_v, float* out_f, double* out_e, int64_t n, const tw_constraints* cons,
                         double* out_residual, int* out_sweeps, hipStream_t s);
int apply_constraints(const tw_constraints* cons, const float* masses, int n_atoms, float* coords, float* velocs, double* state64,
                      double* out_residual, int64_t n, hipStream_t s);
int64_t minimize_workspace_len(int n_atoms, int history);
int minimize(const tw_forcefield* ff, float* coords, double* workspace, int fresh, int history, int n_iterations, double tolerance,
             double max_displacement, double* out_energy, double* out_rms, int* out_iterations, int* out_evaluations, int* out_status,
             int64_t n, hipStream_t s);

#if defined(__HIPCC__) && !defined(TW_AMBER_PROTOTYPES_ONLY)   // tw_api.hip, tw_mh_step.hip: the prototypes alone
// sum over the 64 lanes of a wave, the same bits in every lane
__device__ __forceinline__ double wsum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// pair p of the triangular loop: i * (i - 1) / 2 + j = p, j < i
__device__ __forceinline__ void pair_index(int p, int& i, int& j) {
  i = (int)((sqrt(8.0 * p + 1.0) + 1.0) * 0.5);
  while (i * (i - 1) / 2 > p) --i;
  while ((i + 1) * i / 2 <= p) ++i;
  j = p - i * (i - 1) / 2;
}

// ---- HarmonicBondForce, HarmonicAngleForce: 1/2 k d^2, d = r - r0 or theta - theta0
__device__ __forceinline__ double harmonic_energy(double k, double d) { return 0.5 * k * d * d; }

// theta between v0 = xi - xj and v1 = xk - xj, clamped acos
struct AngleGeom {
  double v0[3], v1[3], d00, d11, theta;
};
__device__ __forceinline__ AngleGeom angle_geom(const double* x, int i, int j, int k) {
  AngleGeom g;
  for (int c = 0; c < 3; ++c) { g.v0[c] = x[3 * i + c] - x[3 * j + c]; g.v1[c] = x[3 * k + c] - x[3 * j + c]; }
  g.d00 = g.v0[0] * g.v0[0] + g.v0[1] * g.v0[1] + g.v0[2] * g.v0[2];
  g.d11 = g.v1[0] * g.v1[0] + g.v1[1] * g.v1[1] + g.v1[2] * g.v1[2];
  const double d01 = g.v0[0] * g.v1[0] + g.v0[1] * g.v1[1] + g.v0[2] * g.v1[2];
  double cs = d01 / sqrt(g.d00 * g.d11);
  cs = fmin(1.0, fmax(-1.0, cs));
  g.theta = acos(cs);
  return g;
}

// ---- PeriodicTorsionForce: the dihedral of a-b-c-d from c0 = r0 x r1 and c1 = r1 x r2; sign convention of OpenMM's reference
// kernel: the sign of r0 . (r1 x r2)
struct TorsionGeom {
  double r0[3], r1[3], r2[3], c0[3], c1[3], n0, n1, phi;
};
__device__ __forceinline__ TorsionGeom torsion_geom(const double* x, int a, int b, int c, int d) {
  TorsionGeom g;
  for (int q = 0; q < 3; ++q) {
    g.r0[q] = x[3 * a + q] - x[3 * b + q];
    g.r1[q] = x[3 * c + q] - x[3 * b + q];
    g.r2[q] = x[3 * c + q] - x[3 * d + q];
  }
  const double *r0 = g.r0, *r1 = g.r1, *r2 = g.r2;
  const double c0[3] = {r0[1] * r1[2] - r0[2] * r1[1], r0[2] * r1[0] - r0[0] * r1[2], r0[0] * r1[1] - r0[1] * r1[0]};
  const double c1[3] = {r1[1] * r2[2] - r1[2] * r2[1], r1[2] * r2[0] - r1[0] * r2[2], r1[0] * r2[1] - r1[1] * r2[0]};
  for (int q = 0; q < 3; ++q) { g.c0[q] = c0[q]; g.c1[q] = c1[q]; }
  g.n0 = c0[0] * c0[0] + c0[1] * c0[1] + c0[2] * c0[2];
  g.n1 = c1[0] * c1[0] + c1[1] * c1[1] + c1[2] * c1[2];
  const double dt = c0[0] * c1[0] + c0[1] * c1[1] + c0[2] * c1[2];
  double cs = dt / sqrt(g.n0 * g.n1);
  cs = fmin(1.0, fmax(-1.0, cs));
  g.phi = acos(cs);
  if (r0[0] * c1[0] + r0[1] * c1[1] + r0[2] * c1[2] < 0) g.phi = -g.phi;
  return g;
}
// k (1 + cos(n phi - phase))
__device__ __forceinline__ double torsion_energy(double per, double phase, double k, double phi) { return k * (1.0 + cos(per * phi - phase)); }

// ---- NonbondedForce
// 4 eps ((sig/r)^12 - (sig/r)^6) from sr6 = (sig/r)^6
__device__ __forceinline__ double lj_energy(double eps, double sr6) { return 4.0 * eps * (sr6 * sr6 - sr6); }
// an exception (1-4 pair; 1-2 / 1-3 carry zeros): its own qq, sig, eps; no cutoff, no reaction field
__device__ __forceinline__ double exception_energy(double qq, double eps, double sr6, double r) {
  return TW_ONE_4PI_EPS0 * qq / r + lj_energy(eps, sr6);
}
// Lorentz-Berthelot combination of two atoms' parameters (atom_par: q, sigma, epsilon, GB radius, GB scale) at squared distance r2
struct NbPair {
  double eps, sr6, qq;
  __device__ __forceinline__ NbPair(const double* pi, const double* pj, double r2) {
    const double sig = 0.5 * (pi[1] + pj[1]);
    eps = sqrt(pi[2] * pj[2]);
    const double sr2 = (sig * sig) / r2;
    sr6 = sr2 * sr2 * sr2;
    qq = TW_ONE_4PI_EPS0 * pi[0] * pj[0];
  }
};
// CutoffNonPeriodic with a reaction field (use_cut = cutoff > 0; cutoff 0: every pair, plain Coulomb): its constants k_rf and c_rf, and
// what multiplies q_i q_j / (4 pi eps0) in the energy.  Plain values, and the choice by use_cut (both constants are 0 without a cutoff)
// stays with the kernels: as a struct, or with the choice in here, every kernel tested cutoff > 0 once more.
__device__ __forceinline__ double rf_k(double rc, double eps_rf) { return (1.0 / (rc * rc * rc)) * (eps_rf - 1.0) / (2.0 * eps_rf + 1.0); }
__device__ __forceinline__ double rf_c(double rc, double eps_rf) { return (1.0 / rc) * (3.0 * eps_rf) / (2.0 * eps_rf + 1.0); }
__device__ __forceinline__ double rf_coulomb(bool use_cut, double krf, double crf, double r, double r2) {
  return use_cut ? (1.0 / r + krf * r2 - crf) : 1.0 / r;
}

// ---- GBSAOBCForce (has_gbsa 1: OBC-II alpha=1 beta=0.8 gamma=4.85 = GBSAOBCForce / amber99_obc.xml; 2: OBC-I alpha=0.8 beta=0
// gamma=2.909125 = implicit/obc1.xml; dielectric offset 0.009 nm, probe 0.14 nm)
struct Obc {
  double offset, probe, alpha, beta, gamma;
  __device__ __forceinline__ explicit Obc(int has_gbsa)
      : offset(0.009), probe(0.14), alpha(has_gbsa == 2 ? 0.8 : 1.0), beta(has_gbsa == 2 ? 0.0 : 0.8), gamma(has_gbsa == 2 ? 2.909125 : 4.85) {}
};
// d/dr of one (i, j) term of atom i's pair integral I_i (computeBornRadii; the term itself stands in the three kernels' own loops, see
// DESIGN.md 4.4): off_i = radius_i - offset of the atom whose radius is integrated, sp = (radius_j - offset) scale_j of the partner
__device__ __forceinline__ double born_pair_dterm(double off_i, double sp, double r, double r2) {
  if (!(off_i < r + sp)) return 0.0;
  const double ad = fabs(r - sp);
  const bool moving = ad >= off_i;                       // l = 1 / |r - sp| follows r; otherwise l = 1 / off_i is constant
  const double l = 1.0 / (moving ? ad : off_i), u = 1.0 / (r + sp), l2 = l * l, u2 = u * u;
  const double dl = moving ? -l2 * (r >= sp ? 1.0 : -1.0) : 0.0, du = -u2;
  double dT = dl - du + 0.25 * (u2 - l2) + 0.5 * r * (u * du - l * dl) - 0.5 * log(u / l) / r2 + 0.5 / r * (du / u - dl / l) -
              0.25 * sp * sp / r2 * (l2 - u2) + 0.5 * sp * sp / r * (l * dl - u * du);
  if (off_i < (sp - r)) dT += -2.0 * dl;
  return dT;
}
// the energy's prefactors: the self term 1/2 pre q^2 / B and the ACE non-polar term 4 pi surface_area_energy (r + probe)^2 (r / B)^6
struct GbEnergy {
  double pre, pi4a;
  __device__ __forceinline__ explicit GbEnergy(const tw_forcefield& ff)
      : pre(-TW_ONE_4PI_EPS0 * (1.0 / ff.solute_dielectric - 1.0 / ff.solvent_dielectric)),
        pi4a(4.0 * 3.14159265358979323846 * ff.surface_area_energy) {}
  __device__ __forceinline__ double ace(const Obc& obc, double rad, double B) const {   // callers: only where B > 0
    const double rr = rad + obc.probe, ratio = rad / B, r3 = ratio * ratio * ratio;
    return pi4a * rr * rr * r3 * r3;
  }
  __device__ __forceinline__ double self(double q, double B) const { return 0.5 * pre * q * q / B; }
};
#endif  // __HIPCC__ && !TW_AMBER_PROTOTYPES_ONLY

}  // namespace tw
