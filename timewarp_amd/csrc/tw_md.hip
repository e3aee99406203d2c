// Analytic forces of the AMBER-style potential of tw_energy.hip, and Langevin dynamics on them: one workgroup per
// conformation (one wave up to 64 atoms, sixteen above), fp64 arithmetic, everything of a conformation (coordinates, velocities,
// forces, Born radii) in LDS.
//
// What this replaces: the hybrid moves of sample_with_model (utils/evaluation_utils.py:439-466 `openmm_step`, called from
// :558-565, :594-602, :623-626) advance a state by `num_openmm_steps` steps of the OpenMM integrator that
// simulation/md.py:213-231 builds (LangevinMiddleIntegrator, or LangevinIntegrator for the oldest datasets; 310 K,
// friction 0.3 / ps, 0.5 fs, md.py:75-93).  OpenMM is a third-party dependency that is not vendored in the reference; the
// functional forms (tw_amber.h) and the integrators below restate its published Reference-platform algorithms (the gradients as
// ReferenceBondForce / AngleBondIxn / ProperDihedralBond / LJCoulombIxn / ReferenceObc::computeBornEnergyForces; the integrators as
// ReferenceLangevinMiddleDynamics, ReferenceStochasticDynamics).  Pinned: the forces against the reference's own OpenMM known-answer file
// (tests/golden/energy_kat_2olx.npz, 40 x 65 x 3 components) and against finite differences of oracle/energy_oracle.c.
// The integrators draw their own Gaussian noise (counter-based, per conformation / step / atom): trajectories are
// statistically, not bitwise, those of OpenMM.
#include "tw_amber.h"

namespace tw {

// F[3 a + c] += v (LDS, fp64 atomics: ds_add_f64)
__device__ __forceinline__ void facc(double* F, int a, double fx, double fy, double fz) {
  atomicAdd(F + 3 * a, fx);
  atomicAdd(F + 3 * a + 1, fy);
  atomicAdd(F + 3 * a + 2, fz);
}

// Bonded terms and 1-4 exceptions of one conformation on ONE wave: energies into the caller's running sum e (by reference: a
// returned partial sum would re-associate the additions), forces into F by LDS atomics in this order.
// a pair's force g (xi - xj) on i, the opposite on j
__device__ __forceinline__ void facc_pair(double* F, int i, int j, double g, double dx, double dy, double dz) {
  facc(F, i, g * dx, g * dy, g * dz);
  facc(F, j, -g * dx, -g * dy, -g * dz);
}
__device__ __forceinline__ void amber_bonded_wave(const tw_forcefield& ff, const double* x, double* F, int lane, double& e) {
  // HarmonicBondForce
  for (int b = lane; b < ff.n_bonds; b += 64) {
    const int i = ff.bond_idx[2 * b], j = ff.bond_idx[2 * b + 1];
    const double dx = x[3 * i] - x[3 * j], dy = x[3 * i + 1] - x[3 * j + 1], dz = x[3 * i + 2] - x[3 * j + 2];
    const double r = sqrt(dx * dx + dy * dy + dz * dz);
    const double d = r - ff.bond_par[2 * b], k = ff.bond_par[2 * b + 1];
    e += harmonic_energy(k, d);
    facc_pair(F, i, j, -k * d / r, dx, dy, dz);
  }
  // HarmonicAngleForce: grad_i theta = (v0 x p) / (|v0|^2 |p|), p = v0 x v1
  for (int a = lane; a < ff.n_angles; a += 64) {
    const int i = ff.angle_idx[3 * a], j = ff.angle_idx[3 * a + 1], k = ff.angle_idx[3 * a + 2];
    const AngleGeom ag = angle_geom(x, i, j, k);
    const double *v0 = ag.v0, *v1 = ag.v1;
    const double d = ag.theta - ff.angle_par[2 * a], kk = ff.angle_par[2 * a + 1];
    e += harmonic_energy(kk, d);
    const double dE = kk * d;
    const double p[3] = {v0[1] * v1[2] - v0[2] * v1[1], v0[2] * v1[0] - v0[0] * v1[2], v0[0] * v1[1] - v0[1] * v1[0]};
    double rp = sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
    if (rp < 1e-12) rp = 1e-12;
    const double ta = -dE / (ag.d00 * rp), tc = dE / (ag.d11 * rp);
    const double fi[3] = {ta * (v0[1] * p[2] - v0[2] * p[1]), ta * (v0[2] * p[0] - v0[0] * p[2]), ta * (v0[0] * p[1] - v0[1] * p[0])};
    const double fk[3] = {tc * (v1[1] * p[2] - v1[2] * p[1]), tc * (v1[2] * p[0] - v1[0] * p[2]), tc * (v1[0] * p[1] - v1[1] * p[0])};
    facc(F, i, fi[0], fi[1], fi[2]);
    facc(F, k, fk[0], fk[1], fk[2]);
    facc(F, j, -fi[0] - fk[0], -fi[1] - fk[1], -fi[2] - fk[2]);
  }
  // PeriodicTorsionForce (gradient as OpenMM's ReferenceProperDihedralBond)
  for (int t = lane; t < ff.n_torsions; t += 64) {
    const int a = ff.torsion_idx[4 * t], b = ff.torsion_idx[4 * t + 1], c = ff.torsion_idx[4 * t + 2], d = ff.torsion_idx[4 * t + 3];
    const TorsionGeom tg = torsion_geom(x, a, b, c, d);
    const double *r0 = tg.r0, *r1 = tg.r1, *r2 = tg.r2;
    const double per = ff.torsion_par[3 * t], phase = ff.torsion_par[3 * t + 1], kk = ff.torsion_par[3 * t + 2];
    e += torsion_energy(per, phase, kk, tg.phi);
    const double dE = -kk * per * sin(per * tg.phi - phase);
    const double nbc2 = r1[0] * r1[0] + r1[1] * r1[1] + r1[2] * r1[2], nbc = sqrt(nbc2);
    const double f0 = (-dE * nbc) / fmax(tg.n0, 1e-24), f3 = (dE * nbc) / fmax(tg.n1, 1e-24);
    const double f1 = (r0[0] * r1[0] + r0[1] * r1[1] + r0[2] * r1[2]) / nbc2;
    const double f2 = (r2[0] * r1[0] + r2[1] * r1[1] + r2[2] * r1[2]) / nbc2;
    double fa[3], fd[3], fb[3], fc[3];
    for (int q = 0; q < 3; ++q) {
      fa[q] = f0 * tg.c0[q];
      fd[q] = f3 * tg.c1[q];
      const double s = f1 * fa[q] - f2 * fd[q];
      fb[q] = fa[q] - s;
      fc[q] = fd[q] + s;
    }
    facc(F, a, fa[0], fa[1], fa[2]);
    facc(F, b, -fb[0], -fb[1], -fb[2]);
    facc(F, c, -fc[0], -fc[1], -fc[2]);
    facc(F, d, fd[0], fd[1], fd[2]);
  }
  // NonbondedForce exceptions
  for (int ex = lane; ex < ff.n_exceptions; ex += 64) {
    const double qq = ff.exc_par[3 * ex], sig = ff.exc_par[3 * ex + 1], eps = ff.exc_par[3 * ex + 2];
    if (qq == 0.0 && eps == 0.0) continue;
    const int i = ff.exc_idx[2 * ex], j = ff.exc_idx[2 * ex + 1];
    const double dx = x[3 * i] - x[3 * j], dy = x[3 * i + 1] - x[3 * j + 1], dz = x[3 * i + 2] - x[3 * j + 2];
    const double r2 = dx * dx + dy * dy + dz * dz, r = sqrt(r2);
    const double sr2 = (sig / r) * (sig / r), sr6 = sr2 * sr2 * sr2;
    e += exception_energy(qq, eps, sr6, r);
    // -dE/dr / r
    facc_pair(F, i, j, (TW_ONE_4PI_EPS0 * qq / r + 4.0 * eps * (12.0 * sr6 * sr6 - 6.0 * sr6)) / r2, dx, dy, dz);
  }
}

// Forces of one conformation.  x [3V], F [3V] (zeroed here), born / dEdB / chain [V] and excl [V*V] in LDS; the wave's
// 64 lanes share the terms.  Returns this lane's share of the potential energy (sum over lanes = E).
__device__ double amber_forces_wave(const tw_forcefield& ff, const double* x, double* F, double* born, double* dEdB,
                                    double* chain, const unsigned* excl, int lane) {
  const int V = ff.n_atoms;
  for (int i = lane; i < 3 * V; i += 64) F[i] = 0.0;
  for (int i = lane; i < V; i += 64) dEdB[i] = 0.0;
  __syncthreads();
  double e = 0.0;
  amber_bonded_wave(ff, x, F, lane, e);
  // NonbondedForce pairs
  const bool use_cut = ff.cutoff > 0.0;
  const double rc = ff.cutoff;
  const double krf = use_cut ? rf_k(rc, ff.rf_dielectric) : 0.0, crf = use_cut ? rf_c(rc, ff.rf_dielectric) : 0.0;
  const int npairs = V * (V - 1) / 2;
  for (int p = lane; p < npairs; p += 64) {
    int i, j;
    pair_index(p, i, j);
    if (excl_test(excl, i * V + j)) continue;
    const double dx = x[3 * i] - x[3 * j], dy = x[3 * i + 1] - x[3 * j + 1], dz = x[3 * i + 2] - x[3 * j + 2];
    const double r2 = dx * dx + dy * dy + dz * dz, r = sqrt(r2);
    if (use_cut && r >= rc) continue;
    const NbPair nb(ff.atom_par + 5 * i, ff.atom_par + 5 * j, r2);
    e += lj_energy(nb.eps, nb.sr6) + nb.qq * rf_coulomb(use_cut, krf, crf, r, r2);
    const double g = 4.0 * nb.eps * (12.0 * nb.sr6 * nb.sr6 - 6.0 * nb.sr6) / r2 + nb.qq * (1.0 / (r2 * r) - (use_cut ? 2.0 * krf : 0.0));
    facc(F, i, g * dx, g * dy, g * dz);
    facc(F, j, -g * dx, -g * dy, -g * dz);
  }
  if (ff.has_gbsa) {
    const Obc obc(ff.has_gbsa);
    const double offset = obc.offset, probe = obc.probe, alpha = obc.alpha, beta = obc.beta, gamma = obc.gamma;
    // Born radii and dB_i / dI_i (I_i = the pair sum below)
    for (int i = lane; i < V; i += 64) {
      const double rad_i = ff.atom_par[5 * i + 3], off_i = rad_i - offset;
      double sum = 0.0;
      for (int j = 0; j < V; ++j) {
        if (j == i) continue;
        const double dx = x[3 * i] - x[3 * j], dy = x[3 * i + 1] - x[3 * j + 1], dz = x[3 * i + 2] - x[3 * j + 2];
        const double r = sqrt(dx * dx + dy * dy + dz * dz);
        if (use_cut && r > rc) continue;
        const double sr_j = (ff.atom_par[5 * j + 3] - offset) * ff.atom_par[5 * j + 4];
        const double r_sr = r + sr_j;
        if (off_i < r_sr) {
          const double rinv = 1.0 / r, ad = fabs(r - sr_j);
          const double l = 1.0 / (off_i > ad ? off_i : ad), u = 1.0 / r_sr, l2 = l * l, u2 = u * u;
          double term = l - u + 0.25 * r * (u2 - l2) + 0.5 * rinv * log(u / l) + 0.25 * sr_j * sr_j * rinv * (l2 - u2);
          if (off_i < (sr_j - r)) term += 2.0 * (1.0 / off_i - l);
          sum += term;
        }
      }
      const double s = 0.5 * off_i * sum, s2 = s * s;
      const double th = tanh(alpha * s - beta * s2 + gamma * s * s2);
      const double B = 1.0 / (1.0 / off_i - th / rad_i);
      born[i] = B;
      chain[i] = B * B * (1.0 - th * th) * (alpha - 2.0 * beta * s + 3.0 * gamma * s2) * 0.5 * off_i / rad_i;  // dB / dI
    }
    __syncthreads();
    const GbEnergy gb(ff);
    const double pre = gb.pre;
    for (int i = lane; i < V; i += 64) {
      const double rad = ff.atom_par[5 * i + 3], B = born[i], q = ff.atom_par[5 * i];
      double dB = 0.0;
      if (B > 0.0) {
        const double ace = gb.ace(obc, rad, B);
        e += ace;
        dB += -6.0 * ace / B;
      }
      e += gb.self(q, B);
      dB += -0.5 * pre * q * q / (B * B);
      atomicAdd(dEdB + i, dB);
    }
    for (int p = lane; p < npairs; p += 64) {
      int i, j;
      pair_index(p, i, j);
      const double dx = x[3 * i] - x[3 * j], dy = x[3 * i + 1] - x[3 * j + 1], dz = x[3 * i + 2] - x[3 * j + 2];
      const double r2 = dx * dx + dy * dy + dz * dz;
      if (use_cut && sqrt(r2) > rc) continue;
      const double a2 = born[i] * born[j], D = r2 / (4.0 * a2), ex = exp(-D);
      const double den2 = r2 + a2 * ex, den = sqrt(den2);
      const double qq = pre * ff.atom_par[5 * i] * ff.atom_par[5 * j];
      e += qq / den - (use_cut ? qq / rc : 0.0);
      const double inv3 = qq / (den2 * den);
      const double g = inv3 * (1.0 - 0.25 * ex);            // -dE/dr / r
      facc(F, i, g * dx, g * dy, g * dz);
      facc(F, j, -g * dx, -g * dy, -g * dz);
      const double dEda = -0.5 * inv3 * ex * (1.0 + D);     // dE / d(B_i B_j)
      atomicAdd(dEdB + i, dEda * born[j]);
      atomicAdd(dEdB + j, dEda * born[i]);
    }
    __syncthreads();
    // chain rule through the Born radii: E depends on x through I_i(r_ij)
    for (int p = lane; p < V * V; p += 64) {
      const int i = p / V, j = p - i * V;
      if (i == j) continue;
      const double rad_i = ff.atom_par[5 * i + 3], off_i = rad_i - offset;
      const double dx = x[3 * i] - x[3 * j], dy = x[3 * i + 1] - x[3 * j + 1], dz = x[3 * i + 2] - x[3 * j + 2];
      const double r2 = dx * dx + dy * dy + dz * dz, r = sqrt(r2);
      if (use_cut && r > rc) continue;
      const double s = (ff.atom_par[5 * j + 3] - offset) * ff.atom_par[5 * j + 4];
      if (!(off_i < r + s)) continue;
      const double ad = fabs(r - s);
      const bool moving = ad >= off_i;                       // l = 1 / |r - s| follows r; otherwise l = 1 / off_i is constant
      const double l = 1.0 / (moving ? ad : off_i), u = 1.0 / (r + s), l2 = l * l, u2 = u * u;
      const double dl = moving ? -l2 * (r >= s ? 1.0 : -1.0) : 0.0, du = -u2;
      double dT = dl - du + 0.25 * (u2 - l2) + 0.5 * r * (u * du - l * dl) - 0.5 * log(u / l) / r2 + 0.5 / r * (du / u - dl / l) -
                  0.25 * s * s / r2 * (l2 - u2) + 0.5 * s * s / r * (l * dl - u * du);
      if (off_i < (s - r)) dT += -2.0 * dl;
      const double g = -dEdB[i] * chain[i] * dT / r;         // force on i along (xi - xj)
      facc(F, i, g * dx, g * dy, g * dz);
      facc(F, j, -g * dx, -g * dy, -g * dz);
    }
  }
  __syncthreads();
  return e;
}

// The same forces with MD_W waves per conformation (r06: molecules above 64 atoms - the reference's 691-atom test protein took 12.5 ms
// per evaluation on one wave, i.e. per Langevin step).  No cross-wave atomics, so that a trajectory stays a function of its seed:
//   A  nonbonded pairs: a wave per atom i, lanes over ALL partners j (every pair is evaluated from both ends - twice the arithmetic of
//      the triangular loop, sixteen times the lanes), butterfly over the wave, F[i] = the row sum (a plain store: one owner per atom);
//      the Born radii the same way
//   B  bonded terms and 1-4 exceptions: wave 0 alone, LDS atomics as in the single-wave kernel (one wave: a fixed order)
//   C  GB pair terms: a wave per atom again - F[i] += row sum, dE/dB_i = self terms + row sum
//   D  the chain rule through the Born radii: atom a collects g_aj + g_ja from its row
// The energy: every pair counted at its j < i end; per-thread partial sums, wave butterflies, the waves' sums added in wave order.
#define MD_W 16
__device__ double amber_forces_block(const tw_forcefield& ff, const double* x, double* F, double* born, double* dEdB, double* chain,
                                     const unsigned* excl, double* part, int tid) {
  const int V = ff.n_atoms, lane = tid & 63, wave = tid >> 6;
  double e = 0.0;
  const bool use_cut = ff.cutoff > 0.0;
  const double rc = ff.cutoff;
  const double krf = use_cut ? rf_k(rc, ff.rf_dielectric) : 0.0, crf = use_cut ? rf_c(rc, ff.rf_dielectric) : 0.0;
  const Obc obc(ff.has_gbsa);
  const double offset = obc.offset, probe = obc.probe, alpha = obc.alpha, beta = obc.beta, gamma = obc.gamma;
  // ---- A: nonbonded pairs and Born radii, a wave per atom
  for (int i = wave; i < V; i += MD_W) {
    const double xi = x[3 * i], yi = x[3 * i + 1], zi = x[3 * i + 2];
    const double* pi = ff.atom_par + 5 * i;
    const double rad_i = pi[3], off_i = rad_i - offset;
    double fx = 0.0, fy = 0.0, fz = 0.0, bsum = 0.0;
    for (int j = lane; j < V; j += 64) {
      if (j == i) continue;
      const double dx = xi - x[3 * j], dy = yi - x[3 * j + 1], dz = zi - x[3 * j + 2];
      const double r2 = dx * dx + dy * dy + dz * dz, r = sqrt(r2);
      const double* pj = ff.atom_par + 5 * j;
      if (!excl_test(excl, i * V + j) && !(use_cut && r >= rc)) {
        const NbPair nb(pi, pj, r2);
        if (j < i) e += lj_energy(nb.eps, nb.sr6) + nb.qq * rf_coulomb(use_cut, krf, crf, r, r2);
        const double g = 4.0 * nb.eps * (12.0 * nb.sr6 * nb.sr6 - 6.0 * nb.sr6) / r2 + nb.qq * (1.0 / (r2 * r) - (use_cut ? 2.0 * krf : 0.0));
        fx += g * dx;
        fy += g * dy;
        fz += g * dz;
      }
      if (ff.has_gbsa && !(use_cut && r > rc)) {
        const double sr_j = (pj[3] - offset) * pj[4];
        const double r_sr = r + sr_j;
        if (off_i < r_sr) {
          const double rinv = 1.0 / r, ad = fabs(r - sr_j);
          const double l = 1.0 / (off_i > ad ? off_i : ad), u = 1.0 / r_sr, l2 = l * l, u2 = u * u;
          double term = l - u + 0.25 * r * (u2 - l2) + 0.5 * rinv * log(u / l) + 0.25 * sr_j * sr_j * rinv * (l2 - u2);
          if (off_i < (sr_j - r)) term += 2.0 * (1.0 / off_i - l);
          bsum += term;
        }
      }
    }
    fx = wsum(fx);
    fy = wsum(fy);
    fz = wsum(fz);
    bsum = wsum(bsum);
    if (lane == 0) {
      F[3 * i] = fx;
      F[3 * i + 1] = fy;
      F[3 * i + 2] = fz;
      if (ff.has_gbsa) {
        const double sb = 0.5 * off_i * bsum, s2 = sb * sb;
        const double th = tanh(alpha * sb - beta * s2 + gamma * sb * s2);
        const double B = 1.0 / (1.0 / off_i - th / rad_i);
        born[i] = B;
        chain[i] = B * B * (1.0 - th * th) * (alpha - 2.0 * beta * sb + 3.0 * gamma * s2) * 0.5 * off_i / rad_i;  // dB / dI
      }
    }
  }
  __syncthreads();
  // ---- B: bonded terms and exceptions on wave 0 (the single-wave kernel's loops)
  if (wave == 0) amber_bonded_wave(ff, x, F, lane, e);
  __syncthreads();
  if (ff.has_gbsa) {
    const GbEnergy gb(ff);
    const double pre = gb.pre;
    // ---- C: GB self and pair terms, a wave per atom
    for (int i = wave; i < V; i += MD_W) {
      const double xi = x[3 * i], yi = x[3 * i + 1], zi = x[3 * i + 2];
      const double Bi = born[i], qi = ff.atom_par[5 * i];
      double fx = 0.0, fy = 0.0, fz = 0.0, dB = 0.0;
      for (int j = lane; j < V; j += 64) {
        if (j == i) continue;
        const double dx = xi - x[3 * j], dy = yi - x[3 * j + 1], dz = zi - x[3 * j + 2];
        const double r2 = dx * dx + dy * dy + dz * dz;
        if (use_cut && sqrt(r2) > rc) continue;
        const double a2 = Bi * born[j], D = r2 / (4.0 * a2), ex = exp(-D);
        const double den2 = r2 + a2 * ex, den = sqrt(den2);
        const double qq = pre * qi * ff.atom_par[5 * j];
        if (j < i) e += qq / den - (use_cut ? qq / rc : 0.0);
        const double inv3 = qq / (den2 * den);
        const double g = inv3 * (1.0 - 0.25 * ex);            // -dE/dr / r
        fx += g * dx;
        fy += g * dy;
        fz += g * dz;
        dB += -0.5 * inv3 * ex * (1.0 + D) * born[j];         // dE / d(B_i B_j) x B_j
      }
      fx = wsum(fx);
      fy = wsum(fy);
      fz = wsum(fz);
      dB = wsum(dB);
      if (lane == 0) {
        const double rad = ff.atom_par[5 * i + 3];
        if (Bi > 0.0) {
          const double ace = gb.ace(obc, rad, Bi);
          e += ace;
          dB += -6.0 * ace / Bi;
        }
        e += gb.self(qi, Bi);
        dB += -0.5 * pre * qi * qi / (Bi * Bi);
        dEdB[i] = dB;
        F[3 * i] += fx;
        F[3 * i + 1] += fy;
        F[3 * i + 2] += fz;
      }
    }
    __syncthreads();
    // ---- D: chain rule through the Born radii; the ordered pair (i, j) pushes i by g_ij (xi - xj) and j by the opposite, so atom a
    //         collects (g_aj + g_ja) (xa - xj) over its row
    for (int a = wave; a < V; a += MD_W) {
      const double xa = x[3 * a], ya = x[3 * a + 1], za = x[3 * a + 2];
      const double off_a = ff.atom_par[5 * a + 3] - offset, s_a = off_a * ff.atom_par[5 * a + 4];
      const double w_a = dEdB[a] * chain[a];
      double fx = 0.0, fy = 0.0, fz = 0.0;
      for (int j = lane; j < V; j += 64) {
        if (j == a) continue;
        const double dx = xa - x[3 * j], dy = ya - x[3 * j + 1], dz = za - x[3 * j + 2];
        const double r2 = dx * dx + dy * dy + dz * dz, r = sqrt(r2);
        if (use_cut && r > rc) continue;
        const double off_j = ff.atom_par[5 * j + 3] - offset, s_j = off_j * ff.atom_par[5 * j + 4];
        const double g = -(w_a * born_pair_dterm(off_a, s_j, r, r2) + dEdB[j] * chain[j] * born_pair_dterm(off_j, s_a, r, r2)) / r;
        fx += g * dx;
        fy += g * dy;
        fz += g * dz;
      }
      fx = wsum(fx);
      fy = wsum(fy);
      fz = wsum(fz);
      if (lane == 0) {
        F[3 * a] += fx;
        F[3 * a + 1] += fy;
        F[3 * a + 2] += fz;
      }
    }
  }
  // ---- the energy: waves' sums in wave order
  e = wsum(e);
  if (lane == 0) part[wave] = e;
  __syncthreads();
  double total = 0.0;
  for (int w = 0; w < MD_W; ++w) total += part[w];
  return total;
}

struct MdLds {
  double *x, *F, *born, *dEdB, *chain, *v, *part;
  unsigned* excl;
};
__device__ __forceinline__ MdLds md_carve(double* smd, int V, bool with_v) {
  MdLds m;
  m.x = smd;
  m.F = m.x + 3 * V;
  m.born = m.F + 3 * V;
  m.dEdB = m.born + V;
  m.chain = m.dEdB + V;
  m.v = m.chain + V;
  m.part = m.v + (with_v ? 3 * V : 0);
  m.excl = (unsigned*)(m.part + MD_W);
  return m;
}
static size_t md_lds_bytes(int V, bool with_v) {
  size_t b = ((size_t)(9 + (with_v ? 3 : 0)) * V + MD_W) * sizeof(double) + excl_bytes(V);
  return (b + 15) / 16 * 16;
}
// W = 1: one wave per conformation (up to 64 atoms), the result is this lane's share of E; W = MD_W: amber_forces_block, E itself
template <int W>
__device__ __forceinline__ double md_forces(const tw_forcefield& ff, const MdLds& m, int tid) {
  if constexpr (W == 1) return amber_forces_wave(ff, m.x, m.F, m.born, m.dEdB, m.chain, m.excl, tid);
  else return amber_forces_block(ff, m.x, m.F, m.born, m.dEdB, m.chain, m.excl, m.part, tid);
}
// E in every lane from what md_forces returned
template <int W>
__device__ __forceinline__ double md_total(double e) {
  if constexpr (W == 1) e = wsum(e);
  return e;
}
// sum over the workgroup, the same bits in every thread: wave butterflies, then the waves' sums in wave order
template <int W>
__device__ __forceinline__ double md_bsum(const MdLds& m, double v, int tid) {
  v = wsum(v);
  if constexpr (W > 1) {
    if ((tid & 63) == 0) m.part[tid >> 6] = v;
    __syncthreads();
    v = 0.0;
    for (int w = 0; w < W; ++w) v += m.part[w];
    __syncthreads();  // part[] is the force kernel's again
  }
  return v;
}

template <int W>
__global__ void __launch_bounds__(64 * W) amber_forces_kernel(const tw_forcefield ff, const float* __restrict__ coords,
                                                               double* __restrict__ out_energy, double* __restrict__ out_forces) {
  extern __shared__ __attribute__((aligned(16))) double smd[];
  constexpr int NTH = 64 * W;
  const int V = ff.n_atoms, lane = threadIdx.x;
  const int64_t n = blockIdx.x;
  MdLds m = md_carve(smd, V, false);
  for (int i = lane; i < 3 * V; i += NTH) m.x[i] = (double)coords[n * 3 * V + i];
  excl_fill(ff.exc_idx, ff.n_exceptions, V, m.excl, lane, NTH);
  const double e = md_total<W>(md_forces<W>(ff, m, lane));
  __syncthreads();
  if (out_energy && lane == 0) out_energy[n] = e;
  for (int i = lane; i < 3 * V; i += NTH) out_forces[n * 3 * V + i] = m.F[i];
}

// counter-based standard normal: splitmix64 of (seed, conformation, step, atom-component) -> two uniforms -> Box-Muller; the step is the
// 64-bit first_step + s of the C ABI (restated in tests/langevin_oracle.py)
__device__ __forceinline__ unsigned long long md_mix(unsigned long long z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ double md_normal(unsigned long long seed, long long n, long long step, int idx) {
  const unsigned long long k = md_mix(seed ^ md_mix((unsigned long long)n * 0x100000001B3ull + (unsigned long long)step) ^
                                      md_mix(0xD6E8FEB86659FD93ull * (unsigned long long)(idx + 1)));
  const unsigned long long k2 = md_mix(k);
  const double u1 = ((double)(k >> 11) + 1.0) * (1.0 / 9007199254740993.0);  // (0, 1)
  const double u2 = (double)(k2 >> 11) * (1.0 / 9007199254740992.0);
  return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}

// one step's update of x and v from the forces in m.F (the schemes are described below); shared by langevin_kernel and
// langevin_trajectory_kernel so that both produce the same stream bit for bit
template <int NTH>
__device__ __forceinline__ void md_update(const MdLds& m, const float* __restrict__ masses, int V, int lane, long long n, long long step,
                                          double dt, double friction, double kbT, int scheme, unsigned long long seed, double a,
                                          double fscale) {
  for (int i = lane; i < 3 * V; i += NTH) {
    const double mass = (double)masses[i / 3];
    const double noise = friction > 0.0 ? md_normal(seed, n, step, i) : 0.0;
    double v = m.v[i], xx = m.x[i];
    if (scheme == 0) {
      v += dt * m.F[i] / mass;
      xx += 0.5 * dt * v;
      v = a * v + sqrt((1.0 - a * a) * kbT / mass) * noise;
      xx += 0.5 * dt * v;
    } else {
      v = a * v + fscale * m.F[i] / mass + sqrt(kbT * (1.0 - a * a) / mass) * noise;
      xx += dt * v;
    }
    m.v[i] = v;
    m.x[i] = xx;
  }
}

// scheme 0: LangevinMiddleIntegrator (leapfrog "LF-middle": v += dt F / m; x += dt/2 v; v <- a v + sqrt(1 - a^2) sqrt(kT/m) N;
//           x += dt/2 v;  a = exp(-friction dt));  velocities live at the half step, as in OpenMM
// scheme 1: LangevinIntegrator of OpenMM <= 7.x:  v <- a v + (1 - a) / friction F / m + sqrt(kT (1 - a^2) / m) N;  x += dt v
// friction == 0 in either scheme is plain leapfrog (used by the energy-conservation test).
template <int W>
__global__ void __launch_bounds__(64 * W) langevin_kernel(const tw_forcefield ff, const float* __restrict__ masses, float* __restrict__ coords,
                                                           float* __restrict__ velocs, int n_steps, double dt, double friction, double kbT,
                                                           int scheme, unsigned long long seed, long long step0, double* __restrict__ out_energy) {
  extern __shared__ __attribute__((aligned(16))) double smd[];
  constexpr int NTH = 64 * W;
  const int V = ff.n_atoms, lane = threadIdx.x;
  const int64_t n = blockIdx.x;
  MdLds m = md_carve(smd, V, true);
  for (int i = lane; i < 3 * V; i += NTH) {
    m.x[i] = (double)coords[n * 3 * V + i];
    m.v[i] = (double)velocs[n * 3 * V + i];
  }
  excl_fill(ff.exc_idx, ff.n_exceptions, V, m.excl, lane, NTH);
  const double a = friction > 0.0 ? exp(-friction * dt) : 1.0;
  const double fscale = friction > 0.0 ? (1.0 - a) / friction : dt;
  double e = 0.0;
  for (int s = 0; s < n_steps; ++s) {
    e = md_forces<W>(ff, m, lane);
    __syncthreads();
    md_update<NTH>(m, masses, V, lane, n, step0 + s, dt, friction, kbT, scheme, seed, a, fscale);
    __syncthreads();
  }
  for (int i = lane; i < 3 * V; i += NTH) {
    coords[n * 3 * V + i] = (float)m.x[i];
    velocs[n * 3 * V + i] = (float)m.v[i];
  }
  if (out_energy) {  // potential energy at the positions the LAST force evaluation saw (before the last update)
    e = md_total<W>(e);
    if (lane == 0) out_energy[n] = e;
  }
}

// The recording variant (tw_langevin_trajectory): the same loop, and at every step r of `report_steps` (strictly increasing, 0 <= r <=
// n_steps, counted from the start of this launch; walked with one running index) frame k of row n: x_r, v_r as float32, F(x_r) as
// float32, [E_pot(x_r), 1/2 sum m v_r^2] as fp64.  The force evaluation at the top of step r IS F(x_r), E(x_r): the frame is written
// after it and before the update; only r == n_steps costs one evaluation more, after the loop.  E_kin: per-thread partial sums, wave
// butterflies, the waves' sums added in wave order (md_bsum's sum, in line: through md_bsum the sixteen-wave kernel is scheduled
// differently) - no atomics, a frame is a function of the seed.  state64 (may be NULL)
// [n_rows, 2, V, 3] carries x, v between launches in fp64: read instead of coords / velocs, written back at the end.  (The state load
// and store stand in line here and in langevin_kernel: as a shared pair of functions they changed the registers, the scratch and the
// compares of both kernels.)
// FULL (tw_langevin_trajectory_opts with TW_RECORD_FULL_STEP_VELOCITIES): the recorded velocity - and E_kin with it - is the stored one
// moved by half a kick of the frame's own forces, v + (dt/2) F / m in fp64, rounded to float32 once at the store.  m.v itself is not
// written: the integration, the carry and the returned state are those of FULL = false.  FULL = false is the code of before.
template <int W, bool FULL>
__device__ __forceinline__ void md_record(const MdLds& m, const float* __restrict__ masses, int V, int lane, double e, double dt,
                                          int64_t frame, float* __restrict__ out_x, float* __restrict__ out_v, float* __restrict__ out_f,
                                          double* __restrict__ out_e) {
  constexpr int NTH = 64 * W;
  e = md_total<W>(e);
  double ek = 0.0;
  for (int i = lane; i < 3 * V; i += NTH) {
    double v = m.v[i];
    if constexpr (FULL) v += 0.5 * dt * m.F[i] / (double)masses[i / 3];
    ek += 0.5 * (double)masses[i / 3] * v * v;
    out_x[frame * 3 * V + i] = (float)m.x[i];
    out_v[frame * 3 * V + i] = (float)v;
    out_f[frame * 3 * V + i] = (float)m.F[i];
  }
  ek = wsum(ek);
  if constexpr (W > 1) {
    if ((lane & 63) == 0) m.part[lane >> 6] = ek;
    __syncthreads();
    ek = 0.0;
    for (int w = 0; w < W; ++w) ek += m.part[w];
    __syncthreads();  // part[] is the force kernel's again
  }
  if (lane == 0) {
    out_e[2 * frame] = e;
    out_e[2 * frame + 1] = ek;
  }
}

template <int W, bool FULL>
__global__ void __launch_bounds__(64 * W)
    langevin_trajectory_kernel(const tw_forcefield ff, const float* __restrict__ masses, float* __restrict__ coords, float* __restrict__ velocs,
                               double* __restrict__ state64, int n_steps, double dt, double friction, double kbT, int scheme,
                               unsigned long long seed, long long step0, const int* __restrict__ report_steps, int n_frames,
                               float* __restrict__ out_x, float* __restrict__ out_v, float* __restrict__ out_f, double* __restrict__ out_e) {
  extern __shared__ __attribute__((aligned(16))) double smd[];
  constexpr int NTH = 64 * W;
  const int V = ff.n_atoms, lane = threadIdx.x;
  const int64_t n = blockIdx.x;
  MdLds m = md_carve(smd, V, true);
  for (int i = lane; i < 3 * V; i += NTH) {
    m.x[i] = state64 ? state64[n * 6 * V + i] : (double)coords[n * 3 * V + i];
    m.v[i] = state64 ? state64[n * 6 * V + 3 * V + i] : (double)velocs[n * 3 * V + i];
  }
  excl_fill(ff.exc_idx, ff.n_exceptions, V, m.excl, lane, NTH);
  const double a = friction > 0.0 ? exp(-friction * dt) : 1.0;
  const double fscale = friction > 0.0 ? (1.0 - a) / friction : dt;
  int k = 0;
  int next = n_frames > 0 ? report_steps[0] : -1;   // the same in every lane: the branches on it are workgroup-uniform
  double e = 0.0;
  for (int s = 0; s < n_steps; ++s) {
    e = md_forces<W>(ff, m, lane);
    __syncthreads();
    if (s == next) {
      md_record<W, FULL>(m, masses, V, lane, e, dt, n * n_frames + k, out_x, out_v, out_f, out_e);
      ++k;
      next = k < n_frames ? report_steps[k] : -1;
    }
    md_update<NTH>(m, masses, V, lane, n, step0 + s, dt, friction, kbT, scheme, seed, a, fscale);
    __syncthreads();
  }
  if (next == n_steps) {   // the state after the last update: the one force evaluation no step needed
    e = md_forces<W>(ff, m, lane);
    __syncthreads();
    md_record<W, FULL>(m, masses, V, lane, e, dt, n * n_frames + k, out_x, out_v, out_f, out_e);
  }
  for (int i = lane; i < 3 * V; i += NTH) {
    coords[n * 3 * V + i] = (float)m.x[i];
    velocs[n * 3 * V + i] = (float)m.v[i];
    if (state64) {
      state64[n * 6 * V + i] = m.x[i];
      state64[n * 6 * V + 3 * V + i] = m.v[i];
    }
  }
}

// ---- energy minimisation (tw_minimize): limited-memory BFGS with an Armijo backtracking line search, one workgroup per conformation.
// The algorithm is written down in include/timewarp_hip.h and restated in tests/minimize_oracle.py.  LDS: the carve of the Langevin
// kernels - m.x is the trial point the force functions read, m.F their output, m.v the search direction.  Everything that survives a
// launch is in the row's fp64 workspace:
//   [0] E  [1] ring head  [2] ring count  [3] iterations  [4] evaluations  [5] status  [6], [7] 0
//   x [3V]  g [3V]  s_0 .. s_{m-1} [m, 3V]  y_0 .. y_{m-1} [m, 3V]  rho [m]  alpha [m] (the two-loop's scratch)
// Element i of every vector - m.v included - is read and written by thread i mod NTH alone (no barrier is needed for them); m.x and m.F
// cross threads inside md_eval's barriers; the header is written by thread 0 at the end, rho and alpha by thread 0 before a barrier.  Every branch below is on values that are the same in all threads of the workgroup.
#define MIN_HDR 8
#define MIN_TRIALS 21   // t, t/2, ..., t / 2^20
__host__ __device__ inline int64_t minimize_ws_len(int V, int hist) { return MIN_HDR + (int64_t)6 * V + (int64_t)hist * (6 * V + 2); }

template <int W>
__device__ __forceinline__ double md_bmax(const MdLds& m, double v, int tid) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  if constexpr (W > 1) {
    if ((tid & 63) == 0) m.part[tid >> 6] = v;
    __syncthreads();
    v = 0.0;
    for (int w = 0; w < W; ++w) v = fmax(v, m.part[w]);
    __syncthreads();
  }
  return v;
}
template <int W>
__device__ __forceinline__ double md_bdot(const MdLds& m, const double* a, const double* b, int n3, int tid) {
  double p = 0.0;
  for (int i = tid; i < n3; i += 64 * W) p += a[i] * b[i];
  return md_bsum<W>(m, p, tid);
}
// E(m.x), forces into m.F; returns E in every thread.  Barriers before (m.x was just written) and after (m.F is read next).
template <int W>
__device__ __forceinline__ double md_eval(const tw_forcefield& ff, const MdLds& m, int tid) {
  __syncthreads();
  const double e = md_total<W>(md_forces<W>(ff, m, tid));
  __syncthreads();
  return e;
}

template <int W>
__global__ void __launch_bounds__(64 * W)
    minimize_kernel(const tw_forcefield ff, float* __restrict__ coords, double* __restrict__ workspace, int fresh, int hist, int n_iterations,
                    double tolerance, double max_disp, double* __restrict__ out_energy, double* __restrict__ out_rms,
                    int* __restrict__ out_iterations, int* __restrict__ out_evaluations, int* __restrict__ out_status) {
  extern __shared__ __attribute__((aligned(16))) double smd[];
  constexpr int NTH = 64 * W;
  const int V = ff.n_atoms, n3 = 3 * V, tid = threadIdx.x;
  const int64_t n = blockIdx.x;
  MdLds m = md_carve(smd, V, true);
  double* ws = workspace + n * minimize_ws_len(V, hist);
  double* wx = ws + MIN_HDR;
  double* wg = wx + n3;
  double* wS = wg + n3;
  double* wY = wS + (int64_t)hist * n3;
  double* wrho = wY + (int64_t)hist * n3;
  double* walpha = wrho + hist;
  excl_fill(ff.exc_idx, ff.n_exceptions, V, m.excl, tid, NTH);
  double E, gg;
  int head, count, iters, evals, status;
  if (fresh) {
    for (int64_t i = tid; i < (int64_t)hist * (2 * n3 + 2); i += NTH) wS[i] = 0.0;   // S, Y, rho, alpha
    for (int i = tid; i < n3; i += NTH) {
      const double xi = (double)coords[n * n3 + i];
      wx[i] = xi;
      m.x[i] = xi;
    }
    E = md_eval<W>(ff, m, tid);
    double p = 0.0;
    for (int i = tid; i < n3; i += NTH) {
      const double gi = -m.F[i];
      wg[i] = gi;
      p += gi * gi;
    }
    gg = md_bsum<W>(m, p, tid);
    head = count = iters = 0;
    evals = 1;
    status = !(isfinite(E) && isfinite(gg)) ? 3 : (sqrt(gg / n3) <= tolerance ? 0 : 1);
  } else {
    E = ws[0];
    head = (int)ws[1], count = (int)ws[2], iters = (int)ws[3], evals = (int)ws[4], status = (int)ws[5];
    gg = md_bdot<W>(m, wg, wg, n3, tid);
    if (status == 1 && sqrt(gg / n3) <= tolerance) status = 0;
  }
  __syncthreads();   // every thread has read the header before thread 0 may rewrite it
  for (int it = 0; it < n_iterations && status == 1; ++it) {
    for (int attempt = 0; attempt < 2; ++attempt) {
      // ---- direction into m.v: two-loop recursion on q = g, d = -q
      for (int i = tid; i < n3; i += NTH) m.v[i] = wg[i];
      for (int j = 0; j < count; ++j) {   // newest to oldest
        const int k = (head - 1 - j + 2 * hist) % hist;
        const double a = wrho[k] * md_bdot<W>(m, wS + (int64_t)k * n3, m.v, n3, tid);
        if (tid == 0) walpha[k] = a;
        for (int i = tid; i < n3; i += NTH) m.v[i] -= a * wY[(int64_t)k * n3 + i];
      }
      if (count > 0) {
        const int k = (head - 1 + hist) % hist;
        const double sy = md_bdot<W>(m, wS + (int64_t)k * n3, wY + (int64_t)k * n3, n3, tid);
        const double yy = md_bdot<W>(m, wY + (int64_t)k * n3, wY + (int64_t)k * n3, n3, tid);
        const double gamma = sy / yy;
        for (int i = tid; i < n3; i += NTH) m.v[i] *= gamma;
      }
      __syncthreads();   // alpha[] written by thread 0 is read by all below
      for (int j = count - 1; j >= 0; --j) {   // oldest to newest
        const int k = (head - 1 - j + 2 * hist) % hist;
        const double b = wrho[k] * md_bdot<W>(m, wY + (int64_t)k * n3, m.v, n3, tid);
        const double c = walpha[k] - b;
        for (int i = tid; i < n3; i += NTH) m.v[i] += c * wS[(int64_t)k * n3 + i];
      }
      for (int i = tid; i < n3; i += NTH) m.v[i] = -m.v[i];
      double gd = md_bdot<W>(m, wg, m.v, n3, tid);
      if (count > 0 && !(gd < 0.0)) {   // not a descent direction: drop the history
        count = 0;
        for (int i = tid; i < n3; i += NTH) m.v[i] = -wg[i];
        gd = md_bdot<W>(m, wg, m.v, n3, tid);
      }
      double p = 0.0;
      for (int i = tid; i < n3; i += NTH) p = fmax(p, fabs(m.v[i]));
      const double dmax = md_bmax<W>(m, p, tid);
      double t = count > 0 ? 1.0 : fmin(1.0, max_disp / dmax);
      t = fmin(t, max_disp / dmax);
      // ---- line search: m.x = x + t d, one force evaluation per trial
      bool accepted = false;
      double Et = 0.0, ggt = 0.0;
      for (int h = 0; h < MIN_TRIALS; ++h) {
        for (int i = tid; i < n3; i += NTH) m.x[i] = wx[i] + t * m.v[i];
        Et = md_eval<W>(ff, m, tid);
        ++evals;
        ggt = md_bdot<W>(m, m.F, m.F, n3, tid);
        if (isfinite(Et) && isfinite(ggt) && Et <= E + 1e-4 * t * gd) {
          accepted = true;
          break;
        }
        t *= 0.5;
      }
      if (accepted) {
        // s = x' - x, y = g' - g into the ring slot at `head` (kept only if the curvature condition holds), then x <- x', g <- g'
        double psy = 0.0, pyy = 0.0;
        for (int i = tid; i < n3; i += NTH) {
          const double si = m.x[i] - wx[i], yi = -m.F[i] - wg[i];
          psy += si * yi;
          pyy += yi * yi;
        }
        const double sy = md_bsum<W>(m, psy, tid), yy = md_bsum<W>(m, pyy, tid);
        const bool push = hist > 0 && sy > 1e-10 * yy;
        for (int i = tid; i < n3; i += NTH) {
          if (push) {
            wS[(int64_t)head * n3 + i] = m.x[i] - wx[i];
            wY[(int64_t)head * n3 + i] = -m.F[i] - wg[i];
          }
          wx[i] = m.x[i];
          wg[i] = -m.F[i];
        }
        if (push) {
          if (tid == 0) wrho[head] = 1.0 / sy;
          head = (head + 1) % hist;
          count = count < hist ? count + 1 : hist;
        }
        __syncthreads();   // rho[] written by thread 0 is read by all in the next two-loop
        E = Et;
        gg = ggt;
        ++iters;
        if (sqrt(gg / n3) <= tolerance) status = 0;
        break;
      }
      if (count > 0) {
        count = 0;   // 21 rejections with a history: once more as steepest descent
      } else {
        status = 2;
        break;
      }
    }
  }
  for (int i = tid; i < n3; i += NTH) coords[n * n3 + i] = (float)wx[i];
  if (tid == 0) {
    ws[0] = E, ws[1] = (double)head, ws[2] = (double)count, ws[3] = (double)iters, ws[4] = (double)evals, ws[5] = (double)status;
    ws[6] = ws[7] = 0.0;
    if (out_energy) out_energy[n] = E;
    if (out_rms) out_rms[n] = sqrt(gg / n3);
    if (out_iterations) out_iterations[n] = iters;
    if (out_evaluations) out_evaluations[n] = evals;
    if (out_status) out_status[n] = status;
  }
}

// ---- holonomic constraints on the bonds to hydrogen (tw_langevin_trajectory_constrained, tw_apply_constraints).  The algorithm is
// written down in include/timewarp_hip.h and restated in tests/constraint_oracle.py.  A cluster - a heavy atom with one to three
// hydrogens - is solved by ONE lane in registers: no cross-lane arithmetic, no atomics, a fixed operation order.  Unused hydrogen slots
// point at the centre with inverse mass 0: their reference vector is exactly 0, their row of the velocity system is lambda = 0, and
// every loop over the slots unrolls with constant indices (no private array is ever indexed by a register).
struct ConsCluster {
  int idx[4];      // centre, h1, h2, h3 (unused: the centre; never stored through)
  double w[4];     // 1 / mass (unused: 0)
  double d2[3];    // squared constrained lengths (unused: 0)
  int k;           // hydrogens: 1 .. 3
};
__device__ __forceinline__ ConsCluster cons_load(const tw_constraints& cs, const float* __restrict__ masses, int cl) {
  ConsCluster q;
  q.idx[0] = cs.atoms[4 * cl];
  q.w[0] = 1.0 / (double)masses[q.idx[0]];
  q.k = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int h = cs.atoms[4 * cl + 1 + a];
    const bool used = h >= 0;
    q.idx[1 + a] = used ? h : q.idx[0];
    q.w[1 + a] = used ? 1.0 / (double)masses[used ? h : 0] : 0.0;
    const double d = used ? cs.lengths[3 * cl + a] : 0.0;
    q.d2[a] = d * d;
    q.k += used ? 1 : 0;
  }
  return q;
}
__device__ __forceinline__ double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
// the atoms of a cluster out of / into an array of 3V doubles
__device__ __forceinline__ void cons_gather(const ConsCluster& q, const double* src, double (&y)[4][3]) {
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int c = 0; c < 3; ++c) y[j][c] = src[3 * q.idx[j] + c];
}
// r_a = y_c - y_{h_a}; exactly 0 in unused slots (whose copy of the centre may be stale once the centre has moved)
__device__ __forceinline__ void cons_refvec(const ConsCluster& q, const double (&y)[4][3], double (&r)[3][3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int c = 0; c < 3; ++c) r[a][c] = a < q.k ? y[0][c] - y[1 + a][c] : 0.0;
}
// P(x; xref): SHAKE sweeps over the cluster's constraints in index order; returns the sweeps used, `resid` the final residual
__device__ __forceinline__ int cons_project_x(const ConsCluster& q, const double (&r)[3][3], double (&x)[4][3], double tol, int max_sweeps,
                                              double& resid) {
  int sweeps = 0;
  for (int s = 0; s < max_sweeps; ++s) {
    ++sweeps;
    bool changed = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (a < q.k) {
        const double sv[3] = {x[0][0] - x[1 + a][0], x[0][1] - x[1 + a][1], x[0][2] - x[1 + a][2]};
        const double delta = q.d2[a] - dot3(sv, sv);
        if (fabs(delta) > tol * q.d2[a]) {
          const double g = delta / (2.0 * dot3(r[a], sv) * (q.w[0] + q.w[1 + a]));
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            x[0][c] += g * q.w[0] * r[a][c];
            x[1 + a][c] -= g * q.w[1 + a] * r[a][c];
          }
          changed = true;
        }
      }
    }
    if (!changed) break;
  }
  resid = 0.0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (a < q.k) {
      const double sv[3] = {x[0][0] - x[1 + a][0], x[0][1] - x[1 + a][1], x[0][2] - x[1 + a][2]};
      resid = fmax(resid, fabs(q.d2[a] - dot3(sv, sv)) / q.d2[a]);
    }
  }
  return sweeps;
}
// Q(v; r): the 3 x 3 system (identity rows in unused slots) by Gaussian elimination without pivoting, in index order
__device__ __forceinline__ void cons_project_v(const ConsCluster& q, const double (&r)[3][3], double (&v)[4][3]) {
  double A[3][3], b[3], lam[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int c = 0; c < 3; ++c) A[a][c] = dot3(r[a], r[c]) * q.w[0];
    A[a][a] += dot3(r[a], r[a]) * q.w[1 + a];
    if (a >= q.k) A[a][a] = 1.0;
    const double dv[3] = {v[0][0] - v[1 + a][0], v[0][1] - v[1 + a][1], v[0][2] - v[1 + a][2]};
    b[a] = dot3(dv, r[a]);
  }
  const double m10 = A[1][0] / A[0][0], m20 = A[2][0] / A[0][0];
  A[1][1] -= m10 * A[0][1];
  A[1][2] -= m10 * A[0][2];
  b[1] -= m10 * b[0];
  A[2][1] -= m20 * A[0][1];
  A[2][2] -= m20 * A[0][2];
  b[2] -= m20 * b[0];
  const double m21 = A[2][1] / A[1][1];
  A[2][2] -= m21 * A[1][2];
  b[2] -= m21 * b[1];
  lam[2] = b[2] / A[2][2];
  lam[1] = (b[1] - A[1][2] * lam[2]) / A[1][1];
  lam[0] = (b[0] - A[0][1] * lam[1] - A[0][2] * lam[2]) / A[0][0];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      v[0][c] -= lam[a] * q.w[0] * r[a][c];
      v[1 + a][c] += lam[a] * q.w[1 + a] * r[a][c];
    }
}

// langevin_trajectory_kernel<W, false> with the constraint phases between the halves of md_update (whose lines stand here once more:
// the existing kernels are not touched).  xr: one more LDS array of 3V doubles behind the carve of the other kernels - the positions
// before the update, from which the reference vectors of the position projection are taken.  Phases of a step, a barrier after each:
//   A  scheme 0: v += dt F / m                      component i on thread i mod NTH
//   B  scheme 0: Q(v; r from x)                     cluster cl on thread cl mod NTH
//   C  xr = x; the rest of md_update's lines        components
//   D  P(x; xr); v += (x - x_u) / dt                clusters; the lane keeps the running maxima of residual and sweeps
template <int W>
__global__ void __launch_bounds__(64 * W)
    langevin_constrained_kernel(const tw_forcefield ff, const float* __restrict__ masses, float* __restrict__ coords, float* __restrict__ velocs,
                                double* __restrict__ state64, int n_steps, double dt, double friction, double kbT, int scheme,
                                unsigned long long seed, long long step0, const int* __restrict__ report_steps, int n_frames,
                                float* __restrict__ out_x, float* __restrict__ out_v, float* __restrict__ out_f, double* __restrict__ out_e,
                                const tw_constraints cs, int xr_offset, double* __restrict__ out_residual, int* __restrict__ out_sweeps) {
  extern __shared__ __attribute__((aligned(16))) double smd[];
  constexpr int NTH = 64 * W;
  const int V = ff.n_atoms, lane = threadIdx.x;
  const int64_t n = blockIdx.x;
  MdLds m = md_carve(smd, V, true);
  double* xr = smd + xr_offset;
  for (int i = lane; i < 3 * V; i += NTH) {
    m.x[i] = state64 ? state64[n * 6 * V + i] : (double)coords[n * 3 * V + i];
    m.v[i] = state64 ? state64[n * 6 * V + 3 * V + i] : (double)velocs[n * 3 * V + i];
  }
  excl_fill(ff.exc_idx, ff.n_exceptions, V, m.excl, lane, NTH);
  const double a = friction > 0.0 ? exp(-friction * dt) : 1.0;
  const double fscale = friction > 0.0 ? (1.0 - a) / friction : dt;
  int k = 0;
  int next = n_frames > 0 ? report_steps[0] : -1;   // the same in every lane: the branches on it are workgroup-uniform
  double e = 0.0;
  double worst_resid = 0.0;
  int worst_sweeps = 0;
  for (int s = 0; s < n_steps; ++s) {
    e = md_forces<W>(ff, m, lane);
    __syncthreads();
    if (s == next) {
      md_record<W, false>(m, masses, V, lane, e, dt, n * n_frames + k, out_x, out_v, out_f, out_e);
      ++k;
      next = k < n_frames ? report_steps[k] : -1;
    }
    if (scheme == 0) {
      for (int i = lane; i < 3 * V; i += NTH) {   // A
        const double mass = (double)masses[i / 3];
        double v = m.v[i];
        v += dt * m.F[i] / mass;
        m.v[i] = v;
      }
      __syncthreads();
      for (int cl = lane; cl < cs.n_clusters; cl += NTH) {   // B
        const ConsCluster q = cons_load(cs, masses, cl);
        double y[4][3], r[3][3];
        cons_gather(q, m.x, y);
        cons_refvec(q, y, r);
        cons_gather(q, m.v, y);
        cons_project_v(q, r, y);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j <= q.k)
#pragma unroll
            for (int c = 0; c < 3; ++c) m.v[3 * q.idx[j] + c] = y[j][c];
      }
      __syncthreads();
    }
    for (int i = lane; i < 3 * V; i += NTH) {   // C
      const double mass = (double)masses[i / 3];
      const double noise = friction > 0.0 ? md_normal(seed, n, step0 + s, i) : 0.0;
      double v = m.v[i], xx = m.x[i];
      xr[i] = xx;
      if (scheme == 0) {
        xx += 0.5 * dt * v;
        v = a * v + sqrt((1.0 - a * a) * kbT / mass) * noise;
        xx += 0.5 * dt * v;
      } else {
        v = a * v + fscale * m.F[i] / mass + sqrt(kbT * (1.0 - a * a) / mass) * noise;
        xx += dt * v;
      }
      m.v[i] = v;
      m.x[i] = xx;
    }
    __syncthreads();
    for (int cl = lane; cl < cs.n_clusters; cl += NTH) {   // D
      const ConsCluster q = cons_load(cs, masses, cl);
      double y[4][3], r[3][3];
      cons_gather(q, xr, y);
      cons_refvec(q, y, r);
      cons_gather(q, m.x, y);
      double resid;
      const int sweeps = cons_project_x(q, r, y, cs.tolerance, cs.max_sweeps, resid);
      worst_resid = fmax(worst_resid, resid);
      worst_sweeps = max(worst_sweeps, sweeps);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j <= q.k)
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const int i = 3 * q.idx[j] + c;
            m.v[i] += (y[j][c] - m.x[i]) / dt;
            m.x[i] = y[j][c];
          }
    }
    __syncthreads();
  }
  if (next == n_steps) {   // the state after the last update: the one force evaluation no step needed
    e = md_forces<W>(ff, m, lane);
    __syncthreads();
    md_record<W, false>(m, masses, V, lane, e, dt, n * n_frames + k, out_x, out_v, out_f, out_e);
  }
  for (int i = lane; i < 3 * V; i += NTH) {
    coords[n * 3 * V + i] = (float)m.x[i];
    velocs[n * 3 * V + i] = (float)m.v[i];
    if (state64) {
      state64[n * 6 * V + i] = m.x[i];
      state64[n * 6 * V + 3 * V + i] = m.v[i];
    }
  }
  if (out_residual || out_sweeps) {   // a kernel argument: uniform
    __syncthreads();                  // part[] (md_record's, the force kernel's) is free
    const double res = md_bmax<W>(m, worst_resid, lane), sw = md_bmax<W>(m, (double)worst_sweeps, lane);
    if (lane == 0) {
      if (out_residual) out_residual[n] = res;
      if (out_sweeps) out_sweeps[n] = (int)sw;
    }
  }
}

// tw_apply_constraints: one wave per row, a cluster per lane straight from and to global memory (clusters are disjoint, atoms outside
// them are not touched).  x <- P(x; xref = x), then v <- Q(v; r from the projected x) when there are velocities.
__global__ void __launch_bounds__(64)
    apply_constraints_kernel(const tw_constraints cs, const float* __restrict__ masses, int V, float* __restrict__ coords,
                             float* __restrict__ velocs, double* __restrict__ state64, double* __restrict__ out_residual) {
  const int lane = threadIdx.x;
  const int64_t n = blockIdx.x;
  double worst = 0.0;
  for (int cl = lane; cl < cs.n_clusters; cl += 64) {
    const ConsCluster q = cons_load(cs, masses, cl);
    double y[4][3], r[3][3];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int c = 0; c < 3; ++c)
        y[j][c] = state64 ? state64[n * 6 * V + 3 * q.idx[j] + c] : (double)coords[n * 3 * V + 3 * q.idx[j] + c];
    cons_refvec(q, y, r);
    double resid;
    cons_project_x(q, r, y, cs.tolerance, cs.max_sweeps, resid);
    worst = fmax(worst, resid);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j <= q.k)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          if (state64) state64[n * 6 * V + 3 * q.idx[j] + c] = y[j][c];
          else coords[n * 3 * V + 3 * q.idx[j] + c] = (float)y[j][c];
        }
    if (state64 || velocs) {
      cons_refvec(q, y, r);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c)
          y[j][c] = state64 ? state64[n * 6 * V + 3 * V + 3 * q.idx[j] + c] : (double)velocs[n * 3 * V + 3 * q.idx[j] + c];
      cons_project_v(q, r, y);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j <= q.k)
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            if (state64) state64[n * 6 * V + 3 * V + 3 * q.idx[j] + c] = y[j][c];
            else velocs[n * 3 * V + 3 * q.idx[j] + c] = (float)y[j][c];
          }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) worst = fmax(worst, __shfl_xor(worst, o));
  if (out_residual && lane == 0) out_residual[n] = worst;
}

// One conformation per workgroup: K1 on one wave up to 64 atoms, KW on MD_W waves above.  Refuses what does not fit the LDS, raises
// the kernel's LDS limit once per instantiation (hence the kernels as template arguments), launches with (*ff, args...).
template <auto K1, auto KW, typename... Args>
static int md_launch(const tw_forcefield* ff, bool with_v, const char* what, const char* per, int64_t n, hipStream_t s, Args... args) {
  const size_t shm = md_lds_bytes(ff->n_atoms, with_v);
  TW_REQUIRE(shm <= (size_t)160 * 1024, "%s: %d atoms need %zu bytes of LDS (one conformation per %s; limit 160 KiB)", what, ff->n_atoms, shm, per);
  static LdsLimit lim1, limw;
  int rc;
  if (ff->n_atoms <= 64) {   // small molecules: one wave per conformation
    if (shm > (size_t)64 * 1024 && (rc = lim1.ensure((const void*)K1, 160 * 1024))) return rc;
    hipLaunchKernelGGL(K1, dim3((unsigned)n), dim3(64), shm, s, *ff, args...);
  } else {
    if (shm > (size_t)64 * 1024 && (rc = limw.ensure((const void*)KW, 160 * 1024))) return rc;
    hipLaunchKernelGGL(KW, dim3((unsigned)n), dim3(64 * MD_W), shm, s, *ff, args...);
  }
  TW_LAUNCH_CHECK();
  return TW_OK;
}

int amber_energy_forces(const tw_forcefield* ff, const float* coords, double* out_energy, double* out_forces, int64_t n, hipStream_t s) {
  if (n == 0) return TW_OK;
  return md_launch<amber_forces_kernel<1>, amber_forces_kernel<MD_W>>(ff, false, "force kernel", "wave", n, s, coords, out_energy, out_forces);
}

int langevin_steps(const tw_forcefield* ff, const float* masses, float* coords, float* velocs, int n_steps, double dt,
                   double friction, double kbT, int scheme, unsigned long long seed, long long step0, double* out_energy,
                   int64_t n, hipStream_t s) {
  if (n == 0 || n_steps <= 0) return TW_OK;
  return md_launch<langevin_kernel<1>, langevin_kernel<MD_W>>(ff, true, "Langevin kernel", "wave", n, s, masses, coords, velocs, n_steps, dt,
                                                              friction, kbT, scheme, seed, step0, out_energy);
}

template <bool FULL>
static int launch_trajectory(const tw_forcefield* ff, const float* masses, float* coords, float* velocs, double* state64, int n_steps,
                             double dt, double friction, double kbT, int scheme, unsigned long long seed, long long step0,
                             const int* report_steps, int n_frames, float* out_x, float* out_v, float* out_f, double* out_e, int64_t n,
                             hipStream_t s) {
  return md_launch<langevin_trajectory_kernel<1, FULL>, langevin_trajectory_kernel<MD_W, FULL>>(
      ff, true, "Langevin kernel", "wave", n, s, masses, coords, velocs, state64, n_steps, dt, friction, kbT, scheme, seed, step0,
      report_steps, n_frames, out_x, out_v, out_f, out_e);
}

int langevin_trajectory(const tw_forcefield* ff, const float* masses, float* coords, float* velocs, double* state64, int n_steps, double dt,
                        double friction, double kbT, int scheme, unsigned long long seed, long long step0, const int* report_steps,
                        int n_frames, float* out_x, float* out_v, float* out_f, double* out_e, int64_t n, bool full_step, hipStream_t s) {
  if (n == 0) return TW_OK;
  return (full_step ? launch_trajectory<true> : launch_trajectory<false>)(ff, masses, coords, velocs, state64, n_steps, dt, friction, kbT,
                                                                          scheme, seed, step0, report_steps, n_frames, out_x, out_v,
                                                                          out_f, out_e, n, s);
}

// md_launch for the constrained kernel: its LDS is the Langevin kernels' carve plus xr [3V] behind it
int langevin_constrained(const tw_forcefield* ff, const float* masses, float* coords, float* velocs, double* state64, int n_steps, double dt,
                         double friction, double kbT, int scheme, unsigned long long seed, long long step0, const int* report_steps,
                         int n_frames, float* out_x, float* out_v, float* out_f, double* out_e, int64_t n, const tw_constraints* cons,
                         double* out_residual, int* out_sweeps, hipStream_t s) {
  const size_t base = md_lds_bytes(ff->n_atoms, true);
  const size_t shm = (base + (size_t)3 * ff->n_atoms * sizeof(double) + 15) / 16 * 16;
  TW_REQUIRE(shm <= (size_t)160 * 1024,
             "constrained Langevin kernel: %d atoms need %zu bytes of LDS (one conformation per workgroup, with the reference positions of "
             "the constraints; limit 160 KiB)", ff->n_atoms, shm);
  if (n == 0) return TW_OK;
  const int xr_offset = (int)(base / sizeof(double));
  static LdsLimit lim1, limw;
  int rc;
  if (ff->n_atoms <= 64) {
    if (shm > (size_t)64 * 1024 && (rc = lim1.ensure((const void*)langevin_constrained_kernel<1>, 160 * 1024))) return rc;
    hipLaunchKernelGGL(langevin_constrained_kernel<1>, dim3((unsigned)n), dim3(64), shm, s, *ff, masses, coords, velocs, state64, n_steps, dt,
                       friction, kbT, scheme, seed, step0, report_steps, n_frames, out_x, out_v, out_f, out_e, *cons, xr_offset,
                       out_residual, out_sweeps);
  } else {
    if (shm > (size_t)64 * 1024 && (rc = limw.ensure((const void*)langevin_constrained_kernel<MD_W>, 160 * 1024))) return rc;
    hipLaunchKernelGGL(langevin_constrained_kernel<MD_W>, dim3((unsigned)n), dim3(64 * MD_W), shm, s, *ff, masses, coords, velocs, state64,
                       n_steps, dt, friction, kbT, scheme, seed, step0, report_steps, n_frames, out_x, out_v, out_f, out_e, *cons,
                       xr_offset, out_residual, out_sweeps);
  }
  TW_LAUNCH_CHECK();
  return TW_OK;
}

int apply_constraints(const tw_constraints* cons, const float* masses, int n_atoms, float* coords, float* velocs, double* state64,
                      double* out_residual, int64_t n, hipStream_t s) {
  if (n == 0) return TW_OK;
  hipLaunchKernelGGL(apply_constraints_kernel, dim3((unsigned)n), dim3(64), 0, s, *cons, masses, n_atoms, coords, velocs, state64,
                     out_residual);
  TW_LAUNCH_CHECK();
  return TW_OK;
}

int64_t minimize_workspace_len(int n_atoms, int history) { return minimize_ws_len(n_atoms, history); }

int minimize(const tw_forcefield* ff, float* coords, double* workspace, int fresh, int history, int n_iterations, double tolerance,
             double max_displacement, double* out_energy, double* out_rms, int* out_iterations, int* out_evaluations, int* out_status,
             int64_t n, hipStream_t s) {
  if (n == 0) return TW_OK;
  return md_launch<minimize_kernel<1>, minimize_kernel<MD_W>>(ff, true, "minimiser", "workgroup", n, s, coords, workspace, fresh, history,
                                                              n_iterations, tolerance, max_displacement, out_energy, out_rms,
                                                              out_iterations, out_evaluations, out_status);
}

}  // namespace tw
