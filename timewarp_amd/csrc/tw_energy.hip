// AMBER-style potential energy on the GPU: one workgroup per conformation - four waves up to 64 atoms (r05: at 22 atoms a single
// wave spent most of its 27 us in the 21 serial iterations of the Born-radius loop with 22 of 64 lanes active; the kernel sits on
// the MH iteration's critical path since the flow's launches fill the chip), sixteen above (r06: the reference's 691-atom test
// protein took 6.2 ms on one wave - a quarter of an MH iteration at 16 proposals) - fp64 arithmetic.
//
// Replaces the OpenMM call chain behind OpenmmPotentialEnergyTorch.forward
// (utils/openmm/openmm_bridge.py:281-294 -> bgflow -> Context.getState(getEnergy=True)) for Systems
// built by simulation/md.py:128-187 (OpenMM 7.7).  The functional forms are those of tw_amber.h, which names the OpenMM
// algorithms they restate; the same maths is restated in plain C in oracle/energy_oracle.c, which is what the parity tests
// compare against.  The structure is this kernel's own: the waves, the tmat table, five separate term sums, for_pairs.
#include "tw_amber.h"

namespace tw {

// W waves per conformation.  W > 1: every loop strides over the whole workgroup.  The Born-radius sums: W = 4 (small molecules)
// computes them pair-parallel into a V x V table that one lane per atom then adds up in the single-wave kernel's order (same radii
// bit for bit); W = 16 (no room for the table) gives every atom a wave - lanes over the partners, partial sums in partner order per
// lane, a butterfly over the wave: the same sums up to the order of the fp64 additions.
template <int W>
__global__ void __launch_bounds__(64 * W) amber_energy_kernel(const tw_forcefield ff, const float* __restrict__ coords,
                                                               double* __restrict__ out, double* __restrict__ terms) {
  extern __shared__ __attribute__((aligned(16))) double smd[];
  constexpr int NTH = 64 * W;
  const int V = ff.n_atoms;
  double* x = smd;             // [V*3]
  double* born = x + 3 * V;    // [V]
  double* part = born + V;     // [W * 5] partial sums of the waves
  double* tmat = part + 5 * W; // [V*V] (W > 1 only)
  unsigned* excl = (unsigned*)(tmat + (W == 4 ? V * V : 0));  // [V*V] bits
  const int64_t n = blockIdx.x;
  const int lane = threadIdx.x;   // (thread of the workgroup)
  for (int i = lane; i < 3 * V; i += NTH) x[i] = (double)coords[n * 3 * V + i];
  excl_fill(ff.exc_idx, ff.n_exceptions, V, excl, lane, NTH);

  double e_bond = 0, e_angle = 0, e_tors = 0, e_nb = 0, e_gb = 0;

  // HarmonicBondForce: 1/2 k (r - r0)^2
  for (int b = lane; b < ff.n_bonds; b += NTH) {
    const int i = ff.bond_idx[2 * b], j = ff.bond_idx[2 * b + 1];
    const double dx = x[3 * i] - x[3 * j], dy = x[3 * i + 1] - x[3 * j + 1], dz = x[3 * i + 2] - x[3 * j + 2];
    const double r = sqrt(dx * dx + dy * dy + dz * dz);
    const double d = r - ff.bond_par[2 * b];
    e_bond += harmonic_energy(ff.bond_par[2 * b + 1], d);
  }
  // HarmonicAngleForce: 1/2 k (theta - theta0)^2
  for (int a = lane; a < ff.n_angles; a += NTH) {
    const int i = ff.angle_idx[3 * a], j = ff.angle_idx[3 * a + 1], k = ff.angle_idx[3 * a + 2];
    const double d = angle_geom(x, i, j, k).theta - ff.angle_par[2 * a];
    e_angle += harmonic_energy(ff.angle_par[2 * a + 1], d);
  }
  // PeriodicTorsionForce: k (1 + cos(n phi - phase))
  for (int t = lane; t < ff.n_torsions; t += NTH) {
    const int a = ff.torsion_idx[4 * t], b = ff.torsion_idx[4 * t + 1], c = ff.torsion_idx[4 * t + 2],
              d = ff.torsion_idx[4 * t + 3];
    const double phi = torsion_geom(x, a, b, c, d).phi;
    e_tors += torsion_energy(ff.torsion_par[3 * t], ff.torsion_par[3 * t + 1], ff.torsion_par[3 * t + 2], phi);
  }
  // NonbondedForce exceptions (1-4 pairs; 1-2/1-3 carry zeros): no cutoff, no reaction field
  for (int e = lane; e < ff.n_exceptions; e += NTH) {
    const double qq = ff.exc_par[3 * e], sig = ff.exc_par[3 * e + 1], eps = ff.exc_par[3 * e + 2];
    if (qq == 0.0 && eps == 0.0) continue;
    const int i = ff.exc_idx[2 * e], j = ff.exc_idx[2 * e + 1];
    const double dx = x[3 * i] - x[3 * j], dy = x[3 * i + 1] - x[3 * j + 1], dz = x[3 * i + 2] - x[3 * j + 2];
    const double r = sqrt(dx * dx + dy * dy + dz * dz);
    const double sr2 = (sig / r) * (sig / r), sr6 = sr2 * sr2 * sr2;
    e_nb += exception_energy(qq, eps, sr6, r);
  }
  // NonbondedForce, all non-excluded pairs inside the cutoff
  const bool use_cut = ff.cutoff > 0.0;
  const double rc = ff.cutoff;
  const double krf = use_cut ? rf_k(rc, ff.rf_dielectric) : 0.0, crf = use_cut ? rf_c(rc, ff.rf_dielectric) : 0.0;
  const int npairs = V * (V - 1) / 2;
  // every pair j < i once: up to four waves a linear pair index strided over the workgroup and decoded; sixteen waves: a wave per
  // row i, lanes over j (no decode - an fp64 square root and two loops per pair - and 238 k pairs at 691 atoms)
  auto for_pairs = [&](auto&& body) {
    if constexpr (W > 4) {
      for (int i = lane >> 6; i < V; i += W)
        for (int j = lane & 63; j < i; j += 64) body(i, j);
    } else {
      for (int p = lane; p < npairs; p += NTH) {
        int i, j;
        pair_index(p, i, j);
        body(i, j);
      }
    }
  };
  for_pairs([&](int i, int j) {
    if (excl_test(excl, i * V + j)) return;
    const double dx = x[3 * i] - x[3 * j], dy = x[3 * i + 1] - x[3 * j + 1], dz = x[3 * i + 2] - x[3 * j + 2];
    const double r2 = dx * dx + dy * dy + dz * dz;
    const double r = sqrt(r2);
    if (use_cut && r >= rc) return;
    const NbPair nb(ff.atom_par + 5 * i, ff.atom_par + 5 * j, r2);
    e_nb += lj_energy(nb.eps, nb.sr6);
    e_nb += nb.qq * rf_coulomb(use_cut, krf, crf, r, r2);
  });
  // GBSA-OBC (has_gbsa 1: OBC-II alpha=1 beta=0.8 gamma=4.85 = GBSAOBCForce / amber99_obc.xml; 2: OBC-I alpha=0.8
  // beta=0 gamma=2.909125 = implicit/obc1.xml; dielectric offset 0.009 nm, probe 0.14 nm)
  if (ff.has_gbsa) {
    const Obc obc(ff.has_gbsa);
    const double offset = obc.offset, alpha = obc.alpha, beta = obc.beta, gamma = obc.gamma;
    // one (i, j) term of atom i's pair integral (OpenMM's ReferenceObc::computeBornRadii)
    auto born_term = [&](int i, int j, double off_i) -> double {
      const double dx = x[3 * i] - x[3 * j], dy = x[3 * i + 1] - x[3 * j + 1], dz = x[3 * i + 2] - x[3 * j + 2];
      const double r = sqrt(dx * dx + dy * dy + dz * dz);
      if (use_cut && r > rc) return 0.0;
      const double off_j = ff.atom_par[5 * j + 3] - offset;
      const double sr_j = off_j * ff.atom_par[5 * j + 4];
      const double r_sr = r + sr_j;
      if (!(off_i < r_sr)) return 0.0;
      const double rinv = 1.0 / r;
      const double ad = fabs(r - sr_j);
      const double l = 1.0 / (off_i > ad ? off_i : ad);
      const double u = 1.0 / r_sr;
      const double l2 = l * l, u2 = u * u;
      const double ratio = log(u / l);
      double term = l - u + 0.25 * r * (u2 - l2) + 0.5 * rinv * ratio + 0.25 * sr_j * sr_j * rinv * (l2 - u2);
      if (off_i < (sr_j - r)) term += 2.0 * (1.0 / off_i - l);
      return term;
    };
    if constexpr (W == 4) {
      for (int p = lane; p < V * V; p += NTH) {
        const int i = p / V, j = p - i * V;
        tmat[p] = i == j ? 0.0 : born_term(i, j, ff.atom_par[5 * i + 3] - offset);
      }
      __syncthreads();
    }
    if constexpr (W > 4) {
      __syncthreads();   // (x is complete)
      for (int i = lane >> 6; i < V; i += W) {
        const double rad_i = ff.atom_par[5 * i + 3];
        const double off_i = rad_i - offset;
        double sum = 0.0;
        for (int j = lane & 63; j < V; j += 64)
          if (j != i) sum += born_term(i, j, off_i);
        sum = wsum(sum);
        sum *= 0.5 * off_i;
        const double s2 = sum * sum, s3 = sum * s2;
        const double th = tanh(alpha * sum - beta * s2 + gamma * s3);
        if ((lane & 63) == 0) born[i] = 1.0 / (1.0 / off_i - th / rad_i);
      }
    } else
    for (int i = lane; i < V; i += NTH) {
      const double rad_i = ff.atom_par[5 * i + 3];
      const double off_i = rad_i - offset;
      double sum = 0.0;
      for (int j = 0; j < V; ++j) {
        if (j == i) continue;
        if constexpr (W == 4) sum += tmat[i * V + j];
        else sum += born_term(i, j, off_i);
      }
      sum *= 0.5 * off_i;
      const double s2 = sum * sum, s3 = sum * s2;
      const double th = tanh(alpha * sum - beta * s2 + gamma * s3);
      born[i] = 1.0 / (1.0 / off_i - th / rad_i);
    }
    __syncthreads();
    const GbEnergy gb(ff);
    const double pre = gb.pre;
    for (int i = lane; i < V; i += NTH) {
      if (born[i] > 0.0) e_gb += gb.ace(obc, ff.atom_par[5 * i + 3], born[i]);
      e_gb += gb.self(ff.atom_par[5 * i], born[i]);
    }
    for_pairs([&](int i, int j) {
      const double dx = x[3 * i] - x[3 * j], dy = x[3 * i + 1] - x[3 * j + 1], dz = x[3 * i + 2] - x[3 * j + 2];
      const double r2 = dx * dx + dy * dy + dz * dz;
      if (use_cut && sqrt(r2) > rc) return;
      const double a2 = born[i] * born[j];
      const double dij = r2 / (4.0 * a2);
      const double den = sqrt(r2 + a2 * exp(-dij));
      const double qq = pre * ff.atom_par[5 * i] * ff.atom_par[5 * j];
      double e = qq / den;
      if (use_cut) e -= qq / rc;
      e_gb += e;
    });
  }
  e_bond = wsum(e_bond); e_angle = wsum(e_angle); e_tors = wsum(e_tors); e_nb = wsum(e_nb); e_gb = wsum(e_gb);
  if constexpr (W > 1) {   // the waves' sums, added in wave order
    if ((lane & 63) == 0) {
      double* q = part + 5 * (lane >> 6);
      q[0] = e_bond; q[1] = e_angle; q[2] = e_tors; q[3] = e_nb; q[4] = e_gb;
    }
    __syncthreads();
    if (lane == 0) {
      e_bond = e_angle = e_tors = e_nb = e_gb = 0.0;
      for (int w = 0; w < W; ++w) {
        e_bond += part[5 * w]; e_angle += part[5 * w + 1]; e_tors += part[5 * w + 2]; e_nb += part[5 * w + 3]; e_gb += part[5 * w + 4];
      }
    }
  }
  if (lane == 0) {
    out[n] = e_bond + e_angle + e_tors + e_nb + e_gb;
    if (terms) {
      terms[5 * n] = e_bond; terms[5 * n + 1] = e_angle; terms[5 * n + 2] = e_tors; terms[5 * n + 3] = e_nb;
      terms[5 * n + 4] = e_gb;
    }
  }
}

int amber_energy(const tw_forcefield* ff, const float* coords, double* out, double* terms, int64_t n, hipStream_t s) {
  if (n == 0) return TW_OK;
  const int V = ff->n_atoms;
  const bool four = V <= 64;   // small molecules: latency-bound, four waves per conformation (+ the V x V table: <= 32 KiB)
  const int W = four ? 4 : 16;
  size_t shm = (size_t)(4 * V + 5 * W + (four ? V * V : 0)) * sizeof(double) + excl_bytes(V);
  shm = (shm + 15) / 16 * 16;
  TW_REQUIRE(shm <= (size_t)160 * 1024, "energy kernel: %d atoms need %zu bytes of LDS (one conformation per workgroup; limit 160 KiB)", V, shm);
  int rc;
  if (four) {
    hipLaunchKernelGGL(amber_energy_kernel<4>, dim3((unsigned)n), dim3(256), shm, s, *ff, coords, out, terms);
  } else {
    static LdsLimit lim;
    if (shm > (size_t)64 * 1024 && (rc = lim.ensure((const void*)amber_energy_kernel<16>, 160 * 1024))) return rc;
    hipLaunchKernelGGL(amber_energy_kernel<16>, dim3((unsigned)n), dim3(1024), shm, s, *ff, coords, out, terms);
  }
  TW_LAUNCH_CHECK();
  return TW_OK;
}

}  // namespace tw
