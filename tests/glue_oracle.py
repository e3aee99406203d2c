"""Float64 restatements of the small kernels that turn a flow pass into a Metropolis-Hastings decision (`tw_centre`,
`tw_kinetic_energy`, `tw_chirality_changed`), the inputs of their tests, and the noise source that makes the chirality guard fire.
TEST INFRASTRUCTURE ONLY: plain numpy / torch float64, fed the float32 values the kernels read.

Every restatement returns the value and the magnitude its error bound is made of (U = 2^-24, one float32 rounding):

  centre            masked mean `com`, `x - com` for every atom, sum_kept |x| per component.  A float32 sum of n kept terms in any
                    order carries at most (n - 1) U sum|x| (first order); the count is exact; the division adds U |com| <= U sum|x| / n:
                    |com - com64| <= U sum_kept |x|, and |xc - xc64| <= that + U |x - com| (one subtraction).
  kinetic_energy    0.5 sum m v^2 / kbT (or 0.5 sum v^2).  All terms are non-negative, so every rounding is relative to a partial
                    sum below the result: three roundings in v^2, one for the mass, n - 1 additions, one division:
                    |out - ref| <= (n + 5) U ref.
  chirality         the triple product (x1 - x0) . ((x2 - x0) x (x3 - x0)) and the sum of the absolute values of its six products.
                    Float32 evaluates it to within 8 U of that sum (three rounded differences, two products, three additions), so a
                    row whose |triple product| exceeds 16 U sum |six products| has the sign the float64 value has.
"""
import functools

import numpy as np
import torch

from tests import helpers as H

U = 2.0 ** -24
SIGN_MARGIN = 16 * U


# ---- restatements -----------------------------------------------------------------------------------------------------------------

def centre(x, masked):
    """get_centre_of_mass (utils/molecule_utils.py:15-29) and the subtraction: (com [n, 3], x - com [n, V, 3] for every atom -
    masked ones included, as the kernel writes them -, sum_kept |x| [n, 3]).  An all-masked row is 0 / 0 = NaN."""
    x = np.asarray(x, dtype=np.float64)
    keep = ~np.asarray(masked).astype(bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        com = (x * keep[:, :, None]).sum(axis=1) / keep.sum(axis=1)[:, None].astype(np.float64)
    return com, x - com[:, None, :], (np.abs(x) * keep[:, :, None]).sum(axis=1)


def kinetic_energy(v, masses, random_velocs, kbT):
    """compute_kinetic_energy (utils/evaluation_utils.py:416-436); `kbT` is taken as the float32 value the C ABI receives.
    Returns (value [n], magnitude [n]): all terms are non-negative, the magnitude is the value."""
    s = (np.asarray(v, dtype=np.float64) ** 2.0).sum(axis=-1)
    if random_velocs:
        e = 0.5 * s.sum(axis=-1)
    else:
        e = 0.5 * (np.asarray(masses, dtype=np.float64) * s).sum(axis=-1) / np.float64(np.float32(kbT))
    return e, e


def chirality(x, centres):
    """(triple product [n, C], sum of the absolute values of its six products [n, C]) (utils/chirality.py:40-62)."""
    x = np.asarray(x, dtype=np.float64)
    c = np.asarray(centres, dtype=np.int64).reshape(-1, 4)
    a, b, d = (x[:, c[:, k]] - x[:, c[:, 0]] for k in (1, 2, 3))
    six = [a[..., 0] * b[..., 1] * d[..., 2], -a[..., 0] * b[..., 2] * d[..., 1], a[..., 1] * b[..., 2] * d[..., 0],
           -a[..., 1] * b[..., 0] * d[..., 2], a[..., 2] * b[..., 0] * d[..., 1], -a[..., 2] * b[..., 1] * d[..., 0]]
    return sum(six), sum(np.abs(t) for t in six)


def changed(x, centres, ref):
    """check_symmetry_change (utils/chirality.py:65-80): any centre's sign differs from `ref`; [n] bool."""
    t, _ = chirality(x, centres)
    return (np.sign(t) != np.asarray(ref, dtype=np.float64).reshape(1, -1)).any(axis=-1)


# ---- inputs of tests/test_glue_kernels_gpu.py (asserted on in tests/test_glue_oracle_cpu.py) ---------------------------------------

ATOMS = (1, 2, 63, 64, 65, 128, 129, 192, 691)
ROWS = (1, 3, 257)
MASKS = ("none", "third", "last_only", "first_64")
ELEMENT_MASSES = np.array([1.008, 12.011, 14.007, 15.999, 32.06], dtype=np.float32)


def cloud(n_rows, n_atoms, offset, seed):
    """A molecule-sized cloud (0.3 nm) at `offset` nm, float32 [n_rows, n_atoms, 3]."""
    rng = np.random.default_rng(seed)
    return (0.3 * rng.normal(size=(n_rows, n_atoms, 3)) + offset).astype(np.float32)


def mask(kind, n_rows, n_atoms, seed):
    """uint8 [n_rows, n_atoms], or None where the kind does not exist at this size."""
    m = np.zeros((n_rows, n_atoms), dtype=np.uint8)
    if kind == "third":         # a random third, different per row; never all of a row
        m[:] = np.random.default_rng(seed).random((n_rows, n_atoms)) < 1.0 / 3.0
        m[np.arange(n_rows), (np.arange(n_rows) * 7) % n_atoms] = 0
    elif kind == "last_only":
        m[:, :-1] = 1
    elif kind == "first_64":    # a whole first pass of the 64 lanes contributes nothing
        if n_atoms < 65:
            return None
        m[:, :64] = 1
    return m


def velocities(n_rows, n_atoms, seed):
    return np.random.default_rng(seed).normal(size=(n_rows, n_atoms, 3)).astype(np.float32)


def masses_of(n_atoms, seed):
    return ELEMENT_MASSES[np.random.default_rng(seed).integers(0, len(ELEMENT_MASSES), size=n_atoms)]


CHIRALITY_ROWS = (1, 127, 128, 129, 257)
CHIRALITY_ATOMS = (4, 22, 65, 691)
CHIRALITY_CENTRES = (0, 1, 2, 5)


@functools.lru_cache(maxsize=None)
def chirality_case(n_rows, n_atoms, n_centres):
    """(launches, centres int32 [C, 4], ref float32 [C], singles).  `launches`: float32 tables [n_rows, n_atoms, 3] - one, or for
    n_rows = 1 one per kind of row, so that a case holds both outcomes.  Rows are a base conformation plus 1e-3 nm noise; rows with
    r % 5 == 3 are mirrored (x -> -x: every centre flips); `singles[c]` is a row in which only centre c is inverted, by exchanging
    the coordinates of two of its substituents.  Centre 0 reads atom 0, centre 1 atom n_atoms - 1; from 22 atoms on no two centres
    share an atom.  Reference signs are those of the base, arranged to alternate + - by the order of the last two substituents."""
    V, Cn = n_atoms, n_centres
    seed = 1000 * n_atoms + n_centres
    while True:        # a base on which no centre is near a plane (|t| > 5 % of its six products)
        rng = np.random.default_rng(seed)
        base = (0.15 * rng.normal(size=(V, 3))).astype(np.float32)
        if V == 4:
            quads = np.array([[0, 1, 2, 3], [3, 2, 1, 0], [1, 0, 3, 2], [2, 3, 0, 1], [0, 3, 1, 2]])[:Cn]
        else:
            p = 1 + rng.permutation(V - 2)
            quads = np.array([[0, p[0], p[1], p[2]], [p[3], p[4], V - 1, p[5]]] + [list(p[6 + 4 * k: 10 + 4 * k]) for k in range(3)])[:Cn]
        quads = quads.reshape(-1, 4).copy()
        t, mag = chirality(base[None], quads) if Cn else (np.ones((1, 0)), np.ones((1, 0)))
        if (np.abs(t) > 0.05 * mag).all():
            break
        seed += 7919
    for c in range(Cn):        # alternate the reference signs: + - + - +
        if np.sign(t[0, c]) != (1.0 if c % 2 == 0 else -1.0):
            quads[c, 2], quads[c, 3] = quads[c, 3], quads[c, 2]
    ref = np.sign(chirality(base[None], quads)[0][0]).astype(np.float32) if Cn else np.zeros(0, dtype=np.float32)

    def table(n, first_row):
        x = base[None] + np.float32(1e-3) * np.random.default_rng(seed + 1).normal(size=(first_row + n, V, 3)).astype(np.float32)[first_row:]
        return np.ascontiguousarray(x.astype(np.float32))

    def invert(x, r, c):
        i, j = quads[c, 1], quads[c, 2]
        x[r, [i, j]] = x[r, [j, i]]

    singles = {}
    if n_rows == 1:
        launches = [table(1, 0), table(1, 1)]
        launches[1][:, :, 0] *= -1.0
        for c in range(Cn):
            x = table(1, 2 + c)
            invert(x, 0, c)
            launches.append(x)
    else:
        x = table(n_rows, 0)
        singles = {c: 10 + 12 * c for c in range(Cn)}
        for c, r in singles.items():
            invert(x, r, c)
        mirrored = [r for r in range(n_rows) if r % 5 == 3 and r not in singles.values()]
        x[mirrored, :, 0] *= -1.0
        launches = [x]
    return launches, quads.astype(np.int32), ref, singles


def coplanar_table(n_rows=130, seed=77):
    """Integer-valued, exactly coplanar quads: every product and sum of the triple product is an integer far below 2^24, so it is
    exactly 0 in float32 (with or without fused multiply-adds) and in float64.  8 atoms, centres (0, 1, 2, 3) and (7, 6, 5, 4)."""
    rng = np.random.default_rng(seed)
    xy = rng.integers(-4, 5, size=(n_rows, 8, 2))
    a, b, c = rng.integers(-2, 3, size=(3, n_rows, 1))
    z = a * xy[..., 0] + b * xy[..., 1] + c
    x = np.concatenate([xy, z[..., None]], axis=-1).astype(np.float32)
    return x, np.array([[0, 1, 2, 3], [7, 6, 5, 4]], dtype=np.int32)


# ---- the noise that makes the guard fire ------------------------------------------------------------------------------------------

ORDINARY_SCALE = 9.1e-4      # e^-7 nm: the ordinary rows keep the noise of the other MH tests whatever the prior


class MirroredRows(H.HostNoise):
    """HostNoise whose named proposal rows are the mirror image of the state: added to their coordinate latent is m - x, x the
    float32 state [V, 3] and m = x with the first coordinate reflected through the plane x0 = mean(x[:, 0]) (computed once, in
    float32, on the host - the device and the oracle instance hand out the same numbers).  A mirror image has the AMBER energy
    of x and every chirality centre inverted.  Ordinary rows get randn * min(prior scale, 9.1e-4).  `uniform` is 0 on
    `accept_rows` (by default the mirrored rows: accepted unless p_acc is exactly 0) and 1 elsewhere (never accepted, p_acc <= 1);
    `uniforms="drawn"` draws them from the generator instead.  `first_call_only`: only the first `latents` call mirrors (the
    exploration loop: after it the explorers differ).  Rows count through the flattened [S * B] leading dimensions."""

    def __init__(self, seed, x, rows, device="cpu", first_call_only=False, accept_rows=None, uniforms="crafted"):
        super().__init__(seed, device)
        x = torch.as_tensor(x, dtype=torch.float32).reshape(-1, 3)
        m = x.clone()
        m[:, 0] = 2.0 * x[:, 0].mean() - x[:, 0]
        self.displacement = m - x
        self.rows = list(rows)
        self.accept_rows = list(rows if accept_rows is None else accept_rows)
        self.first_call_only, self.uniforms, self.calls = first_call_only, uniforms, 0

    def latents(self, S, B, V, scale_c, scale_v):
        sc = torch.clamp(torch.as_tensor(scale_c).detach().cpu().to(torch.float32), max=ORDINARY_SCALE)
        zc = torch.randn((S, B, V, 3), generator=self.g) * sc
        zv = torch.randn((S, B, V, 3), generator=self.g) * torch.as_tensor(scale_v).detach().cpu()
        if self.rows and not (self.first_call_only and self.calls > 0):
            zc.view(S * B, V, 3)[self.rows] += self.displacement
        self.calls += 1
        return zc.to(self.device), zv.to(self.device)

    def uniform(self, S):
        if self.uniforms == "drawn":
            return super().uniform(S)
        u = torch.ones(S)
        u[self.accept_rows] = 0.0
        return u.to(self.device)


# ---- the guard's scenarios on alanine dipeptide, through the CPU oracle (shared by the CPU and the GPU file) -----------------------

S_PROPOSALS = 8
MIRRORED = (2, 5)
NOISE_SEED = 3
CENTRES_ONE = ((8, 6, 9, 14),)                        # find_chirality_centers: the alpha carbon with N, HA, C
CENTRES_TWO = ((8, 6, 9, 14), (8, 6, 10, 14))         # ... and with N, CB, C


@functools.lru_cache(maxsize=None)
def alanine():
    from timewarp_amd import synthetic
    from timewarp_amd.forcefield import alanine_dipeptide_amber99sb

    types, coords, masses = synthetic.alanine_dipeptide_state()
    v0 = torch.randn(1, 22, 3, generator=torch.Generator().manual_seed(9)) * 0.05
    return types, coords, masses, v0, alanine_dipeptide_amber99sb()


def guard_arguments(guard):
    """None, or (centres int64 [C, 4], reference signs [1, C]) for guard "one", "two" (the second reference sign deliberately
    negated: every row is penalised) and "two_swapped" (the same two entries in the other order)."""
    from oracle import mh_oracle as mo

    if guard == "off":
        return None
    _, coords, _, _, _ = alanine()
    centres = torch.tensor(CENTRES_ONE if guard == "one" else CENTRES_TWO)
    signs = mo.compute_chirality_sign(coords[None], centres)
    if guard != "one":
        signs[:, 1] = -signs[:, 1]
    if guard == "two_swapped":
        centres, signs = centres.flip(0), signs.flip(1)
    return centres, signs


def chain_kwargs(random_velocs):
    kw = dict(accept=True, num_proposal_steps=S_PROPOSALS)
    if random_velocs:
        kw.update(random_velocs=True, resample_velocs=True)
    return kw


def chain_noise(device="cpu", accept=True, x=None, rows=MIRRORED, seed=NOISE_SEED, **kw):
    return MirroredRows(seed, alanine()[1] if x is None else x, rows, device=device, accept_rows=None if accept else (), **kw)


def mh_sd(random_velocs, coords_log_scale=-2.0):
    return H.mh_state_dict("scaled", random_velocs, coords_log_scale=coords_log_scale)


@functools.lru_cache(maxsize=None)
def oracle_chain(random_velocs, guard, accept, num_samples):
    """One iteration of oracle/mh_oracle.sample_with_model (C energy oracle, full-size kernel weights, 8 proposals, rows 2 and 5
    mirrored).  accept=False: u = 1 everywhere, nothing is accepted and all 8 rows are recorded."""
    from oracle import mh_oracle as mo

    types, coords, masses, v0, tables = alanine()
    kw = chain_kwargs(random_velocs)
    g = guard_arguments(guard)
    if g is not None:
        kw.update(chirality_centers=g[0], reference_signs=g[1])
    return mo.sample_with_model(types[None], coords[None], v0, torch.zeros(1, 22, dtype=torch.bool),
                                mo.OracleModel(mh_sd(random_velocs), H.FULL_KERNEL_SPEC), H.OracleAmberEnergy(tables), masses,
                                num_samples, chain_noise(accept=accept), **kw)


EXPLORE = dict(P=8, steps=2, threshold=60.0, coords_log_scale=-6.0, noise_seed=11, v_seed=4)


@functools.lru_cache(maxsize=None)
def oracle_explore(with_centres):
    from oracle import mh_oracle as mo

    types, coords, masses, _, tables = alanine()
    e = EXPLORE
    v0 = torch.randn(22, 3, generator=torch.Generator().manual_seed(e["v_seed"]))
    centres = torch.tensor(CENTRES_ONE) if with_centres else torch.zeros((0, 4), dtype=torch.int64)
    noise = MirroredRows(e["noise_seed"], coords, MIRRORED, first_call_only=True)
    return mo.explore(types[None], coords[None], v0[None], torch.zeros(1, 22, dtype=torch.bool),
                      mo.OracleModel(mh_sd(True, e["coords_log_scale"]), H.FULL_KERNEL_SPEC), H.OracleAmberEnergy(tables), centres,
                      e["steps"], e["P"], e["threshold"], noise)
