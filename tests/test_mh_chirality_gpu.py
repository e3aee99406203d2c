"""The chirality guard FIRES: Metropolis-Hastings iterations in which two of the eight proposals are the mirror image of the state
(tests/glue_oracle.MirroredRows: same AMBER energy, the alpha carbon inverted), on alanine dipeptide with the full-size kernel flow and
the coordinate prior e^-2 nm.  With the guard off the first mirrored row is accepted; with it on both rows carry the penalty and
nothing is accepted - so `tw_chirality_changed`, its copies inside `mh_finish_kernel` / `mhc_finish_kernel`, the + 2000 of the accept
kernels and the + 10000 of exploration.py decide what these tests see.  tests/test_glue_oracle_cpu.py asserts the same facts on the
oracle side (exponents 2.5 / 2.2 without the guard, 2002 with it).

Every route against oracle/mh_oracle.py on the same draws, at the tolerances of tests/test_mh_gpu.py: `tw_mh_iteration` and the
op-by-op route, exact-f32 and split-fp16 flow kernels, both velocity treatments; a table of two centres with its second reference
sign negated, in both orders; three lock-step chains of which one has mirrored rows; the exploration loop."""
import numpy as np
import pytest
import torch

from oracle import mh_oracle as mo
from tests import glue_oracle as go
from tests import helpers as H
from tests.test_mh_gpu import _assert_chain_matches_oracle as _assert_chain

pytestmark = pytest.mark.gpu

STATS = ("acceptance_indicator", "acceptance", "p_xy", "p_yx", "exponent", "energies_pot", "energies_kin", "energies_pot_delta",
         "energies_kin_delta")
PENALTY_ROUNDING = 2.0 ** -13        # float32 spacing in [1024, 2048): E_pot / kT + 2000 is near 1960
_models, _runs = {}, {}


def dev():
    return torch.device("cuda", 0)


def _assert_chain_matches_oracle(got, ref):
    """tests/test_mh_gpu.py's comparison at the tolerances its full-size tests pass it (full-size flow, AMBER energy kernel:
    test_multichain_full_size_vs_oracle, test_adaptive_parallelism_...): 1e-5 on the states, 2e-4 on the statistics."""
    worst = {f: H.rel_err(np.asarray(getattr(got[3], f), np.float64), np.asarray(getattr(ref[3], f), np.float64)) for f in STATS[1:]
             if np.asarray(getattr(got[3], f)).shape == np.asarray(getattr(ref[3], f)).shape}
    print("rel err vs oracle: coords %.2e velocs %.2e" % (H.rel_err(got[0], ref[0]) if got[0].shape == ref[0].shape else -1,
                                                          H.rel_err(got[1], ref[1]) if got[1].shape == ref[1].shape else -1),
          " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    _assert_chain(got, ref, tol=1e-5, stat_tol=2e-4)


def model_for(path, random_velocs, coords_log_scale=-2.0):
    key = (path, random_velocs, coords_log_scale)
    if key not in _models:
        _models[key] = H.tw_kernel_model(go.mh_sd(random_velocs, coords_log_scale), path=path)
    return _models[key]


def energy_fn():
    from timewarp_amd.energy import AmberPotentialEnergyTorch

    return AmberPotentialEnergyTorch(go.alanine()[4])


def product_chain(monkeypatch, fused, path, random_velocs, guard, accept, num_samples):
    """One iteration of the product's sample_with_model on the MirroredRows draws; TW_MH_FUSED = `fused`, and the route really taken
    is asserted.  Results are kept: several tests look at the same run."""
    from timewarp_amd.dataloader import single_state_batch
    from timewarp_amd.utils import evaluation_utils as eu

    key = (fused, path, random_velocs, guard, accept, num_samples)
    if key in _runs:
        return _runs[key]
    types, coords, masses, v0, _ = go.alanine()
    kw = go.chain_kwargs(random_velocs)
    g = go.guard_arguments(guard)
    if g is not None:
        kw.update(chirality_centers=g[0], reference_signs=g[1])
    model = model_for(path, random_velocs)
    calls = []
    real = eu.MetropolisHastingsChain._iteration_fused
    monkeypatch.setattr(eu.MetropolisHastingsChain, "_iteration_fused", lambda self: (calls.append(1), real(self))[1])
    monkeypatch.setenv("TW_MH_FUSED", fused)
    got = eu.sample_with_model(single_state_batch("ad", types, coords, v0[0]), model, dev(), energy_fn(), masses, num_samples,
                               disable_tqdm=True, noise=go.chain_noise("cuda", accept=accept), **kw)
    H.assert_not_demoted(model)
    assert len(calls) == (1 if fused == "1" else 0), (fused, calls)       # one iteration, on the route asked for
    _runs[key] = got
    return got


def assert_same_bytes(a, b, rows=slice(None)):
    assert a[2] == b[2]
    for f in STATS:
        assert np.array_equal(np.asarray(getattr(a[3], f))[rows], np.asarray(getattr(b[3], f))[rows]), f


@pytest.mark.parametrize("random_velocs", [True, False])
@pytest.mark.parametrize("path", [1, 3])
@pytest.mark.parametrize("fused", ["1", "0"])
def test_guard_decides_the_chain_vs_oracle(monkeypatch, fused, path, random_velocs):
    S, (r0, r1) = go.S_PROPOSALS, go.MIRRORED
    ordinary = [r for r in range(S) if r not in go.MIRRORED]
    runs = {}
    for name, guard, accept, n in (("off", "off", True, r0 + 1), ("off_all", "off", False, S), ("on", "one", True, S)):
        runs[name] = product_chain(monkeypatch, fused, path, random_velocs, guard, accept, n)
        _assert_chain_matches_oracle(runs[name], go.oracle_chain(random_velocs, guard, accept, n))
    off, off_all, on = runs["off"], runs["off_all"], runs["on"]
    # guard off: the first mirrored row is accepted and becomes the state
    assert off[2] == 1 and off[3].acceptance_indicator.astype(bool).tolist() == [False] * r0 + [True]
    _, coords, _, _, _ = go.alanine()
    mirror = coords.clone()
    mirror[:, 0] = 2 * coords[:, 0].mean() - coords[:, 0]
    assert float(np.abs(off[0][-1] - mirror.numpy()).max()) < 0.01 < float(np.abs(off[0][-1] - coords.numpy()).max())
    # guard on: nothing is accepted, the state stays
    assert on[2] == 0 and not on[3].acceptance_indicator.any() and on[0].shape[0] == S + 1 and (on[0] == coords.numpy()[None]).all()
    # the penalty is 2000 on rows 2 and 5 and nothing anywhere else
    d = on[3].energies_pot.astype(np.float64) - off_all[3].energies_pot.astype(np.float64)
    print("E_pot / kT of the mirrored rows", off_all[3].energies_pot[[r0, r1]], "->", on[3].energies_pot[[r0, r1]], "exponents",
          on[3].exponent[[r0, r1]])
    assert (np.abs(d[[r0, r1]] - 2000.0) <= PENALTY_ROUNDING).all(), d
    assert (on[3].exponent[[r0, r1]] > 1900).all() and (on[3].acceptance[[r0, r1]] == 0).all()
    assert (off_all[3].exponent[[r0, r1]] < 20).all()
    assert_same_bytes(on, off_all, ordinary)
    for f in ("p_xy", "p_yx", "energies_kin", "energies_kin_delta"):      # the mirrored rows too, where no energy enters
        assert np.array_equal(getattr(on[3], f), getattr(off_all[3], f)), f


@pytest.mark.parametrize("random_velocs", [True, False])
@pytest.mark.parametrize("path", [1, 3])
def test_fused_and_op_by_op_routes_give_the_same_bytes_with_the_guard_on(monkeypatch, path, random_velocs):
    a = product_chain(monkeypatch, "1", path, random_velocs, "one", True, go.S_PROPOSALS)
    b = product_chain(monkeypatch, "0", path, random_velocs, "one", True, go.S_PROPOSALS)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and (a[3].energies_pot > 1900).sum() == 2
    assert_same_bytes(a, b)


@pytest.mark.parametrize("guard", ["two", "two_swapped"])
@pytest.mark.parametrize("fused", ["1", "0"])
def test_every_table_entry_is_read_with_its_own_reference_sign(monkeypatch, fused, guard):
    """Centres (8, 6, 9, 14) and (8, 6, 10, 14), the second reference sign negated - and the two entries in the other order: every
    row is penalised and nothing is accepted even at u = 0.  A kernel that reads one entry, or one sign for all, penalises two rows."""
    S = go.S_PROPOSALS
    got = product_chain(monkeypatch, fused, 3, False, guard, True, S)
    _assert_chain_matches_oracle(got, go.oracle_chain(False, guard, True, S))
    plain = product_chain(monkeypatch, fused, 3, False, "off", False, S)
    d = got[3].energies_pot.astype(np.float64) - plain[3].energies_pot.astype(np.float64)
    assert got[2] == 0 and not got[3].acceptance_indicator.any() and (np.abs(d - 2000.0) <= PENALTY_ROUNDING).all(), d
    assert (got[3].exponent > 1900).all()


@pytest.mark.parametrize("fused", ["1", "0"])
def test_lock_step_chains_penalise_the_rows_of_their_own_chain(monkeypatch, fused):
    """Three chains in one call (row = proposal * 3 + chain); chain 1 has mirrored rows, chains 0 and 2 have none.  Each chain against
    the oracle loop on its own draws; chain 1 bit for bit the single chain of the same draws; the penalty on chain 1's rows only.
    The exact-f32 flow kernels: their row arithmetic does not depend on the number of rows in the launch."""
    from timewarp_amd.dataloader import single_state_batch
    from timewarp_amd.utils.multichain import MetropolisHastingsChains, sample_with_model_chains

    monkeypatch.setenv("TW_MH_FUSED", fused)
    S, Cn, path = go.S_PROPOSALS, 3, 1
    types, coords, masses, v0, tables = go.alanine()
    g = torch.Generator().manual_seed(21)
    starts = [coords + 0.0005 * torch.randn(coords.shape, generator=g), coords, coords + 0.0005 * torch.randn(coords.shape, generator=g)]
    vels = [v0[0] + 0.01 * torch.randn(22, 3, generator=g), v0[0], v0[0] + 0.01 * torch.randn(22, 3, generator=g)]
    model = model_for(path, False)
    energy = energy_fn()
    probe = MetropolisHastingsChains([single_state_batch("ad", types, coords, v0[0])], model, dev(), energy, masses, S)
    assert probe._fused == (fused == "1")

    def noises(device):
        # chain 1: the single chain's source; chains 0 and 2: ordinary rows only (u = 1: every row is recorded)
        return [go.chain_noise(device, x=x, rows=go.MIRRORED if c == 1 else (), seed=go.NOISE_SEED if c == 1 else 50 + c)
                for c, x in enumerate(starts)]

    centres, signs = go.guard_arguments("one")
    for guard, n in (("one", S), ("off", go.MIRRORED[0] + 1)):
        kw = dict(chirality_centers=centres, reference_signs=signs) if guard == "one" else {}
        refs = [mo.sample_with_model(types[None], x[None], v[None], torch.zeros(1, 22, dtype=torch.bool),
                                     mo.OracleModel(go.mh_sd(False), H.FULL_KERNEL_SPEC), H.OracleAmberEnergy(tables), masses, n, nz,
                                     accept=True, num_proposal_steps=S, **kw)
                for x, v, nz in zip(starts, vels, noises("cpu"))]
        multi = sample_with_model_chains([single_state_batch("ad", types, x, v) for x, v in zip(starts, vels)], model, dev(), energy,
                                         masses, n, S, noises=noises("cuda"), sync_every=1, **kw)
        H.assert_not_demoted(model)
        for got, ref in zip(multi, refs):
            _assert_chain_matches_oracle(got, ref)
        single = product_chain(monkeypatch, fused, path, False, guard, True, n)
        assert np.array_equal(multi[1][0], single[0]) and np.array_equal(multi[1][1], single[1])
        assert_same_bytes(multi[1], single)
        if guard == "one":
            assert [m[2] for m in multi] == [0, 0, 0]
            assert np.flatnonzero(multi[1][3].energies_pot > 1900).tolist() == list(go.MIRRORED)
            assert (multi[0][3].energies_pot < 1000).all() and (multi[2][3].energies_pot < 1000).all()
            assert len(multi[0][3].energies_pot) == len(multi[2][3].energies_pot) == S
        else:
            assert [m[2] for m in multi] == [0, 1, 0]


@pytest.mark.parametrize("path", [1, 3])
def test_exploration_keeps_the_mirrored_explorers_in_place(monkeypatch, path):
    """`explore` with 8 explorers, of which 2 and 5 are offered the mirror image in the first step: they stay (+ 10000 against a
    threshold of 60 kJ/mol), the other six move; without centres all eight move.  Positions and energies against mo.explore."""
    from timewarp_amd import exploration
    from timewarp_amd.dataloader import single_state_batch

    e = go.EXPLORE
    P, steps = e["P"], e["steps"]
    types, coords, masses, _, tables = go.alanine()
    model = model_for(path, True, e["coords_log_scale"])
    adj = torch.from_numpy(tables.bond_idx.astype(np.int64))
    v0 = torch.randn(22, 3, generator=torch.Generator().manual_seed(e["v_seed"]))
    noise = lambda: go.MirroredRows(e["noise_seed"], coords, go.MIRRORED, device="cuda", first_call_only=True)
    batch = single_state_batch("ad", types, coords, v0, adj_list=adj)
    assert exploration.find_chirality_centers(adj, types[None]).tolist() == [list(c) for c in go.CENTRES_ONE]
    for with_centres in (True, False):
        if not with_centres:
            monkeypatch.setattr(exploration, "find_chirality_centers", lambda *a, **k: torch.zeros((0, 4), dtype=torch.int64))
        pos, en = exploration.explore(batch, model, "cuda", energy_fn(), steps, P, e["threshold"], noise=noise())
        H.assert_not_demoted(model)
        pos, en = pos.cpu(), en.cpu()
        rpos, ren = go.oracle_explore(with_centres)
        moved = (pos[:P] != coords[None]).any(-1).any(-1).tolist()
        assert moved == ([r not in go.MIRRORED for r in range(P)] if with_centres else [True] * P)
        assert torch.equal((pos[P:] != pos[:-P]).any(-1).any(-1), (rpos[P:] != rpos[:-P]).any(-1).any(-1))
        assert pos.shape == (steps * P, 22, 3) and en.shape == (steps * P, 1)
        print(f"exploration vs oracle: positions {H.rel_err(pos, rpos):.2e} energies {float((en - ren).abs().max()):.2e} kJ/mol")
        assert H.rel_err(pos, rpos) < 1e-5
        assert float((en - ren).abs().max()) < 2e-3            # kJ/mol, fp32 energies of ~ -50 .. +100


def test_the_loops_refuse_a_centre_off_the_molecule(monkeypatch):
    """A centre index outside 0 .. n_atoms - 1 is a ValueError on the host, where the table is first taken in."""
    from timewarp_amd import exploration
    from timewarp_amd.dataloader import single_state_batch
    from timewarp_amd.utils.evaluation_utils import MetropolisHastingsChain
    from timewarp_amd.utils.multichain import MetropolisHastingsChains

    types, coords, masses, v0, tables = go.alanine()
    model, energy = model_for(3, False), energy_fn()
    batch = single_state_batch("ad", types, coords, v0[0], adj_list=torch.from_numpy(tables.bond_idx.astype(np.int64)))
    for table in ([[8, 6, 9, 22]], [[8, -1, 9, 14]]):
        bad = dict(chirality_centers=torch.tensor(table), reference_signs=torch.ones(1, 1))
        with pytest.raises(ValueError, match="chirality_centers"):
            MetropolisHastingsChain(batch, model, dev(), energy, masses, accept=True, num_proposal_steps=4, **bad)
        with pytest.raises(ValueError, match="chirality_centers"):
            MetropolisHastingsChains([batch, batch], model, dev(), energy, masses, 4, **bad)
        monkeypatch.setattr(exploration, "find_chirality_centers", lambda *a, **k: torch.tensor(table))
        with pytest.raises(ValueError, match="chirality_centers"):
            exploration.explore(batch, model, "cuda", energy, 1, 2, 60.0)
