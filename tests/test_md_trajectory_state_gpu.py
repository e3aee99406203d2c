"""`LangevinDynamics.trajectory` with the fp64 carry: `coords` / `velocs` beside a `state` must be its float32 cast (a stale state
is refused, not silently preferred), and None for both continues from the state alone, bit for bit as with them."""
import numpy as np
import pytest
import torch

from tests.test_langevin_gpu import FIRST_STEP, dynamics, free_energy, free_state
from tests.test_md_trajectory_gpu import FRAME_KEYS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("V", [22, 65])
def test_a_stale_state_is_refused_and_none_continues_from_the_state(V):
    masses, x, v = free_state(V, 3)
    gx, gv = torch.from_numpy(x).cuda(), torch.from_numpy(v).cuda()
    make = lambda: dynamics(free_energy(V), masses, 0.0005, 0.3, 0, 5, FIRST_STEP)
    reports = [[0, 2, 5], [1, 7]]

    md = make()
    state = md.new_state(gx, gv)
    cx, cv, first = md.trajectory(gx, gv, reports[0], state=state)
    # the state has moved on: the inputs of the first call are no longer its cast, the outputs of that call are
    before = state.clone()
    for bad in [(gx, gv), (cx, gv), (gx, cv)]:
        with pytest.raises(ValueError, match="not the float32 cast"):
            md.trajectory(*bad, reports[1], state=state)
    assert md.steps_done == FIRST_STEP + 5 and torch.equal(state, before)          # refused before anything ran
    cx2, cv2, second = md.trajectory(cx, cv, reports[1], state=state)

    md = make()
    state2 = md.new_state(gx, gv)
    nx, nv, n_first = md.trajectory(None, None, reports[0], state=state2)
    nx2, nv2, n_second = md.trajectory(None, None, reports[1], state=state2)
    assert nx.shape == (3, V, 3) and nx.dtype == torch.float32
    assert torch.equal(nx, cx) and torch.equal(nv, cv) and torch.equal(nx2, cx2) and torch.equal(nv2, cv2) and torch.equal(state, state2)
    for a, b in ((first, n_first), (second, n_second)):
        assert all(torch.equal(getattr(a, k), getattr(b, k)) for k in FRAME_KEYS) and np.array_equal(a.step, b.step)
    assert not torch.equal(cx2, cx) and md.steps_done == FIRST_STEP + 12
