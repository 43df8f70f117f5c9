"""CPU: the executor's geometry of an alltoall, the P x P count matrix.  Rank
r's lists for the planner are row r then column r (gloo_hip_alltoall_lists,
the derivation planFor uses for the rank itself and for its peers).  Fed to
gloo_hip_plan_ex they must give the plans tests/alltoall_sim.py accepts over
three runs with no barrier, with an arena of column r's sum, for ragged
matrices with empty blocks, a zero row, a zero column and a rank with nothing
either way."""
import numpy as np
import pytest

import alltoall_sim as sim
import plan_sim
from test_alltoall_plan import payloads

SIZES = (1, 2, 3, 5, 8)


def matrix(P, seed):
    rng = np.random.default_rng(1000 + seed)
    M = rng.integers(0, 40, (P, P))
    M[rng.random((P, P)) < 0.3] = 0
    if P > 1:
        M[P - 1, :] = 0        # a rank that sends nothing, not even to itself
    if P > 2:
        M[:, 1] = 0            # a rank that receives nothing
    if P > 3:
        M[2, :] = 0            # a rank with nothing either way
        M[:, 2] = 0
    return [[int(v) for v in row] for row in M]


def lists(M, r):
    import gloo_amd
    P = len(M)
    return gloo_amd.alltoall_lists(r, P, [v for row in M for v in row])


@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_row_and_column_give_the_plans_the_simulator_accepts(P, seed, monkeypatch):
    M = matrix(P, seed)
    if P > 3:
        assert not any(M[2]) and not any(row[2] for row in M)
    for r in range(P):
        got = lists(M, r)
        assert got[:P] == M[r] and got[P:] == [M[q][r] for q in range(P)]
        # in_counts_q[r] == out_counts_r[q] for every pair, by construction
        for q in range(P):
            assert lists(M, q)[r] == got[P + q]
        steps, arena = plan_sim.get_plan("alltoall", r, P, 0, 1, recv=got, nin=1, elem_size=1)
        assert arena == (sum(M[q][r] for q in range(P)) if P > 1 else 0)
        assert (len(steps) == 0) == (not any(M[r]) and not any(M[q][r] for q in range(P)))
    monkeypatch.setattr(sim, "recv_elems", lists)  # the simulator's plans now come from the C derivation
    for s in range(3):
        sim.simulate(M, payloads(M, 10 * seed + s), seed=s)


def test_an_empty_matrix_is_the_even_form_and_other_lengths_are_refused():
    import ctypes

    import gloo_amd
    out = (ctypes.c_int * 8)()
    with pytest.raises(gloo_amd.GlooHipError) as e:
        gloo_amd.alltoall_lists(0, 2, [1, 2, 3])
    assert "3 entries for 2 ranks" in str(e.value)
    assert gloo_amd.lib.gloo_hip_alltoall_lists(3, 3, (ctypes.c_int * 9)(), out) == -4
