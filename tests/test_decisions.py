"""The decision table (decision_cases.py) on the GPU: every row for 24 steps at the requested G = 1, 8 (37 envs) and
64 (13 envs), four engines in lock step (k_step and k_tick, the lanes' execution and the leader's) against one oracle
per env inside guard bands (step_runner.py): the reset observation, then observations, listed rewards bit-exact,
flags, `listed` and the autoreset flag at every step, the full state at every terminal step, after every autoreset
and at the end, the RNG stream at the end.  Two rows also run through step_graph, and the wander row (no autoreset:
its envs are stepped on after their end, and the wandering zombies' draws are deferred to the leader) at every G the
step kernels are compiled for.  test_decision_plan.py shows on the CPU that the rows reach the branches they name."""
import pytest

import decision_cases as D
from step_instantiations import GS as ALL_GS
from step_runner import run_engines

pytestmark = pytest.mark.gpu

CASES = [(r.id, g, False) for r in D.ROWS for g in sorted(D.ENVS)]
CASES += [(rid, g, True) for rid in D.GRAPHED for g in sorted(D.ENVS)]
CASES += [("wander", g, False) for g in ALL_GS if g not in D.ENVS]
COMBOS = [(k, p) for k in ("k_step", "k_tick") for p in (1, -1)]


@pytest.mark.parametrize("rid,g,graph", CASES, ids=["%s-G%d-%s" % (c[0], c[1], "graph" if c[2] else "eager")
                                                     for c in CASES])
def test_row(rid, g, graph):
    row = D.BY_ID[rid]
    n = D.ENVS.get(g, 37)
    builders = [row.builder(n, g, k, p) for k, p in COMBOS]
    expect = [{"envs": n, "lanes_per_env": g, "step_kernel": k, "par_exec": 1 if p >= 0 else 0} for k, p in COMBOS]
    resets, _ = run_engines(builders, row.make, row.seeds(n), D.STEPS, row, graph=graph, states_at=(D.STEPS,),
                            expect=expect, terminal=True, keep=row.keep)
    assert (sum(resets) == 0) if row.keep else (sum(resets) >= n), resets
