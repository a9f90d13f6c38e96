"""Every way an episode can end (terminal_outcomes.py) at every lane count on the GPU, against the C oracle: every
env at every step (observations, the listed agents' rewards as float64 bits, done, truncated, the autoreset flag
and `listed`), the full state of every env at the step it ends (the pending env still shows the terminal world)
and at the step of its autoreset, the RNG stream after the last step and, on the rows with ZS_FLAG_DEATH_LOG, the
death log of every terminal step against the things the oracle removed; flags, rewards and actions inside 0x5A
guard bands (step_runner.py).  test_terminal_outcomes_plan.py shows on the CPU that the oracle's runs of these
rows hold the outcomes they claim."""
import pytest

import step_instantiations as S
import terminal_outcomes as TO
from step_runner import run_engines

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("row", TO.ROWS, ids=[r.id for r in TO.ROWS])
def test_terminal_outcome(row):
    pars = (1, -1)
    resets, _ = run_engines([row.builder(par_exec=p) for p in pars], row.make, row.seeds(), S.STEPS, row,
                            states_at=(S.STEPS,), expect=[row.describe(p) for p in pars], terminal=True)
    assert sum(resets) >= 3  # envs ended and went through their autoreset
