"""-m gpu: guard-band tests (tests/isolation.py) of the 'temporal' family — every row of tests/isolation_cases.py with that family
name, under both guard fills and every kernel variant the row lists.  Exact assertions only: same bits as the call on tight operands,
every guard byte untouched, every input unchanged."""
import pytest

import isolation_run as run
from isolation_cases import family

pytestmark = pytest.mark.gpu
ROWS = family("temporal")


@pytest.mark.parametrize("row", ROWS, ids=[c.name for c in ROWS])
def test_isolation_temporal(row):
    run.run_case(row)


def test_isolation_temporal_variant_runs():
    """Runs after the rows above (file order): what executed, per kernel variant."""
    run.check_counts("temporal", ROWS)
