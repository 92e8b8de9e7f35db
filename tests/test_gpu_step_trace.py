"""Which launches the forward issues, in which order, for which model: every row of tests/step_trace_cases.py against
tests/golden/step_traces.json. No kernel runs (VogEngine.describe_steps), so the rows cost their engines only."""
import pytest

from tests import step_trace_cases as stc


def test_fixture_covers_every_step_name_and_row():
    """CPU: the recorded rows are the table's rows, and between them they launch every step the builder can produce."""
    fx = stc.load_fixture()
    assert sorted(fx) == sorted(stc.row_id(r) for r in stc.ROWS)
    seen = {n for rec in fx.values() for n in rec["trace"]}
    missing = [n for n in stc.STEP_NAMES if n not in seen]
    assert not missing, f"no row launches {missing}"
    # and nothing the list does not know: single names, or "a+b" of two of them
    single = {n for n in stc.STEP_NAMES if "+" not in n}
    for n in sorted(seen):
        assert all(p in single for p in n.split("+")), n


@pytest.mark.gpu
@pytest.mark.parametrize("row", stc.ROWS, ids=stc.row_id)
def test_launch_trace_equals_fixture(row):
    want = stc.load_fixture()[stc.row_id(row)]
    got = stc.trace_row(row)
    assert got["trace"] == want["trace"]
    assert got == want
