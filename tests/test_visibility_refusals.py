"""not-gpu: the rows of tests/visrefusals.py that need no device — the refusals of srz.visibility that look at no tensor, and the
first tensor clause of each function — on a stub set and meta tensors: each call raises the row's exception with exactly the row's
text before anything reaches the library (the stub has no library behind it).  tests/test_gpu_visibility_refusals.py runs every row."""
import pytest

import visrefusals as X

HOST_ROWS = [r for r in X.ROWS if r.host]


@pytest.fixture(scope="module")
def kit():
    return X.stub_kit()


@pytest.mark.parametrize("row", HOST_ROWS, ids=X.row_id)
def test_refusal(kit, row):
    assert X.check(kit, row) is not None


def test_the_table_covers_every_function_and_says_what_each_new_refusal_replaced():
    """every function of VALID has rows, at least one of them without a device; a row either pins a text the layer has always had or
    names what the call did before"""
    assert {r.fn for r in X.ROWS} == set(X.VALID)
    assert {r.fn for r in HOST_ROWS} == set(X.VALID)
    assert {r.was for r in X.ROWS} == {None, "AttributeError", "TypeError", "unchecked"}
    assert all(r.exc is ValueError and r.text for r in X.ROWS)
    for fn in X.VIS_FUNCTIONS:  # a host tensor and a buffer of another set's shape, for every function that takes a vis
        faults = [r.fault["vis"] for r in X.ROWS if r.fn == fn and r.was == "unchecked" and "vis" in r.fault]
        assert any(t.dev == "cpu" for t in faults) and any(t.shape != (2, 4, X.H, X.W) for t in faults), fn
