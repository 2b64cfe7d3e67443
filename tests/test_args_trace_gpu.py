"""Argument traces (tests/args_trace.py): every igemm / conv / attention entry point of omgsr_amd.ops hands the library the argument blocks,
and makes the host-side queries, that tests/golden/args_trace.json recorded - field for field, pointer offsets included, in the same order.
The launching entry points are stubbed, so nothing but GroupNorm, cast and quantise kernels run. The expected values come from
tools/record_args_trace.py run against the ops.py whose blob id the file stores; a change of ops.py that is meant to alter what a kernel
is asked to do re-records them."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import args_trace as T  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return T.load_golden()


def test_the_table_and_the_recording_hold_the_same_cases(golden):
    assert len(golden["ops_blob"]) == 40
    assert sorted(golden["cases"]) == sorted(T.CASES)


@pytest.mark.parametrize("name", list(T.CASES))
def test_args_trace(golden, name):
    got, want = T.run_case(name), golden["cases"][name]
    assert len(got["trace"]) == len(want["trace"]) and [c[0] for c in got["trace"]] == [c[0] for c in want["trace"]], \
        f"library calls: {[c[0] for c in got['trace']]}, recorded {[c[0] for c in want['trace']]}"
    for i, (g, w) in enumerate(zip(got["trace"], want["trace"])):
        assert g == w, f"call {i} ({g[0]}) differs from the recording"
    assert got["returns"] == want["returns"]
    assert got == want
