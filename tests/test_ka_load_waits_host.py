"""The streamed load phase of stftRealKernel<4, ...> as a listing check (tools/ka_load_waits.py on the tree's spectrum_real.hip, compiled
with the build's flags; no GPU): the design's own consequences, per instantiation that is said to stream.

A channel workgroup's thread issues 22 requests before its first barrier: the two window phases, the sixteen sample rows in the order
pass 1 consumes them, four table requests behind them.  The load counter is waited for in order, so:
  * the first wait with vector work behind it is the one for the first row pair: fourteen rows are still due then, and the allowance
    of two covers requests the scheduler moves -- at least 12 requests outstanding.  (In request order every row stood in front of the
    first window operation: the old listing waits at vmcnt(2), vmcnt(5) or vmcnt(8) there.)
  * behind the last request the waits form a ladder, one rung per row pair: non-increasing counts, at least eight distinct ones.
Waits in FRONT of the last request are not rungs: they stand in the lane-predicated table blocks among the requests (register reuse),
and a count there rises with every request issued behind it; the old listing has them too.
The forms that hold more values in flight (Mid-Side, a fetched window) keep the request order and must show no such ladder."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

STREAMED = ("stftRealKernel<4, true, 0, false>", "stftRealKernel<4, true, 1, false>", "stftRealKernel<4, true, 4, false>",
            "stftRealKernel<4, true, 4, true>")
REQUEST_ORDER = ("stftRealKernel<4, true, 2, false>", "stftRealKernel<4, true, 3, false>", "stftRealKernel<4, false, 0, false>",
                 "stftRealKernel<4, false, 1, false>", "stftRealKernel<4, false, 2, false>", "stftRealKernel<4, false, 3, false>")


@pytest.fixture(scope="module")
def roles(tmp_path_factory):
    import ka_load_waits as klw
    if not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc") or os.environ.get("HIPCC")):
        pytest.skip("no hipcc")
    listing = klw.listing_of_source(str(tmp_path_factory.mktemp("ka") / "real.s"))
    return {name: klw.summary(events) for name, events in klw.channel_roles(listing).items()}


def test_every_instantiation_is_found(roles):
    assert set(roles) == set(STREAMED) | set(REQUEST_ORDER), sorted(roles)


@pytest.mark.parametrize("name", STREAMED)
def test_streamed_instantiation_waits_row_pair_by_row_pair(roles, name):
    s = roles[name]
    assert s["requests"] >= 2 + 16 + 2, (name, s["requests"])
    first = s["first_working_wait"]
    assert first is not None and first[0] >= 12, (name, "the first wait with vector work behind it leaves fewer than 12 requests outstanding", first)
    counts = [n for n, _ in s["ladder"]]
    assert counts == sorted(counts, reverse=True), (name, "the waits behind the last request do not fall", counts)
    assert len(set(counts)) >= 8, (name, "fewer than eight distinct counts: not one wait per row pair", counts)
    # the rungs carry the work: vector instructions follow the waits of the row pairs in front of the last one (eight pairs, the last
    # apart, and one more for rungs the scheduler merges), not only the last wait
    assert sum(1 for n, v in s["ladder"] if n >= 4 and v > 0) >= 6, (name, s["ladder"])


@pytest.mark.parametrize("name", REQUEST_ORDER)
def test_other_forms_keep_the_request_order(roles, name):
    s = roles[name]
    assert len(set(n for n, _ in s["ladder"])) <= 3, (name, s["ladder"])
