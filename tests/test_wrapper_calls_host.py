"""Every public call of pomcpp_amd/batch.py that reaches the library (the constructor, close() and the module functions included)
played without a GPU, a library or torch (tests/wrapper_standin.py) and compared with the
record of the same calls made from the batch.py before the wrapper's argument rules were folded (tests/golden/wrapper_calls.json):
the entry points reached, in order, with every scalar argument and every field of every spec, addresses by role; which tensors the
call allocated and where it returns them; what it filled; how it ordered the streams; how many tapes and views it left; and, for a
refusal, its class, the argument its text names and that no library function was reached."""
import json
import os
import sys

from tests import wrapper_standin as W

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wrapper_calls.json")


def test_every_call_reaches_the_library_as_recorded(monkeypatch):
    from pomcpp_amd import batch
    want = json.load(open(GOLDEN))
    monkeypatch.setitem(sys.modules, "torch", W.standin_torch())
    got = json.loads(json.dumps(W.play(batch)))   # (tuples become lists, as in the record)
    assert sorted(got) == sorted(want) and len(want) > 250
    wrong = [f"{cid}:\n  recorded {want[cid]}\n  now      {got[cid]}" for cid in want if got[cid] != want[cid]]
    assert not wrong, f"{len(wrong)} of {len(want)} calls differ:\n" + "\n".join(wrong)
    refused = [r for r in want.values() if "refused" in r]
    assert len(refused) > 70 and not any(r["reached"] for r in refused)
    assert all(r["refused"][0] == "ValueError" and " " not in r["refused"][1].replace("outside the batch", "") for r in refused), \
        "a recorded refusal does not name its argument"


def test_the_standin_torch_is_gone_again():
    assert not hasattr(sys.modules.get("torch"), "events")
