"""The host contract of the layered calls (planes, delta, stored, static, plane-static, segment-static, context-static)
and of the adaptive coder's own entry points under them (plain, split, `_v`, base, const; every parameter class): every
workspace and bound value, every kernel-name string and the return code of every refusal that is decided before any HIP
call equal what tests/golden/layer_contract.json and tests/golden/adaptive_contract.json hold.

The fixture is recorded results only: tools/record_layer_contract.py wrote it from the library built at the commit before
the launch layer was put on shared helpers (one layout stage, one transform launcher, one static-coder argument filler), and
it is recorded anew only when a change means to alter one of these values; the adaptive part was recorded the same way at the
commit before the adaptive launch code was put on one plan per call and one argument core.  The collection runs in a child process that
sees no GPU, because its refusal rows pass dummy device pointers: a row the library stops refusing then fails in the runtime
(IO_ERROR, which the collection itself rejects) and launches nothing."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT
from redux_amd import _lib


@pytest.fixture(scope="module")
def contract():
    _lib.lib()                                   # (the library exists: a missing one fails here, with the loader's message)
    want, got = {}, {}
    for part, fixture in (("layered", "layer_contract.json"), ("adaptive", "adaptive_contract.json")):
        run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "record_layer_contract.py"), "--lib", _lib.LIB_PATH,
                              "--part", part], capture_output=True, text=True)
        assert run.returncode == 0, run.stderr[-2000:]
        join(want, json.load(open(os.path.join(ROOT, "tests", "golden", fixture))))
        join(got, json.loads(run.stdout))
    return want, got


def join(whole, part):
    """Adds one part's rows to `whole`; its kernel-name rows index its own strings, which go behind those already there."""
    if not whole:
        whole.update(sizes={}, refusals={}, names={"strings": [], "rows": {}})
    assert not (set(part["sizes"]) & set(whole["sizes"])) and not (set(part["refusals"]) & set(whole["refusals"]))
    whole["sizes"].update(part["sizes"])
    whole["refusals"].update(part["refusals"])
    first = len(whole["names"]["strings"])
    whole["names"]["strings"] += part["names"]["strings"]
    whole["names"]["rows"].update({name: [first + i for i in row] for name, row in part["names"]["rows"].items()})


def test_workspace_and_bound_values(contract):
    want, got = contract
    assert sorted(got["sizes"]) == sorted(want["sizes"])
    for name in want["sizes"]:
        assert got["sizes"][name] == want["sizes"][name], name
    assert sum(len(v) for v in want["sizes"].values()) > 3000 and any(v for v in want["sizes"]["redux_decode_stored_workspace_bytes"])


def test_kernel_names(contract):
    want, got = contract
    text = lambda d, name: [d["names"]["strings"][i] for i in d["names"]["rows"][name]]
    assert sorted(got["names"]["rows"]) == sorted(want["names"]["rows"])
    for name in want["names"]["rows"]:
        assert text(got, name) == text(want, name), name
    assert len(want["names"]["strings"]) >= 10


def test_refusal_codes(contract):
    want, got = contract
    assert sorted(got["refusals"]) == sorted(want["refusals"]) and len(want["refusals"]) == 28
    for fn in want["refusals"]:
        assert got["refusals"][fn] == want["refusals"][fn], fn
        assert sum(" and " in label for label in want["refusals"][fn]) >= 2, fn   # two faults at once: the order of the checks
        assert all(rc in (_lib.INVALID_INPUT, _lib.OUTPUT_TOO_SMALL, _lib.UNSUPPORTED) for rc in want["refusals"][fn].values())
