"""The container's accessors on valid and damaged containers, against the outcomes recorded in
tests/golden/container_outcomes.json (tests/golden/make_container_outcomes.py): every accessor gives what it gave when
the file was recorded, except that element_size() and static_table(), which once read only the header and table, may
now reject a container that unpack() rejects, with unpack()'s exception."""
import importlib.util
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")


def _recorder():
    spec = importlib.util.spec_from_file_location("make_container_outcomes",
                                                  os.path.join(GOLDEN, "make_container_outcomes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_container_outcomes_match_recording():
    from redux_amd import container
    mod = _recorder()
    rec = json.load(open(os.path.join(GOLDEN, "container_outcomes.json")))
    assert rec["accessors"] == list(mod.ACCESSORS)
    assert sorted(rec["cases"]) == sorted(name for name, *_ in mod.INPUTS)
    bad, checked = [], 0
    for name, *spec in mod.INPUTS:
        var = mod.variations(*mod.make_input(*spec))
        row = rec["cases"][name]
        assert row["variations"] == len(var), name
        want = {acc: [mod.decode(t, rec["results"]) for t in mod.unrle(row[acc])] for acc in mod.ACCESSORS}
        for i, (label, buf) in enumerate(var):
            rejected = want["unpack"][i]  # unpack's exception, when it raised one
            rejected = rejected if isinstance(rejected, str) and not rejected.startswith("#") else None
            for acc in mod.ACCESSORS:
                got = mod.outcome(getattr(container, acc), buf)
                checked += 1
                if got == want[acc][i]:
                    continue
                if acc in ("element_size", "static_table") and rejected is not None and got == rejected:
                    continue
                bad.append((name, label, acc, want[acc][i], got))
    assert checked > 30000
    assert not bad, bad[:20]
