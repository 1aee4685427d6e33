"""The options in front of the coder, as a cross product: model kind x element_size x filter x base x base_op x constant x
stored x unit_layouts, given to compress_blocks, decompress_blocks (without and with a length), DeviceEncoder, DeviceDecoder
and container.pack, against the outcomes recorded in tests/golden/front_outcomes.json
(tests/golden/make_front_outcomes.py).  Every call must refuse its arguments (InvalidInput), or get as far as the library
or torch, exactly where it did when the file was recorded: the library and torch are replaced by a sentinel, so no GPU is
needed, and a refusal that moved behind the first library call shows as a changed outcome."""
import importlib.util
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")


def _recorder():
    spec = importlib.util.spec_from_file_location("make_front_outcomes", os.path.join(GOLDEN, "make_front_outcomes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_front_outcomes_match_recording(monkeypatch):
    mod = _recorder()
    rec = json.load(open(os.path.join(GOLDEN, "front_outcomes.json")))
    assert rec["axes"] == [[name, list(values)] for name, values in mod.AXES]
    assert rec["calls"] == list(mod.CALLS)
    combos = list(mod.combinations())
    assert len(rec["outcomes"]) == len(combos) == 2880
    api, container, models = mod.setup()
    mod.patch(monkeypatch.setattr)
    bad = []
    for combo, want in zip(combos, rec["outcomes"]):
        got = mod.outcomes(api, container, models, combo)
        if got != want:
            bad.append((dict(zip((name for name, _ in mod.AXES), combo)), want, got))
    assert not bad, (len(bad), bad[:10])
    # the recording is not all refusals: some of every call's combinations go through
    for i, call in enumerate(mod.CALLS):
        assert any(row[i] != "I" for row in rec["outcomes"]), call
