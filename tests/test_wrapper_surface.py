"""The Python wrapper against tests/golden/wrapper_surface.json (scripts/record_wrapper_surface.py wrote it from the commit it names; what is
recorded, and how, is tests/wrapper_script.py): the names, signatures, dtypes and constants the classes expose, every option converter's
struct bytes or exception, and the library calls every method makes.  A move of wrapper code between modules must leave all three as they are.
The built library serves the *_default entry points; no GPU.
"""
import json
import os

import pytest

import wrapper_script as S
from godotoceanwaves_amd.wave_generator import WaveGenerator as W

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wrapper_surface.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def now(golden):
    return S.record(golden["recorded_from"])


def differing(a, b):
    return sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))


def test_recorded_from_a_commit(golden):
    assert len(golden["recorded_from"]) >= 7 and set(golden["recorded_from"]) <= set("0123456789abcdef")


@pytest.mark.parametrize("cls", ["WaveGenerator", "WaveGeneratorGroup", "WaveCascadeParameters"])
@pytest.mark.parametrize("part", ["names", "instance", "properties", "callables", "dtypes", "constants"])
def test_surface(golden, now, cls, part):
    a, b = golden["surface"][cls][part], now["surface"][cls][part]
    if isinstance(a, dict):
        assert differing(a, b) == []
    assert a == b


def test_module_names(golden, now):
    for k in ("wave_generator", "G_DEPTH"):
        assert golden["surface"][k] == now["surface"][k]


def test_the_seventeen_records_are_all_there(golden):
    assert len(golden["surface"]["WaveGenerator"]["dtypes"]) == 17


@pytest.mark.parametrize("name", list(S.CONVERTERS) + ["present_size", "camera", "rays", "box_hull", "box_mass_properties", "clipmap_origin", "JONSWAP"])
def test_options(golden, now, name):
    a, b = golden["options"][name], now["options"][name]
    if isinstance(a, dict):
        assert differing(a, b) == []
        if name in S.CONVERTERS:
            assert b["a struct comes back itself"] is True
            assert {"None", "{}", "all", "unknown"} | set(S.CONVERTERS[name][1]) <= set(b)
    assert a == b


def test_call_traces(golden, now):
    assert differing(golden["traces"], now["traces"]) == []
    assert list(golden["traces"]) == list(now["traces"])


def test_every_method_is_traced_or_named_with_its_reason(golden, now):
    """every public method and property of the generator and the group drives the stand-in library under a label that starts with its name, is
    a converter or static helper of the options part, or is excluded by name"""
    assert golden["excluded"] == S.EXCLUDED and list(S.EXCLUDED) == ["readback_wait"]
    labels = list(now["traces"])
    covered = set(now["options"]) | set(S.EXCLUDED) | {"JONSWAP_alpha", "JONSWAP_peak_angular_frequency"}
    for cls, prefix in (("WaveGenerator", ""), ("WaveGeneratorGroup", "group ")):
        rec = now["surface"][cls]
        for name in list(rec["callables"]) + rec["properties"]:
            if name.startswith("_") and name != "_process":
                continue
            assert name in covered or any(label == prefix + name or label.startswith(prefix + name + " ") for label in labels), (cls, name)


def test_a_missing_entry_point_is_an_error():
    """the stand-in library knows the header's entry points only"""
    with pytest.raises(AttributeError):
        S.StubLibrary().ow_no_such_call
    assert W().context is None
