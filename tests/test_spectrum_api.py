"""The public surface of ``ramannoodle_amd.spectrum`` is frozen: ``tests/golden/spectrum_api.json`` was recorded from
commit a1dc1eb, before the spectrum classes were put on one series holder, and the module must still describe itself
the same way.  Record again (only when the surface is meant to change) with ``python -m tests.test_spectrum_api``."""
import inspect
import json
from pathlib import Path

import ramannoodle_amd.spectrum as spectrum

GOLDEN = Path(__file__).parent / "golden" / "spectrum_api.json"


def _own(value) -> bool:
    module = getattr(value, "__module__", "") or ""
    return module == spectrum.__name__ or module.startswith(spectrum.__name__ + ".")


def _describe_class(cls) -> dict:
    members = {}
    for name in dir(cls):
        if name.startswith("_"):
            continue
        member = inspect.getattr_static(cls, name)
        if isinstance(member, property):
            members[name] = "property"
        elif inspect.isfunction(member):
            members[name] = str(inspect.signature(member))
        else:
            members[name] = type(member).__name__
    bases = sorted(base.__name__ for base in cls.__mro__[1:] if not base.__name__.startswith("_") and base is not object)
    return {"kind": "class", "init": str(inspect.signature(cls)), "members": members, "bases": bases}


def describe() -> dict:
    """Every public name the module defines: its kind; a function's signature; a class's constructor signature, the
    signature of each public method (``"property"`` for a property), inherited ones included, and its public bases."""
    surface = {}
    for name, value in sorted(vars(spectrum).items()):
        if name.startswith("_"):
            continue
        if inspect.isclass(value) and _own(value):
            surface[name] = _describe_class(value)
        elif inspect.isfunction(value) and _own(value):
            surface[name] = {"kind": "function", "signature": str(inspect.signature(value))}
        elif isinstance(value, int) and name.isupper():  # MAX_GROUPS, MAX_SELECTED
            surface[name] = {"kind": "constant", "value": value}
    return surface


def test_public_surface_is_the_recorded_one():
    recorded = json.loads(GOLDEN.read_text())
    now = describe()
    assert sorted(now) == sorted(recorded)
    for name in recorded:
        assert now[name] == recorded[name], name


if __name__ == "__main__":
    GOLDEN.write_text(json.dumps(describe(), indent=1, sort_keys=True) + "\n")
    print(f"{len(describe())} names -> {GOLDEN}")
