"""Every environment switch is in one documented table (distributed_learning_amd/knobs.py).

Checks that each ``DLA_*`` variable read anywhere in the package or the native sources (``Knob``
declarations in csrc, ``knobs.get`` in Python) is listed -- the native ones with the default and the file
they are declared with -- that neither side reads one behind the table's back, and that the bench record's
``knobs`` field is empty at defaults and names what was changed.
"""
import os
import re

from distributed_learning_amd import knobs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _files(sub, exts):
    for d, _, fs in os.walk(os.path.join(ROOT, sub)):
        for f in fs:
            if f.endswith(exts):
                yield os.path.join(d, f)


# a native knob is one declaration of csrc/include/dla_knob.h's type, its name and default as literals:
#   Knob::on_unless_0("NAME") (default 1), Knob::off_unless_1("NAME") (default 0),
#   Knob::integer("NAME", d[, floor]), Knob::positive("NAME", d[, cap]), Knob::real("NAME", d)
_DECL = re.compile(r'Knob::(on_unless_0|off_unless_1|integer|positive|real)\(\s*"([A-Z0-9_]+)"\s*(?:,\s*([-+0-9.eE]+))?')
_KNOB_H = os.path.join("csrc", "include", "dla_knob.h")


def _native_declarations():
    """{name: (default as float, file relative to the repository)} of every native knob declaration."""
    found = {}
    for p in _files("csrc", (".cpp", ".h", ".hip")):
        rel = os.path.relpath(p, ROOT)
        if rel == _KNOB_H or rel.startswith(os.path.join("csrc", "tests")):
            continue
        for form, name, default in _DECL.findall(open(p).read()):
            assert name not in found, f"DLA_{name} is declared twice ({found[name][1]} and {rel})"
            if form in ("on_unless_0", "off_unless_1"):
                assert not default, f"{rel}: {name}: the on/off forms take no default"
                default = "1" if form == "on_unless_0" else "0"
            assert default, f"{rel}: {name}: the default must be a literal at the declaration"
            found[name] = (float(default), rel)
    return found


def test_native_knob_declarations_match_the_table():
    found = _native_declarations()
    assert found, "no native knob declaration found (pattern broken?)"
    missing = sorted(n for n in found if n not in knobs.TABLE)
    assert not missing, f"native knobs missing from knobs.TABLE: {missing}"
    for name, (default, rel) in sorted(found.items()):
        k = knobs.TABLE[name]
        assert float(k.default) == default, f"{name}: knobs.TABLE says default {k.default}, {rel} declares {default}"
        assert k.where == rel, f"{name}: knobs.TABLE says it is read in {k.where}, it is declared in {rel}"
    undeclared = sorted(n for n, k in knobs.TABLE.items() if k.where.startswith("csrc/") and n not in found)
    assert not undeclared, f"knobs.TABLE lists native knobs that no file under csrc/ declares: {undeclared}"


def test_native_code_reads_the_environment_only_through_the_knob_type():
    offenders = [os.path.relpath(p, ROOT) for p in _files("csrc", (".cpp", ".h", ".hip"))
                 if os.path.relpath(p, ROOT) != _KNOB_H and 'getenv("DLA_' in open(p).read()]
    assert not offenders, f'getenv("DLA_...") outside {_KNOB_H}: {offenders}'


def test_python_reads_knobs_through_the_table():
    rx = re.compile(r'os\.environ(?:\.get)?[\[(]\s*"DLA_([A-Z0-9_]+)"')
    offenders = []
    for p in list(_files("distributed_learning_amd", (".py",))) + [os.path.join(ROOT, "bench.py")]:
        if p.endswith("knobs.py"):
            continue
        for n in rx.findall(open(p).read()):
            offenders.append((os.path.relpath(p, ROOT), n))
    assert not offenders, f"read DLA_* through knobs.get instead: {offenders}"
    rx2 = re.compile(r'knobs\.(?:get|flag|env_name)\("([A-Z0-9_]+)"\)')
    used = set()
    for p in list(_files("distributed_learning_amd", (".py",))) + [os.path.join(ROOT, "bench.py")]:
        used |= set(rx2.findall(open(p).read()))
    assert used and all(n in knobs.TABLE for n in used), sorted(used - set(knobs.TABLE))


def test_non_default_reports_changes_only():
    env = {"DLA_WGRAD_DEFER": "3x3", "DLA_TILE256": "0", "DLA_TYPO": "1", "PATH": "/bin"}
    assert knobs.non_default(env) == {"TILE256": "0", "DLA_TYPO": "1"}
    assert knobs.non_default({}) == {}
    assert "| `WGRAD_DEFER` |" in knobs.table_markdown()
