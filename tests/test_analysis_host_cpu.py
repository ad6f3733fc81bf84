"""The host layer the analysis calls and the two Hermite steppers share (csrc/nbx_analysis.hpp), read off the source: it is
host-only, each of its functions is defined in that header and nowhere else in csrc/, no host file keeps a private copy of the
ragged extents loop, and each of the thirteen translation units that stand on it lists it in its Makefile rule.  That it
compiles is shown by the thirteen units compiling (each module's own CPU test cross-compiles its unit)."""
import os
import re

from conftest import ROOT, PKG

CSRC = os.path.join(PKG, "csrc")
HEADER = "nbx_analysis.hpp"
UNITS = ("field", "neighbours", "paircount", "tracers", "knn", "fof", "binaries", "tidal", "clumps", "nlist", "jerk", "hermite", "advance")
# a definition: the name after a return type at the start of a line, its parameter list, an opening brace on the same line
DEFINED = {name: re.compile(r"^(?:inline )?(?:int|long long|const char\*|GridExtents) %s\([^;{]*\) \{" % name, re.M)
           for name in ("ensure_bytes", "range_bodies", "range_noun", "object_bodies", "bodies_noun", "ragged_member_table", "ragged_extents",
                        "read_back")}
OWN_OVERLOADS = {("nbx_advance.hip", "object_bodies"): 1, ("nbx_advance.hip", "bodies_noun"): 1}  # a context's, which only that call takes


def _code(name):
    return re.sub(r"//.*", "", open(os.path.join(CSRC, name)).read())


def test_the_header_is_host_only_hidden_and_in_the_layers_namespace():
    code = _code(HEADER)
    for word in ("__global__", "__device__", "_kernels.hpp", "hipLaunchKernelGGL"):
        assert word not in code, word
    assert set(re.findall(r'#include "([^"]+)"', code)) == {"nbx_ensemble_internal.hpp", "nbx_ragged_internal.hpp", "nbx_field_shape.hpp"}
    assert code.index("#pragma GCC visibility push(hidden)") < code.index("namespace nbx_detail {") < code.index("#pragma GCC visibility pop")
    assert "class " not in code and "virtual" not in code  # plain functions and small templates
    # no scratch field of any call is named, comments included: a caller hands in the addresses of its own
    obj = open(os.path.join(CSRC, "nbx_object.hpp")).read()
    fields = re.findall(r"void\* (\w+_(?:part|out|tab|pts|lab|rec|work|seg|scan|index|r2|keep|cand|clock|pos|vel)) = nullptr;", obj)
    assert len(fields) > 40
    text = open(os.path.join(CSRC, HEADER)).read()
    for field in fields + ["herm_tab_src"]:
        assert not re.search(r"\b%s\b" % field, text), field


def test_each_shared_function_is_defined_in_the_header_and_nowhere_else():
    for name, pattern in DEFINED.items():
        where = {f: len(pattern.findall(_code(f))) for f in sorted(os.listdir(CSRC))}
        where = {f: k for f, k in where.items() if k}
        own = {f: k for (f, n), k in OWN_OVERLOADS.items() if n == name}
        header = where.pop(HEADER, 0)
        assert header >= 1 and where == own, (name, header, where)
    code = _code(HEADER)
    assert len(DEFINED["ensure_bytes"].findall(code)) == 1 and len(DEFINED["ragged_member_table"].findall(code)) == 1
    assert len(DEFINED["ragged_extents"].findall(code)) == 1 and len(DEFINED["read_back"].findall(code)) == 1
    for name in ("range_bodies", "range_noun", "object_bodies", "bodies_noun"):  # an ensemble's and a ragged ensemble's
        assert len(DEFINED[name].findall(code)) == 2, name
    for text in ('"count * n exceeds"', '"the bodies of the range exceed"', '"members * n exceeds"', '"the bodies of the members exceed"'):
        assert code.count(text) == 1, text
    helper = code[code.index("int read_back("):]
    helper = helper[:helper.index("\n}\n")]
    assert len(re.findall(r"hipStreamSynchronize\(o->stream\)", helper)) == 2  # one synchronisation, and the one of the failure path


def test_no_host_file_keeps_a_copy_of_the_extents_loop_or_of_the_table_loop():
    for f in sorted(os.listdir(CSRC)):
        if f.endswith(".hip"):
            code = _code(f)
            assert "columns = std::max(columns" not in code, f
            if f[4:-4] in UNITS:
                assert '"the member table"' not in code and "device_table(" not in code, f  # built by ragged_member_table alone
    assert _code(HEADER).count('"the member table"') == 1


def test_every_unit_includes_the_header_and_its_makefile_rule_lists_it_at_the_same_position():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    for unit in UNITS:
        assert '#include "%s"' % HEADER in _code("nbx_%s.hip" % unit), unit
        rule = re.search(r"^\$\(PKG\)/nbx_%s\.o: \$\(CSRC\)/nbx_%s\.hip(.*)\n" % (unit, unit), mk, re.M)
        assert rule, unit
        deps = rule.group(1).split()
        assert deps[:2] == ["$(CSRC)/nbx_%s_kernels.hpp" % unit, "$(CSRC)/" + HEADER], (unit, deps[:3])
    assert mk.count(HEADER) == len(UNITS)  # and no other unit does
