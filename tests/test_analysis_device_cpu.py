"""The device layer the kernel headers that launch by field_shape share (csrc/nbx_tilewalk.hpp), read off the source: it is inline
device code only, each of its functions and structs is defined in that header and nowhere else in csrc/, no unit keeps a private
copy of a piece it took -- the units that keep one are listed here by name, with DESIGN.md's reason -- and each of the thirteen
units that stand on it includes it and lists it in its Makefile rule.  That it compiles is shown by the thirteen units compiling
(each module's own CPU test cross-compiles its unit)."""
import os
import re

from conftest import ROOT, PKG

CSRC = os.path.join(PKG, "csrc")
HEADER = "nbx_tilewalk.hpp"
UNITS = ("field", "neighbours", "paircount", "tracers", "knn", "fof", "binaries", "tidal", "clumps", "nlist", "jerk", "hermite", "advance")
ALONE = "timescale"  # launches by the same shape and stays as it was: both shared pieces it could take measured slower
FUNCTIONS = ("zero_record", "whole_record", "member_group", "member_at", "tile_masked")
STRUCTS = ("PosMember", "OutMember", "VelMember", "MemberGroup", "MemberAt", "TileWalk", "TileWalk2")
# the per-call member structs: the shared layout under the call's own name (kernel-argument data: the name is in the kernels' symbols)
MEMBERS = {"PosMember": ("FieldMember", "TracerMember", "PcMember"), "OutMember": ("NbMember", "KnnMember", "NlMember", "TidalMember"),
           "VelMember": ("JerkMember", "BoundMember", "ClumpMember", "HermiteMember", "AdvanceMember")}
# who keeps a copy of its own, and why
KEEPS_SEARCH = {"clumps": "the shared lookup changes the finish kernel's vector instructions",
                "hermite": "the shared lookup adds a load and a 64-bit subtraction to the finish kernel", "advance": "as hermite",
                "fof": "a layout of its own, two offsets to search by"}
KEEPS_WALK = {"binaries": "rescales .w before staging", "clumps": "stages the labels too", "hermite": "predicts before staging",
              "advance": "predicts before staging", "knn": "the shared walk changes the register copies of the pair-work kernels",
              "nlist": "as knn", "paircount": "as knn",
              "neighbours": "a two-build A/B put its fp32 call 1 % above the parent's median with the shared walk, 0.2 % with its own", ALONE: "measured slower than the parent's range"}
KEEPS_GATE = {"knn": "the shared gate changes the ragged kernels' vector compares", "paircount": "as knn, and the SGPR spills",
              "fof": "a layout of its own, neutral rows"}
KEEPS_PREDICATE = {"paircount": "the shared predicate measured slower than the parent's range in fp64", "nlist": "as paircount",
                   ALONE: "as paircount, in fp32", "clumps": "another rule: j != i alone"}
SEARCH, STAGE, RECORD = "while (lo < hi)", re.compile(r"\(\w+ \+ 1\) \* kTile \+ t"), 'asm volatile("" ::"v"(r.w))'
PREDICATE = re.compile(r"j0 \+ kTile > g_lo\) \|\| j0 \+ kTile > n")
GATE = "(int)blockIdx.x >= s.columns"


def _code(name):
    return re.sub(r"//.*", "", open(os.path.join(CSRC, name)).read())


def _kernels(unit):
    return _code("nbx_%s_kernels.hpp" % unit)


def test_the_header_is_inline_device_code_and_names_no_call():
    code = _code(HEADER)
    assert "__global__" not in code and "hipLaunchKernelGGL" not in code and "_kernels.hpp" not in code
    assert set(re.findall(r'#include ["<]([^">]+)[">]', code)) == {"nbx_pair.hpp", "nbx_field_shape.hpp"}
    assert "namespace nbx {" in code and "class " not in code and "virtual" not in code
    free = re.findall(r"^__device__ __forceinline__ [\w:<> ]+ (\w+)\(", code, re.M)
    assert sorted(free) == sorted(FUNCTIONS), free  # the free functions are the shared ones; the rest are the structs' members
    assert code.count("__device__ __forceinline__") >= len(FUNCTIONS) and "__host__" not in code
    # comments included: the per-call tests read every file of csrc/ for each other's names
    text = open(os.path.join(CSRC, HEADER)).read().replace("nbx_field_shape.hpp", "")  # the shape rule it stands on
    for unit in UNITS:
        for word in ("nbx_%s" % unit, "%s_kernel" % unit, "%s_body" % unit, "%s_finish" % unit, "%s_tile" % unit):
            assert word not in text, word
    for word in ("jerk", "knn", "fof", "tidal", "clump", "nlist", "hermite", "paircount", "tracer", "neighbour", "binaries", "timescale",
                 "nb_", "nl_", "pc_", "ts_", "bound_", "Nb", "Nl", "Pc", "Knn", "Jerk", "Bound", "Clump", "Hermite", "Advance", "Fof"):
        assert word not in text, word


def test_each_shared_function_and_struct_is_defined_in_the_header_and_nowhere_else():
    for f in sorted(os.listdir(CSRC)):
        code = _code(f)
        for name in FUNCTIONS:
            n = len(re.findall(r"^__device__ __forceinline__ [\w:<> ]+ %s\(" % name, code, re.M))
            assert n == (1 if f == HEADER else 0), (f, name, n)
        for name in STRUCTS:
            n = len(re.findall(r"^struct %s \{" % name, code, re.M))
            assert n == (1 if f == HEADER else 0), (f, name, n)
    # field order and sizes of the three layouts: what the hosts' makers fill, in this order
    code = _code(HEADER)
    for name, fields in (("PosMember", "pos_off n reserved"), ("OutMember", "pos_off out_off n reserved"),
                         ("VelMember", "pos_off vel_off out_off n reserved")):
        body = code[code.index("struct %s {" % name):]
        body = body[:body.index("};")]
        assert re.findall(r"(?:unsigned long long|int) (\w+);", body) == fields.split(), name
        assert len(re.findall(r"unsigned long long \w+;", body)) == len(fields.split()) - 2, name
    # every per-call member struct is its layout under the call's name, and FofMember stays a layout of its own
    everything = "".join(_code(f) for f in sorted(os.listdir(CSRC)))
    for layout, names in MEMBERS.items():
        for name in names:
            assert everything.count("struct %s : %s {};" % (name, layout)) == 1 and not re.search(r"struct %s \{" % name, everything), name
    assert len(re.findall(r"^struct FofMember \{", _kernels("fof"), re.M)) == 1


def test_no_unit_keeps_a_private_copy_of_a_piece_it_took():
    assert _code(HEADER).count(RECORD) == 1 and _code(HEADER).count(SEARCH) == 1 and len(STAGE.findall(_code(HEADER))) == 2
    assert len(PREDICATE.findall(_code(HEADER))) == 1 and "__syncthreads();" in _code(HEADER)
    for f in sorted(os.listdir(CSRC)):
        if f == HEADER or f == "nbx_diag_body.hpp":  # the diagnostics' walk accumulates after every tile: not this layer's
            continue
        unit = f[4:-12] if f.endswith("_kernels.hpp") else None
        code = _code(f)
        assert RECORD not in code, f  # the whole-record read: nobody keeps one
        assert (SEARCH in code) == (unit in KEEPS_SEARCH), f
        assert bool(STAGE.search(code)) == (unit in KEEPS_WALK), f
        assert bool(PREDICATE.search(code)) == (unit in KEEPS_PREDICATE and unit != "clumps"), f
        if unit in UNITS:
            assert (GATE in code) == (unit in KEEPS_GATE), f
    # and who took a piece uses it
    for unit in ("neighbours", "knn", "nlist", "paircount", "binaries", "jerk", "hermite", "advance"):
        assert "whole_record(" in _kernels(unit), unit
    for unit in ("neighbours", "knn", "nlist", "tidal", "jerk", "binaries"):
        assert "member_at(" in _kernels(unit), unit
    for unit in ("neighbours", "nlist", "tidal", "jerk", "binaries", "clumps", "hermite", "advance"):
        assert "member_group(" in _kernels(unit) and "if (g.elsewhere()) return;" in _kernels(unit), unit
    for unit in ("field", "tracers"):  # one m for every member: every column is the member's, the splits alone are tested, as before
        assert "member_group(" in _kernels(unit) and "if ((int)blockIdx.y >= g.shape.splits) return;" in _kernels(unit), unit
    for unit in ("neighbours", "knn", "binaries"):
        assert "tile_masked(j0, g_lo, g_hi, n)" in _kernels(unit), unit
    for unit in ("field", "tracers", "tidal", "fof"):
        assert "TileWalk<T4> walk(" in _kernels(unit) and "walk.stage(tile, " in _kernels(unit), unit
    assert "TileWalk2<T4> walk(posm, velm, n, split, tiles_per_split);" in _kernels("jerk") and "walk.stage(ptile, vtile, k);" in _kernels("jerk")
    for unit in UNITS:  # the LDS arrays and the shape rule stay each unit's own
        assert "__shared__ T4 " in _kernels(unit) and "__shared__" not in _code(HEADER), unit


def test_every_unit_includes_the_header_and_its_makefile_rule_lists_it():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    for unit in UNITS:
        assert '#include "%s"' % HEADER in _kernels(unit), unit
        assert '#include "nbx_field_shape.hpp"' in _kernels(unit), unit
        rule = re.search(r"^\$\(PKG\)/nbx_%s\.o: \$\(CSRC\)/nbx_%s\.hip(.*)\n" % (unit, unit), mk, re.M)
        assert rule and "$(CSRC)/" + HEADER in rule.group(1).split(), unit
    assert mk.count(HEADER) == len(UNITS)  # and no other unit does
    for f in sorted(os.listdir(CSRC)):
        if f != HEADER and not (f.endswith("_kernels.hpp") and f[4:-12] in UNITS):
            assert HEADER not in _code(f), f
